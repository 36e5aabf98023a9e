"""us per 2^20-block atlas of the colour targets (BC1, BC3) beside ETC1 / ETC2, BC4 / BC5 and EAC R11:
    python tools/exp/colour_time.py [--targets etc1,etc2,bc4,bc5,r11,bc1,bc3] [--rounds 3] [--launches 64]
Atlases: 64 x 2^20 blocks drawn from the 608 reference UASTC vectors (seeded), block pitch 1024.  Per target and round:
  lone    bu_time_uastc_launches_streams_window on one stream (`launches` timed launches, cold rotation over the 64 atlases)
  four    the same on four streams
  batch   one bu_uastc_transcode_batch_device call over all 64 atlases, hip events around it, / 64
Prints one line per target and round, then the median of the rounds.  Run it under rocprofv3 --kernel-trace --stats for the kernel view."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import _lib, synth  # noqa: E402

TGT = {"etc1": _lib.ETC1, "etc2": _lib.ETC2, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG, "r11": _lib.EAC_R11, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA}
ap = argparse.ArgumentParser()
ap.add_argument("--targets", default="etc1,etc2,bc4,bc5,r11,bc1,bc3")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=64)
ap.add_argument("--atlases", type=int, default=64)
a = ap.parse_args()
N, NBUF, BPR = 1 << 20, a.atlases, 1024
vp = ctypes.c_void_p
lib = _lib.load()
lib.bu_time_uastc_launches_streams_window.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                                      ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_float),
                                                      ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
dev = torch.device("cuda", 0)
g = synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin"))
gu = torch.from_numpy(g["uastc"]).to(dev)
ins = []
for k in range(NBUF):
    gen = torch.Generator(device=dev)
    gen.manual_seed(k + 1)
    ins.append(gu[torch.randint(0, gu.shape[0], (N,), device=dev, generator=gen)].contiguous())
outs = [torch.empty((N, 16), dtype=torch.uint8, device=dev) for _ in range(NBUF)]
A = vp * NBUF
ip, op = A(*[x.data_ptr() for x in ins]), A(*[x.data_ptr() for x in outs])
sizes = (ctypes.c_size_t * NBUF)(*[N] * NBUF)
h = vp()
assert lib.bu_context_create(0, ctypes.byref(h)) == 0
torch.cuda.synchronize()


def window(t, ns, first):
    ev, host, late = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int(0)
    st = lib.bu_time_uastc_launches_streams_window(h, t, ip, op, NBUF, first, N, BPR, 16, a.launches, ns, ns, None, ctypes.byref(ev), ctypes.byref(host), None,
                                                   ctypes.byref(late))
    assert st == 0, st
    return max(ev.value, host.value) / a.launches * 1e3


def batch(t):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    assert lib.bu_uastc_transcode_batch_device(h, t, NBUF, ip, sizes, op, BPR, None, None, vp(s.cuda_stream)) == 0
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / NBUF


res = {}
for r in range(a.rounds):
    for name in a.targets.split(","):
        t = TGT[name]
        batch(t)  # (warm)
        row = (window(t, 1, r * 7), window(t, 4, r * 7 + 3), batch(t))
        res.setdefault(name, []).append(row)
        print("round %d %-5s lone %7.1f  four %7.1f  batch %7.1f us per atlas" % ((r, name) + row), flush=True)
for name, rows in res.items():
    m = np.median(np.array(rows), 0)
    print("median %-5s lone %7.1f  four %7.1f  batch %7.1f us per atlas" % (name, m[0], m[1], m[2]), flush=True)
torch.cuda.synchronize()
lib.bu_context_destroy(h)  # (the context's streams and events go before the runtime's own teardown at exit)
