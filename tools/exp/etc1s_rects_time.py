"""us per call of bu_etc1s_transcode_rects_device against the routes a caller had without it:
    python tools/exp/etc1s_rects_time.py [--targets bc1,bc3,rg11,rgba,etc1] [--rounds 3] [--calls 16]
A 512 x 512-block slice pair (2^18 blocks, colour and alpha indices; ETC1 takes the colour slice alone), codebooks of 4096 endpoints + 8192 selectors, four
index-array pairs in a cold rotation, HIP events around `calls` calls on a caller stream, / calls; one line per round and the median of the rounds.
  pages     256 pages of 32 x 32 blocks -- the whole slice, page by page -- into a page cache at pitch 4096, ONE rectangle call (four launches of 64 jobs)
  2d-copy   the same work without the call: the whole-slice device call into a tight buffer, then one 2-D device copy per page (hipMemcpy2DAsync where the
            process's HIP runtime can be found, else a strided torch copy)
  whole     one rectangle job over the whole slice at the tight pitch
  plain     the whole-slice device call (the L2-gather launch at this size): the yardstick of `whole`
BASISU_HIP_LIB=... times another build of the library."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import Context, _lib, synth  # noqa: E402

TGT = {"etc1": _lib.ETC1, "rgba": _lib.RGBA32, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG,
       "r11": _lib.EAC_R11, "rg11": _lib.EAC_RG11}
ap = argparse.ArgumentParser()
ap.add_argument("--targets", default="bc1,bc3,rg11,rgba,etc1")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=16)
a = ap.parse_args()
NBUF, NB, PAGE, PITCH = 4, 512, 32, 4096
N, N_EP, N_SEL = NB * NB, 4096, 8192
dev = torch.device("cuda", 0)
ctx = Context(0)
lib, h = ctx._lib, ctx._h
s = torch.cuda.Stream()


def hip_runtime():
    """the HIP runtime this process already uses (torch's), for hipMemcpy2DAsync"""
    try:
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                rt = ctypes.CDLL(line.split()[-1])
                rt.hipMemcpy2DAsync.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                                ctypes.c_void_p]
                rt.hipMemcpy2DAsync.restype = ctypes.c_int
                return rt
    except (OSError, AttributeError):
        pass
    return None


rt = hip_runtime()
print("2-D copies: %s" % ("hipMemcpy2DAsync" if rt else "strided torch copies"), flush=True)
ep, rows = synth.etc1s_codebooks(N_EP, N_SEL, seed=7)
sel = np.zeros((N_SEL, 8), dtype=np.uint8)
sel[:, :4] = rows
d_ep = torch.from_numpy(ep.view(np.int32)).to(dev)
d_sel = torch.from_numpy(sel.reshape(-1)).to(dev)
idx = [torch.from_numpy(synth.etc1s_indices(N, N_EP, N_SEL, seed=k).view(np.int32)).to(dev) for k in range(2 * NBUF)]
tight = [torch.empty(N * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
cache = [torch.empty(256 * 4 * PAGE * PITCH, dtype=torch.uint8, device=dev) for _ in range(NBUF)]  # 256 page slots of up to 128 rows at the pitch
torch.cuda.synchronize()
CB = (d_ep.data_ptr(), N_EP, d_sel.data_ptr(), N_SEL)


def plain(name, k, out):
    if name == "etc1":
        st = lib.bu_etc1s_transcode_etc1_device(h, idx[k].data_ptr(), N, *CB, out, None, s.cuda_stream)
    elif name == "rgba":
        st = lib.bu_etc1s_decode_rgba_device(h, idx[k].data_ptr(), idx[NBUF + k].data_ptr(), NB, NB, *CB, out, None, s.cuda_stream)
    else:
        st = lib.bu_etc1s_transcode_device(h, TGT[name], idx[k].data_ptr(), idx[NBUF + k].data_ptr(), N, *CB, out, None, s.cuda_stream)
    assert st == 0, (name, st)


def geometry(name):
    """row bytes of a block, output rows per block row"""
    return (16, 4) if name == "rgba" else (_lib.BLOCK_BYTES[TGT[name]], 1)


def job_tables(name):
    rb, rpb = geometry(name)
    pages, whole = [], []
    for k in range(NBUF):
        aidx = None if name == "etc1" else idx[NBUF + k].data_ptr()
        arr = (_lib.Etc1sRectJob * 256)()
        for p in range(256):
            arr[p] = _lib.Etc1sRectJob(idx[k].data_ptr(), aidx, NB, PAGE * (p % 16), PAGE * (p // 16), PAGE, PAGE, cache[k].data_ptr() + p * rpb * PAGE * PITCH, PITCH, 0)
        pages.append(arr)
        whole.append((_lib.Etc1sRectJob * 1)(_lib.Etc1sRectJob(idx[k].data_ptr(), aidx, NB, 0, 0, NB, NB, tight[k].data_ptr(), NB * rb, 0)))
    return pages, whole


def rects(name, arr):
    st = lib.bu_etc1s_transcode_rects_device(h, TGT[name], len(arr), arr, *CB, None, s.cuda_stream)
    assert st == 0, (name, st)


def copies(name, k):
    rb, rpb = geometry(name)
    spitch, width, height = NB * rb, PAGE * rb, rpb * PAGE
    if rt:
        for p in range(256):
            src = tight[k].data_ptr() + (p // 16) * height * spitch + (p % 16) * width
            st = rt.hipMemcpy2DAsync(cache[k].data_ptr() + p * height * PITCH, PITCH, src, spitch, width, height, 3, s.cuda_stream)
            assert st == 0, st
    else:
        src = tight[k][:rpb * NB * spitch].view(rpb * NB, spitch)
        with torch.cuda.stream(s):
            for p in range(256):
                dst = cache[k][p * height * PITCH:(p + 1) * height * PITCH].view(height, PITCH)
                dst[:, :width].copy_(src[(p // 16) * height:(p // 16 + 1) * height, (p % 16) * width:(p % 16 + 1) * width])


res = {}
for r in range(a.rounds):
    for name in a.targets.split(","):
        pages, whole = job_tables(name)
        routes = {"pages": lambda k: rects(name, pages[k]), "2d-copy": lambda k: (plain(name, k, tight[k].data_ptr()), copies(name, k)),
                  "whole": lambda k: rects(name, whole[k]), "plain": lambda k: plain(name, k, tight[k].data_ptr())}
        for route, call in routes.items():
            for k in range(NBUF):  # (warm)
                call(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(a.calls):
                call(i % NBUF)
            e1.record(s)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.calls
            res.setdefault((name, route), []).append(us)
            print("round %d %-5s %-8s %9.1f us per call" % (r, name, route, us), flush=True)
print("%-5s %10s %10s %10s %10s %12s   (us per call, median of %d rounds; parity unpinned)" % ("", "pages", "2d-copy", "whole", "plain", "whole/plain", a.rounds))
for name in a.targets.split(","):
    m = {route: float(np.median(res[name, route])) for route in ("pages", "2d-copy", "whole", "plain")}
    print("%-5s %10.1f %10.1f %10.1f %10.1f %12.3f" % (name, m["pages"], m["2d-copy"], m["whole"], m["plain"], m["whole"] / m["plain"]), flush=True)
torch.cuda.synchronize()
ctx.close()
