"""us per call of bu_uastc_transcode_rects_device beside the closest routes without it:
    python tools/exp/rects_time.py [--targets bc7,etc1,rgba] [--rounds 3] [--calls 16] [--sets 16]      (--calls: the pages loops)
  pages   256 pages of 32 x 32 blocks cut at seeded positions from four 4096^2 slices (1024 x 1024 blocks each, separate allocations) into a page cache
          with 4096-byte pitch.
            rects   ONE call of bu_uastc_transcode_rects_device (256 jobs)
            rows    bu_uastc_transcode_batch_device over the pages' 8192 block rows as 32-block slices into a tight buffer, then one hipMemcpy2DAsync
                    per page into the cache -- what a caller does without the call
  whole   one 4096^2 slice:
            rects   one job over the whole slice at a padded pitch (the row + 256 bytes)
            plain   bu_uastc_transcode_device, tight
Content: known-answer blocks drawn uniformly (every mode, mixed).  Cold: `sets` sets of four slices (16 MiB a slice: 16 sets = 1 GiB of input).  A `whole`
call takes the next of the sets x 4 slices and the next of `sets` outputs, a timing loop is one walk over all of them (64 calls: 1 GiB read, 16 outputs of
8 - 65 MiB written, each again only after the 15 others).  A `pages` call takes the next set: its 256 pages are 4 MiB of the set's 64 MiB, so the 16 calls of
a loop read 64 MiB in all and the same pages again in the next round -- that comparison is bound by the host's enqueues, not by memory.  HIP events around
the calls of a loop on one stream, / calls; one line per round, then the median.
BASISU_HIP_LIB=... times another build of the library; a build without the call (the parent commit's) runs the `rows` and `plain` routes only.  The
library is bound here, not through basisu_rs_amd._lib, so that both builds load."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import synth  # noqa: E402

TGT = {"astc": (0, 16, 1), "bc7": (1, 16, 1), "etc1": (2, 8, 1), "etc2": (3, 16, 1), "rgba": (4, 16, 4)}  # bu_target, bytes of a block per output row, rows per block
ap = argparse.ArgumentParser()
ap.add_argument("--targets", default="bc7,etc1,rgba")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=16)
ap.add_argument("--sets", type=int, default=16)
a = ap.parse_args()
vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64


class RectJob(ctypes.Structure):
    _fields_ = [("d_in", vp), ("in_blocks_per_row", ctypes.c_uint32), ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("w", ctypes.c_uint32),
                ("h", ctypes.c_uint32), ("d_out", vp), ("out_pitch_bytes", u64), ("index_base", u64)]


L = ctypes.CDLL(os.environ.get("BASISU_HIP_LIB") or os.path.join(ROOT, "basisu_rs_amd", "libbasisu_hip.so"))
L.bu_context_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
L.bu_context_destroy.argtypes = [vp]
L.bu_uastc_transcode_device.argtypes = [vp, ctypes.c_int, vp, sz, vp, sz, u64, vp, vp]
L.bu_uastc_transcode_batch_device.argtypes = [vp, ctypes.c_int, sz, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp), sz, vp, vp, vp]
HAVE_RECTS = hasattr(L, "bu_uastc_transcode_rects_device")
if HAVE_RECTS:
    L.bu_uastc_transcode_rects_device.argtypes = [vp, ctypes.c_int, sz, ctypes.POINTER(RectJob), vp, vp]
# the HIP runtime this process already maps (PyTorch-ROCm brings its own): hipMemcpy2DAsync
hip_path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
HIP = ctypes.CDLL(hip_path)
HIP.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, ctypes.c_int, vp]
D2D = 3

dev = torch.device("cuda", 0)
h = vp()
assert L.bu_context_create(0, ctypes.byref(h)) == 0
s = torch.cuda.Stream()
sp = s.cuda_stream
NB, PAGE, NPAGES, NSL = 1024, 32, 256, 4
gold = torch.from_numpy(synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin"))["uastc"]).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(4096)
slices = [[gold[torch.randint(0, 608, (NB * NB,), generator=gen, device=dev)].contiguous() for _ in range(NSL)] for _ in range(a.sets)]
rng = np.random.default_rng(7)
pages = [[(int(rng.integers(0, NSL)), PAGE * int(rng.integers(0, NB // PAGE)), PAGE * int(rng.integers(0, NB // PAGE))) for _ in range(NPAGES)] for _ in range(a.sets)]
torch.cuda.synchronize()
res = {}


def timed(key, call, warm, calls):
    for k in range(warm):
        call(k)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(calls):
        call(i)
    e1.record(s)
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / calls
    res.setdefault(key, []).append(us)
    print("round  %-18s %9.1f us per call" % ("%s %s %s" % key, us), flush=True)


for name in a.targets.split(","):
    t, rb, rpb = TGT[name]
    bb = rb * rpb
    PITCH = 4096
    per_row = PITCH // (PAGE * rb)            # page slots side by side in a cache row
    slot_rows = -(-NPAGES // per_row)
    cache = [torch.empty(slot_rows * PAGE * rpb * PITCH, dtype=torch.uint8, device=dev) for _ in range(a.sets)]
    tight = [torch.empty(NPAGES * PAGE * PAGE * bb, dtype=torch.uint8, device=dev) for _ in range(a.sets)]

    def slot(k, p):
        return cache[k].data_ptr() + (p // per_row) * PAGE * rpb * PITCH + (p % per_row) * PAGE * rb

    # the tables of both routes, built once (the enqueue is what is timed)
    jobs, rows_in, rows_out = [], [], []
    for k in range(a.sets):
        jobs.append((RectJob * NPAGES)(*[RectJob(slices[k][sl].data_ptr(), NB, x0, y0, PAGE, PAGE, slot(k, p), PITCH, 0) for p, (sl, x0, y0) in enumerate(pages[k])]))
        rows_in.append((vp * (NPAGES * PAGE))(*[slices[k][sl].data_ptr() + 16 * ((y0 + r) * NB + x0) for (sl, x0, y0) in pages[k] for r in range(PAGE)]))
        rows_out.append((vp * (NPAGES * PAGE))(*[tight[k].data_ptr() + i * PAGE * bb for i in range(NPAGES * PAGE)]))
    rows_n = (sz * (NPAGES * PAGE))(*([PAGE] * (NPAGES * PAGE)))

    def pages_rects(i):
        k = i % a.sets
        assert L.bu_uastc_transcode_rects_device(h, t, NPAGES, jobs[k], None, sp) == 0

    def pages_rows(i):
        k = i % a.sets
        assert L.bu_uastc_transcode_batch_device(h, t, NPAGES * PAGE, rows_in[k], rows_n, rows_out[k], PAGE, None, None, sp) == 0
        for p in range(NPAGES):  # a page's 32 row slices lie back to back in the tight buffer: PAGE * rpb rows of PAGE * rb bytes
            assert HIP.hipMemcpy2DAsync(slot(k, p), PITCH, tight[k].data_ptr() + p * PAGE * PAGE * bb, PAGE * rb, PAGE * rb, PAGE * rpb, D2D, sp) == 0

    # both routes fill the cache with the same bytes
    if HAVE_RECTS:
        pages_rects(0)
        torch.cuda.synchronize()
        ref = cache[0].clone()
        cache[0].zero_()
        pages_rows(0)
        torch.cuda.synchronize()
        assert slot_rows * per_row == NPAGES and torch.equal(ref, cache[0]), name  # (the slots tile the cache exactly)

    wpitch = NB * rb + 256
    flat = [sl for st in slices for sl in st]  # the whole-slice calls walk every slice of the rotation
    whole_out = [torch.empty(NB * rpb * wpitch, dtype=torch.uint8, device=dev) for _ in range(a.sets)]
    whole_jobs = [(RectJob * 1)(RectJob(flat[i].data_ptr(), NB, 0, 0, NB, NB, whole_out[i % a.sets].data_ptr(), wpitch, 0)) for i in range(len(flat))]

    def whole_rects(i):
        assert L.bu_uastc_transcode_rects_device(h, t, 1, whole_jobs[i % len(flat)], None, sp) == 0

    def whole_plain(i):
        assert L.bu_uastc_transcode_device(h, t, flat[i % len(flat)].data_ptr(), NB * NB, whole_out[i % a.sets].data_ptr(), NB, 0, None, sp) == 0

    for r in range(a.rounds):
        if HAVE_RECTS:
            timed((name, "pages", "rects"), pages_rects, 4, a.calls)
        timed((name, "pages", "rows"), pages_rows, 2, a.calls)
        if HAVE_RECTS:
            timed((name, "whole", "rects"), whole_rects, 4, len(flat))
        timed((name, "whole", "plain"), whole_plain, 4, len(flat))
    del cache, tight, whole_out, jobs, rows_in, rows_out, whole_jobs
for key, v in res.items():
    print("median %-18s %9.1f us per call" % ("%s %s %s" % key, float(np.median(v))), flush=True)
torch.cuda.synchronize()
L.bu_context_destroy(h)
