"""us per ETC1S slice of the ETC1S targets (BC1, BC3, BC4, BC5, EAC R11, EAC RG11) beside ETC1S -> ETC1 / RGBA32:
    python tools/exp/etc1s_targets_time.py [--targets etc1,rgba,bc1,bc3,bc4,bc5,r11,rg11] [--sizes 20,22] [--rounds 3] [--launches 16]
Codebooks (synth.etc1s_codebooks): "staged" 4096 endpoints + 8192 selectors (49 KiB: the LDS-staged kernel from 2^19 blocks), "gather"
24000 + 24000 (188 KiB, more than the 152 KiB the staged kernels may use: the L2 gather at every size).  Per codebook, size and target: 4
index arrays (random indices, with a paired alpha slice), `launches` device calls on a caller stream in a cold rotation over them, hip
events around the loop, / launches.  Prints one line per round and the median.  BASISU_HIP_LIB=... times another build of the library
(the A/B of the palette form against a build that decodes RGBA32 and runs the 16-texel encoders).  Run it under
rocprofv3 --kernel-trace --stats for the kernel view."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import Context, _lib, synth  # noqa: E402

TGT = {"etc1": _lib.ETC1, "rgba": _lib.RGBA32, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG,
       "r11": _lib.EAC_R11, "rg11": _lib.EAC_RG11}
BOOKS = {"staged": (4096, 8192), "gather": (24000, 24000)}
ap = argparse.ArgumentParser()
ap.add_argument("--targets", default="etc1,rgba,bc1,bc3,bc4,bc5,r11,rg11")
ap.add_argument("--sizes", default="20,22")
ap.add_argument("--books", default="staged,gather")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=16)
a = ap.parse_args()
NBUF = 4
dev = torch.device("cuda", 0)
ctx = Context(0)
lib = ctx._lib
h = ctx._h
s = torch.cuda.Stream()
res = {}
for book in a.books.split(","):
    n_ep, n_sel = BOOKS[book]
    ep, rows = synth.etc1s_codebooks(n_ep, n_sel, seed=7)
    sel = np.zeros((n_sel, 8), dtype=np.uint8)
    sel[:, :4] = rows
    d_ep = torch.from_numpy(ep.view(np.int32)).to(dev)
    d_sel = torch.from_numpy(sel.reshape(-1)).to(dev)
    for lg in (int(x) for x in a.sizes.split(",")):
        n = 1 << lg
        idx = [torch.from_numpy(synth.etc1s_indices(n, n_ep, n_sel, seed=k).view(np.int32)).to(dev) for k in range(2 * NBUF)]
        out = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
        torch.cuda.synchronize()

        def launch(name, k):
            t = TGT[name]
            if name == "etc1":
                st = lib.bu_etc1s_transcode_etc1_device(h, idx[k].data_ptr(), n, d_ep.data_ptr(), n_ep, d_sel.data_ptr(), n_sel, out[k].data_ptr(),
                                                        None, s.cuda_stream)
            elif name == "rgba":
                st = lib.bu_etc1s_decode_rgba_device(h, idx[k].data_ptr(), idx[NBUF + k].data_ptr(), 1024, n // 1024, d_ep.data_ptr(), n_ep,
                                                     d_sel.data_ptr(), n_sel, out[k].data_ptr(), None, s.cuda_stream)
            else:
                st = lib.bu_etc1s_transcode_device(h, t, idx[k].data_ptr(), idx[NBUF + k].data_ptr(), n, d_ep.data_ptr(), n_ep, d_sel.data_ptr(),
                                                   n_sel, out[k].data_ptr(), None, s.cuda_stream)
            assert st == 0, (name, st)

        for r in range(a.rounds):
            for name in a.targets.split(","):
                for k in range(NBUF):  # (warm)
                    launch(name, k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for i in range(a.launches):
                    launch(name, i % NBUF)
                e1.record(s)
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / a.launches
                res.setdefault((book, lg, name), []).append(us)
                print("round %d %-6s 2^%d %-5s %8.1f us per slice" % (r, book, lg, name, us), flush=True)
        del idx, out
for (book, lg, name), v in res.items():
    print("median %-6s 2^%d %-5s %8.1f us per slice" % (book, lg, name, float(np.median(v))), flush=True)
torch.cuda.synchronize()
ctx.close()
