"""us per image of the encoder from pixels to UASTC (bu_rgba_encode_uastc_device) beside the BC1 encode of the same images:
    python tools/exp/uastc_encode_time.py [--sizes 4096] [--rounds 3] [--launches 8]
Inputs: per size s, four images of s x s pixels (a multiple of 16 wide, so the 16-byte loads): the RGBA32 unpack, by the library itself, of UASTC atlases
of (s / 4)^2 blocks, block i = golden UASTC block h(i) mod 608 (bench.py's uniform mix of the 19 modes, a seed per atlas) -- blocks with and without
alpha, smooth and busy, a few solid.  Rows:
    alpha     the images as they are: solid, opaque, grey and alpha blocks mixed, as the source atlas mixes its modes
    opaque    the same images with A := 255: every non-solid block takes the three RGB candidates, no etc2tm search
    bc1       bu_rgba_encode_blocks_device to BC1 of the first set, in the same run
Per row: `launches` device calls on a caller stream in a cold rotation over the four buffers, hip events around the loop, / launches; the median of
`rounds`.  Also prints the share of each UASTC mode in the encoder's output.  BASISU_HIP_LIB selects another build of the library, for an A/B."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import Context, _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="4096")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=8)
a = ap.parse_args()
NBUF = 4
dev = torch.device("cuda", 0)
ctx = Context(0)
s = torch.cuda.Stream()
golden = synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin"))["uastc"]
print("library %s" % _lib.LIB_PATH, flush=True)
for size in [int(v) for v in a.sizes.split(",")]:
    bpr = size // 4
    n = bpr * bpr
    rgba = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    for k in range(NBUF):
        src = torch.from_numpy(synth.atlas_from_indices(golden, synth.gold_indices(n, seed=synth.GOLD_SEED + 17 * k)).reshape(-1)).to(dev)
        ctx.transcode_device(_lib.RGBA32, src, n, rgba[k], bpr)
    torch.cuda.synchronize()
    opaque = [t.clone() for t in rgba]
    for t in opaque:
        t.view(-1, 4)[:, 3] = 255
    out = [torch.zeros(n * 16, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    bc1 = [torch.zeros(n * 8, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    rows = {
        "alpha": lambda k: ctx.encode_uastc_device(rgba[k], size, size, out[k], stream=s),
        "opaque": lambda k: ctx.encode_uastc_device(opaque[k], size, size, out[k], stream=s),
        "bc1": lambda k: ctx.encode_blocks_device(_lib.BC1_RGB, rgba[k], size, size, bc1[k], stream=s),
    }
    res = {}
    for r in range(a.rounds):
        for row in rows:
            for k in range(NBUF):  # (warm)
                rows[row](k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for i in range(a.launches):
                rows[row](i % NBUF)
            e1.record(s)
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.launches
            res.setdefault(row, []).append(us)
            print("size %d round %d %-6s %10.1f us" % (size, r, row, us), flush=True)
            if r == 0 and row != "bc1":
                modes = synth.block_modes(out[0].cpu().numpy().reshape(-1, 16))
                share = np.bincount(modes, minlength=20) / modes.size
                print("size %d %-6s modes %s" % (size, row, " ".join("%d:%.3f" % (m, share[m]) for m in range(20) if share[m] > 0)), flush=True)
    for row, v in res.items():
        us = float(np.median(v))
        print("median size %d %-6s %10.1f us  %6.1f ns per block  %5.1fx bc1" % (size, row, us, us * 1e3 / n, us / float(np.median(res["bc1"]))), flush=True)
    del rgba, opaque, out, bc1
    torch.cuda.empty_cache()
torch.cuda.synchronize()
ctx.close()
