"""us per image of the encoders from pixels (bu_rgba_encode_blocks_device) beside the two launches that bracket them:
    python tools/exp/encode_time.py [--formats bc4,bc5,r11,rg11,bc1,bc3] [--sizes 4096,8192] [--rounds 3] [--launches 16]
Inputs: per size s, four UASTC atlases of (s / 4)^2 blocks, block i = golden UASTC block h(i) mod 608 (bench.py's uniform mix of the 19 modes, a seed
per atlas), and their RGBA32 unpack by the library itself as the s x s images -- so the encoders see exactly the texels the transcode sees, and the
blocks they write are the transcode's.  Per row: `launches` device calls on a caller stream in a cold rotation over the four buffers, hip events around
the loop, / launches; the median of `rounds`.  Rows per format:
    enc       bu_rgba_encode_blocks_device, tight pitch 4 s (a multiple of 16: the 16-byte loads)
    enc+4     the same image at pitch 4 s + 4 (BC4 and BC1 only: the 4-byte loads)
    uastc     bu_uastc_transcode_device to the same format over the atlases the images were unpacked from (the yardstick: enc / uastc is printed)
    dec       bu_blocks_decode_rgba_device of the same blocks back to an s x s image (the same bytes in the other direction)
Prints us, the ratio to the uastc row and the fraction of an 8 TB/s roofline over (64 + block bytes) x blocks.  BASISU_HIP_LIB selects another
build of the library, for an A/B.  Run it under rocprofv3 --kernel-trace --stats for the kernel view."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import Context, _lib, synth  # noqa: E402

FMT = {"bc4": _lib.BC4_R, "bc5": _lib.BC5_RG, "r11": _lib.EAC_R11, "rg11": _lib.EAC_RG11, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA}
ap = argparse.ArgumentParser()
ap.add_argument("--formats", default=",".join(FMT))
ap.add_argument("--sizes", default="4096,8192")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=16)
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
    uastc = [torch.from_numpy(synth.atlas_from_indices(golden, synth.gold_indices(n, seed=synth.GOLD_SEED + 17 * k)).reshape(-1)).to(dev) for k in range(NBUF)]
    rgba = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    for k in range(NBUF):
        ctx.transcode_device(_lib.RGBA32, uastc[k], n, rgba[k], bpr)
    torch.cuda.synchronize()
    pitch4 = 4 * size + 4
    rgba4 = []  # the same images at the unaligned pitch
    for k in range(NBUF):
        t = torch.zeros(size * pitch4, dtype=torch.uint8, device=dev)
        t.view(size, pitch4)[:, : 4 * size] = rgba[k].view(size, 4 * size)
        rgba4.append(t)
    back = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    res = {}
    for name in a.formats.split(","):
        f, bb = FMT[name], _lib.BLOCK_BYTES[FMT[name]]
        blocks = [torch.zeros(n * bb, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
        ref = [torch.zeros(n * bb, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
        rows = {
            "enc": lambda k: ctx.encode_blocks_device(f, rgba[k], size, size, blocks[k], stream=s),
            "uastc": lambda k: ctx.transcode_device(f, uastc[k], n, ref[k], bpr, stream=s),
            "dec": lambda k: ctx.decode_blocks_device(f, ref[k], n, back[k], bpr, stream=s),
        }
        if name in ("bc4", "bc1"):
            rows["enc+4"] = lambda k: ctx.encode_blocks_device(f, rgba4[k], size, size, blocks[k], in_pitch=pitch4, stream=s)
        for r in range(a.rounds):
            for row in ("uastc", "enc", "enc+4", "dec"):
                if row not in rows:
                    continue
                for k in range(NBUF):  # (warm)
                    rows[row](k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for i in range(a.launches):
                    rows[row](i % NBUF)
                e1.record(s)
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / a.launches
                res.setdefault((name, row), []).append(us)
                print("size %d round %d %-4s %-5s %9.1f us" % (size, r, name, row, us), flush=True)
                if row.startswith("enc") and r == 0 and not all(torch.equal(blocks[k], ref[k]) for k in range(NBUF)):
                    print("size %d %-4s %-5s DIFFERS from the transcode" % (size, name, row), flush=True)
                    sys.exit(1)
        del blocks, ref
    for (name, row), v in res.items():
        us, base = float(np.median(v)), float(np.median(res[name, "uastc"]))
        nbytes = ((16 if row == "uastc" else 64) + _lib.BLOCK_BYTES[FMT[name]]) * n
        print("median size %d %-4s %-5s %9.1f us  %5.2fx uastc  %5.2f of 8 TB/s" % (size, name, row, us, us / base, nbytes / (us * 1e-6) / 8e12), flush=True)
    del uastc, rgba, rgba4, back
    torch.cuda.empty_cache()
torch.cuda.synchronize()
ctx.close()
