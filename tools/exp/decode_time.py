"""us per 2^20 blocks of the block decoders (bu_blocks_decode_rgba_device) beside the existing UASTC -> RGBA32 launch:
    python tools/exp/decode_time.py [--formats astc,bc7,etc1,etc2,bc4,bc5,r11,rg11,bc1,bc3] [--lg 20] [--rounds 3] [--launches 16]
Inputs: four atlases of 2^lg blocks, block i = golden UASTC block h(i) mod 608 (bench.py's uniform mix of the 19 modes, a seed per atlas), transcoded
by the library itself to each format -- so BC7 and ASTC mix modes inside every wave.  Per format: `launches` device calls on a caller stream in a
cold rotation over the four buffers (16 + 64 MiB each), hip events around the loop, / launches; the median of `rounds`.  The yardstick row "uastc"
is bu_uastc_transcode_device(BU_TARGET_RGBA32) over the same atlases in the same run.  Prints us and the fraction of an 8 TB/s roofline over
(block bytes + 64) x 2^lg bytes.  Run it under rocprofv3 --kernel-trace --stats for the kernel view."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from basisu_rs_amd import Context, _lib, synth  # noqa: E402

FMT = {"astc": _lib.ASTC, "bc7": _lib.BC7, "etc1": _lib.ETC1, "etc2": _lib.ETC2, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG, "r11": _lib.EAC_R11,
       "rg11": _lib.EAC_RG11, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA}
ap = argparse.ArgumentParser()
ap.add_argument("--formats", default=",".join(FMT))
ap.add_argument("--lg", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=16)
a = ap.parse_args()
NBUF, BPR = 4, 1024
n = 1 << a.lg
dev = torch.device("cuda", 0)
ctx = Context(0)
s = torch.cuda.Stream()
golden = synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin"))["uastc"]
uastc = [torch.from_numpy(synth.atlas_from_indices(golden, synth.gold_indices(n, seed=synth.GOLD_SEED + 17 * k)).reshape(-1)).to(dev) for k in range(NBUF)]
out = [torch.empty(n * 64, dtype=torch.uint8, device=dev) for _ in range(NBUF)]
names = ["uastc"] + a.formats.split(",")
blocks = {"uastc": uastc}
for name in names[1:]:
    blocks[name] = [torch.empty(n * _lib.BLOCK_BYTES[FMT[name]], dtype=torch.uint8, device=dev) for _ in range(NBUF)]
    for k in range(NBUF):
        ctx.transcode_device(FMT[name], uastc[k], n, blocks[name][k], BPR)
torch.cuda.synchronize()


def launch(name, k):
    if name == "uastc":
        ctx.transcode_device(_lib.RGBA32, uastc[k], n, out[k], BPR, stream=s)
    else:
        ctx.decode_blocks_device(FMT[name], blocks[name][k], n, out[k], BPR, stream=s)


res = {}
for r in range(a.rounds):
    for name in names:
        for k in range(NBUF):  # (warm)
            launch(name, k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for i in range(a.launches):
            launch(name, i % NBUF)
        e1.record(s)
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.launches
        res.setdefault(name, []).append(us)
        print("round %d %-5s %8.1f us" % (r, name, us), flush=True)
for name, v in res.items():
    us = float(np.median(v))
    nbytes = ((16 if name == "uastc" else _lib.BLOCK_BYTES[FMT[name]]) + 64) * n
    print("median %-5s 2^%d blocks %8.1f us  %5.2f of 8 TB/s  %5.2fx the uastc row" % (name, a.lg, us, nbytes / (us * 1e-6) / 8e12, us / float(np.median(res["uastc"]))),
          flush=True)
torch.cuda.synchronize()
ctx.close()
