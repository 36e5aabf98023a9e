"""What the block decoders (bu_blocks_decode_rgba) must write, from the suite's existing witnesses and never from the code
under test, and the inputs the CPU and the GPU tests share.

expected(dec, fmt, blocks)   -> (texels [n, 64] uint8, status [n]) from
    oracle/bu_decoders.c (pyoracle.Decoders)          ASTC, BC7, the EAC alpha half of ETC2, ETC1 and the colour half of ETC2
    tests/colour_model.py: bc1_decode                 BC1, and BC3's colour half rebuilt in four-colour form from the same palette expression
    tests/channel_model.py: bc4_decode / r11_decode   BC4, BC5, BC3's alpha half, EAC R11 / RG11
  with the rounding of section 4.9: an exact rational num / den becomes (2 num + den) // (2 den); R11's 11-bit t becomes (255 t + 1023) // 2047.
  A failing block is 64 zero bytes with status 1 (BU_ERR_INVALID_MODE: the oracle's RESERVED and ILLEGAL) or 17 (BU_ERR_UNSUPPORTED).
emul_decoder(tmp_path_factory) -> the product's block code as a stand-alone ASan + UBSan program, for tests/test_decode_blocks.py and
  tests/test_decode_fields.py (the latter judges ASTC and BC7 -- and oracle/bu_decoders.c itself -- by tests/astc_model.py and a third party).
"""
import os
import subprocess

import numpy as np

import channel_model as cm
import colour_model as col
from basisu_rs_amd import _lib

FORMATS = {"astc": _lib.ASTC, "bc7": _lib.BC7, "etc1": _lib.ETC1, "etc2": _lib.ETC2, "bc4": _lib.BC4_R, "bc5": _lib.BC5_RG, "r11": _lib.EAC_R11,
           "rg11": _lib.EAC_RG11, "bc1": _lib.BC1_RGB, "bc3": _lib.BC3_RGBA}
BLOCK_BYTES = {k: _lib.BLOCK_BYTES[v] for k, v in FORMATS.items()}
OK, INVALID, UNSUPPORTED = 0, _lib.ERR_INVALID_MODE, _lib.ERR_UNSUPPORTED
ORACLE_CLASS = np.array([OK, INVALID, UNSUPPORTED, INVALID])  # DEC_OK, DEC_RESERVED, DEC_UNSUPPORTED, DEC_ILLEGAL of bu_decoders.c


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EMUL = []


def emul_decoder(tmp_path_factory):
    """fmt, blocks -> (texels [n, 64], status [n]) through the sanitizer build of the product's block code (tests/host_emul/bu_emul_decode_main.cpp
    under AddressSanitizer and UBSan), a child process per call; compiled once per session"""
    if _EMUL:
        return _EMUL[0]
    d = tmp_path_factory.mktemp("emul_decode")
    exe = str(d / "bu_emul_decode")
    src = os.path.join(ROOT, "tests", "host_emul", "bu_emul_decode_main.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "basisu_rs_amd", "csrc"), "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(fmt, blocks):
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES[fmt])
        n = blocks.shape[0]
        with open(d / "in.bin", "wb") as f:
            f.write(np.int32(FORMATS[fmt]).tobytes() + blocks.tobytes())
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        o = np.fromfile(d / "out.bin", dtype=np.uint8)
        assert o.size == 65 * n
        return o[: 64 * n].reshape(n, 64), o[64 * n:].astype(np.int64)

    _EMUL.append(run)
    return run


def _round(num, den):
    return (2 * num + den) // (2 * den)


def _bc4(blk):
    num, den = cm.bc4_decode(blk)
    return _round(num, den[:, None])


def _r11(blk):
    return (255 * cm.r11_decode(blk) + 1023) // 2047


def _channels(x, y=None):
    n = x.shape[0]
    out = np.zeros((n, 16, 4), dtype=np.int64)
    out[:, :, 0] = x
    if y is not None:
        out[:, :, 1] = y
    out[:, :, 3] = 255
    return out


def _bc1(blk, four):
    """BC1 texels [n, 16, 4]; four = True: the four-colour form whatever the order of the endpoints (BC3's colour half; alpha left 0)"""
    num, den, opaque = col.bc1_decode(blk)
    out = np.zeros(num.shape[:2] + (4,), dtype=np.int64)
    if four:
        b = np.asarray(blk, dtype=np.uint8).astype(np.int64)
        w0, w1 = b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8)
        c0, c1 = col.expand(np.stack([w0 >> 11, (w0 >> 5) & 63, w0 & 31], -1)), col.expand(np.stack([w1 >> 11, (w1 >> 5) & 63, w1 & 31], -1))
        pal4 = np.stack([3 * c0, 3 * c1, 2 * c0 + c1, c0 + 2 * c1], 1)
        code = ((b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24))[:, None] >> (2 * np.arange(16, dtype=np.int64))) & 3
        out[:, :, :3] = _round(np.take_along_axis(pal4, code[:, :, None], 1), 3)
        return out
    out[:, :, :3] = np.where(opaque[:, :, None], _round(num, den[:, None, None]), 0)
    out[:, :, 3] = np.where(opaque, 255, 0)
    return out


def expected(dec, fmt, blocks):
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES[fmt])
    n = blocks.shape[0]
    st = np.zeros(n, dtype=np.int64)
    if fmt == "astc" or fmt == "bc7":
        px, ost = (dec.astc if fmt == "astc" else dec.bc7)(blocks)
        st = ORACLE_CLASS[ost]
        px = px.reshape(n, 16, 4).astype(np.int64)
    elif fmt == "etc1" or fmt == "etc2":
        px, fields = dec.etc1_both(blocks[:, -8:])
        px = px.reshape(n, 16, 4).astype(np.int64)
        st = np.where(fields["mode"] >= 2, UNSUPPORTED, OK)
        if fmt == "etc2":
            px[:, :, 3] = dec.eac_alpha(blocks)
    elif fmt == "bc4":
        px = _channels(_bc4(blocks))
    elif fmt == "bc5":
        px = _channels(_bc4(blocks[:, :8]), _bc4(blocks[:, 8:]))
    elif fmt == "r11":
        px = _channels(_r11(blocks))
    elif fmt == "rg11":
        px = _channels(_r11(blocks[:, :8]), _r11(blocks[:, 8:]))
    elif fmt == "bc1":
        px = _bc1(blocks, False)
    else:
        px = _bc1(blocks[:, 8:], True)
        px[:, :, 3] = _bc4(blocks[:, :8])
    px = np.where((st == OK)[:, None, None], px, 0)
    assert px.min() >= 0 and px.max() <= 255
    return px.astype(np.uint8).reshape(n, 64), st


def image(texels, bpr):
    """block texels [n, 64] -> the row-major RGBA8 image [4 * rows, 16 * bpr] bytes"""
    n = texels.shape[0]
    return np.ascontiguousarray(texels.reshape(n // bpr, bpr, 4, 16).transpose(0, 2, 1, 3)).reshape(4 * (n // bpr), 16 * bpr)


def random_blocks(fmt, n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, BLOCK_BYTES[fmt]), dtype=np.uint8)


def shaped_astc(n, seed):
    """random 128-bit blocks with the block mode forced onto a 4x4 weight grid: bits 0-1 = R >> 1, 2-3 = 0, 4 = R & 1, 5-6 = 2, 7-8 = 0 with R uniform
    in 2..7; bits 9-10 (high precision, dual plane) stay random; bits 23-24 = 0 (one endpoint mode for all partitions)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    R = rng.integers(2, 8, size=n).astype(np.uint32)
    w = a[:, :4].copy().view("<u4").reshape(-1)
    w &= ~np.uint32(0x1FF | (3 << 23))
    w |= (R >> 1) | ((R & 1) << 4) | np.uint32(2 << 5)
    a[:, :4] = w.view(np.uint8).reshape(-1, 4)
    return a


def astc_groups(blocks):
    """header fields of ASTC blocks that are not void-extent: partitions 1..4, dual plane flag, endpoint mode (the shared one)"""
    w = blocks[:, :4].copy().view("<u4").reshape(-1).astype(np.int64)
    parts = ((w >> 11) & 3) + 1
    dual = (w >> 10) & 1
    cem = np.where(parts == 1, (w >> 13) & 15, (w >> 25) & 15)
    return parts, dual, cem


def encoder_outputs(oracle, uastc):
    """all ten formats' blocks for the given UASTC blocks, made on the CPU: the oracle's transcoders and the numpy models of sections 4.4 / 4.5"""
    rgba, st = oracle.batch("rgba", uastc)
    assert (st == 0).all()
    out = {k: oracle.batch(k, uastc)[0] for k in ("astc", "bc7", "etc1", "etc2")}
    for k in ("bc4", "bc5", "r11", "rg11"):
        out[k] = cm.encode(k, rgba)
    for k in ("bc1", "bc3"):
        out[k] = col.encode(k, rgba)
    return out, rgba


def edge_blocks():
    """the edge blocks of the issue, by construction: {format: [n, bytes]}"""
    e = {}
    # BC1: w0 == w1 and w0 < w1, every code including 3
    codes = np.array([0x1B, 0xE4, 0xFF, 0x00], dtype=np.uint8)  # texels cycle through 3, 2, 1, 0 / 0..3 / all 3 / all 0
    bc1 = []
    for w0, w1 in ((0x8410, 0x8410), (0x0000, 0xFFFF), (0x1234, 0xFEDC), (0xFFFF, 0xFFFF), (0x0000, 0x0000), (0xFEDC, 0x1234)):
        bc1.append([w0 & 255, w0 >> 8, w1 & 255, w1 >> 8] + list(codes))
    e["bc1"] = np.array(bc1, dtype=np.uint8)
    # BC4: r0 == r1 and r0 < r1 with codes 6 and 7 (the string 0..7 repeated covers every code)
    sel = sum((i % 8) << (3 * i) for i in range(16))
    selb = [(sel >> (8 * k)) & 255 for k in range(6)]
    e["bc4"] = np.array([[r0, r1] + selb for r0, r1 in ((77, 77), (0, 0), (255, 255), (10, 200), (0, 255), (200, 10), (254, 255), (1, 0))], dtype=np.uint8)
    e["bc5"] = np.concatenate([e["bc4"], e["bc4"][::-1]], axis=1)
    e["bc3"] = np.concatenate([e["bc4"][:6], e["bc1"]], axis=1)
    # EAC: multiplier 0, and values clamped at both ends (base 0 / 255 with the widest tables and multiplier 15)
    selr = sum((i % 8) << (45 - 3 * i) for i in range(16))
    selrb = [(selr >> (8 * (5 - k))) & 255 for k in range(6)]
    eac = [[base, (mult << 4) | table] + selrb for base in (0, 3, 128, 252, 255) for mult in (0, 1, 15) for table in (0, 13, 15)]
    e["r11"] = np.array(eac, dtype=np.uint8)
    e["rg11"] = np.concatenate([e["r11"], e["r11"][::-1]], axis=1)
    # ETC1: differential blocks whose second base colour is exactly 0 and exactly 31 (in range), and one step beyond (T / H / planar)
    etc = []
    for c, d in ((3, -3), (4, -4), (28, 3), (27, 3), (0, 0), (31, 0), (2, -3), (29, 3)):
        byte = (c << 3) | (d & 7)
        for ch in range(3):
            hdr = [(1 << 3) | 0, (1 << 3) | 0, (1 << 3) | 0]  # other channels: 1 + 0
            hdr[ch] = byte
            for flip in (0, 1):
                etc.append(hdr + [(5 << 5) | (2 << 2) | 2 | flip, 0x12, 0x34, 0xC3, 0xA5])
    e["etc1"] = np.array(etc, dtype=np.uint8)
    alpha = np.array(eac, dtype=np.uint8)
    reps = -(-e["etc1"].shape[0] // alpha.shape[0])
    e["etc2"] = np.concatenate([np.tile(alpha, (reps, 1))[: e["etc1"].shape[0]], e["etc1"]], axis=1)
    # ASTC: LDR void-extent blocks (all-ones extent), an HDR one (unsupported) and one with the reserved bits clear (invalid)
    # then an extent that is ordered (s 10..20, t 5..30: decodes), one that is not (s 20..10: invalid) and a reserved block mode (bits 0-1 = 00,
    # bits 6-8 = 111, not void-extent: invalid)
    def void(bits12, rgba16, extent=(0x1FFF, 0x1FFF, 0x1FFF, 0x1FFF)):
        w = 0x1FC | (bits12 << 9) | sum(v << (12 + 13 * k) for k, v in enumerate(extent))
        b = list(int(w).to_bytes(8, "little"))
        for v in rgba16:
            b += [v & 255, v >> 8]
        return b
    e["astc"] = np.array([void(6, (0x1234, 0xFFFF, 0x0000, 0x80FF)), void(6, (0xFF00, 0x00FF, 0x7F80, 0xFFFF)), void(7, (0x3C00, 0x3C00, 0x3C00, 0x3C00)),
                          void(2, (1, 2, 3, 4)), void(0, (1, 2, 3, 4)), void(6, (0x1234, 0xFFFF, 0x0000, 0x80FF), (10, 20, 5, 30)),
                          void(6, (0x1234, 0xFFFF, 0x0000, 0x80FF), (20, 10, 5, 30)), [0xC4, 0x01] + [0x55] * 14], dtype=np.uint8)
    e["bc7"] = np.array([[0] * 16, [0] + [0xFF] * 15, [0x80] + [0] * 15, [0x80] + [0xFF] * 15, [0x40] + [0xFF] * 15, [0x01] + [0xFF] * 15], dtype=np.uint8)
    return e
