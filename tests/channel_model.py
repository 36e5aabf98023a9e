"""Independent numpy model of the one- and two-channel targets (BC4, BC5, EAC R11, EAC RG11) and spec decoders for them.

The encoders are written from the rules of DESIGN.md section 4.4, not from the kernel:
  input  v[i] = byte c of texel i (i = 4y + x) of the block's RGBA32 decode; c = 0 (R) or 3 (A)
  BC4    mn, mx; byte 0 = mx, byte 1 = mn; q = floor((14 (v - mn) + d) / 2d) (d = mx - mn; d = 0: every selector 0);
         code q = 7 -> 0, q = 0 -> 1, else 8 - q; texel i's code at bits 3i of the little-endian 48-bit string in bytes 2..7
  R11    t = (2047 v + 127) // 255; solid: mult 0, table 13, base = min(mn >> 3, 255); else every table k with
         mult = min(15, ceil(span / 8R)), base = min(255, (mn + mx + 8 mult) // 16), values clamp(8 base + 4 + 8 mult mod, 0, 2047),
         nearest value (lower j on a tie), E_k = sum of squared errors, the smallest E_k (lower k on a tie);
         byte 0 = base, byte 1 = mult << 4 | table, bytes 2..7 the 48-bit string big-endian with pixel id = 4x + y at bits 45 - 3 id
  BC5 = BC4(R) + BC4(A), RG11 = R11(R) + R11(A)

The decoders are written from the Khronos Data Format Specification (BC4 UNORM, section "BC4"; ETC2 EAC R11 unsigned, section
"Format R11 EAC"), again without looking at the encoders.
"""
import numpy as np

# Khronos Data Format Specification, table "Intensity modifier sets for the alpha component" (ETC2 EAC), rows 0..15, spec order j = 0..7
EAC_MODS = np.array([
    [-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
    [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
    [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
    [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8],
], dtype=np.int64)
EAC_RANGE = EAC_MODS.max(1) - EAC_MODS.min(1)

CHANNEL_TARGETS = {"bc4": (6, 8), "bc5": (7, 16), "r11": (8, 8), "rg11": (9, 16)}  # name -> (bu_target, bytes per block)
# texel i = 4y + x of the 48-bit string position id = 4x + y (EAC is column-major)
_ID_TEXEL = np.array([4 * (pid & 3) + (pid >> 2) for pid in range(16)])
CHUNK = 4096


def channel(rgba, c):
    """rgba [n, 64] (RGBA32 bytes of each block, row-major texels) -> v [n, 16] int64, channel byte c"""
    return np.asarray(rgba, dtype=np.uint8).reshape(-1, 16, 4)[:, :, c].astype(np.int64)


def _u48_bytes(x, big_endian):
    """[n] int64 holding 48 bits -> [n, 6] uint8"""
    sh = np.arange(6, dtype=np.int64) * 8
    if big_endian:
        sh = sh[::-1]
    return ((x[:, None] >> sh[None, :]) & 0xFF).astype(np.uint8)


def bc4_encode(v):
    v = np.asarray(v, dtype=np.int64)
    mn, mx = v.min(1), v.max(1)
    d = (mx - mn)[:, None]
    q = np.where(d == 0, 7, (14 * (v - mn[:, None]) + d) // np.maximum(2 * d, 1))
    assert ((q >= 0) & (q <= 7)).all()
    code = np.where(q == 7, 0, np.where(q == 0, 1, 8 - q))
    bits = (code << (3 * np.arange(16, dtype=np.int64))).sum(1)
    out = np.zeros((v.shape[0], 8), dtype=np.uint8)
    out[:, 0], out[:, 1] = mx, mn
    out[:, 2:] = _u48_bytes(bits, big_endian=False)
    return out


def r11_targets(v):
    return (2047 * np.asarray(v, dtype=np.int64) + 127) // 255


def _nearest(val, t):
    """val [n, 8] (spec order), t [n, 16] -> j [n, 16] (first minimum = lower j), chosen value [n, 16]"""
    dist = np.abs(val[:, None, :] - t[:, :, None])
    j = dist.argmin(-1)
    return j, np.take_along_axis(val, j, 1)


def r11_search(t):
    """the non-solid rule for every table: mult, base [n, 16 tables], E [n, 16]"""
    mn, mx = t.min(1), t.max(1)
    span = (mx - mn)[:, None]
    mult = np.minimum(15, -(-span // (8 * EAC_RANGE[None, :])))
    base = np.minimum(255, (mn[:, None] + mx[:, None] + 8 * mult) // 16)
    val = np.clip(8 * base[:, :, None] + 4 + 8 * mult[:, :, None] * EAC_MODS[None], 0, 2047)  # [n, k, 8]
    dist = np.abs(val[:, :, None, :] - t[:, None, :, None])  # [n, k, 16, 8]
    j = dist.argmin(-1)
    chosen = np.take_along_axis(val, j.reshape(j.shape[0], 16, 16), 2)
    err = ((chosen - t[:, None, :]) ** 2).sum(-1)
    return mult, base, err


def r11_fields(v):
    """(base, mult, table, selectors j [n, 16] by texel, values [n, 16] the block decodes to, E [n, 16] or None rows of solid blocks)"""
    t = r11_targets(v)
    n = t.shape[0]
    mn, mx = t.min(1), t.max(1)
    solid = mn == mx
    base = np.minimum(mn >> 3, 255)
    mult = np.zeros(n, dtype=np.int64)
    table = np.full(n, 13, dtype=np.int64)
    err = np.zeros((n, 16), dtype=np.int64)
    for c0 in range(0, n, CHUNK):
        sl = slice(c0, min(n, c0 + CHUNK))
        m, b, e = r11_search(t[sl])
        err[sl] = e
        k = e.argmin(1)  # first minimum: the lower k
        ns = ~solid[sl]
        r = np.arange(k.size)
        table[sl] = np.where(ns, k, 13)
        mult[sl] = np.where(ns, m[r, k], 0)
        base[sl] = np.where(ns, b[r, k], base[sl])
    scale = np.where(mult == 0, 1, 8 * mult)
    val = np.clip(8 * base[:, None] + 4 + scale[:, None] * EAC_MODS[table], 0, 2047)
    j, chosen = _nearest(val, t)
    return base, mult, table, j, chosen, err, solid


def r11_encode(v):
    base, mult, table, j, _, _, _ = r11_fields(v)
    bits = (j[:, _ID_TEXEL] << (45 - 3 * np.arange(16, dtype=np.int64))).sum(1)
    out = np.zeros((j.shape[0], 8), dtype=np.uint8)
    out[:, 0] = base
    out[:, 1] = (mult << 4) | table
    out[:, 2:] = _u48_bytes(bits, big_endian=True)
    return out


def encode(name, rgba):
    """the target's blocks [n, bytes] from the RGBA32 decode of the same blocks"""
    enc = bc4_encode if name in ("bc4", "bc5") else r11_encode
    one = enc(channel(rgba, 0))
    if name in ("bc4", "r11"):
        return one
    return np.concatenate([one, enc(channel(rgba, 3))], axis=1)


# ---- spec decoders ----------------------------------------------------------------------------------------------------------
def bc4_decode(blk):
    """BC4 UNORM blocks [n, 8] -> (num [n, 16], den [n]) exact rationals per texel (den 7 in the 8-value mode, 5 in the 6-value mode)"""
    blk = np.asarray(blk, dtype=np.uint8).astype(np.int64)
    r0, r1 = blk[:, 0:1], blk[:, 1:2]
    bits = (blk[:, 2:] << (8 * np.arange(6, dtype=np.int64))).sum(1)
    code = (bits[:, None] >> (3 * np.arange(16, dtype=np.int64))) & 7
    eight = r0 > r1
    num8 = np.where(code == 0, 7 * r0, np.where(code == 1, 7 * r1, (8 - code) * r0 + (code - 1) * r1))
    num6 = np.where(code == 0, 5 * r0, np.where(code == 1, 5 * r1, np.where(code == 6, 0, np.where(code == 7, 5 * 255,
                                                                                                   (6 - code) * r0 + (code - 1) * r1))))
    num = np.where(eight, num8, num6)
    den = np.where(eight[:, 0], 7, 5)
    return num, den


def r11_decode(blk):
    """EAC R11 unsigned blocks [n, 8] -> 11-bit values [n, 16] by texel (i = 4y + x)"""
    blk = np.asarray(blk, dtype=np.uint8).astype(np.int64)
    base, mult, table = blk[:, 0], blk[:, 1] >> 4, blk[:, 1] & 15
    bits = (blk[:, 2:] << (8 * np.arange(5, -1, -1, dtype=np.int64))).sum(1)
    pid = np.arange(16, dtype=np.int64)
    j_by_id = (bits[:, None] >> (45 - 3 * pid)) & 7
    mod = np.take_along_axis(EAC_MODS[table], j_by_id, 1)
    scale = np.where(mult == 0, 1, 8 * mult)
    val_by_id = np.clip(8 * base[:, None] + 4 + scale[:, None] * mod, 0, 2047)
    out = np.zeros_like(val_by_id)
    out[:, _ID_TEXEL] = val_by_id
    return out


def r11_block(base, mult, table, t):
    """the block the rule builds for the given fields (nearest value, lower j on a tie) -- for the table-search check"""
    n = t.shape[0]
    scale = np.where(mult == 0, 1, 8 * mult)
    val = np.clip(8 * base[:, None] + 4 + scale[:, None] * EAC_MODS[table], 0, 2047)
    j, _ = _nearest(val, t)
    bits = (j[:, _ID_TEXEL] << (45 - 3 * np.arange(16, dtype=np.int64))).sum(1)
    out = np.zeros((n, 8), dtype=np.uint8)
    out[:, 0] = base
    out[:, 1] = (mult << 4) | table
    out[:, 2:] = _u48_bytes(bits, big_endian=True)
    return out
