"""Independent numpy model of the colour targets (BC1, BC3) and a spec decoder for BC1.

The encoder is written from the rule of DESIGN.md section 4.5, not from the kernel:
  input   x[i] = (R, G, B) of texel i (i = 4y + x) of the block's RGBA32 decode; A only for BC3
  helpers e5(c) = c << 3 | c >> 2, e6(c) = c << 2 | c >> 4; q5(v) = (31 v + 127) // 255, q6(v) = (63 v + 127) // 255;
          w = r5 << 11 | g6 << 5 | b5
  selectors for expanded endpoints E0, E1: d = E1 - E0, D = d.d, s = (x - E0).d, q = #{j in 1..3 : 6 s > (2j - 1) D};
          error E = sum |3x - ((3 - q) E0 + q E1)|^2
  solid   (all 16 RGB equal): per channel the pair (a, b) of OM5 / OM6 (exhaustive search below); every q = 1
  else    covariance of 16x - S, scaled to 16 bits; axis = column of the largest diagonal, four products with the matrix; the
          texels with the largest / smallest projection, quantised, are c0 / c1; one least-squares pass, kept if it lowers E
  order   w(c0) < w(c1): swap, q -> 3 - q; w(c0) == w(c1): every q = 0; BC1 index of q: 0, 2, 3, 1
  BC1     bytes 0..1 w(c0), 2..3 w(c1) little-endian, 4..7 the indices, texel i at bits 2i
  BC3     BC4 of A (channel_model.bc4_encode) followed by the BC1 block
Every intermediate is asserted to fit the bounds DESIGN.md states, which the device code relies on for 32-bit arithmetic.

The decoder is written from the Khronos Data Format Specification (section "BC1"), again without looking at the encoder: both
modes, colours as exact rationals.
"""
import numpy as np

import channel_model as cm

COLOUR_TARGETS = {"bc1": (11, 8), "bc3": (12, 16)}  # name -> (bu_target, bytes per block)
BITS = np.array([5, 6, 5])
MAXQ = (1 << BITS) - 1
I32 = 1 << 31


def e5(c):
    c = np.asarray(c, dtype=np.int64)
    return (c << 3) | (c >> 2)


def e6(c):
    c = np.asarray(c, dtype=np.int64)
    return (c << 2) | (c >> 4)


def expand(c):
    """[..., 3] 5/6/5-bit endpoints -> 8-bit"""
    return np.stack([e5(c[..., 0]), e6(c[..., 1]), e5(c[..., 2])], -1)


def quant(x):
    """[..., 3] 8-bit values -> 5/6/5 bits, rounded to nearest"""
    x = np.asarray(x, dtype=np.int64)
    return (MAXQ * x + 127) // 255


def word(c):
    return (c[..., 0] << 11) | (c[..., 1] << 5) | c[..., 2]


def _om_table(bits):
    """v -> (a, b): the pair minimising |2 e(a) + e(b) - 3v|, then |a - b|, then a, then b (exhaustive)"""
    n = 1 << bits
    e = e5(np.arange(n)) if bits == 5 else e6(np.arange(n))
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = a.ravel(), b.ravel()
    out = np.zeros((256, 2), dtype=np.int64)
    for v in range(256):
        err = np.abs(2 * e[a] + e[b] - 3 * v)
        k = np.lexsort((b, a, np.abs(a - b), err))[0]
        out[v] = a[k], b[k]
    return out


OM5 = _om_table(5)
OM6 = _om_table(6)


def rgb_of(rgba):
    """rgba [n, 64] -> x [n, 16, 3] int64"""
    return np.asarray(rgba, dtype=np.uint8).reshape(-1, 16, 4)[:, :, :3].astype(np.int64)


def selectors(x, e0, e1):
    """x [n, 16, 3], expanded endpoints e0 / e1 [n, 3] -> q [n, 16], E [n], tie [n] (some 6 s == (2j - 1) D with D > 0)"""
    d = e1 - e0
    D = (d * d).sum(-1)
    s = ((x - e0[:, None, :]) * d[:, None, :]).sum(-1)
    assert (np.abs(6 * s) < I32).all() and (5 * D < I32).all()
    thr = (2 * np.arange(1, 4) - 1)[None, None, :] * D[:, None, None]
    six = 6 * s[:, :, None]
    q = (six > thr).sum(-1)
    tie = ((six == thr) & (D[:, None, None] > 0)).any((1, 2))
    p = (3 - q)[:, :, None] * e0[:, None, :] + q[:, :, None] * e1[:, None, :]
    E = ((3 * x - p) ** 2).sum((1, 2))
    assert (E <= 48 * 765 * 765).all()
    return q, E, tie


def _bitlen(v):
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros(v.shape, dtype=np.int64)
    for k in range(64):
        out = np.where(v >> k != 0, k + 1, out)
    return out


def _norm(u):
    """u [n, 3] -> u >> max(0, bitlen(max |u_c|) - 13), arithmetic shift"""
    sh = np.maximum(0, _bitlen(np.abs(u).max(-1)) - 13)
    return u >> sh[:, None]


def fields(rgba):
    """every step of the rule: dict of c0, c1 (5/6/5 after ordering), q (after ordering), idx (BC1 indices), and per-block classes"""
    x = rgb_of(rgba)
    n = x.shape[0]
    solid = (x == x[:, :1, :]).all((1, 2))
    # ---- solid: the per-channel tables ----
    v = x[:, 0, :]
    sa = np.stack([OM5[v[:, 0], 0], OM6[v[:, 1], 0], OM5[v[:, 2], 0]], -1)
    sb = np.stack([OM5[v[:, 0], 1], OM6[v[:, 1], 1], OM5[v[:, 2], 1]], -1)
    # ---- other blocks ----
    S = x.sum(1)
    dev = 16 * x - S[:, None, :]
    C = np.einsum("nia,nib->nab", dev, dev)
    assert (np.abs(C) < (1 << 28)).all()
    sh = np.maximum(0, _bitlen(np.abs(C).max((1, 2))) - 16)
    Cs = C >> sh[:, None, None]
    k = np.argmax(np.stack([Cs[:, 0, 0], Cs[:, 1, 1], Cs[:, 2, 2]], -1), -1)  # (first maximum on a tie)
    v0 = _norm(Cs[np.arange(n), :, k])
    w = v0
    for _ in range(4):
        cv = np.einsum("nab,nb->na", Cs, w)
        assert (np.abs(cv) < 3 * (1 << 29)).all()
        w = _norm(cv)
    zero = (w == 0).all(-1)
    w = np.where(zero[:, None], v0, w)
    p = (x * w[:, None, :]).sum(-1)
    hi, lo = np.argmax(p, 1), np.argmin(p, 1)  # (lowest i on a tie)
    r = np.arange(n)
    # a tie that the rule decides: another texel of a different colour shares the largest (smallest) projection
    tie_hl = np.zeros(n, dtype=bool)
    for ext, pick in ((p.max(1), hi), (p.min(1), lo)):
        tie_hl |= ((p == ext[:, None]) & (x != x[r, pick][:, None, :]).any(-1)).any(1)
    c0, c1 = quant(x[r, hi]), quant(x[r, lo])
    q, E, tie_sel = selectors(x, expand(c0), expand(c1))
    # one least-squares pass in thirds
    a, b = 3 - q, q
    Saa, Sbb, Sab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    Sax, Sbx = (a[:, :, None] * x).sum(1), (b[:, :, None] * x).sum(1)
    det = Saa * Sbb - Sab * Sab
    assert (det >= 0).all() and (det <= 20736).all()
    pos = det > 0
    dd = np.where(pos, det, 1)[:, None]
    NA = 3 * (Sbb[:, None] * Sax - Sab[:, None] * Sbx)
    NB = 3 * (Saa[:, None] * Sbx - Sab[:, None] * Sax)
    m = MAXQ[None, :]
    assert (np.abs(2 * m * NA) < 670_000_000).all() and (np.abs(2 * m * NB) < 670_000_000).all()
    r0 = np.clip((2 * m * NA + 255 * dd) // (510 * dd), 0, m)
    r1 = np.clip((2 * m * NB + 255 * dd) // (510 * dd), 0, m)
    q2, E2, tie2 = selectors(x, expand(r0), expand(r1))
    kept = pos & (E2 < E)
    c0 = np.where(kept[:, None], r0, c0)
    c1 = np.where(kept[:, None], r1, c1)
    q = np.where(kept[:, None], q2, q)
    tie_sel = np.where(kept, tie2, tie_sel)
    # ---- the solid path's endpoints, then the ordering of both ----
    c0 = np.where(solid[:, None], sa, c0)
    c1 = np.where(solid[:, None], sb, c1)
    q = np.where(solid[:, None], 1, q)
    w0, w1 = word(c0), word(c1)
    swap = w0 < w1
    c0, c1 = np.where(swap[:, None], c1, c0), np.where(swap[:, None], c0, c1)
    q = np.where(swap[:, None], 3 - q, q)
    eq = w0 == w1
    q = np.where(eq[:, None], 0, q)
    idx = np.array([0, 2, 3, 1])[q]
    offdiag = np.stack([C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]], -1)
    ns = ~solid
    return dict(c0=c0, c1=c1, q=q, idx=idx, solid=solid,
                det0=ns & (det == 0), kept=ns & kept, rejected=ns & pos & ~kept, swap=ns & swap, eq=ns & eq,
                tie_hl=ns & tie_hl, tie_sel=ns & tie_sel, sh=ns & (sh > 0), anti=ns & (offdiag < 0).any(-1), zero=ns & zero)


def bc1_from_fields(f):
    n = f["c0"].shape[0]
    out = np.zeros((n, 8), dtype=np.uint8)
    w0, w1 = word(f["c0"]), word(f["c1"])
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = w0 & 0xFF, w0 >> 8, w1 & 0xFF, w1 >> 8
    bits = (f["idx"] << (2 * np.arange(16, dtype=np.int64))).sum(1)
    for k in range(4):
        out[:, 4 + k] = (bits >> (8 * k)) & 0xFF
    return out


def bc1_encode(rgba):
    return bc1_from_fields(fields(rgba))


def encode(name, rgba):
    """the target's blocks [n, bytes] from the RGBA32 decode of the same blocks"""
    one = bc1_encode(rgba)
    if name == "bc1":
        return one
    return np.concatenate([cm.bc4_encode(cm.channel(rgba, 3)), one], axis=1)


# ---- spec decoder -------------------------------------------------------------------------------------------------------------
def bc1_decode(blk):
    """BC1 blocks [n, 8] -> (num [n, 16, 3], den [n], opaque [n, 16]): texel colour = num / den exactly.  color0 > color1 (as 16-bit
    integers): four colours, den 3 (c0, c1, (2 c0 + c1) / 3, (c0 + 2 c1) / 3).  Otherwise three colours and transparent black, den 2
    (c0, c1, (c0 + c1) / 2, black with alpha 0).  RGB565 endpoints widen to 8 bits by bit replication."""
    blk = np.asarray(blk, dtype=np.uint8).astype(np.int64)
    w0 = blk[:, 0] | (blk[:, 1] << 8)
    w1 = blk[:, 2] | (blk[:, 3] << 8)

    def rgb(wd):
        return np.stack([e5(wd >> 11), e6((wd >> 5) & 63), e5(wd & 31)], -1)

    c0, c1 = rgb(w0), rgb(w1)
    bits = blk[:, 4] | (blk[:, 5] << 8) | (blk[:, 6] << 16) | (blk[:, 7] << 24)
    code = (bits[:, None] >> (2 * np.arange(16, dtype=np.int64))) & 3
    four = w0 > w1
    pal4 = np.stack([3 * c0, 3 * c1, 2 * c0 + c1, c0 + 2 * c1], 1)  # [n, 4, 3] in thirds
    pal3 = np.stack([2 * c0, 2 * c1, c0 + c1, 0 * c0], 1)  # in halves
    pal = np.where(four[:, None, None], pal4, pal3)
    num = np.take_along_axis(pal, code[:, :, None], 1)
    den = np.where(four, 3, 2)
    opaque = four[:, None] | (code != 3)
    return num, den, opaque
