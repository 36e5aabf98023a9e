"""Independent numpy model of the encoder from pixels to UASTC blocks (bu_rgba_encode_uastc): test-only helper.

Written from the rule of section 4.11, not from the kernel.  Nothing here reads the product's tables: dequantised endpoint levels and weights come
from tests/astc_model.py (the ASTC specification's unquantisation rows), the EAC modifiers from tests/channel_model.py, the ETC1 modifiers are the
specification's.  Integer arithmetic only; the widths the device code relies on are asserted.

  input    x[i] = (R, G, B, A) of texel i = 4y + x of the block (tests/encode_cases.to_blocks: the gather of section 4.10)
  class    all 16 texels equal -> mode 8; else every A == 255 -> modes 5, 0, 18 on (R, G, B); else R == G == B everywhere -> mode 15 on (R, A);
           else modes 14, 12, 10 on (R, G, B, A).  The lowest E wins, the earlier mode of the list on a tie.
  fit      for the mode's C channels, endpoint range and weight bits:
           1  S = sum x, dev = 16 x - S, Cov = sum dev dev^T (< 2^29), shifted right until it fits 16 bits; axis v0 = the column of the largest
              diagonal entry (the first on a tie); w = v0, then four times w = norm(Cov w), norm(u) = u >> max(0, bitlen(max |u|) - 12); a zero
              w falls back to v0
           2  p_i = x_i . w; H = the texel of the largest p, L = of the smallest (lowest i on a tie); every channel of both goes to the index of
              the nearest dequantised level of the range (the lower level on a tie).  L is the endpoint of weight 0, H of weight 64
           3  palette entry k, channel c = ((257 lo (64 - W_k) + 257 hi W_k + 32) >> 6) >> 8 with the dequantised lo, hi (the decoder's
              interpolation); texel i takes the entry of the smallest squared distance over the C channels (lowest k on a tie); E = their sum
           4  a_i = 64 - W_k(i), b_i = W_k(i); Saa, Sbb, Sab, Sax, Sbx; det = Saa Sbb - Sab^2; NA = max(0, Sbb Sax - Sab Sbx), NB = max(0, Saa Sbx -
              Sab Sax) per channel; t = max(0, bitlen(largest of the 2C numerators) - 23); with N' = N >> t, det' = det >> t: skipped if det' == 0,
              else value = min(255, (128 N' + det') // (2 det')), quantised as in 2; palette and assignment as in 3; kept only if E' < E
  anchor   weight index of texel 0 >= half the palette: the endpoints swap and every index k becomes max - k
  hints    BC1 hint bits 0.  (flip, diff, inten0, inten1, bias) of the non-solid modes: the lowest tuple of the smallest squared RGB error, against the
           source, of the ETC1 block the transcoder writes for them, decoded; all 32 biases, none in modes 10 and 12 (etc1_search).  etc2tm of modes 15, 14, 12, 10:
           the byte mult << 4 | table, mult 1..15, table 0..15, of the smallest sum over texels of (EAC value the transcoder picks for the DECODED
           alpha - source alpha)^2, the lowest byte on a tie.  Mode 8: (d, i, s, r, g, b) of the smallest squared RGB error of the ETC1 block the
           transcoder writes, decoded; the lowest tuple on a tie
  bytes    mode code, flags, endpoints (trit groups of five as base-3 bytes, then the plain bits), weights without the top bit of texel 0
"""
import numpy as np

import astc_model as am
import channel_model as cm

# mode -> (code, code bits, endpoint range, weight bits, channels of x)
MODES = {5: (0xB, 5, 20, 3, (0, 1, 2)), 0: (0x1, 4, 19, 4, (0, 1, 2)), 18: (0x9, 4, 11, 5, (0, 1, 2)), 15: (0x5, 7, 20, 4, (0, 3)),
         14: (0xD, 5, 20, 2, (0, 1, 2, 3)), 12: (0x6, 3, 19, 3, (0, 1, 2, 3)), 10: (0x2, 3, 13, 4, (0, 1, 2, 3))}
OPAQUE, GREY, ALPHA = (5, 0, 18), (15,), (14, 12, 10)
ETC1_INTEN = np.array([[2, 8], [5, 17], [9, 29], [13, 42], [18, 60], [24, 80], [33, 106], [47, 183]], dtype=np.int64)
ETC1_MODS = np.stack([-ETC1_INTEN[:, 1], -ETC1_INTEN[:, 0], ETC1_INTEN[:, 0], ETC1_INTEN[:, 1]], 1)  # selector 0..3 in rising order


def _levels(r):
    return np.array([am.unquant_colour(r, v) for v in range(am.levels(r))], dtype=np.int64)


def _quant_table(lv):
    """value 0..255 -> index of the nearest level, the lower level on a tie"""
    out = np.zeros(256, dtype=np.int64)
    for v in range(256):
        out[v] = np.lexsort((lv, np.abs(lv - v)))[0]
    return out


LEVELS = {r: _levels(r) for r in (11, 13, 19, 20)}
QUANT = {r: _quant_table(LEVELS[r]) for r in LEVELS}
WEIGHTS = {wb: np.array([am.unquant_weight({2: 2, 3: 5, 4: 8, 5: 11}[wb], k) for k in range(1 << wb)], dtype=np.int64) for wb in (2, 3, 4, 5)}
RANGE_BITS = {11: (5, False), 13: (4, True), 19: (6, True), 20: (8, False)}  # plain bits per value, a trit in front of them


def _bitlen(v):
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros(v.shape, dtype=np.int64)
    for k in range(62):
        out = np.where(v >> k != 0, k + 1, out)
    return out


def _norm12(u):
    sh = np.maximum(0, _bitlen(np.abs(u).max(-1)) - 12)
    return u >> sh[:, None]


def palette(lo, hi, wb):
    """dequantised endpoints [n, C] -> [n, K, C]"""
    W = WEIGHTS[wb][None, :, None]
    return ((257 * lo[:, None, :] * (64 - W) + 257 * hi[:, None, :] * W + 32) >> 6) >> 8


def assign(x, pal):
    d = ((pal[:, None, :, :] - x[:, :, None, :]) ** 2).sum(-1)  # [n, 16, K]
    k = d.argmin(-1)  # (the first minimum)
    return k, d.min(-1).sum(-1)


def fit(x, r, wb):
    """x [n, 16, C] -> (lo index, hi index [n, C], k [n, 16], E [n], kept [n], paths: name -> [n] bool, the PATHS this fit took)"""
    n, _, C = x.shape
    lv, q = LEVELS[r], QUANT[r]
    S = x.sum(1)
    dev = 16 * x - S[:, None, :]
    Cov = np.einsum("nia,nib->nab", dev, dev)
    assert (np.abs(Cov) < (1 << 29)).all()
    sh = np.maximum(0, _bitlen(np.abs(Cov).max((1, 2))) - 16)
    Cs = Cov >> sh[:, None, None]
    assert (np.abs(Cs) <= 65536).all()
    kk = np.argmax(np.stack([Cs[:, c, c] for c in range(C)], -1), -1)
    v0 = _norm12(Cs[np.arange(n), :, kk])
    w = v0
    for _ in range(4):
        cv = np.einsum("nab,nb->na", Cs, w)
        assert (np.abs(cv) < (1 << 31)).all()
        w = _norm12(cv)
    w = np.where((w == 0).all(-1)[:, None], v0, w)
    p = (x * w[:, None, :]).sum(-1)
    rows = np.arange(n)
    H, L = x[rows, np.argmax(p, 1)], x[rows, np.argmin(p, 1)]
    lo, hi = q[L], q[H]
    k, E = assign(x, palette(lv[lo], lv[hi], wb))
    # one least-squares pass
    b = WEIGHTS[wb][k]
    a = 64 - b
    Saa, Sbb, Sab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    Sax, Sbx = (a[:, :, None] * x).sum(1), (b[:, :, None] * x).sum(1)
    det = Saa * Sbb - Sab * Sab
    assert (det >= 0).all() and (det <= (1 << 30)).all()
    rawA, rawB = Sbb[:, None] * Sax - Sab[:, None] * Sbx, Saa[:, None] * Sbx - Sab[:, None] * Sax
    NA, NB = np.maximum(0, rawA), np.maximum(0, rawB)
    assert (NA < (1 << 36)).all() and (NB < (1 << 36)).all()
    t = np.maximum(0, _bitlen(np.maximum(NA, NB).max(-1)) - 23)
    d2 = det >> t
    ok = d2 > 0
    dd = np.where(ok, d2, 1)[:, None]
    ua, ub = (128 * (NA >> t[:, None]) + dd) // (2 * dd), (128 * (NB >> t[:, None]) + dd) // (2 * dd)
    ra, rb = np.minimum(255, ua), np.minimum(255, ub)
    lo2, hi2 = q[ra], q[rb]
    k2, E2 = assign(x, palette(lv[lo2], lv[hi2], wb))
    kept = ok & (E2 < E)
    paths = dict(csh0=sh == 0, ls_skipped=~ok, ls_tie=ok & (E2 == E), ls_neg=((rawA < 0) | (rawB < 0)).any(-1),
                 ls_sat=ok & ((ua > 255) | (ub > 255)).any(-1), eq_endpoints=(lo == hi).all(-1))
    lo, hi = np.where(kept[:, None], lo2, lo), np.where(kept[:, None], hi2, hi)
    k, E = np.where(kept[:, None], k2, k), np.where(kept, E2, E)
    return lo, hi, k, E, kept, paths


# ---- hints ------------------------------------------------------------------------------------------------------------------------------------
def eac_values(mn, mx, tm):
    """the eight values (specification order) of the EAC block the transcoder writes for decoded alphas in mn..mx and the byte tm -> [..., 8], centre"""
    table, mult = tm & 15, tm >> 4
    mods = cm.EAC_MODS[table]
    mm, rng = mods[..., 3], mods[..., 7] - mods[..., 3]
    centre = (2 * (mn * (rng + mm) - mx * mm) + rng) // (2 * rng)
    return np.clip(centre[..., None] + mods * mult[..., None], 0, 255), centre


def eac_decode(a_dec, tm):
    """decoded UASTC alpha [n, 16], etc2tm [n] (mult != 0) -> the alpha of the EAC block the transcoder writes, decoded [n, 16]"""
    mn, mx = a_dec.min(1), a_dec.max(1)
    val, _ = eac_values(mn, mx, tm)  # [n, 8]
    k = np.abs(val[:, None, :] - a_dec[:, :, None]).argmin(-1)  # the first minimum over k = 0..7
    out = np.take_along_axis(val, k, 1)
    return np.where((mn == mx)[:, None], a_dec, out)


def etc2tm_search(a_dec, a_src, chunk=256):
    cand = np.array([m << 4 | t for m in range(1, 16) for t in range(16)], dtype=np.int64)  # rising byte value
    out = np.zeros(a_dec.shape[0], dtype=np.int64)
    for s in range(0, a_dec.shape[0], chunk):
        ad, asrc = a_dec[s:s + chunk], a_src[s:s + chunk]
        n = ad.shape[0]
        err = np.zeros((n, cand.size), dtype=np.int64)
        for j, tm in enumerate(cand):
            err[:, j] = ((eac_decode(ad, np.full(n, tm)) - asrc) ** 2).sum(1)
        out[s:s + chunk] = cand[err.argmin(1)]
    return out


def mode8_etc1_decode(d, i, s, c):
    """the two sub-block values of one channel of the ETC1 block written for mode-8 flags (u8 wrapping of the individual form) -> [..., 2]"""
    byte = np.where(d == 1, c << 3, (c << 4) | c) & 0xFF
    b0 = np.where(d == 1, (byte >> 3) << 3 | (byte >> 3) >> 2, (byte >> 4) * 17)
    b1 = np.where(d == 1, b0, (byte & 15) * 17)  # (differential: the stored delta bits are 0)
    m = ETC1_MODS[i, s]
    return np.stack([np.clip(b0 + m, 0, 255), np.clip(b1 + m, 0, 255)], -1)


def mode8_hints(rgb):
    """rgb [n, 3] -> (d, i, s, r, g, b) [n, 6]: the lowest tuple of the smallest error 8 (v0 - x)^2 + 8 (v1 - x)^2 summed over the channels.  For a
    fixed (d, i, s) the channels are independent, so the lowest tuple takes every channel's lowest best value: that is the brute force over 2^21 tuples."""
    n = rgb.shape[0]
    best = np.full(n, 1 << 62, dtype=np.int64)
    out = np.zeros((n, 6), dtype=np.int64)
    c = np.arange(32)
    for d in range(2):
        for i in range(8):
            for s in range(4):
                v = mode8_etc1_decode(np.int64(d), np.int64(i), np.int64(s), c)  # [32, 2]
                e = 8 * ((v[None, None, :, :] - rgb[:, :, None, None]) ** 2).sum(-1)  # [n, 3, 32]
                cb, tot = e.argmin(-1), e.min(-1).sum(-1)
                better = tot < best
                best = np.where(better, tot, best)
                out = np.where(better[:, None], np.concatenate([np.tile([d, i, s], (n, 1)), cb], 1), out)
    return out


# ---- the ETC1 hints of the non-solid modes -----------------------------------------------------------------------------------------------------
LUM = np.array([108, 366, 38], dtype=np.int64)
_YY, _XX = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")


def etc1_half(f):
    """[4, 4] (y, x): the half a texel lies in -- rows 0-1 / 2-3 when flipped, else columns 0-1 / 2-3"""
    return ((_YY >= 2) if f else (_XX >= 2)).astype(np.int64)


def etc1_bases(dec, f, d, bias):
    """the two base colours, widened to 8 bits, that the transcoder's ETC1 rule derives from the block's decoded texels dec [n, 4, 4, 3] for the scalars
    flip f, diff d and bias (None: the mode has no bias field) -> [n, 2, 3].  The rule as tests/etc_model.py states it."""
    from etc_model import DELTA

    half = etc1_half(f)
    sums = np.stack([(dec * (half == h)[None, :, :, None]).sum((1, 2)) for h in (0, 1)], 1)
    limit = 31 if d else 15
    v = (sums * limit + 1020) // 2040
    if bias is not None:
        delta = DELTA[bias][None]
        at0, atl, moved = v == 0, v == limit, v + delta
        refl = ~at0 & ~atl & ((moved < 0) | (moved > limit))
        v = np.where(at0, np.where(delta == -2, 3, delta + 1), np.where(atl, v + delta - 1, np.where(refl, v - delta, moved)))
        assert ((v >= 0) & (v <= limit)).all()
    c0, c1 = v[:, 0], v[:, 1]
    if d:
        c1 = c0 + np.clip(c1 - c0, -4, 3)
    c = np.stack([c0, c1], 1)
    return (c << 3) | (c >> 2) if d else c * 17


def etc1_texels(dec, f, ext, i0, i1):
    """the decoded ETC1 texels [n, 4, 4, 3]: candidates = clamp(base + modifier), a texel's selector = the number of luma thresholds
    (L_a + L_b) // 2 of its half at or below the luma of its DECODED UASTC texel.  i0, i1: scalars or [n]"""
    n = dec.shape[0]
    half = etc1_half(f).reshape(16)
    mods = np.stack([ETC1_MODS[np.broadcast_to(i0, (n,))], ETC1_MODS[np.broadcast_to(i1, (n,))]], 1)  # [n, 2, 4]
    cand = np.clip(ext[:, :, None, :] + mods[:, :, :, None], 0, 255)  # [n, 2, 4, 3]
    lc = cand @ LUM
    thr = (lc[:, :, :-1] + lc[:, :, 1:]) // 2  # [n, 2, 3]
    lum = dec.reshape(n, 16, 3) @ LUM
    sel = (lum[:, :, None] >= thr[:, half, :]).sum(-1)  # [n, 16]
    return cand[np.arange(n)[:, None], half[None, :], sel].reshape(n, 4, 4, 3)


def etc1_decode(dec, hints, has_bias):
    """dec [n, 4, 4, 3], hints [n, 5] = (flip, diff, inten0, inten1, bias) per block -> the texels of the ETC1 block the transcoder writes, decoded"""
    out = np.zeros_like(dec)
    for key in {tuple(r) for r in np.concatenate([hints[:, [0, 1, 4]], has_bias[:, None].astype(np.int64)], 1).tolist()}:
        f, d, b, hb = key
        m = (hints[:, 0] == f) & (hints[:, 1] == d) & (hints[:, 4] == b) & (has_bias == bool(hb))
        out[m] = etc1_texels(dec[m], f, etc1_bases(dec[m], f, d, b if hb else None), hints[m, 2], hints[m, 3])
    return out


def etc1_search(dec, src, has_bias):
    """dec, src [n, 4, 4, 3], one has_bias for all -> hints [n, 5]: the lowest (flip, diff, inten0, inten1, bias) of the smallest squared error.  For a
    fixed (flip, diff, bias) the two halves are independent, so each half's lowest best table gives the lowest tuple of that base: that is the brute
    force over all 2 * 2 * 8 * 8 * 32 tuples."""
    n = dec.shape[0]
    best, bestkey = np.full(n, 1 << 62, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for f in (0, 1):
        half = etc1_half(f)
        for d in (0, 1):
            for b in (range(32) if has_bias else (0,)):
                ext = etc1_bases(dec, f, d, b if has_bias else None)
                herr = np.zeros((n, 2, 8), dtype=np.int64)
                for t in range(8):
                    e = ((etc1_texels(dec, f, ext, t, t) - src) ** 2).sum(-1)  # [n, 4, 4]
                    for h in (0, 1):
                        herr[:, h, t] = (e * (half == h)[None]).sum((1, 2))
                i0, i1 = herr[:, 0].argmin(1), herr[:, 1].argmin(1)
                tot = herr[:, 0].min(1) + herr[:, 1].min(1)
                key = (f << 12) | (d << 11) | (i0 << 8) | (i1 << 5) | b
                better = (tot < best) | ((tot == best) & (key < bestkey))
                best, bestkey = np.where(better, tot, best), np.where(better, key, bestkey)
    return np.stack([bestkey >> 12, (bestkey >> 11) & 1, (bestkey >> 8) & 7, (bestkey >> 5) & 7, bestkey & 31], 1)


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------------
def _pack(mode, lo, hi, k, etc2tm, etc1):
    code, cbits, r, wb, ch = MODES[mode]
    bits, trit = RANGE_BITS[r]
    K = 1 << wb
    if k[0] >= K // 2:
        lo, hi, k = hi, lo, K - 1 - k
    v, pos = code, cbits
    m1012 = 10 <= mode <= 12
    pos += 1 if m1012 else 2  # BC1 hints: 0
    f, d, i0, i1, b = (int(t) for t in etc1)
    v |= (f | d << 1 | i0 << 2 | i1 << 5) << pos
    pos += 8
    if not m1012:
        v |= b << pos
        pos += 5
    if len(ch) != 3:
        v |= int(etc2tm) << pos
        pos += 8
    idx = [int(t) for pair in zip(lo, hi) for t in pair]  # lo, hi of channel 0, lo, hi of channel 1, ...
    if trit:
        tr = [i >> bits for i in idx]
        for g in range(0, len(tr), 5):
            grp = tr[g:g + 5]
            v |= sum(t * 3 ** j for j, t in enumerate(grp)) << pos
            pos += {5: 8, 4: 7, 3: 5, 2: 4, 1: 2}[len(grp)]
    for i in idx:
        v |= (i & ((1 << bits) - 1)) << pos
        pos += bits
    w = sum(int(kk) << (wb * i) for i, kk in enumerate(k))
    assert not (w >> (wb - 1)) & 1
    w = (w & ((1 << (wb - 1)) - 1)) | (w >> wb << (wb - 1))
    v |= w << pos
    assert pos + 16 * wb - 1 <= 128
    return v


# What encode_fields reports per block beside the bytes, for the fit of the CHOSEN mode where the path is one of the fit's:
PATHS = {
    "csh0": "fit 1: the covariance fits 16 bits as it is, the shift is 0",
    "ls_skipped": "fit 4: det >> t == 0, the least-squares pass is skipped",
    "ls_tie": "fit 4: the pass ran and reached E' == E, so it is not kept",
    "ls_neg": "fit 4: a numerator was negative and clamped at 0",
    "ls_sat": "fit 4: a value above 255 was clamped (the pass ran)",
    "eq_endpoints": "fit 2: L and H quantise to the same level in every channel",
    "anchor_swap": "anchor: texel 0's index is in the upper half, the endpoints swap",
    "mode_tie": "class: a candidate mode later in the list reached the chosen mode's E and lost",
    "alpha_flat": "hints: a non-solid block of modes 15, 14, 12, 10 whose decoded alpha is constant (etc2tm is 0x10 without a search)",
    "hints_zero": "hints: the ETC1 search of a non-solid block ended on (0, 0, 0, 0, 0)",
    "diff": "hints: the chosen ETC1 fields of a non-solid block use the differential form",
}


def encode_fields(rgba):
    """rgba [n, 64] uint8 -> dict: mode [n], E [n] (over the mode's channels), blocks [n, 16] uint8, decode [n, 16, 4] (the UASTC decode the model
    expects), etc2tm [n] (0 where the mode has none), m8 [n, 6], kept [n] (the least-squares pass won in the chosen mode), etc1 [n, 5], and one
    boolean [n] per name of PATHS: what the block took on its way (report only: no byte depends on them; all False in mode 8)"""
    x4 = np.asarray(rgba, dtype=np.uint8).reshape(-1, 16, 4).astype(np.int64)
    n = x4.shape[0]
    solid = (x4 == x4[:, :1]).all((1, 2))
    opaque = ~solid & (x4[:, :, 3] == 255).all(1)
    grey = ~solid & ~opaque & (x4[:, :, 0] == x4[:, :, 1]).all(1) & (x4[:, :, 0] == x4[:, :, 2]).all(1)
    alpha = ~solid & ~opaque & ~grey
    mode = np.full(n, 8, dtype=np.int64)
    E = np.zeros(n, dtype=np.int64)
    kept = np.zeros(n, dtype=bool)
    decode = x4.copy()
    etc2tm = np.zeros(n, dtype=np.int64)
    blocks = np.zeros((n, 16), dtype=np.uint8)
    m8 = np.zeros((n, 6), dtype=np.int64)
    etc1 = np.zeros((n, 5), dtype=np.int64)  # (flip, diff, inten0, inten1, bias) of the non-solid blocks; bias 0 where the mode has none
    paths = {name: np.zeros(n, dtype=bool) for name in PATHS}
    words = [0] * n
    for cls, cands in ((opaque, OPAQUE), (grey, GREY), (alpha, ALPHA)):
        sel = np.nonzero(cls)[0]
        if sel.size == 0:
            continue
        best = None
        for m in cands:
            _, _, r, wb, ch = MODES[m]
            x = x4[sel][:, :, list(ch)]
            lo, hi, k, e, kp, fp = fit(x, r, wb)
            fp["anchor_swap"] = k[:, 0] >= (1 << wb) // 2
            if best is None:
                best = dict(m=np.full(sel.size, m), lo=[None] * sel.size, hi=[None] * sel.size, k=k.copy(), e=e.copy(), kp=kp.copy(),
                            tie=np.zeros(sel.size, dtype=bool), fp={name: v.copy() for name, v in fp.items()})
                win = np.ones(sel.size, dtype=bool)
            else:
                win = e < best["e"]
                best["tie"] = ~win & (best["tie"] | (e == best["e"]))  # (a new winner has no later candidate yet)
                for name, v in fp.items():
                    best["fp"][name] = np.where(win, v, best["fp"][name])
            for j in np.nonzero(win)[0]:
                best["lo"][j], best["hi"][j] = lo[j], hi[j]
            best["m"] = np.where(win, m, best["m"])
            best["e"] = np.where(win, e, best["e"])
            best["kp"] = np.where(win, kp, best["kp"])
            best["k"] = np.where(win[:, None], k, best["k"])
        mode[sel], E[sel], kept[sel] = best["m"], best["e"], best["kp"]
        paths["mode_tie"][sel] = best["tie"]
        for name, v in best["fp"].items():
            paths[name][sel] = v
        for j, g in enumerate(sel):
            m = int(best["m"][j])
            _, _, r, wb, ch = MODES[m]
            lv = LEVELS[r]
            pal = palette(lv[best["lo"][j]][None], lv[best["hi"][j]][None], wb)[0]  # [K, C]
            d = pal[best["k"][j]]  # [16, C]
            if len(ch) == 3:
                decode[g, :, :3] = d
            elif len(ch) == 2:
                decode[g, :, :3], decode[g, :, 3] = d[:, :1], d[:, 1]
            else:
                decode[g] = d
        if cands is not OPAQUE:
            etc2tm[sel] = etc2tm_search(decode[sel][:, :, 3], x4[sel][:, :, 3])
            paths["alpha_flat"][sel] = (decode[sel][:, :, 3] == decode[sel][:, :1, 3]).all(1)
        src3, dec3 = x4[sel][:, :, :3].reshape(-1, 4, 4, 3), decode[sel][:, :, :3].reshape(-1, 4, 4, 3)
        nb = np.isin(best["m"], (10, 12))  # (modes 10 - 12 carry no bias field)
        for grp, hb in ((nb, False), (~nb, True)):
            if grp.any():
                etc1[sel[grp]] = etc1_search(dec3[grp], src3[grp], hb)
        paths["hints_zero"][sel] = (etc1[sel] == 0).all(1)
        paths["diff"][sel] = etc1[sel, 1] == 1
        for j, g in enumerate(sel):
            words[g] = _pack(int(best["m"][j]), best["lo"][j], best["hi"][j], best["k"][j], etc2tm[g], etc1[g])
    sel = np.nonzero(solid)[0]
    if sel.size:
        m8[sel] = mode8_hints(x4[sel, 0, :3])
        for g in sel:
            r, gg, b, a = (int(v) for v in x4[g, 0])
            d, i, s, cr, cg, cb = (int(v) for v in m8[g])
            words[g] = 0x17 | (r | gg << 8 | b << 16 | a << 24) << 5 | d << 37 | i << 38 | s << 41 | cr << 43 | cg << 48 | cb << 53
    for g in range(n):
        blocks[g] = np.frombuffer(int(words[g]).to_bytes(16, "little"), dtype=np.uint8)
    return dict(mode=mode, E=E, blocks=blocks, decode=decode, etc2tm=etc2tm, m8=m8, kept=kept, etc1=etc1, **paths)


def encode(rgba):
    return encode_fields(rgba)["blocks"]
