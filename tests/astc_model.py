"""ASTC 4x4 LDR blocks BUILT from their fields, with the texels those fields mean: a packer written from the Khronos ASTC specification, not a parser.
Nothing here comes from oracle/, from the package or from the product's tables, and no block is ever decoded from its bits to get its expected
texels: build() turns (weight range, dual plane, partitions, seed, endpoint mode, quantised colours, quantised weights, filler) into the 16 block
bytes AND into the 64 texel bytes, each straight from the fields.  The decoders under test and the oracle are both judged by it.

build(fields) -> (block [16] uint8, texels [64] uint8 or None, status)     status: OK / INVALID / UNSUPPORTED below (this module's own numbering)
case_set()    -> the deterministic list of Case the tests share, built once per process (about 6000 blocks, a few seconds)
"""
import functools
import random
from collections import namedtuple

import numpy as np

OK, INVALID, UNSUPPORTED = 0, 1, 2

# ---- integer sequences (specification: "Integer Sequence Encoding") --------------------------------------------------------------------------
# the 21 ranges in rising order of their level count: (bits, trit, quint)
RANGES = [(1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 1), (1, 1, 0), (3, 0, 0), (1, 0, 1), (2, 1, 0), (4, 0, 0), (2, 0, 1), (3, 1, 0), (5, 0, 0), (3, 0, 1),
          (4, 1, 0), (6, 0, 0), (4, 0, 1), (5, 1, 0), (7, 0, 0), (5, 0, 1), (6, 1, 0), (8, 0, 0)]
TRIT_PIECES, QUINT_PIECES = (2, 2, 1, 2, 1), (3, 2, 2)  # m0 T[1:0] m1 T[3:2] m2 T[4] m3 T[6:5] m4 T[7]; m0 Q[2:0] m1 Q[4:3] m2 Q[6:5]


def levels(r):
    b, t, q = RANGES[r]
    return (3 if t else 5 if q else 1) << b


def ise_bits(r, n):
    b, t, q = RANGES[r]
    return n * b + ((8 * n + 4) // 5 if t else 0) + ((7 * n + 2) // 3 if q else 0)


def _f(v, hi, lo):
    return (v >> lo) & ((1 << (hi - lo + 1)) - 1)


def trit_decode(T):
    """the specification's equations: the 8 bits T -> (t0, t1, t2, t3, t4)"""
    if _f(T, 4, 2) == 7:
        C = _f(T, 7, 5) << 2 | _f(T, 1, 0)
        t4 = t3 = 2
    else:
        C = _f(T, 4, 0)
        if _f(T, 6, 5) == 3:
            t4, t3 = 2, _f(T, 7, 7)
        else:
            t4, t3 = _f(T, 7, 7), _f(T, 6, 5)
    if _f(C, 1, 0) == 3:
        t2, t1, t0 = 2, _f(C, 4, 4), _f(C, 3, 3) << 1 | (_f(C, 2, 2) & ~_f(C, 3, 3) & 1)
    elif _f(C, 3, 2) == 3:
        t2, t1, t0 = 2, 2, _f(C, 1, 0)
    else:
        t2, t1, t0 = _f(C, 4, 4), _f(C, 3, 2), _f(C, 1, 1) << 1 | (_f(C, 0, 0) & ~_f(C, 1, 1) & 1)
    return (t0, t1, t2, t3, t4)


def quint_decode(Q):
    """the specification's equations: the 7 bits Q -> (q0, q1, q2)"""
    if _f(Q, 2, 1) == 3 and _f(Q, 6, 5) == 0:
        n0 = ~_f(Q, 0, 0) & 1
        return (4, 4, _f(Q, 0, 0) << 2 | (_f(Q, 4, 4) & n0) << 1 | (_f(Q, 3, 3) & n0))
    if _f(Q, 2, 1) == 3:
        q2, C = 4, _f(Q, 4, 3) << 3 | (~_f(Q, 6, 5) & 3) << 1 | _f(Q, 0, 0)
    else:
        q2, C = _f(Q, 6, 5), _f(Q, 4, 0)
    if _f(C, 2, 0) == 5:
        q1, q0 = 4, _f(C, 4, 3)
    else:
        q1, q0 = _f(C, 4, 3), _f(C, 2, 0)
    return (q0, q1, q2)


def _invert(decode, width):
    pre = {}
    for v in range(1 << width):
        pre.setdefault(decode(v), []).append(v)
    return pre


TRIT_PRE, QUINT_PRE = _invert(trit_decode, 8), _invert(quint_decode, 7)  # digits -> every T / Q that decodes to them


def _group(r):
    b, t, q = RANGES[r]
    return (5, TRIT_PIECES, trit_decode, 8) if t else (3, QUINT_PIECES, quint_decode, 7) if q else (1, (0,), None, 0)


def preimages(r, digits):
    """every T (Q) whose first len(digits) digits are `digits` and whose bits past a last, cut-short group's are zero"""
    size, pieces, decode, width = _group(r)
    kept = sum(pieces[: len(digits)])
    return [v for v in range(1 << kept) if decode(v)[: len(digits)] == tuple(digits)]


def pack_ise(values, r, pre=None, pick=min):
    """values (each below levels(r)) -> (the bit string as an int, bit 0 first; its length).  pre = {group number: the T or Q value to use} (it must
    decode to that group's digits); the other groups take pick(candidates)"""
    b = RANGES[r][0]
    size, pieces, decode, width = _group(r)
    out = pos = 0
    for g in range(0, len(values), size):
        vals = values[g:g + size]
        assert all(0 <= v < levels(r) for v in vals)
        packed = 0
        if decode:
            cands = preimages(r, [v >> b for v in vals])
            packed = pre[g // size] if pre and g // size in pre else pick(cands)
            assert packed in cands
        for i, v in enumerate(vals):
            out |= (v & ((1 << b) - 1)) << pos
            pos += b
            out |= (packed & ((1 << pieces[i]) - 1)) << pos
            pos += pieces[i]
            packed >>= pieces[i]
    assert pos == ise_bits(r, len(values)) and out >> pos == 0
    return out, pos


def unpack_ise(bits, r, n):
    """the n values of a bit string made by pack_ise, read back with the same equations (for the self-checks only)"""
    b = RANGES[r][0]
    size, pieces, decode, width = _group(r)
    values, pos = [], 0
    for g in range(0, n, size):
        k = min(size, n - g)
        m, packed, sh = [], 0, 0
        for i in range(k):
            m.append((bits >> pos) & ((1 << b) - 1))
            pos += b
            packed |= ((bits >> pos) & ((1 << pieces[i]) - 1)) << sh
            pos += pieces[i]
            sh += pieces[i]
        digits = decode(packed) if decode else (0,)
        values += [digits[i] << b | m[i] for i in range(k)]
    return values


# ---- unquantisation (specification: the A / B / C rows of "Endpoint Unquantization" and "Weight Unquantization") -----------------------------
# (trit?, bits) -> (B's bit pattern, most significant first, in the letters of the value's bits b = bit 1, c = bit 2, ...; C)
COLOUR_ROWS = {(1, 1): ("000000000", 204), (1, 2): ("b000b0bb0", 93), (1, 3): ("cb000cbcb", 44), (1, 4): ("dcb000dcb", 22), (1, 5): ("edcb000ed", 11),
               (1, 6): ("fedcb000f", 5), (0, 1): ("000000000", 113), (0, 2): ("b0000bb00", 54), (0, 3): ("cb0000cbc", 26), (0, 4): ("dcb0000dc", 13),
               (0, 5): ("edcb0000e", 6)}
WEIGHT_ROWS = {(1, 1): ("0000000", 50), (1, 2): ("b000b0b", 23), (1, 3): ("cb000cb", 11), (0, 1): ("0000000", 28), (0, 2): ("b0000b0", 13)}


def _replicate(v, b, width):
    s = format(v, "0%db" % b) * (width // b + 1)
    return int(s[:width], 2)


def _abc(v, b, rows, trit, width):
    pattern, C = rows[(trit, b)]
    D, m = v >> b, v & ((1 << b) - 1)
    A = ((1 << width) - 1) if m & 1 else 0
    B = 0
    for ch in pattern:
        B = B << 1 | (0 if ch == "0" else (m >> (ord(ch) - ord("a"))) & 1)
    T = (D * C + B) ^ A
    return (A & (1 << (width - 2))) | (T >> 2)


def unquant_colour(r, v):
    b, t, q = RANGES[r]
    return _abc(v, b, COLOUR_ROWS, t, 9) if t or q else _replicate(v, b, 8)


def unquant_weight(r, v):
    b, t, q = RANGES[r]
    if b == 0:
        w = ((0, 32, 63) if t else (0, 16, 32, 47, 63))[v]
    elif t or q:
        w = _abc(v, b, WEIGHT_ROWS, t, 7)
    else:
        w = _replicate(v, b, 6)
    return w + 1 if w > 32 else w


# ---- header rules --------------------------------------------------------------------------------------------------------------------------
def weight_range(R, hp):
    return (6 if hp else 0) + R - 2  # R 2..7: 2, 3, 4, 5, 6, 8 levels; high precision: 10, 12, 16, 20, 24, 32


def layout(R, hp, dual, parts, cem):
    """-> dict(wr, n_weights, wbits, cpos, n_vals, cr, legal): cr = the largest range whose n_vals values fit the bits between the header and the
    weights (and the plane selector), or -1; legal = the specification's rule for this header"""
    wr, nw = weight_range(R, hp), 32 if dual else 16
    wbits, cpos, n_vals = ise_bits(wr, nw), 17 if parts == 1 else 29, parts * 2 * (cem // 4 + 1)
    avail = 128 - wbits - cpos - (2 if dual else 0)
    fits = [r for r in range(21) if ise_bits(r, n_vals) <= avail]
    cr = max(fits) if fits else -1
    legal = 24 <= wbits <= 96 and not (dual and parts == 4) and n_vals <= 18 and cr >= 4
    return dict(wr=wr, n_weights=nw, wbits=wbits, cpos=cpos, n_vals=n_vals, cr=cr, legal=legal)


HEADERS = [(R, hp, dual, parts, cem) for R in range(2, 8) for hp in (0, 1) for dual in (0, 1) for parts in (1, 2, 3, 4) for cem in (0, 4, 8, 12)]
LEGAL = [h for h in HEADERS if layout(*h)["legal"]]
ILLEGAL = [h for h in HEADERS if not layout(*h)["legal"]]


# ---- partitions (specification: "Partition Pattern Generation") ------------------------------------------------------------------------------
def _hash52(p):
    M = 0xFFFFFFFF
    p ^= p >> 15
    p = (p - (p << 17)) & M
    p = (p + (p << 7)) & M
    p = (p + (p << 4)) & M
    p ^= p >> 5
    p = (p + (p << 16)) & M
    p ^= p >> 7
    p ^= p >> 3
    p = (p ^ (p << 6)) & M
    p ^= p >> 17
    return p


def partition_of(seed, x, y, parts):
    """select_partition for a 4x4 block: fewer than 31 texels, so the coordinates are doubled; z = 0"""
    if parts == 1:
        return 0
    x, y = 2 * x, 2 * y
    seed += (parts - 1) * 1024
    rnum = _hash52(seed)
    s = [(rnum >> (4 * k)) & 15 for k in range(8)]  # seed1..seed8; seed9..seed12 multiply z
    s = [v * v for v in s]
    if seed & 1:
        sh1, sh2 = (4 if seed & 2 else 5), (6 if parts == 3 else 5)
    else:
        sh1, sh2 = (6 if parts == 3 else 5), (4 if seed & 2 else 5)
    s = [v >> (sh2 if k & 1 else sh1) for k, v in enumerate(s)]
    a = (s[0] * x + s[1] * y + (rnum >> 14)) & 63
    b = (s[2] * x + s[3] * y + (rnum >> 10)) & 63
    c = (s[4] * x + s[5] * y + (rnum >> 6)) & 63 if parts >= 3 else 0
    d = (s[6] * x + s[7] * y + (rnum >> 2)) & 63 if parts >= 4 else 0
    if a >= b and a >= c and a >= d:
        return 0
    if b >= c and b >= d:
        return 1
    return 2 if c >= d else 3


# ---- endpoints -------------------------------------------------------------------------------------------------------------------------------
def blue_contracts(cem, v):
    """whether the endpoint pair of unquantised values v swaps and blue-contracts: s1 < s0 (modes 8 and 12 only; a tie does not)"""
    return cem >= 8 and v[1] + v[3] + v[5] < v[0] + v[2] + v[4]


def endpoints(cem, v):
    """unquantised values of one partition -> ((r, g, b, a) of endpoint 0, of endpoint 1)"""
    if cem == 0:
        return (v[0], v[0], v[0], 255), (v[1], v[1], v[1], 255)
    if cem == 4:
        return (v[0], v[0], v[0], v[2]), (v[1], v[1], v[1], v[3])
    a0, a1 = (v[6], v[7]) if cem == 12 else (255, 255)
    if blue_contracts(cem, v):
        return ((v[1] + v[5]) >> 1, (v[3] + v[5]) >> 1, v[5], a1), ((v[0] + v[4]) >> 1, (v[2] + v[4]) >> 1, v[4], a0)
    return (v[0], v[2], v[4], a0), (v[1], v[3], v[5], a1)


# ---- the builder -----------------------------------------------------------------------------------------------------------------------------
def _bytes(blk):
    return np.frombuffer(int(blk).to_bytes(16, "little"), dtype=np.uint8).copy()


def build(f):
    """f["kind"]:
      "block" (default): R, hp, dual, ccs, parts, seed, cem, colours, weights, filler [, colour_pre, weight_pre: {group: T or Q}].  A header the
          rule calls illegal: the header, everything above it = filler, INVALID.
      "void":  hdr (bit 9), bits10_11, s_lo, s_hi, t_lo, t_hi (13 bits each), rgba16 (four 16-bit values)
      "mode":  mode (the 11 block-mode bits), filler (the other 117 bits), status (the class the caller derives from the block-mode table)"""
    kind = f.get("kind", "block")
    if kind == "mode":
        return _bytes(f["mode"] | (f["filler"] & ((1 << 117) - 1)) << 11), None, f["status"]
    if kind == "void":
        blk = 0x1FC | f["hdr"] << 9 | f["bits10_11"] << 10 | f["s_lo"] << 12 | f["s_hi"] << 25 | f["t_lo"] << 38 | f["t_hi"] << 51
        for c, v in enumerate(f["rgba16"]):
            blk |= v << (64 + 16 * c)
        ext = (f["s_lo"], f["s_hi"], f["t_lo"], f["t_hi"])
        if f["hdr"]:
            st = UNSUPPORTED
        elif f["bits10_11"] != 3:
            st = INVALID
        elif ext != (0x1FFF,) * 4 and (f["s_lo"] >= f["s_hi"] or f["t_lo"] >= f["t_hi"]):
            st = INVALID
        else:
            st = OK
        tex = np.array([v >> 8 for v in f["rgba16"]] * 16, dtype=np.uint8) if st == OK else None
        return _bytes(blk), tex, st
    R, hp, dual, parts, cem = f["R"], f["hp"], f["dual"], f["parts"], f["cem"]
    L = layout(R, hp, dual, parts, cem)
    blk = (R >> 1) | (R & 1) << 4 | 2 << 5 | hp << 9 | dual << 10 | (parts - 1) << 11  # the 4 x 4 weight grid: bits 2-3 = 0, A = 2, B = 0
    blk |= cem << 13 if parts == 1 else f["seed"] << 13 | cem << 25  # (the endpoint-mode selector, bits 23-24, is 00)
    if not L["legal"]:
        return _bytes(blk | (f["filler"] & ((1 << (128 - L["cpos"])) - 1)) << L["cpos"]), None, INVALID
    colours, weights = f["colours"], f["weights"]
    assert len(colours) == L["n_vals"] and len(weights) == L["n_weights"]
    cs, cbits = pack_ise(colours, L["cr"], f.get("colour_pre"))
    ws, wbits = pack_ise(weights, L["wr"], f.get("weight_pre"))
    lo, hi = L["cpos"] + cbits, 128 - wbits - (2 if dual else 0)
    assert wbits == L["wbits"] and lo <= hi
    blk |= cs << L["cpos"] | (f["filler"] & ((1 << (hi - lo)) - 1)) << lo
    if dual:
        blk |= f["ccs"] << hi
    for k in range(wbits):
        blk |= ((ws >> k) & 1) << (127 - k)
    # the texels, from the fields
    vpp = L["n_vals"] // parts
    ends = [endpoints(cem, [unquant_colour(L["cr"], c) for c in colours[p * vpp:(p + 1) * vpp]]) for p in range(parts)]
    uw = [unquant_weight(L["wr"], w) for w in weights]
    tex = np.zeros((16, 4), dtype=np.uint8)
    for i in range(16):
        e0, e1 = ends[partition_of(f["seed"], i & 3, i >> 2, parts)]
        for ch in range(4):
            w = uw[2 * i + (1 if ch == f["ccs"] else 0)] if dual else uw[i]
            tex[i, ch] = ((e0[ch] * 257 * (64 - w) + e1[ch] * 257 * w + 32) >> 6) >> 8
    return _bytes(blk), tex.reshape(64), OK


# ---- the case set ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "tag fields block texels status")  # texels: 64 zero bytes where status != OK
PER_HEADER = 8


def _random_fields(rng, h, weights="any", colours="any"):
    R, hp, dual, parts, cem = h
    L = layout(*h)
    nc, nw = levels(L["cr"]) if L["legal"] else 2, levels(L["wr"])
    # "ends": only the two stored values that unquantise to the lowest and to the highest level (0 and 255; 0 and 64)
    cends = [v for v in range(nc) if unquant_colour(L["cr"], v) in (0, 255)] if L["legal"] else [0, 1]
    wends = [v for v in range(nw) if unquant_weight(L["wr"], v) in (0, 64)]
    assert len(cends) == 2 and len(wends) == 2
    draw = lambda n, top, ends, how: [rng.randrange(top) if how == "any" else rng.choice(ends) for _ in range(n)]
    return dict(R=R, hp=hp, dual=dual, parts=parts, cem=cem, ccs=rng.randrange(4), seed=rng.randrange(1024), filler=rng.getrandbits(128),
                colours=draw(L["n_vals"], nc, cends, colours), weights=draw(L["n_weights"], nw, wends, weights))


def _pick_header(want):
    return next(h for h in LEGAL if want(h, layout(*h)))


def _contraction_fields(rng, h, kinds):
    """random fields whose partition p is of kind kinds[p]: "gt" (s1 > s0), "tie" (s1 == s0, distinct endpoints) or "lt" (s1 < s0: contraction)"""
    f = _random_fields(rng, h)
    L, vpp = layout(*h), 2 * (h[4] // 4 + 1)
    for p, kind in enumerate(kinds):
        while True:
            c = [rng.randrange(levels(L["cr"])) for _ in range(vpp)]
            if kind == "tie":
                c[1], c[3], c[5] = c[2], c[4], c[0]  # the same three values in another order
            v = [unquant_colour(L["cr"], x) for x in c]
            s0, s1 = v[0] + v[2] + v[4], v[1] + v[3] + v[5]
            if (kind == "tie" and s0 == s1 and v[0] != v[1]) or (kind == "gt" and s1 > s0) or (kind == "lt" and s1 < s0):
                break
        f["colours"][p * vpp:(p + 1) * vpp] = c
    return f


@functools.lru_cache(maxsize=None)
def case_set():
    cases = []

    def add(tag, f):
        block, tex, st = build(f)
        assert (tex is None) == (st != OK)
        cases.append(Case(tag, f, block, np.zeros(64, dtype=np.uint8) if tex is None else tex, st))

    # every legal header: random fields; block 0 of each with weights 0 / max only, block 1 with colours 0 / max only
    rng = random.Random(0xA57C)
    for h in LEGAL:
        for k in range(PER_HEADER):
            add("legal", _random_fields(rng, h, weights="ends" if k == 0 else "any", colours="ends" if k == 1 else "any"))
    # every T and Q value, non-canonical ones included, in the first full group of the colour stream and of the weight stream
    rng = random.Random(0x7151)
    for stream, trit in (("colours", 1), ("colours", 0), ("weights", 1), ("weights", 0)):
        key = "cr" if stream == "colours" else "wr"
        size = 5 if trit else 3
        h = _pick_header(lambda h, L: RANGES[L[key]][1 if trit else 2] and (L["n_vals"] if stream == "colours" else L["n_weights"]) >= size)
        r = layout(*h)[key]
        for packed in range(256 if trit else 128):
            f = _random_fields(rng, h)
            digits = (trit_decode if trit else quint_decode)(packed)
            for i, d in enumerate(digits):
                f[stream][i] = d << RANGES[r][0] | (f[stream][i] & ((1 << RANGES[r][0]) - 1))
            f[stream[:-1] + "_pre"] = {0: packed}
            add("%s-%s" % ("trit" if trit else "quint", stream), f)
    # every partition map: endpoint mode 0 with e0 == e1, a value of its own per partition; 2-bit weights (R = 4: 32 weight bits; R = 2 alone would
    # be 16, below the legal 24) leave 8-bit colours even for four partitions
    rng = random.Random(0x9A87)
    for parts in (2, 3, 4):
        h = (4, 0, 0, parts, 0)
        assert layout(*h)["legal"] and layout(*h)["cr"] == 20
        for seed in range(1024):
            f = _random_fields(rng, h)
            vals = rng.sample(range(256), parts)
            f["seed"], f["colours"] = seed, [v for v in vals for _ in (0, 1)]
            add("partition", f)
    # blue contraction: every partition of one kind; then one partition contracting beside one that does not
    rng = random.Random(0xB1CE)
    for cem in (8, 12):
        hs = [h for h in LEGAL if h[4] == cem]
        multi = [h for h in hs if h[3] >= 2]
        for kind in ("gt", "tie", "lt"):
            for k in range(50):
                h = hs[rng.randrange(len(hs))]
                add("contract-" + kind, _contraction_fields(rng, h, [kind] * h[3]))
        for k in range(50):
            h = multi[rng.randrange(len(multi))]
            kinds = ["lt", "gt"] if k & 1 else ["gt", "lt"]
            add("contract-mixed", _contraction_fields(rng, h, kinds + [rng.choice(("gt", "tie", "lt")) for _ in range(h[3] - 2)]))
    # dual plane: every selector for every endpoint mode, the selector on a channel the mode holds constant included
    rng = random.Random(0xD0A1)
    for cem in (0, 4, 8, 12):
        hs = [h for h in LEGAL if h[4] == cem and h[2] == 1]
        for ccs in range(4):
            for k in range(4):
                f = _random_fields(rng, hs[rng.randrange(len(hs))])
                f["ccs"] = ccs
                add("dual", f)
    # void extent
    rng = random.Random(0x701D)
    ones = dict(s_lo=0x1FFF, s_hi=0x1FFF, t_lo=0x1FFF, t_hi=0x1FFF)

    def void(**kw):
        f = dict(kind="void", hdr=0, bits10_11=3, rgba16=[rng.getrandbits(16) for _ in range(4)], **ones)
        f.update(kw)
        add("void", f)

    for k in range(4):
        void()
    void(rgba16=[0x00FF, 0xFF00, 0x80FF, 0x7F00])  # the top byte, not a rounding of the 16 bits
    for k in range(8):
        s, t = sorted(rng.sample(range(0x2000), 2)), sorted(rng.sample(range(0x2000), 2))
        void(s_lo=s[0], s_hi=s[1], t_lo=t[0], t_hi=t[1])
    void(s_lo=0, s_hi=1, t_lo=0, t_hi=1)
    void(s_lo=0x1FFE, s_hi=0x1FFF, t_lo=0x1FFE, t_hi=0x1FFF)
    void(s_lo=20, s_hi=10, t_lo=5, t_hi=30)
    void(s_lo=10, s_hi=10, t_lo=5, t_hi=30)
    void(s_lo=5, s_hi=30, t_lo=30, t_hi=5)
    void(s_lo=5, s_hi=30, t_lo=30, t_hi=30)
    void(s_lo=0x1FFF, s_hi=0x1FFF, t_lo=5, t_hi=30)  # all ones on s only: an extent, and s is not ordered
    void(s_lo=0x1FFF, s_hi=0x1FFF, t_lo=0x1FFF, t_hi=0x1FFE)
    for bits in (0, 1, 2):
        void(bits10_11=bits)
    void(hdr=1)
    void(hdr=1, rgba16=[0x3C00] * 4)
    # reserved block modes: bits [1:0] = 00 with bits [8:6] = 111 and not void-extent (60), and bits [3:0] = 0000 (128)
    rng = random.Random(0x4E5E)
    for mode in range(1 << 11):
        if (mode & 0x1FF) != 0x1FC and ((mode & 3) == 0 and ((mode >> 6) & 7) == 7 or (mode & 15) == 0):
            add("reserved-111" if (mode & 3) == 0 and ((mode >> 6) & 7) == 7 else "reserved-0000", dict(kind="mode", mode=mode, filler=rng.getrandbits(117), status=INVALID))
    # the headers that are illegal by construction (in-scope endpoint mode, selector 00: the class does not depend on the order of the checks)
    rng = random.Random(0x111E)
    for h in ILLEGAL:
        add("illegal", _random_fields(rng, h))
    return tuple(cases)


def group_key(c):
    """(weight range, dual, partitions, endpoint mode) of a block case; void-extent and mode cases sort behind them"""
    f = c.fields
    return (weight_range(f["R"], f["hp"]), f["dual"], f["parts"], f["cem"]) if f.get("kind", "block") == "block" else (99, 0, 0, 0)


def arrays(cases=None):
    """-> (blocks [n, 16], texels [n, 64], status [n]) of the case set"""
    cases = case_set() if cases is None else cases
    return np.stack([c.block for c in cases]), np.stack([c.texels for c in cases]), np.array([c.status for c in cases], dtype=np.int64)
