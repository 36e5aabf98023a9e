"""An independent truth under the ASTC and BC7 decoders of DESIGN.md section 4.9, on the CPU.

ASTC: tests/astc_model.py BUILDS blocks from their fields and derives the texels from the same fields, so neither oracle/bu_decoders.c nor
bu_decode_blocks.hpp is judged by a sibling written from the same reading of the specification: each is compared with the model, byte for byte.
BC7 (and the colour / channel order of BC1, BC3, BC4, BC5): Pillow's DDS reader, recorded in tests/golden/bc7_third_party.bin (always on) and live
where Pillow is installed.  The product's block code runs as the stand-alone ASan + UBSan program of tests/decode_cases.py; nothing built with a
sanitizer is loaded into this process."""
import collections
import os

import numpy as np
import pytest

import astc_model as am
import decode_cases as dc
from oracle.pyoracle import Decoders

CLASS = np.array([dc.OK, dc.INVALID, dc.UNSUPPORTED])  # astc_model's OK, INVALID, UNSUPPORTED
FIXTURE = os.path.join(dc.ROOT, "tests", "golden", "bc7_third_party.bin")


@pytest.fixture(scope="module")
def dec():
    return Decoders()


@pytest.fixture(scope="module")
def emul_decode(tmp_path_factory):
    return dc.emul_decoder(tmp_path_factory)


def load_bc7_fixture():
    rec = np.fromfile(FIXTURE, dtype=np.uint8).reshape(1024, 80)
    return np.ascontiguousarray(rec[:, :16]), np.ascontiguousarray(rec[:, 16:])


# ---- the model checks itself -------------------------------------------------------------------------------------------------------------------
def test_model_trit_and_quint_maps_cover_every_tuple():
    assert len(am.TRIT_PRE) == 243 and set(am.TRIT_PRE) == {(a, b, c, d, e) for a in range(3) for b in range(3) for c in range(3) for d in range(3) for e in range(3)}
    assert len(am.QUINT_PRE) == 125 and set(am.QUINT_PRE) == {(a, b, c) for a in range(5) for b in range(5) for c in range(5)}
    assert sum(len(v) for v in am.TRIT_PRE.values()) == 256 and sum(len(v) for v in am.QUINT_PRE.values()) == 128


def test_model_weight_unquantisation_is_symmetric():
    for wr in range(12):
        top = am.levels(wr) - 1
        uq = [am.unquant_weight(wr, q) for q in range(top + 1)]
        # unquant(max - q) == 64 - unquant(q), q counting the levels in rising order of their weight: a range with a trit or quint AND bits
        # stores its levels in another order (its lowest bit mirrors the level, so there the partner of the stored value v is v ^ 1)
        rising = sorted(uq)
        assert rising[0] == 0 and rising[top] == 64 and len(set(uq)) == top + 1
        assert all(rising[top - q] == 64 - rising[q] for q in range(top + 1)), wr
        bits, trit, quint = am.RANGES[wr]
        mixed = bits and (trit or quint)
        assert all(am.unquant_weight(wr, q ^ 1 if mixed else top - q) == 64 - uq[q] for q in range(top + 1)), wr
    for cr in range(4, 21):
        top = am.levels(cr) - 1
        uq = [am.unquant_colour(cr, q) for q in range(top + 1)]
        assert min(uq) == 0 and max(uq) == 255 and len(set(uq)) == top + 1, cr


def test_model_sequences_read_back():
    """packing then reading a sequence with the model's own equations returns the values: every range, lengths that cut the last group short,
    canonical and arbitrary preimages"""
    import random

    rng = random.Random(5)
    for r in range(21):
        for n in (1, 2, 3, 4, 5, 6, 7, 8, 16, 18, 32):
            for pick in (min, max, rng.choice):
                vals = [rng.randrange(am.levels(r)) for _ in range(n)]
                bits, nbits = am.pack_ise(vals, r, pick=pick)
                assert nbits == am.ise_bits(r, n) and am.unpack_ise(bits, r, n) == vals


# ---- the case set is what the issue asks for: every count from the fields ---------------------------------------------------------------------
def _header(c):
    f = c.fields
    return (f["R"], f["hp"], f["dual"], f["parts"], f["cem"])


def test_case_set_counts():
    cases = am.case_set()
    by = collections.defaultdict(list)
    for c in cases:
        by[c.tag].append(c)
    assert len(am.HEADERS) == 384 and len(am.LEGAL) == 163 and len(am.ILLEGAL) == 221
    # every legal header at least 8 times; weights / colours at the ends of their ranges among them; every colour and weight range
    per = collections.Counter(_header(c) for c in by["legal"])
    assert set(per) == set(am.LEGAL) and min(per.values()) >= 8 and all(c.status == am.OK for c in by["legal"])
    lay = [am.layout(*_header(c)) for c in by["legal"]]
    assert {L["cr"] for L in lay} == set(range(4, 21)) and {L["wr"] for L in lay} == set(range(12))
    assert sum({am.unquant_weight(L["wr"], w) for w in c.fields["weights"]} <= {0, 64} for c, L in zip(by["legal"], lay)) >= 163
    assert sum({am.unquant_colour(L["cr"], v) for v in c.fields["colours"]} <= {0, 255} for c, L in zip(by["legal"], lay)) >= 163
    # every T and Q value in the first full group of both streams
    for tag, key, n in (("trit-colours", "colour_pre", 256), ("trit-weights", "weight_pre", 256), ("quint-colours", "colour_pre", 128), ("quint-weights", "weight_pre", 128)):
        assert sorted(c.fields[key][0] for c in by[tag]) == list(range(n)) and all(c.status == am.OK for c in by[tag])
        L = am.layout(*_header(by[tag][0]))
        rng_ = am.RANGES[L["cr" if "colour" in key else "wr"]]
        assert rng_[1 if tag.startswith("trit") else 2] == 1 and (L["n_vals"] if "colour" in key else L["n_weights"]) >= (5 if tag.startswith("trit") else 3)
    # every partition map, each texel showing its partition whatever the weights
    assert sorted((c.fields["parts"], c.fields["seed"]) for c in by["partition"]) == [(p, s) for p in (2, 3, 4) for s in range(1024)]
    for c in by["partition"]:
        f = c.fields
        col = f["colours"]
        assert f["cem"] == 0 and am.layout(*_header(c))["cr"] == 20 and col[0::2] == col[1::2] and len(set(col[0::2])) == f["parts"]
        want = [col[2 * am.partition_of(f["seed"], i & 3, i >> 2, f["parts"])] for i in range(16)]
        assert c.texels.reshape(16, 4)[:, 0].tolist() == want and (c.texels.reshape(16, 4)[:, 3] == 255).all()
    # blue contraction, by the unquantised sums of the fields
    def kinds(c):
        L, f = am.layout(*_header(c)), c.fields
        vpp = L["n_vals"] // f["parts"]
        out = []
        for p in range(f["parts"]):
            v = [am.unquant_colour(L["cr"], x) for x in f["colours"][p * vpp:(p + 1) * vpp]]
            s0, s1 = v[0] + v[2] + v[4], v[1] + v[3] + v[5]
            out.append("gt" if s1 > s0 else "tie" if s1 == s0 else "lt")
        return out
    for cem in (8, 12):
        for kind in ("gt", "tie", "lt"):
            mine = [c for c in by["contract-" + kind] if c.fields["cem"] == cem]
            assert len(mine) >= 50 and all(set(kinds(c)) == {kind} for c in mine)
        mixed = [c for c in by["contract-mixed"] if c.fields["cem"] == cem]
        assert len(mixed) >= 50 and all("lt" in kinds(c) and "gt" in kinds(c) for c in mixed)
        assert {kinds(c)[0] for c in mixed} == {"lt", "gt"}  # the contracting partition comes first in some, second in others
    # dual plane: every selector for every endpoint mode
    assert {(c.fields["cem"], c.fields["ccs"]) for c in by["dual"]} == {(m, s) for m in (0, 4, 8, 12) for s in range(4)} and all(c.fields["dual"] for c in by["dual"])
    # void extent
    v = collections.Counter()
    for c in by["void"]:
        f = c.fields
        ones = (f["s_lo"], f["s_hi"], f["t_lo"], f["t_hi"]) == (0x1FFF,) * 4
        what = ("hdr" if f["hdr"] else "bits" if f["bits10_11"] != 3 else "ones" if ones else "s>" if f["s_lo"] > f["s_hi"] else "s=" if f["s_lo"] == f["s_hi"]
                else "t>" if f["t_lo"] > f["t_hi"] else "t=" if f["t_lo"] == f["t_hi"] else "ordered")
        v[what] += 1
        assert c.status == {"hdr": am.UNSUPPORTED, "ones": am.OK, "ordered": am.OK}.get(what, am.INVALID)
        if c.status == am.OK:
            assert c.texels.reshape(16, 4).tolist() == [[x >> 8 for x in f["rgba16"]]] * 16
    assert set(v) == {"hdr", "bits", "ones", "ordered", "s>", "s=", "t>", "t="} and v["bits"] == 3 and v["ordered"] >= 8
    # reserved block modes and illegal headers
    assert len(by["reserved-111"]) == 60 and all((c.fields["mode"] & 3) == 0 and ((c.fields["mode"] >> 6) & 7) == 7 and (c.fields["mode"] & 0x1FF) != 0x1FC for c in by["reserved-111"])
    zeros = [c.fields["mode"] for c in by["reserved-111"] + by["reserved-0000"] if (c.fields["mode"] & 15) == 0]
    assert sorted(zeros) == [m for m in range(1 << 11) if (m & 15) == 0] and len(zeros) == 128
    assert sorted(_header(c) for c in by["illegal"]) == sorted(am.ILLEGAL)
    assert all(c.status == am.INVALID and not c.texels.any() for t in ("reserved-111", "reserved-0000", "illegal") for c in by[t])
    assert 5000 <= len(cases) <= 7000


# ---- both decoders against the model -----------------------------------------------------------------------------------------------------------
def _against_model(got, got_st, who):
    cases = am.case_set()
    blocks, texels, status = am.arrays()
    want_st = CLASS[status]
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, "%s: status differs at %d cases, e.g. %s" % (who, bad.size, [(cases[i].tag, int(got_st[i]), int(want_st[i]), cases[i].fields) for i in bad[:3]])
    bad = np.flatnonzero((got != texels).any(axis=1))
    assert bad.size == 0, "%s: texels differ at %d cases %s, e.g. %s: %s against %s" % (
        who, bad.size, collections.Counter(cases[i].tag for i in bad), cases[bad[0]].fields, got[bad[0]].tolist(), texels[bad[0]].tolist())
    assert not got[want_st != dc.OK].any(), "a failing block is written as zeros"


def test_astc_product_block_code_against_the_model(emul_decode):
    got, st = emul_decode("astc", am.arrays()[0])
    _against_model(got, st, "bu_decode_blocks.hpp")


def test_astc_oracle_against_the_model(dec):
    blocks = am.arrays()[0]
    px, ost = dec.astc(blocks)
    st = dc.ORACLE_CLASS[ost]
    _against_model(np.where((st == dc.OK)[:, None], px.reshape(-1, 64), 0), st, "oracle/bu_decoders.c")
    assert not px.reshape(-1, 64)[st != dc.OK].any()


# ---- BC7 and the BC1 / BC3 / BC4 / BC5 orders against a third party ------------------------------------------------------------------------------
def test_bc7_fixture_is_stratified():
    blocks, _ = load_bc7_fixture()
    v = [int.from_bytes(b.tobytes(), "little") for b in blocks]
    for mode in range(8):
        mine = v[128 * mode:128 * (mode + 1)]
        assert all(x & ((1 << (mode + 1)) - 1) == 1 << mode for x in mine)
        nb = {0: 4, 1: 6, 2: 6, 3: 6, 4: 3, 5: 2, 6: 0, 7: 6}[mode]  # partition bits; mode 4: rotation and index selector; mode 5: rotation
        per = collections.Counter((x >> (mode + 1)) & ((1 << nb) - 1) for x in mine)
        assert len(per) == 1 << nb and set(per.values()) == {128 >> nb}


def test_bc7_third_party_fixture(emul_decode, dec):
    """always on: the recorded Pillow texels of 1024 valid blocks, 128 per mode"""
    blocks, want = load_bc7_fixture()
    got, st = emul_decode("bc7", blocks)
    assert (st == 0).all() and np.array_equal(got, want)
    px, ost = dec.bc7(blocks)
    assert (ost == 0).all() and np.array_equal(px.reshape(-1, 64), want)


def test_bc7_random_blocks_against_pillow(emul_decode, dec):
    """the 200 000 random blocks of test_random_blocks: on every block the oracle calls valid, Pillow, the oracle and the product's block code agree"""
    pytest.importorskip("PIL")
    import pillow_blocks

    blocks = dc.random_blocks("bc7", 200_000, seed=100 + dc.FORMATS["bc7"])
    px, ost = dec.bc7(blocks)
    ok = ost == 0
    assert ok.sum() >= 199_000
    third = pillow_blocks.decode("bc7", blocks[ok]).reshape(-1, 64)
    got, st = emul_decode("bc7", blocks)
    assert ((st == 0) == ok).all()
    assert np.array_equal(px.reshape(-1, 64)[ok], third) and np.array_equal(got[ok], third)


@pytest.mark.parametrize("fmt", ["bc1", "bc3", "bc4", "bc5"])
def test_bc_random_blocks_within_one_of_pillow(emul_decode, fmt):
    """index order, endpoint order and the three-colour form against an outsider.  The bound of 1 is Pillow's truncation of num / den against section
    4.9's round half up: the two differ by less than 1, so the bytes by at most 1.  BC1's alpha (0 or 255, no division) is identical."""
    pytest.importorskip("PIL")
    import pillow_blocks

    blocks = dc.random_blocks(fmt, 32_000, seed=300 + dc.FORMATS[fmt])
    third = pillow_blocks.decode(fmt, blocks).astype(np.int64)
    got, st = emul_decode(fmt, blocks)
    assert (st == 0).all()
    got = got.reshape(-1, 16, 4).astype(np.int64)
    channels = {"bc1": (0, 1, 2, 3), "bc3": (0, 1, 2, 3), "bc4": (0,), "bc5": (0, 1)}[fmt]  # the channels the format carries
    for ch in channels:
        worst = int(np.abs(got[:, :, ch] - third[:, :, ch]).max())
        print("%s channel %d: largest difference from Pillow %d" % (fmt, ch, worst))
        assert worst <= 1, (fmt, ch, worst)
    if fmt == "bc1":
        assert np.array_equal(got[:, :, 3], third[:, :, 3]) and (got[:, :, 3] == 0).any()
