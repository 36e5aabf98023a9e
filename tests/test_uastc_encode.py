"""The encoder from pixels to UASTC of DESIGN.md section 4.11 on the CPU: bu_uastc_encode.hpp -- the header the gfx950 kernel includes -- compiled for the
host and compared with the numpy model (tests/uastc_encode_model.py); the model's blocks judged by the oracle and the independent decoders, which know
nothing of the model; the quality gates against the BC1 / BC3 models; the same header in a stand-alone program under AddressSanitizer and UBSan, run as a
child process (nothing built with a sanitizer is loaded into this process); and the argument rules decided before a device is needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import channel_model as cm
import colour_model as col
import encode_cases as ec
import uastc_encode_cases as uc
import uastc_encode_model as um
from basisu_rs_amd import _lib
from oracle.pyoracle import Decoders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
PADS = (0, 4, 64)  # pitch - 4 * width
ALPHA_MODES = (15, 14, 12, 10)


@pytest.fixture(scope="module")
def dec():
    return Decoders()


@pytest.fixture(scope="module")
def emul_uastc(tmp_path_factory):
    """(flat image bytes, w, h, pitch) -> blocks [nby, nbx, 16] through the plain host build of bu_uastc_encode.hpp"""
    so = str(tmp_path_factory.mktemp("emul_uastc_encode") / "libbu_emul_uastc_encode.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", so,
                        os.path.join(HOST_EMUL, "bu_emul_uastc_encode.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.bu_emul_uastc_encode_image.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    lib.bu_emul_uastc_encode_image.restype = ctypes.c_int
    lib.bu_emul_uastc_encode_quant.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.bu_emul_uastc_encode_quant.restype = ctypes.c_int

    def run(buf, w, h, pitch):
        nbx, nby = ec.blocks_of(w, h)
        assert buf.size == ec.image_bytes(w, h, pitch)
        out = np.zeros((nby, nbx, 16), dtype=np.uint8)
        assert lib.bu_emul_uastc_encode_image(buf.ctypes.data, w, h, pitch, out.ctypes.data) == 0
        return out

    run.lib = lib
    return run


EDGE = [("edge", name) for name in uc.EDGE_FAMILIES]  # a case of the edge set: one family of 64 blocks, 64 per row


def _id(case):
    return "edge-%s" % case[1] if case[0] == "edge" else uc.case_id(case)


def _fields(case):
    return uc.edge_fields(case[1]) if case[0] == "edge" else uc.fields(*case)


def _src(case):
    if case[0] == "edge":
        return uc.edge_blocks(case[1]).astype(np.int64)
    return ec.to_blocks(uc.image(*case)).reshape(-1, 16, 4).astype(np.int64)


def _nbx(case):
    return 64 if case[0] == "edge" else ec.blocks_of(case[2], case[3])[0]


def _mode_error(f, decode, src):
    """squared error over the channels of each block's mode: RGB, RGBA, or (R, A) for mode 15; 0 channels differ in mode 8"""
    d2 = (decode - src) ** 2
    rgb, a = d2[:, :, :3].sum((1, 2)), d2[:, :, 3].sum(1)
    m = f["mode"]
    return np.where(np.isin(m, (5, 0, 18)), rgb, np.where(m == 15, d2[:, :, 0].sum(1) + a, rgb + a))


# ---- 1: the host build is the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.CASES, ids=uc.case_id)
def test_host_build_against_the_model(emul_uastc, case):
    """every case, tight and padded pitches; the padding bytes differ from call to call"""
    _, _, w, h = case
    want = uc.expected(*case)
    for pad in PADS:
        pitch = 4 * w + pad
        fill = np.random.default_rng(100 * uc.CASES.index(case) + pad).integers(0, 256, size=ec.image_bytes(w, h, pitch), dtype=np.uint8)
        got = emul_uastc(ec.pitched(uc.image(*case), pitch, fill), w, h, pitch)
        bad = np.argwhere((got != want).any(-1))
        assert bad.size == 0, "%s pad %d: blocks (by, bx) %s differ" % (uc.case_id(case), pad, bad[:5].tolist())


@pytest.mark.parametrize("order", ("sorted", "mixed"))
def test_host_build_against_the_model_on_the_edge_blocks(emul_uastc, order):
    """the edge families as a strip four pixels high, family by family and in the class-mixed order, tight and on a pitch the fast loads cannot take"""
    blocks, want = uc.edge_sorted() if order == "sorted" else uc.edge_mixed()[:2]
    img = uc.strip(blocks)
    w = img.shape[1]
    for pad in (0, 4):
        pitch = 4 * w + pad
        fill = np.random.default_rng(7 + pad).integers(0, 256, size=ec.image_bytes(w, 4, pitch), dtype=np.uint8)
        got = emul_uastc(ec.pitched(img, pitch, fill), w, 4, pitch)[0]
        bad = np.nonzero((got != want).any(-1))[0]
        assert bad.size == 0, "%s pad %d: blocks %s differ" % (order, pad, bad[:5].tolist())


def test_quantiser_tables_built_from_the_decode_table(emul_uastc):
    """value -> nearest level of ranges 11, 13, 19 as the product builds it from BuTables::deq == the model's, built from the ASTC specification's rows"""
    for r in (11, 13, 19):
        q = np.zeros(256, dtype=np.uint8)
        assert emul_uastc.lib.bu_emul_uastc_encode_quant(r, q.ctypes.data) == 0
        assert (q == um.QUANT[r]).all(), r
    assert emul_uastc.lib.bu_emul_uastc_encode_quant(20, None) == -1


# ---- 2, 3, 4: the blocks, judged without the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.CASES + EDGE, ids=_id)
def test_oracle_accepts_every_block_and_finds_the_claimed_error(oracle, dec, case):
    f = _fields(case)
    nbx = _nbx(case)
    st, bad, rgba = oracle.decode_to_rgba(f["blocks"].tobytes(), nbx)
    assert st == 0, (st, bad)
    tex, st = oracle.batch("rgba", f["blocks"])
    assert (st == 0).all()
    tex = tex.reshape(-1, 16, 4).astype(np.int64)
    assert (tex == f["decode"]).all()
    assert (_mode_error(f, tex, _src(case)) == f["E"]).all()
    # the exact round trip through ASTC pins the anchor rule and the trit packing
    astc, st = oracle.batch("astc", f["blocks"])
    assert (st == 0).all()
    back, st = dec.astc(astc)
    assert (st == 0).all() and (back.reshape(-1, 16, 4) == tex).all()
    for target in ("bc7", "etc1", "etc2"):
        st, bad, _ = oracle.transcode(target, f["blocks"].tobytes())
        assert st == 0, (target, st, bad)


# ---- 4b: the class rule, from the pixels and the bytes alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.CASES + EDGE, ids=_id)
def test_class_rule_from_the_pixels_alone(case):
    """16 equal texels -> 8; else every A == 255 -> 5, 0 or 18; else R == G == B -> 15; else 14, 12 or 10.  near_opaque and near_grey are one texel
    away from the next class"""
    src = _src(case)
    bad = uc.class_rule_violations(src, _fields(case)["blocks"])
    assert bad.size == 0, "%s: blocks %s" % (_id(case), bad[:5].tolist())
    if case == ("edge", "near_opaque"):
        assert (uc.block_class(src) == 3).all() and ((src[:, :, 3] != 255).sum(1) == 1).all()
    if case == ("edge", "near_grey"):
        assert (uc.block_class(src) == 3).all() and ((src[:, :, 0] != src[:, :, 1]).sum(1) == 1).all() and (src[:, :, 0] == src[:, :, 2]).all()


# ---- 5: every mode of the rule is reached -------------------------------------------------------------------------------------------------------
def test_every_mode_is_chosen():
    seen = np.concatenate([uc.fields(*c)["mode"] for c in uc.CASES])
    assert set(seen.tolist()) == {8, 5, 0, 18, 15, 14, 12, 10}
    kept = np.concatenate([uc.fields(*c)["kept"] for c in uc.CASES])
    assert kept.any() and (~kept & (seen != 8)).any()  # the least-squares pass both wins and loses


# the family that is there for each path of uastc_encode_model.PATHS
PATH_FAMILY = {"csh0": "tiny", "ls_skipped": "level_tripod", "ls_tie": "tiny_opaque", "ls_neg": "two_level", "ls_sat": "two_level_opaque",
               "eq_endpoints": "level_tripod", "anchor_swap": "anti", "mode_tie": "tiny", "alpha_flat": "one_channel_0", "hints_zero": "dark",
               "diff": "halves"}


def test_every_path_is_taken_and_left_alone():
    """every path the model reports is taken by a block of the family that is there for it, and not taken by some non-solid block of the set"""
    assert set(PATH_FAMILY) == set(um.PATHS)
    fitted = uc.edge_field("mode") != 8
    for path, family in PATH_FAMILY.items():
        hits = {name: int(uc.edge_fields(name)[path].sum()) for name in uc.EDGE_FAMILIES}
        print("%-12s %s" % (path, ", ".join("%s %d" % kv for kv in hits.items() if kv[1])))
        assert hits[family] > 0, "no block of %s takes %s (%s)" % (family, path, um.PATHS[path])
        assert (~uc.edge_field(path) & fitted).any(), "every non-solid block of the edge set takes %s" % path
    assert not (uc.edge_field("ls_skipped") & uc.edge_field("kept")).any()


def test_every_wave_of_the_mixed_strip_holds_all_four_classes():
    """what the GPU tests rely on: class of block i of edge_mixed == i % 4, computed from the pixels; so every aligned run of 64 blocks -- one wave
    of the kernel -- holds solid, opaque, grey-with-alpha and RGBA blocks; and the strip is a reordering that drops no block"""
    blocks, want, order = uc.edge_mixed()
    cls = uc.block_class(blocks)
    assert (cls == np.arange(cls.size) % 4).all()
    for s in range(0, cls.size, 64):
        assert set(cls[s:s + 64].tolist()) == {0, 1, 2, 3}, "the run of 64 blocks at %d holds classes %s" % (s, sorted(set(cls[s:s + 64].tolist())))
    sb, se = uc.edge_sorted()
    assert set(order.tolist()) == set(range(sb.shape[0])) and (blocks == sb[order]).all() and (want == se[order]).all()
    assert (uc.strip(blocks).reshape(4, -1, 4, 4).transpose(1, 0, 2, 3).reshape(-1, 16, 4) == blocks).all()
    assert (ec.to_blocks(uc.strip(blocks)).reshape(-1, 16, 4) == blocks).all()  # the strip's blocks in the kernel's order are the blocks


def test_the_mixed_pattern_mixes_the_classes_in_every_block_row():
    cls = uc.block_class(ec.to_blocks(uc.mixed_pattern())).reshape(16, 16)
    for row in cls:
        assert set(row.tolist()) == {0, 1, 2, 3}
    assert (uc.formula_image(64, 64) != uc.mixed_pattern()).any() and (uc.formula_image(64, 64)[..., [0, 3]] == uc.mixed_pattern()[..., [0, 3]]).all()


# ---- 6: exactness -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in uc.CASES if c[1] in ("solid", "checker")], ids=uc.case_id)
def test_solid_and_two_colour_blocks_are_exact(case):
    f = uc.fields(*case)
    assert (f["E"] == 0).all() and (f["decode"] == _src(case)).all()
    if case[1] == "solid":
        assert (f["mode"] == 8).all()
    elif case[2] * case[3] > 1:  # (a checker of one pixel is a solid block)
        assert (f["mode"] != 8).all()


@pytest.mark.parametrize("name", ("outlier", "solid_extremes", "two_colour"))
def test_blocks_of_at_most_two_colours_are_exact(oracle, name):
    """arbitrary colours, not the checker's: E == 0 and the oracle's decode of the block is the source"""
    f, src = uc.edge_fields(name), uc.edge_blocks(name).astype(np.int64)
    word = src[:, :, 0] | src[:, :, 1] << 8 | src[:, :, 2] << 16 | src[:, :, 3] << 24
    distinct = np.array([np.unique(w).size for w in word])
    assert (distinct <= 2).all() and ((distinct == 1) == (f["mode"] == 8)).all()
    assert (f["E"] == 0).all() and (f["decode"] == src).all()
    tex, st = oracle.batch("rgba", f["blocks"])
    assert (st == 0).all() and (tex.reshape(-1, 16, 4) == src).all()


# ---- 7: quality gates against the parent commit's encoders ---------------------------------------------------------------------------------------
UNIT = 36 * 1225  # errors of the rational decoders below are whole numbers of 1 / UNIT: BC1's denominators are 2 and 3, BC4's 5 and 7


def _bc1_rgb_error(src_blocks):
    """total squared RGB error of colour_model.bc1_encode + bc1_decode, in units of 1 / UNIT"""
    num, den, _ = col.bc1_decode(col.bc1_encode(src_blocks))
    e = ((num - den[:, None, None] * col.rgb_of(src_blocks)) ** 2).sum((1, 2))  # den^2 times the error
    return int((e * (UNIT // (den * den))).sum())


def _bc4_error(a):
    """total squared error of channel_model.bc4_encode + bc4_decode of the channel a [n, 16], in units of 1 / UNIT"""
    num, den = cm.bc4_decode(cm.bc4_encode(a))
    e = ((num - den[:, None] * a) ** 2).sum(1)
    return int((e * (UNIT // (den * den))).sum())


@pytest.mark.parametrize("kind", ("random", "gradient", "checker"))
@pytest.mark.parametrize("shape", ((257, 8), (64, 64)), ids=lambda s: "%dx%d" % s)
def test_opaque_images_beat_bc1(kind, shape):
    case = ("opaque", kind) + shape
    E, bc1 = int(uc.fields(*case)["E"].sum()), _bc1_rgb_error(ec.to_blocks(uc.image(*case)))
    print("%s: UASTC E %d, BC1 %.1f" % (uc.case_id(case), E, bc1 / UNIT))
    assert UNIT * E <= bc1


def test_correlated_alpha_beats_bc3():
    case = ("ag", "gradient", 64, 64)
    src = ec.to_blocks(uc.image(*case))
    E, bc3 = int(uc.fields(*case)["E"].sum()), _bc1_rgb_error(src) + _bc4_error(cm.channel(src, 3))
    print("%s: UASTC E %d, BC3 %.1f" % (uc.case_id(case), E, bc3 / UNIT))
    assert UNIT * E <= bc3


def test_uncorrelated_alpha_is_recorded_not_gated():
    """random alpha against random colour: single-plane modes lose to BC3 here (DESIGN.md section 4.11 records the figure as the cost of leaving the
    dual-plane modes out); printed, not asserted"""
    case = ("plain", "random", 255, 9)
    src = ec.to_blocks(uc.image(*case))
    print("%s: UASTC E %d, BC3 %.1f" % (uc.case_id(case), int(uc.fields(*case)["E"].sum()), (_bc1_rgb_error(src) + _bc4_error(cm.channel(src, 3))) / UNIT))


# ---- 8: hints -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in uc.CASES if c[0] != "opaque"] + [("edge", n) for n in ("one_channel_3", "bright", "dark", "near_opaque")], ids=_id)
def test_etc2tm_and_the_alpha_the_transcoder_writes(oracle, dec, case):
    f = _fields(case)
    has = np.isin(f["mode"], ALPHA_MODES)
    assert ((f["etc2tm"] >> 4) != 0)[has].all() and (f["etc2tm"][~has] == 0).all()
    etc2, st = oracle.batch("etc2", f["blocks"])
    assert (st == 0).all()
    alpha = dec.eac_alpha(etc2).astype(np.int64)
    if has.any():
        assert (alpha[has] == um.eac_decode(f["decode"][has][:, :, 3], f["etc2tm"][has])).all()
        # the search is a search: no other byte does better on the block, the lowest wins a tie (spot check of 32 blocks against the brute force)
        src_a = _src(case)[has][:, :, 3]
        for j in np.linspace(0, has.sum() - 1, min(32, has.sum())).astype(int):
            ad = f["decode"][has][j:j + 1, :, 3]
            errs = [int(((um.eac_decode(ad, np.array([tm])) - src_a[j]) ** 2).sum()) for tm in range(16, 256)]
            assert f["etc2tm"][has][j] == 16 + int(np.argmin(errs))


CODE_SIZE = {5: 5, 0: 4, 18: 4, 15: 7, 14: 5, 12: 3, 10: 3}


def _with_etc1_hints(blocks, modes, hints):
    """copies of UASTC blocks [n, 16] with their ETC1 fields replaced by hints [n, 5] = (flip, diff, inten0, inten1, bias); written from the field
    positions of the format (the flags follow the mode code and the BC1 hint bits: one bit in modes 10 - 12, which have no bias field, else two)"""
    out = np.array(blocks, dtype=np.uint8)
    w = out[:, :8].copy().view("<u8").reshape(-1)
    for j in range(out.shape[0]):
        m = int(modes[j])
        m1012 = m in (10, 12)
        pos, nbits = CODE_SIZE[m] + (1 if m1012 else 2), 8 if m1012 else 13
        f, d, i0, i1, bias = (int(v) for v in hints[j])
        v = f | d << 1 | i0 << 2 | i1 << 5 | (0 if m1012 else bias << 8)
        w[j] = (int(w[j]) & ~(((1 << nbits) - 1) << pos)) | (v << pos)
    out[:, :8] = w.view(np.uint8).reshape(-1, 8)
    return out


def _etc1_rgb(oracle, dec, blocks):
    """the oracle's UASTC -> ETC1 transcode of the blocks, decoded by the independent ETC1 decoder -> [n, 16, 3]"""
    etc1, st = oracle.batch("etc1", blocks)
    assert (st == 0).all()
    return dec.etc1(etc1).reshape(-1, 16, 4)[:, :, :3].astype(np.int64)


@pytest.mark.parametrize("case", [c for c in uc.CASES if c[1] != "solid" and c[2] * c[3] > 1], ids=uc.case_id)
def test_etc1_hints_against_the_all_zero_hints(oracle, dec, case):
    """per block: the ETC1 block the transcoder writes for the chosen hints decodes to what the model predicts, and its squared RGB error against the source
    is at most that of the same block with all-zero hints -- both measured through the oracle's transcode and the independent decoder"""
    f = uc.fields(*case)
    k = f["mode"] != 8
    assert k.any()
    blocks, modes, hints = f["blocks"][k], f["mode"][k], f["etc1"][k]
    src = _src(case)[k][:, :, :3]
    got = _etc1_rgb(oracle, dec, blocks)
    want = um.etc1_decode(f["decode"][k][:, :, :3].reshape(-1, 4, 4, 3), hints, ~np.isin(modes, (10, 12)))
    assert (got == want.reshape(-1, 16, 3)).all()
    assert (blocks == _with_etc1_hints(blocks, modes, hints)).all()  # the fields sit where the format puts them
    zero = _etc1_rgb(oracle, dec, _with_etc1_hints(blocks, modes, np.zeros_like(hints)))
    e_got, e_zero = ((got - src) ** 2).sum((1, 2)), ((zero - src) ** 2).sum((1, 2))
    assert (e_got <= e_zero).all()
    print("%s: ETC1 squared error %d with the chosen hints, %d with all-zero hints" % (uc.case_id(case), e_got.sum(), e_zero.sum()))


def test_etc1_hints_are_the_brute_force(oracle, dec):
    """a few blocks of every non-solid mode: all 2 * 2 * 8 * 8 * 32 tuples (2 * 2 * 8 * 8 where the mode has no bias field), each through the oracle's
    transcode and the independent decoder; the chosen tuple is the first minimum in the order (flip, diff, inten0, inten1, bias).  Nothing of the
    model's factored search is used."""
    picked = {}
    for case in uc.CASES:
        f = uc.fields(*case)
        for j in np.nonzero(f["mode"] != 8)[0]:
            m = int(f["mode"][j])
            if len(picked.setdefault(m, [])) < 2:
                picked[m].append((case, j))
    assert set(picked) == {5, 0, 18, 15, 14, 12, 10}
    # and at the clamps: two blocks each of the families whose base colours or modifiers sit at 0 / 255 or at the differential clamp
    for name in ("dark", "bright_opaque", "two_level_opaque", "two_level", "grey_a_anti", "ramp_sat", "halves"):
        f = uc.edge_fields(name)
        assert (f["mode"][[0, 33]] != 8).all()
        for j in (0, 33):
            picked.setdefault(int(f["mode"][j]), []).append((("edge", name), j))
    assert sum(len(v) for v in picked.values()) == 14 + 14
    for m, blocks in picked.items():
        nb = 1 if m in (10, 12) else 32
        tuples = np.array([(fl, d, i0, i1, b) for fl in range(2) for d in range(2) for i0 in range(8) for i1 in range(8) for b in range(nb)])
        for case, j in blocks:
            f = _fields(case)
            variants = _with_etc1_hints(np.repeat(f["blocks"][j:j + 1], len(tuples), 0), np.full(len(tuples), m), tuples)
            err = ((_etc1_rgb(oracle, dec, variants) - _src(case)[j, :, :3][None]) ** 2).sum((1, 2))
            assert tuple(tuples[int(np.argmin(err))]) == tuple(f["etc1"][j]), (m, _id(case), j)


M8_EXTREMES = (0, 1, 2, 5, 6, 7, 8, 20)  # of solid_extremes, for the brute force: 0, 255, pure red, grey 7, 8, 247, 248, and a mixed colour


@pytest.mark.parametrize("case", [c for c in uc.CASES if c[1] == "solid" or c[3] == 1] + [("edge", "solid_extremes")], ids=_id)
def test_mode8_etc1_fields(oracle, dec, case):
    """the ETC1 block the transcoder writes for the chosen (d, i, s, r, g, b) decodes to what the model expects, and the tuple is the lowest of the best"""
    f = _fields(case)
    m8 = f["mode"] == 8
    assert m8.any()
    etc1, st = oracle.batch("etc1", f["blocks"][m8])
    assert (st == 0).all()
    tex = dec.etc1(etc1).reshape(-1, 16, 4)[:, :, :3].astype(np.int64)
    src = _src(case)[m8][:, :, :3]
    h = f["m8"][m8]
    want = np.stack([um.mode8_etc1_decode(h[:, 0], h[:, 1], h[:, 2], h[:, 3 + c]) for c in range(3)], -1)  # [n, 2 sub-blocks, 3]
    assert (tex.reshape(-1, 4, 4, 3)[:, :, :2] == want[:, None, None, 0]).all() and (tex.reshape(-1, 4, 4, 3)[:, :, 2:] == want[:, None, None, 1]).all()
    err = ((tex - src) ** 2).sum((1, 2))
    # optimality and the tie order, apart from um.mode8_hints: for up to four blocks, every (d, i, s) with every 5-bit value per channel (64 x 32 per
    # channel; the channels are independent for a fixed (d, i, s), so this is the brute force over all tuples), each block built and sent through the
    # oracle's transcode and the independent decoder
    if case[0] == "edge":
        assert m8.all() and [tuple(v) for v in src[[0, 1, 5, 6, 7, 8], 0]] == [(c, c, c) for c in (0, 255, 7, 8, 247, 248)]
    for j in (M8_EXTREMES if case[0] == "edge" else np.unique(np.linspace(0, m8.sum() - 1, 4).astype(int))):
        block = f["blocks"][m8][j]
        word = int.from_bytes(block.tobytes(), "little") & ((1 << 37) - 1)
        variants, dis = [], []
        for d in range(2):
            for i in range(8):
                for sel in range(4):
                    for c in range(32):
                        variants.append(word | d << 37 | i << 38 | sel << 41 | c << 43 | c << 48 | c << 53)
                        dis.append((d, i, sel))
        vb = np.frombuffer(b"".join(v.to_bytes(16, "little") for v in variants), dtype=np.uint8).reshape(-1, 16)
        e = ((_etc1_rgb(oracle, dec, vb) - src[j][None]) ** 2).sum(1).reshape(64, 32, 3)  # [(d, i, s), value, channel]: the value is in all three channels
        tot = e.min(1).sum(1)
        first = int(np.argmin(tot))
        assert tuple(h[j]) == dis[32 * first] + tuple(int(e[first, :, c].argmin()) for c in range(3))
        assert err[j] == tot[first]


# ---- 9: the stand-alone build under the sanitizers -------------------------------------------------------------------------------------------------
def test_stand_alone_build_under_asan_and_ubsan(tmp_path):
    """every block of every shape, gathered from a heap image of exactly (h - 1) * pitch + 4 w bytes (one byte past the last pixel is a heap overflow) and
    encoded under -fsanitize=address,undefined; the checksum of the blocks is the model's"""
    exe = str(tmp_path / "bu_emul_uastc_encode_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                        "-I" + CSRC, "-o", exe, os.path.join(HOST_EMUL, "bu_emul_uastc_encode_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(w, h, pad) for (w, h) in ((1, 1), (5, 3), (255, 9), (12, 203)) for pad in PADS]
    r = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    sums = {}
    for (w, h, pad), line in zip(cases, lines):
        if (w, h) not in sums:
            f = um.encode_fields(ec.to_blocks(uc.formula_image(w, h)))
            sums[(w, h)] = ec.weighted_sum(f["blocks"])
            if w * h > 100:
                assert len(set(f["mode"].tolist())) >= 4  # solid, opaque and alpha tiles are all there
        assert [int(v) for v in line.split()] == [w, h, pad, sums[(w, h)]], (w, h, pad)


# ---- 10: argument rules decided before a device is needed ------------------------------------------------------------------------------------------
# Every refusal below is returned before the context is looked at, so a block of zeroed memory stands in for one; a null context is refused whatever
# else is passed.  The calls that would reach the device (valid arguments and a non-empty image) are the GPU tests'.
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_device_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255

    def call(c=ctypes.addressof(fake), src=p, w=32, h=8, in_pitch=0, dst=p + 4096, out_pitch=0):
        return lib.bu_rgba_encode_uastc_device(c, src, w, h, in_pitch, dst, out_pitch, None)

    rows = [dict(src=None), dict(dst=None), dict(src=p + 2), dict(src=p + 1), dict(dst=p + 4096 + 8), dict(dst=p + 4096 + 4)]
    rows += [dict(in_pitch=4 * 32 - 4), dict(in_pitch=4 * 32 + 2), dict(in_pitch=4), dict(in_pitch=4 * 32 + 2, h=0)]
    rows += [dict(out_pitch=16 * 8 - 16), dict(out_pitch=16 * 8 + 8), dict(out_pitch=16, h=0)]
    rows += [dict(w=(1 << 30) + 1), dict(w=1 << 40), dict(w=(1 << 64) - 1)]  # nbx above 2^28
    A = _lib.ERR_ARGUMENT
    for row in rows:
        assert call(**row) == A, row
        assert call(c=None, **row) == A, row
    assert call(c=None) == A and call(c=None, w=0) == A
    for row in (dict(w=0), dict(h=0), dict(w=0, h=0), dict(w=0, src=None, dst=None), dict(h=0, in_pitch=4 * 32 + 64, out_pitch=16 * 8 + 48)):
        assert call(**row) == _lib.OK, row
    assert call(dst=4096 + 16, src=4, w=0) == _lib.OK  # the smallest alignments
    assert call(w=1 << 30, h=0) == _lib.OK  # nbx = 2^28 is the widest image


def test_host_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    src, dst = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)

    def call(c=ctypes.addressof(fake), data=src, w=32, h=8, in_pitch=0, out=dst, out_bytes=4096):
        return lib.bu_rgba_encode_uastc(c, data, w, h, in_pitch, out, out_bytes)

    A = _lib.ERR_ARGUMENT
    for row in (dict(data=None), dict(out=None), dict(in_pitch=4 * 32 - 4), dict(in_pitch=4 * 32 + 2), dict(w=(1 << 30) + 1)):
        assert call(**row) == A, row
        assert call(c=None, **row) == A, row
    assert call(c=None) == A
    assert call(out_bytes=16 * 8 * 2 - 1) == _lib.ERR_OUTPUT_SIZE and call(w=5, h=5, out_bytes=63) == _lib.ERR_OUTPUT_SIZE
    assert call(w=0) == _lib.OK and call(h=0, data=None, out=None, out_bytes=0) == _lib.OK


def test_the_block_formats_encoder_still_refuses_what_has_no_rule(lib):
    """ASTC, BC7, ETC1 and ETC2 come by bu_uastc_transcode of this encoder's blocks, not from bu_rgba_encode_blocks"""
    fake = ctypes.create_string_buffer(1 << 16)
    for t in (0, 1, 2, 3):
        assert lib.bu_rgba_encode_blocks_device(ctypes.addressof(fake), t, None, 0, 0, 0, None, 0, None) == _lib.ERR_ARGUMENT


def test_binding_rust_facade_and_header_spell_the_two_calls_alike():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basisu_hip.h")).read(), flags=re.S)
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name, n_params in (("bu_rgba_encode_uastc_device", 8), ("bu_rgba_encode_uastc", 7)):
        m = re.search(r"bu_status\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n_params
        assert name in _lib.SYMBOLS
        m = re.search(r"fn %s\s*\((.*?)\)\s*->\s*c_int;" % name, rs, flags=re.S)
        assert m and m.group(1).count(":") == n_params and ("ffi::%s(" % name) in lib_rs
    assert re.search(r"pub fn encode_uastc\(", lib_rs) and re.search(r"pub unsafe fn encode_uastc_device\(", lib_rs)
