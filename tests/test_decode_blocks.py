"""The block decoders of DESIGN.md section 4.9 on the CPU: bu_decode_blocks.hpp -- the header the gfx950 decode kernels include -- compiled for the host
into a stand-alone program (tests/host_emul/bu_emul_decode_main.cpp) under AddressSanitizer and UBSan, run as a child process, and compared byte for
byte, statuses included, with the suite's witnesses (tests/decode_cases.py: oracle/bu_decoders.c and the numpy spec decoders).  Nothing built with a
sanitizer is loaded into this process.  Then the argument rules of the two entry points that are decided before a device is needed."""
import ctypes
import os

import numpy as np
import pytest

import decode_cases as dc
from basisu_rs_amd import _lib
from oracle.pyoracle import Decoders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAND = 200_000


@pytest.fixture(scope="module")
def dec():
    return Decoders()


@pytest.fixture(scope="module")
def emul_decode(tmp_path_factory):
    return dc.emul_decoder(tmp_path_factory)


def _compare(emul_decode, dec, fmt, blocks, what):
    want, want_st = dc.expected(dec, fmt, blocks)
    got, got_st = emul_decode(fmt, blocks)
    bad = np.flatnonzero(got_st != want_st)
    assert bad.size == 0, "%s %s: status differs at blocks %s: got %s, want %s" % (fmt, what, bad[:5], got_st[bad[:5]], want_st[bad[:5]])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s %s: texels differ at blocks %s, e.g. block bytes %s" % (fmt, what, bad[:5], blocks[bad[0]].tolist())
    assert not got[want_st != 0].any(), "a failing block is written as zeros"
    return want, want_st


@pytest.fixture(scope="module")
def encoded(oracle, golden):
    return dc.encoder_outputs(oracle, golden["uastc"])


@pytest.mark.parametrize("fmt", list(dc.FORMATS))
def test_encoder_outputs_of_the_golden_blocks(emul_decode, dec, encoded, golden, fmt):
    """what the library's encoders make of the 608 golden UASTC blocks (on the CPU: oracle and numpy models) decodes as the witnesses say;
    ASTC decodes to the golden RGBA32 vectors exactly (UASTC is an ASTC subset)"""
    blocks, rgba = encoded
    assert blocks[fmt].shape[0] == 608
    want, st = _compare(emul_decode, dec, fmt, blocks[fmt], "golden")
    assert (st == 0).all()
    if fmt == "astc":
        assert (rgba == golden["rgba"]).all()
        assert (emul_decode("astc", golden["astc"])[0] == golden["rgba"]).all()


@pytest.mark.parametrize("fmt", list(dc.FORMATS))
def test_random_blocks(emul_decode, dec, fmt):
    """200 000 random blocks per format, class for class; BC7 reaches every mode and the reserved byte, ETC every overflow class"""
    blocks = dc.random_blocks(fmt, N_RAND, seed=100 + dc.FORMATS[fmt])
    want, st = _compare(emul_decode, dec, fmt, blocks, "random")
    if fmt == "bc7":
        b0 = blocks[:, 0].astype(np.int64)
        mode = np.where(b0 == 0, 8, np.log2(np.maximum(b0 & -b0, 1)).astype(np.int64))
        counts = np.bincount(mode, minlength=9)
        assert (counts >= 300).all(), counts  # modes 0..7 and the reserved byte 0
        assert ((st != 0) == (mode == 8)).all() and (st[mode == 8] == dc.INVALID).all()
    elif fmt in ("etc1", "etc2"):
        modes = dec.etc1_fields(blocks[:, -8:])["mode"]
        counts = np.bincount(modes, minlength=5)
        assert (counts[2:] >= 3000).all(), counts  # T, H, planar
        assert (st[modes >= 2] == dc.UNSUPPORTED).all() and (st[modes < 2] == 0).all()
    elif fmt == "astc":
        assert (st == dc.OK).sum() >= 100 and (st == dc.UNSUPPORTED).sum() >= 1000 and (st == dc.INVALID).sum() >= 1000
    else:
        assert (st == 0).all()  # no invalid encodings


def test_astc_blocks_shaped_onto_the_4x4_grid(emul_decode, dec):
    """random blocks whose block mode is forced onto a 4x4 weight grid: every partition count, dual plane and all four endpoint modes, counted on the
    ORACLE's classification; a block the oracle calls unsupported or illegal must come back as zeros with that class"""
    blocks = dc.shaped_astc(N_RAND, seed=4)
    _, ost = dec.astc(blocks)
    ok = ost == 0
    assert ok.sum() >= 15000 and (ost == 2).sum() >= 1000 and (ost == 3).sum() >= 1000, np.bincount(ost, minlength=4)
    parts, dual, cem = dc.astc_groups(blocks[ok])
    groups = [(parts == p).sum() for p in (1, 2, 3, 4)] + [(dual == 1).sum()] + [(cem == m).sum() for m in (0, 4, 8, 12)]
    assert min(groups) >= 1000, groups
    _compare(emul_decode, dec, "astc", blocks, "shaped")


def test_edge_blocks(emul_decode, dec):
    edges = dc.edge_blocks()
    assert set(edges) == set(dc.FORMATS)
    st = {}
    for fmt, blocks in edges.items():
        st[fmt] = _compare(emul_decode, dec, fmt, blocks, "edge")[1]
    # the cases are what they claim to be
    b = edges["bc1"].astype(int)
    w0, w1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    assert (w0 == w1).any() and (w0 < w1).any() and (w0 > w1).any()
    got = emul_decode("bc1", edges["bc1"])[0].reshape(-1, 16, 4)
    assert (got[w0 <= w1][:, :, 3] == 0).any() and (got[w0 > w1][:, :, 3] == 255).all()  # code 3 of the three-colour form
    r = edges["bc4"].astype(int)
    assert (r[:, 0] == r[:, 1]).any() and (r[:, 0] < r[:, 1]).any()
    g4 = emul_decode("bc4", edges["bc4"])[0].reshape(-1, 16, 4)[:, :, 0]
    assert (g4[r[:, 0] <= r[:, 1]][:, 6] == 0).all() and (g4[r[:, 0] <= r[:, 1]][:, 7] == 255).all()  # codes 6 and 7 of the 6-value ramp
    e = edges["r11"].astype(int)
    assert ((e[:, 1] >> 4) == 0).any()
    g11 = emul_decode("r11", edges["r11"])[0].reshape(-1, 16, 4)[:, :, 0]
    assert (g11 == 0).any() and (g11 == 255).any()  # clamped at both ends
    assert list(st["etc1"][:36:6]) == [0, 0, 0, 0, 0, 0] and (st["etc1"][36:] == dc.UNSUPPORTED).all()  # second base colour 0 / 31 decode; -1 / 32 do not
    assert list(st["astc"][:5]) == [0, 0, dc.UNSUPPORTED, dc.INVALID, dc.INVALID]
    assert list(st["astc"][5:]) == [0, dc.INVALID, dc.INVALID]  # an ordered extent, an ill-ordered one, a reserved block mode
    got = emul_decode("astc", edges["astc"])[0]
    assert got[5].reshape(16, 4).tolist() == [[0x12, 0xFF, 0x00, 0x80]] * 16 and not got[6:].any()
    assert list(st["bc7"]) == [dc.INVALID, dc.INVALID, 0, 0, 0, 0]


# ---- argument rules decided before a device is needed ---------------------------------------------------------------------------------------
# Every refusal below is returned before the context is looked at, so a block of zeroed memory stands in for one: the calls that would reach the
# device (valid arguments with blocks to decode) are the GPU tests'.
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_device_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(fake)
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 255) & ~255
    A = _lib.ERR_ARGUMENT

    def call(c=ctx, fmt=_lib.BC7, src=p, n=64, dst=p + 4096, bpr=8, pitch=0):
        return lib.bu_blocks_decode_rgba_device(c, fmt, src, n, dst, bpr, pitch, 0, None, None)

    assert call(c=None) == A
    for fmt in (4, 5, 10, 13, -1, 1 << 20):
        assert call(fmt=fmt) == A and call(fmt=fmt, n=0) == A
    assert call(src=None) == A and call(dst=None) == A
    assert call(bpr=0) == A and call(bpr=0, n=0) == A
    assert call(n=63) == A and call(n=65, bpr=64) == A  # whole block rows only
    assert call(src=p + 8) == A and call(dst=p + 4096 + 8) == A  # 16-byte blocks, 16-byte pixel rows
    assert call(fmt=_lib.BC1_RGB, src=p + 4) == A
    for pitch in (8, 16 * 8 - 16, 16 * 8 + 8, 16 * 8 + 4):
        assert call(pitch=pitch) == A
    # nothing to do is not an error: no launch, the context is not touched (null buffers are allowed then)
    assert call(n=0) == _lib.OK and call(n=0, src=None, dst=None) == _lib.OK and call(n=0, pitch=16 * 8 + 48) == _lib.OK
    assert call(fmt=_lib.BC1_RGB, src=p + 8, n=0) == _lib.OK  # the smallest alignment an 8-byte format needs


def test_host_form_argument_rules(lib):
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(fake)
    src, dst = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(1 << 16)
    bad = ctypes.c_uint64(0)

    def call(c=ctx, fmt=_lib.ASTC, nbytes=1024, bpr=8, out=dst, out_bytes=1 << 16, data=src):
        return lib.bu_blocks_decode_rgba(c, fmt, data, nbytes, bpr, out, out_bytes, ctypes.byref(bad))

    A = _lib.ERR_ARGUMENT
    assert call(c=None) == A
    for fmt in (4, 5, 10, 13, -1):
        assert call(fmt=fmt) == A
    assert call(data=None) == A and call(out=None) == A and call(bpr=0) == A
    assert call(nbytes=1024 + 8) == _lib.ERR_LENGTH and call(fmt=_lib.ETC1, nbytes=1024 + 4) == _lib.ERR_LENGTH
    assert call(nbytes=1024, bpr=7) == A  # 64 blocks are no whole number of 7-block rows
    assert call(out_bytes=64 * 64 - 1) == _lib.ERR_OUTPUT_SIZE
    assert call(nbytes=0) == _lib.OK and call(nbytes=0, data=None) == _lib.OK


def test_binding_rust_facade_and_header_spell_the_two_calls_alike():
    import re

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basisu_hip.h")).read(), flags=re.S)
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    lib_rs = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name, n_params in (("bu_blocks_decode_rgba_device", 10), ("bu_blocks_decode_rgba", 8)):
        m = re.search(r"bu_status\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n_params
        assert name in _lib.SYMBOLS
        assert re.search(r"fn %s\s*\(" % name, rs) and ("ffi::%s(" % name) in lib_rs
    assert re.search(r"pub fn decode_blocks\(", lib_rs) and re.search(r"pub unsafe fn decode_blocks_device\(", lib_rs)
