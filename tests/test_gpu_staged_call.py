"""The blocking host-pointer entry points on the shapes their shared protocol (csrc/bu_staged_call.hpp) decides about, where the other GPU tests leave a
gap: 65 blocks (one full wave and a ragged one) in page-locked buffers that start 8 bytes past 16-byte alignment -- the kernels move 16-byte vectors, so
such a buffer is staged like pageable memory and the bytes are the same -- beside aligned ones, which the kernels read and write directly; a clean input
and a failing one each.  Every buffer lies between the guard bands of tests/gpu_guard.py.  Expected bytes: the golden vectors, the oracle, the decoders
of tests/decode_cases.py, for the block encoders the identity with the transcoder (tests/test_gpu_encode_blocks.py), and for the UASTC encoder the numpy
model's blocks (tests/uastc_encode_cases.py)."""
import numpy as np
import pytest

import basis_builder as bb
import basisu_rs_amd as bu
import decode_cases as dc
import gpu_guard as gg
from basisu_rs_amd import BasisuError, _lib, synth
from oracle.pyoracle import Decoders
from test_gpu_file_drivers import READ, breaking_flip, make_cases

pytestmark = pytest.mark.gpu
N = 65
POISON = 0xAB
OFFSETS = (0, 8)  # of a page-locked buffer from 256-byte alignment: mapped, staged


class Pinned:
    """page-locked arenas of the given sizes at `offset`, freed and their bands checked on the way out"""

    def __init__(self, ctx, offset, *sizes):
        self.arenas = [gg.Arena("page-locked buffer %d at +%d" % (i, offset), s, gg.GUARD_MIN, offsets=offset, where="pinned", ctx=ctx) for i, s in enumerate(sizes)]

    def __enter__(self):
        for a in self.arenas:
            a.data()[:] = POISON
        return [a.data() for a in self.arenas]

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                for a in self.arenas:
                    a.check()
        finally:
            for a in self.arenas:
                a.free()


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ["bc7", "astc", "etc2"])
def test_uastc_transcode_page_locked(ctx, golden, name, offset):
    idx = synth.gold_indices(N, seed=41)
    fmt = {"bc7": _lib.BC7, "astc": _lib.ASTC, "etc2": _lib.ETC2}[name]
    with Pinned(ctx, offset, N * 16, N * 16) as (pin_in, pin_out):
        assert pin_in.ctypes.data % 16 == offset and pin_out.ctypes.data % 16 == offset
        pin_in[:] = golden["uastc"][idx].reshape(-1)
        for src, dst in ((pin_in, pin_out), (pin_in, None), (golden["uastc"][idx], pin_out)):  # both sides, one side each
            if dst is not None:
                dst[:] = POISON
            got = ctx.transcode(fmt, src, out=dst)
            assert np.array_equal(got.reshape(N, 16), golden[name][idx]), (name, offset)
        bad = synth.atlas_err(golden["uastc"], N, [64, 33], seed=41)
        pin_in[:] = bad.reshape(-1)
        with pytest.raises(BasisuError) as e:
            ctx.transcode(fmt, pin_in, out=pin_out)
        assert e.value.first_bad_block == 33 and e.value.status in (_lib.ERR_INVALID_MODE, _lib.ERR_INVALID_PATTERN)
        good = np.ones(N, dtype=bool)
        good[[33, 64]] = False
        assert np.array_equal(pin_out.reshape(N, 16)[good], golden[name][idx][good])  # the slice is complete around the failing blocks


@pytest.mark.parametrize("offset", OFFSETS)
def test_rgba_rows_into_a_page_locked_image(ctx, golden, offset):
    """bpr = 5: 15 blocks are three whole rows.  13 blocks -- a ragged last row, whose stores at the image pitch would pass the 64 * 13 bytes of the
    caller's buffer -- never reach a kernel: bu_uastc_decode_to_rgba refuses them (uastc.rs:95), and nothing of the buffer is written."""
    idx = synth.gold_indices(15, seed=43)
    blocks = golden["uastc"][idx]
    with Pinned(ctx, offset, 64 * 13) as (out13,):
        with pytest.raises(BasisuError, match="invalid argument"):
            ctx.decode_to_rgba(blocks[:13], 5, out=out13)
        assert (out13 == POISON).all()
    with Pinned(ctx, offset, 64 * 15) as (out15,):
        img = ctx.decode_to_rgba(blocks, 5, out=out15).reshape(3, 4, 5, 16)
        assert np.array_equal(np.ascontiguousarray(img.transpose(0, 2, 1, 3)).reshape(15, 64), golden["rgba"][idx])


@pytest.mark.parametrize("offset", OFFSETS)
def test_decode_blocks_page_locked(ctx, golden, offset):
    """65 BC7 blocks, 13 per row; then one block no decoder takes"""
    idx = synth.gold_indices(N, seed=47)
    blocks = np.ascontiguousarray(golden["bc7"][idx])
    texels, status = dc.expected(Decoders(), "bc7", blocks)
    assert (status == 0).all()
    want = dc.image(texels, 13).reshape(-1)
    with Pinned(ctx, offset, N * 16, N * 64) as (pin_in, pin_out):
        pin_in[:] = blocks.reshape(-1)
        assert np.array_equal(ctx.decode_blocks(_lib.BC7, pin_in, 13, out=pin_out), want)
        assert np.array_equal(ctx.decode_blocks(_lib.BC7, pin_in, 13), want)
        pin_out[:] = POISON
        assert np.array_equal(ctx.decode_blocks(_lib.BC7, blocks, 13, out=pin_out), want)
        pin_in[16 * 40:16 * 41] = 0  # mode bits 0: a reserved BC7 block
        with pytest.raises(BasisuError) as e:
            ctx.decode_blocks(_lib.BC7, pin_in, 13, out=pin_out)
        assert e.value.status == _lib.ERR_INVALID_MODE and e.value.first_bad_block == 40


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ["bc5", "rg11", "bc3"])
def test_encode_blocks_page_locked(ctx, golden, name, offset):
    """encode_blocks(fmt, decode_to_rgba(uastc)) == transcode(fmt, uastc) on one row of 65 blocks (no status word: an encoder refuses nothing)"""
    fmt = dc.FORMATS[name]
    uastc = golden["uastc"][synth.gold_indices(N, seed=53)]
    rgba = ctx.decode_to_rgba(uastc, N).copy()
    want = ctx.transcode(fmt, uastc).copy()
    with Pinned(ctx, offset, rgba.size, N * 16) as (pin_in, pin_out):
        pin_in[:] = rgba
        for src, dst in ((pin_in, pin_out), (pin_in, None), (rgba, pin_out)):
            if dst is not None:
                dst[:] = POISON
            assert np.array_equal(ctx.encode_blocks(fmt, src, 4 * N, 4, out=dst), want), (name, offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_encode_uastc_page_locked(ctx, offset):
    """the first 65 blocks of the class-mixed edge strip (tests/uastc_encode_cases.py) == the model's.  The one staged call with two kernels, the second of
    which reads back what the first wrote into the caller's buffer and stores over it: mapped (+0) and staged (+8)"""
    import uastc_encode_cases as uc

    blocks, want, _ = uc.edge_mixed()
    image = uc.strip(blocks[:N]).reshape(-1)
    with Pinned(ctx, offset, image.size, N * 16) as (pin_in, pin_out):
        assert pin_in.ctypes.data % 16 == offset and pin_out.ctypes.data % 16 == offset
        pin_in[:] = image
        for src, dst in ((pin_in, pin_out), (pin_in, None), (image, pin_out)):
            if dst is not None:
                dst[:] = POISON
            assert np.array_equal(ctx.encode_uastc(src, 4 * N, 4, out=dst).reshape(N, 16), want[:N]), offset


# ---- the whole-file drivers: a page-locked output, mapped and staged, of the intact file and of one whose damage both CRCs hide ---------------
FILE_CASES = ("uastc, host crc", "etc1s one launch, crc up front", "etc1s streamed, crc up front")


@pytest.fixture(scope="module")
def files(golden, oracle):
    """name -> (target, file, the oracle's images, the damaged and resealed file, the oracle's status of that)"""
    out = {}
    cases = make_cases(golden)
    for name in FILE_CASES:
        target, f, damage, _, _ = cases[name]
        st, _, want = oracle.read_to(target, f)
        assert st == 0
        g, broken = breaking_flip(oracle, target, f, damage[0])
        out[name] = (target, f, [(w, h, s, d.tobytes()) for (w, h, s, d) in want], bb.reseal(g), broken)
    return out


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", FILE_CASES)
def test_file_drivers_into_a_page_locked_output(ctx, files, name, offset):
    target, f, want, damaged, broken = files[name]
    fn, read_target = READ[target]
    with Pinned(ctx, offset, bu.read_query(read_target, f)[1]) as (out,):
        imgs = fn(f, ctx, out=out)
        assert [(g.w, g.h, g.stride, np.asarray(g.data).tobytes()) for g in imgs] == want
        with pytest.raises(BasisuError) as e:
            fn(damaged, ctx, out=out)
        assert e.value.status == broken
        assert [(g.w, g.h, g.stride, np.asarray(g.data).tobytes()) for g in fn(f, ctx, out=out)] == want  # the context serves the next call
