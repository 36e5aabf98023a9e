"""bu_read_file_to on the device: ETC1S files to BC1, BC3, BC4, BC5, EAC R11 and EAC RG11 through both front doors (the one-launch path
and the streamed one from 32 768 blocks), bit for bit against the numpy models applied to the oracle's RGBA32 read of the same file;
delegation of what bu_read_to already serves; host-detected errors and the context's state after them.  Run on the GPU box: pytest -m gpu."""
import os

import numpy as np
import pytest

import basis_builder as bb
import test_etc1s_targets as tet
from file_shape_cases import check_model as _check_model, tuples as _tuples, want_blocks as _want
from basisu_rs_amd import (BasisuError, TargetTextureFormat, _lib, read_file_query, read_file_to, read_header, read_slice_descs, read_to_astc,
                           read_to_bc1, read_to_bc3, read_to_bc4, read_to_bc5, read_to_bc7, read_to_eac_r11, read_to_eac_rg11, read_to_etc1,
                           read_to_etc2, read_to_rgba, write_uastc_file)

pytestmark = pytest.mark.gpu
NAMES = tuple(tet.TARGETS)
# 4096 blocks: a whole number of 64-block units; 561: ends mid-unit and its units straddle rows; one block
SMALL = [(64, 64), (33, 17), (1, 1)]
STREAMED = [(192, 192), (33, 17), (1, 1)]  # 37 426 blocks per plane: above BU_ETC1S_STREAM_MIN_BLOCKS


@pytest.fixture(scope="module")
def small(oracle):
    out = {}
    for alpha in (True, False):
        f = bb.etc1s_file(np.random.default_rng(61), SMALL, n_codebook=1024, alpha=alpha)[0]
        out[alpha] = (f, _want(oracle, f, alpha))
    return out


@pytest.fixture(scope="module")
def streamed(oracle):
    f = bb.etc1s_file(np.random.default_rng(905), STREAMED, n_codebook=1024, alpha=True)[0]
    return f, _want(oracle, f, True)


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
@pytest.mark.parametrize("name", NAMES)
def test_small_file_equals_the_model(ctx, small, name, alpha):
    f, want = small[alpha]
    t = tet.TARGETS[name][0]
    got = read_file_to(t, f, ctx)
    assert len(got) == 3 and read_file_query(t, f) == (3, sum(len(g.data) for g in got))
    _check_model(got, want, name)
    assert _tuples(read_file_to(TargetTextureFormat(t), f, ctx)) == _tuples(got)


def _read(t, f, ctx, env=None, out=None):
    if env:
        os.environ[env] = "1"
    try:
        return read_file_to(t, f, ctx, out=out)
    finally:
        if env:
            os.environ.pop(env, None)


@pytest.mark.parametrize("name", NAMES)
def test_streamed_front_door_equals_the_one_launch_path(ctx, streamed, name):
    f, want = streamed
    t = tet.TARGETS[name][0]
    got = _read(t, f, ctx)
    a = _tuples(got)
    assert len(a) == 3
    assert _tuples(_read(t, f, ctx, "BU_ETC1S_ONE_LAUNCH")) == a
    assert _tuples(_read(t, f, ctx, "BU_ETC1S_ONE_THREAD")) == a
    if name in ("bc3", "rg11"):  # both read A
        _check_model(got, want, name)
    if name == "bc1":  # a page-locked output: the bands store into it directly
        pinned = ctx.host_alloc(read_file_query(t, f)[1])
        try:
            assert _tuples(_read(t, f, ctx, out=pinned)) == a
        finally:
            ctx.host_free(pinned)


def test_uastc_file_is_read_to(ctx, golden):
    blocks = golden["uastc"][:48]
    f = write_uastc_file([dict(data=blocks[:32].tobytes(), orig_w=32, orig_h=16, nbx=8, nby=4),
                          dict(data=blocks[32:].tobytes(), orig_w=16, orig_h=16, nbx=4, nby=4, image_index=1)])
    same = {_lib.ASTC: read_to_astc, _lib.BC7: read_to_bc7, _lib.ETC1: read_to_etc1, _lib.ETC2: read_to_etc2,
            _lib.RGBA32: lambda *a: read_to_rgba(*a)[1], _lib.BC4_R: read_to_bc4, _lib.BC5_RG: read_to_bc5, _lib.EAC_R11: read_to_eac_r11,
            _lib.EAC_RG11: read_to_eac_rg11, _lib.BC1_RGB: read_to_bc1, _lib.BC3_RGBA: read_to_bc3}
    assert len(same) == 11
    for t, fn in same.items():
        got = _tuples(read_file_to(t, f, ctx))
        assert len(got) == 2 and got == _tuples(fn(f, ctx)), t


@pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])
def test_etc1s_file_to_etc1_and_rgba32_is_read_to(ctx, small, alpha):
    f = small[alpha][0]
    assert _tuples(read_file_to(_lib.ETC1, f, ctx)) == _tuples(read_to_etc1(f, ctx))
    assert _tuples(read_file_to(_lib.RGBA32, f, ctx)) == _tuples(read_to_rgba(f, ctx)[1])
    for t in (_lib.ASTC, _lib.BC7, _lib.ETC2):
        with pytest.raises(BasisuError) as e:
            read_file_to(t, f, ctx)
        assert e.value.status == _lib.ERR_UNSUPPORTED


def _status(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return _lib.OK
    except BasisuError as e:
        return e.status


def test_host_detected_errors_leave_the_context_usable(ctx, small):
    f, want = small[True]

    def good():  # a good call on the same context after an error
        _check_model(read_file_to(_lib.BC3_RGBA, f, ctx), want, "bc3")

    flipped = bytearray(f)
    flipped[-1] ^= 0x10  # payload damage, CRCs left alone
    assert _status(read_file_to, _lib.BC1_RGB, bytes(flipped), ctx) == _lib.ERR_DATA_CRC
    good()
    # a damaged symbol stream behind recomputed CRCs: the first of a few single-bit flips in slice 2 that bu_read_to(RGBA) refuses
    d = read_slice_descs(f, read_header(f))[2]
    found = None
    for pos in range(d.file_ofs + 1, d.file_ofs + d.file_size, max(d.file_size // 24, 1)):
        g = bytearray(f)
        g[pos] ^= 0x04
        g = bb.reseal(bytes(g))
        st = _status(read_to_rgba, g, ctx)
        if st != _lib.OK:
            found = (g, st)
            break
    assert found is not None, "no flip in the slice's stream was refused"
    assert _status(read_file_to, _lib.BC3_RGBA, found[0], ctx) == found[1]
    good()
    nbytes = read_file_query(_lib.BC1_RGB, f)[1]
    assert _status(read_file_to, _lib.BC1_RGB, f, ctx, out=np.empty(nbytes - 1, dtype=np.uint8)) == _lib.ERR_OUTPUT_SIZE
    assert len(read_file_to(_lib.BC1_RGB, f, ctx, out=np.empty(nbytes, dtype=np.uint8))) == 3
    good()
