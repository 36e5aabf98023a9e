"""The whole-file calls on the device over the files of tests/file_shape_cases.py -- a cube map with mips, block counts either side of a 64-block unit, a
texture array of 144 small images, a mip chain down to one block -- with and without alpha pairs, to all eight outputs of an ETC1S file: ETC1 and RGBA32
byte for byte against the oracle's read of the same file, BC1, BC3, BC4, BC5, EAC R11 and EAC RG11 against the numpy models applied to the oracle's RGBA32
read.  The two files above 32 768 blocks through the streamed front door (decode on two threads and on one), through the one-launch path, and into
page-locked outputs; four files of different sizes back to back on one context; damaged slices of the array, which must report the reference's first failing
slice in file order through every door; the same shapes as UASTC files, whose slices form one run.  Run on the GPU box: pytest -m gpu."""
import os

import numpy as np
import pytest

import basis_builder as bb
import basisu_rs_amd as bu
import file_shape_cases as fsc
import test_etc1s_targets as tet
from basisu_rs_amd import _lib, synth

pytestmark = pytest.mark.gpu
OUTPUTS = ("etc1", "rgba") + tuple(tet.TARGETS)
BU_TARGET = dict({"etc1": _lib.ETC1, "rgba": _lib.RGBA32}, **{k: v[0] for k, v in tet.TARGETS.items()})
BLOCK_BYTES = dict({"etc1": 8, "rgba": 64}, **{k: v[1] for k, v in tet.TARGETS.items()})
DOORS = (None, "BU_ETC1S_ONE_LAUNCH", "BU_ETC1S_ONE_THREAD")  # the environment variable that takes the call off its default path
ALPHA = pytest.mark.parametrize("alpha", [True, False], ids=["alpha", "opaque"])


class Expected:
    """what every read must give: the oracle's reads of a file once, the model blocks of a target on first use"""

    def __init__(self, oracle):
        self.oracle, self.images, self.want, self.models = oracle, {}, {}, {}

    def check(self, name, alpha, output, hdr, imgs):
        f = fsc.etc1s_file(name, alpha)
        if output in ("etc1", "rgba"):
            if (name, alpha, output) not in self.images:
                self.images[name, alpha, output] = fsc.oracle_images(self.oracle, output, f)
            want_hdr, want = self.images[name, alpha, output]
            assert hdr == want_hdr
            assert len(imgs) == len(want)
            for k, (g, w) in enumerate(zip(fsc.tuples(imgs), want)):
                assert g[:3] == w[:3], (output, k)
                assert g[3] == w[3], "%s image %d differs from the oracle's" % (output, k)
            return
        if (name, alpha) not in self.want:
            self.want[name, alpha] = fsc.want_blocks(self.oracle, f, alpha)
        if (name, alpha, output) not in self.models:
            self.models[name, alpha, output] = fsc.model_blocks(self.want[name, alpha], output)
        fsc.check_model(imgs, self.want[name, alpha], output, self.models[name, alpha, output])


@pytest.fixture(scope="module")
def expected(oracle):
    return Expected(oracle)


def read(ctx, output, f, env=None, pinned=False):
    """-> (the header as a list, [Image]) of the call that serves `output`; pinned: into a page-locked output, which the kernels store into directly.
    The variables are read per call."""
    out = None
    if env:
        os.environ[env] = "1"
    try:
        if pinned:
            out = ctx.host_alloc(bu.read_file_query(BU_TARGET[output], f)[1])
            out[:] = 0xA5
        if output == "rgba":
            hdr, imgs = bu.read_to_rgba(f, ctx, out=out)
        elif output == "etc1":
            hdr, imgs = bu.read_header(f), bu.read_to_etc1(f, ctx, out=out)
        else:
            hdr, imgs = bu.read_header(f), bu.read_file_to(BU_TARGET[output], f, ctx, out=out)
        return hdr.as_list(), [bu.Image(g.w, g.h, g.stride, np.array(g.data)) for g in imgs]
    finally:
        if env:
            os.environ.pop(env, None)
        if out is not None:
            ctx.host_free(out)


def status(ctx, output, f, env=None):
    try:
        read(ctx, output, f, env)
        return _lib.OK
    except bu.BasisuError as e:
        return e.status


# ---- results ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output", OUTPUTS)
@ALPHA
@pytest.mark.parametrize("name", fsc.NAMES)
def test_every_shape_to_every_output(ctx, expected, name, alpha, output):
    fsc.check_door(name, alpha)
    f = fsc.etc1s_file(name, alpha)
    hdr, imgs = read(ctx, output, f)
    expected.check(name, alpha, output, hdr, imgs)
    n_images, n_blocks = fsc.TOTALS[name]
    per_image = 2 if alpha and output == "etc1" else 1  # ETC1: every slice is an image of its own
    assert bu.read_file_query(BU_TARGET[output], f) == (n_images * per_image, n_blocks * per_image * BLOCK_BYTES[output])
    assert sum(len(g.data) for g in imgs) == n_blocks * per_image * BLOCK_BYTES[output]


# ---- doors and output kinds ---------------------------------------------------------------------------------------------------------
@ALPHA
@pytest.mark.parametrize("name", fsc.STREAMED)
def test_streamed_shapes_through_every_door(ctx, expected, name, alpha):
    """(consecutive reads differ in their output, so that what the last read left in the context's output mirror is never what this one should write)"""
    f = fsc.etc1s_file(name, alpha)
    default = {}
    for env in DOORS:
        for output in OUTPUTS:
            hdr, imgs = read(ctx, output, f, env)
            expected.check(name, alpha, output, hdr, imgs)
            assert fsc.tuples(imgs) == default.setdefault(output, fsc.tuples(imgs)), (env, output)


@pytest.mark.parametrize("output", ["etc1", "rgba", "bc1", "rg11"])
@pytest.mark.parametrize("name", fsc.STREAMED)
def test_streamed_shapes_into_a_page_locked_output(ctx, expected, name, output):
    """the bands store into host memory directly: a band launched a unit short leaves the fill pattern, one launched a unit long writes the next image"""
    hdr, imgs = read(ctx, output, fsc.etc1s_file(name, True), pinned=True)
    expected.check(name, True, output, hdr, imgs)


# ---- buffer reuse -------------------------------------------------------------------------------------------------------------------
def test_files_of_different_sizes_back_to_back_on_one_context(ctx, expected):
    """the context keeps its page-locked index buffer, the auxiliary buffer with the slice table, the output mirror and the token buffer between calls: a
    smaller file behind a larger one runs over stale index words and a stale table.  One pass."""
    cube = []
    for name in ("mip_chain_192", "cube_mips", "array_240", "cube_mips"):
        for output in ("rgba", "bc3"):
            hdr, imgs = read(ctx, output, fsc.etc1s_file(name, True))
            expected.check(name, True, output, hdr, imgs)
            if name == "cube_mips":
                cube.append((output, hdr, fsc.tuples(imgs)))
    assert cube[:2] == cube[2:]


# ---- errors in file order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("images", [(100,), (7,), (7, 100)], ids=["image 100", "image 7", "both"])
def test_damaged_array_slices_report_the_first_in_file_order(ctx, oracle, expected, images):
    """array_240 with alpha, streamed with the CRC deferred: 288 slices decoded by the pool threads in whatever order they finish.  The reference walks the
    slices in file order, so with images 7 and 100 damaged the status is image 7's, whichever thread fails first.  (Every slice damaged this way, and by
    any single bit flipped in its first 60 bytes, fails with the same status, "out of bounds": the status alone cannot tell which of the two slices a door
    named, so what this holds is the oracle's status through every door and a context that reads the intact file correctly directly afterwards.)"""
    f = fsc.etc1s_file("array_240", True)
    g = fsc.damaged(f, images, True)
    assert len(g) == len(f) >= fsc.CRC_DEFER_BYTES
    want = oracle.read_to("rgba", g)[0]
    assert want != 0  # 64 inverted bytes do not survive the symbol decoder
    assert want == oracle.read_to("rgba", fsc.damaged(f, images[:1], True))[0]  # the oracle names the first failing slice
    for env in DOORS:
        for output in ("rgba", "bc1"):
            assert status(ctx, output, g, env) == want, (env, output)
            hdr, imgs = read(ctx, output, f, env)  # the intact file directly afterwards
            expected.check("array_240", True, output, hdr, imgs)


def test_damaged_cube_map_slice(ctx, oracle, expected):
    """the same on the one-launch path: the 16 x 16-block level of the third face"""
    f = fsc.etc1s_file("cube_mips", True)
    assert fsc.dims_of("cube_mips")[13] == (16, 16)
    g = fsc.damaged(f, (13,), True)
    want = oracle.read_to("rgba", g)[0]
    assert want != 0
    for output in ("rgba", "bc1"):
        assert status(ctx, output, g) == want, output
        hdr, imgs = read(ctx, output, f)
        expected.check("cube_mips", True, output, hdr, imgs)


# ---- UASTC files of the same shapes -------------------------------------------------------------------------------------------------
UASTC_OUTPUTS = {"bc7": _lib.BC7, "etc1": _lib.ETC1, "rgba": _lib.RGBA32, "bc3": _lib.BC3_RGBA}


@pytest.fixture(scope="module")
def uastc(golden):
    """name -> (file, golden indices per image): the slices back to back, so all of them form one run (bu_uastc_file_layout) and one launch for the
    block-linear targets, with one-block images inside it"""
    out = {}
    for n, name in enumerate(("cube_mips", "unit_edges")):
        dims = fsc.dims_of(name)
        idx = [synth.gold_indices(x * y, seed=700 + 50 * n + i) for i, (x, y) in enumerate(dims)]
        f = bb.uastc_file([golden["uastc"][ix] for ix in idx], dims)
        descs = bu.read_slice_descs(f)
        assert all(a.file_ofs + a.file_size == b.file_ofs and a.file_size == 16 * x * y for a, b, (x, y) in zip(descs, descs[1:], dims))
        out[name] = (f, idx)
    return out


def uastc_want(golden, oracle, name, f, idx, output):
    """[(w, h, stride, bytes)]: geometry as the oracle reports it (BC3, which it does not write: BC7's, both 16 bytes a block), bytes gathered from the 608
    known answers (BC3: the colour model of their RGBA32)"""
    st, _, geometry = oracle.read_to(output if output != "bc3" else "bc7", f)
    assert st == 0 and len(geometry) == len(idx)
    want = []
    for (w, h, stride, _), ix, (nbx, nby) in zip(geometry, idx, fsc.dims_of(name)):
        if output == "rgba":  # blocks of 4 rows x 16 bytes -> an image at its own pitch
            data = golden["rgba"][ix].reshape(nby, nbx, 4, 16).transpose(0, 2, 1, 3)
        elif output == "bc3":
            data = tet.model("bc3", golden["rgba"][ix])
        else:
            data = golden[output][ix]
        want.append((w, h, stride, np.ascontiguousarray(data).tobytes()))
    return want


@pytest.mark.parametrize("output", list(UASTC_OUTPUTS))
@pytest.mark.parametrize("name", ["cube_mips", "unit_edges"])
def test_uastc_files_of_the_same_shapes(ctx, golden, oracle, uastc, name, output):
    f, idx = uastc[name]
    want = uastc_want(golden, oracle, name, f, idx, output)
    assert [(w, h) for w, h, _, _ in want] == [(4 * x - 1, 4 * y - 2) for x, y in fsc.dims_of(name)]
    got = fsc.tuples(bu.read_file_to(UASTC_OUTPUTS[output], f, ctx))
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (output, k, fsc.dims_of(name)[k])
    assert bu.read_file_query(UASTC_OUTPUTS[output], f) == (len(idx), sum(len(w[3]) for w in want))


@pytest.mark.parametrize("output", list(UASTC_OUTPUTS))
def test_uastc_invalid_mode_in_a_one_block_image_inside_the_run(ctx, golden, oracle, uastc, output):
    f, idx = uastc["cube_mips"]
    assert fsc.dims_of("cube_mips")[17] == (1, 1)  # the last level of the third face: slices before and behind it in the run
    g = bytearray(f)
    pos = bu.read_slice_descs(f)[17].file_ofs
    g[pos] = (g[pos] & 0x80) | 69  # no UASTC mode
    g = bb.reseal(bytes(g))
    want = oracle.read_to(output if output != "bc3" else "bc7", g)[0]
    assert want == _lib.ERR_INVALID_MODE
    with pytest.raises(bu.BasisuError) as e:
        bu.read_file_to(UASTC_OUTPUTS[output], g, ctx)
    assert e.value.status == want
    assert fsc.tuples(bu.read_file_to(UASTC_OUTPUTS[output], f, ctx)) == uastc_want(golden, oracle, "cube_mips", f, idx, output)
