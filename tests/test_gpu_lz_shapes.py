"""The kernels get the same bytes whichever host path decoded the file: the device files of tests/lz_shape_cases.py -- an empty history_rle table with
16-bit selector codes (the fast loop and the two-thread form refuse, the exact loop decodes) and slices that are one predictor run and one selector run,
with alpha pairs -- each at 3122 blocks (one launch) and at 33 816 blocks (streamed; the 192 x 176-block first slice is a two-thread slice where the
tables allow it), to all eight outputs of an ETC1S file: ETC1 and RGBA32 byte for byte against the oracle's read of the file, BC1, BC3, BC4, BC5, EAC R11 and
EAC RG11 against the numpy models of the oracle's RGBA32.  The streamed files also through the one-launch path and with every slice on one thread.  One file
slice by slice, the slice back-ends fed by the product's host decode against the oracle's fed by the encoder's record.  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import basis_builder as bb
import basisu_rs_amd as bu
import file_shape_cases as fsc
import lz_shape_cases as lz
import test_gpu_file_shapes as tgf

pytestmark = pytest.mark.gpu
FILES = pytest.mark.parametrize("recipe,size", lz.GPU_FILES, ids=["%s-%s" % k for k in lz.GPU_FILES])


class Expected:
    """what every read of a file must give: the oracle's reads once, the model blocks of a target on first use (as tests/test_gpu_file_shapes.py keeps them)"""

    def __init__(self, oracle):
        self.oracle, self.images, self.want, self.models = oracle, {}, {}, {}

    def check(self, recipe, size, output, hdr, imgs):
        f = lz.gpu_file(recipe, size)[0]
        alpha = lz.GPU_RECIPES[recipe][0]["alpha"]
        key = (recipe, size)
        if output in ("etc1", "rgba"):
            if key + (output,) not in self.images:
                self.images[key + (output,)] = fsc.oracle_images(self.oracle, output, f)
            want_hdr, want = self.images[key + (output,)]
            assert hdr == want_hdr and len(imgs) == len(want)
            for k, (g, w) in enumerate(zip(fsc.tuples(imgs), want)):
                assert g[:3] == w[:3], (output, k)
                assert g[3] == w[3], "%s image %d differs from the oracle's" % (output, k)
            return
        if key not in self.want:
            self.want[key] = fsc.want_blocks(self.oracle, f, alpha)
        if key + (output,) not in self.models:
            self.models[key + (output,)] = fsc.model_blocks(self.want[key], output)
        fsc.check_model(imgs, self.want[key], output, self.models[key + (output,)])


@pytest.fixture(scope="module")
def expected(oracle):
    return Expected(oracle)


@pytest.mark.parametrize("output", tgf.OUTPUTS)
@FILES
def test_every_file_to_every_output(ctx, expected, recipe, size, output):
    lz.check_gpu_door(recipe, size)
    f = lz.gpu_file(recipe, size)[0]
    hdr, imgs = tgf.read(ctx, output, f)
    expected.check(recipe, size, output, hdr, imgs)
    alpha = lz.GPU_RECIPES[recipe][0]["alpha"]
    per_image = 2 if alpha and output == "etc1" else 1  # ETC1: every slice is an image of its own
    n_blocks = sum(x * y for x, y in lz.GPU_DIMS[size])
    assert bu.read_file_query(tgf.BU_TARGET[output], f) == (3 * per_image, n_blocks * per_image * tgf.BLOCK_BYTES[output])


@pytest.mark.parametrize("recipe", list(lz.GPU_RECIPES))
def test_streamed_files_through_every_door(ctx, expected, recipe):
    """the default door (where split_ok() allows it the first slice on two threads), the one-launch path, every slice on one thread: equal results.
    (Consecutive reads differ in their output, so that what the last read left in the context's output mirror is never what this one should write.)"""
    assert lz.GPU_DOORS[recipe, "large"][0]
    f = lz.gpu_file(recipe, "large")[0]
    default = {}
    for env in tgf.DOORS:
        for output in tgf.OUTPUTS:
            hdr, imgs = tgf.read(ctx, output, f, env)
            expected.check(recipe, "large", output, hdr, imgs)
            assert fsc.tuples(imgs) == default.setdefault(output, fsc.tuples(imgs)), (env, output)


def test_slice_back_ends_on_the_host_decode_against_the_oracle_on_the_record(ctx, oracle):
    """bu.basislz_decode -> the slice kernels, against the oracle's slice back-ends fed with the encoder's record and the encoder's codebooks"""
    f, ep, rows, streams = lz.gpu_file("one_run_alpha", "small")
    sel = oracle.selectors_from_rows(rows)
    descs = bu.read_slice_descs(f)
    assert len(descs) == len(streams) == 6
    for k in range(0, 6, 2):
        nbx, nby = descs[k].num_blocks_x, descs[k].num_blocks_y
        (pep, psel, pidx), (_, _, paidx) = bu.basislz_decode(f, k), bu.basislz_decode(f, k + 1)
        want, awant = bb.index_words(streams[k]), bb.index_words(streams[k + 1])
        assert (pidx == want).all() and (paidx == awant).all()
        assert (ctx.etc1s_transcode_to_etc1(pidx, pep, psel) == oracle.etc1s_to_etc1(want, ep, sel)).all()
        assert (ctx.etc1s_transcode_to_etc1(paidx, pep, psel) == oracle.etc1s_to_etc1(awant, ep, sel)).all()
        assert (ctx.etc1s_decode_to_rgba(pidx, None, nbx, nby, pep, psel) == oracle.etc1s_to_rgba(want, None, nbx, nby, ep, sel)).all()
        assert (ctx.etc1s_decode_to_rgba(pidx, paidx, nbx, nby, pep, psel) == oracle.etc1s_to_rgba(want, awant, nbx, nby, ep, sel)).all()
