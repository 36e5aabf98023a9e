"""The files of tests/file_shape_cases.py on the CPU: the constants the module restates are the source's, every shape takes the front door and the CRC mode
its row says, the oracle reads every file, and the layout (bu_etc1s_file_layout) with the kernels' unit search (bu_etc1s_unit_slice) over each file's slice
table -- 37 and 145 entries, images smaller than a unit, last units part empty -- through the stand-alone host build of tests/test_file_layout.py, with and
without UBSan, against that module's layout model."""
import os
import re
import subprocess

import pytest

import file_shape_cases as fsc
from test_file_layout import ETC1S_TARGETS, check_etc1s_layout, layout  # noqa: F401  (layout: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
CASES = [(name, alpha) for name in fsc.NAMES for alpha in (True, False)]
IDS = ["%s-%s" % (name, "alpha" if alpha else "opaque") for name, alpha in CASES]


def test_constants_are_pinned_to_the_source():
    """a changed threshold fails here instead of silently moving a shape to the other door or CRC mode"""
    src = open(os.path.join(CSRC, "bu_capi_file.hpp")).read()
    sched = open(os.path.join(CSRC, "bu_etc1s_stream.hpp")).read()  # the scheduler of the streamed door: the constants and the two rules that are functions
    m = re.findall(r"constexpr size_t BU_ETC1S_STREAM_MIN_BLOCKS = (\d+), BU_ETC1S_BAND_BLOCKS = (\d+);", src + sched)
    assert len(m) == 1 and (int(m[0][0]), int(m[0][1])) == (fsc.STREAM_MIN_BLOCKS, fsc.BAND_BLOCKS) and "BU_ETC1S_BAND_BLOCKS = " in sched
    # the two places that name the streamed door's threshold: the deferred CRC of an ETC1S file, and the choice of the door by the file's total blocks
    defer = re.findall(r"len >= \(\(size_t\)(\d+) << (\d+)\) && !getenv\(\"BU_ETC1S_ONE_LAUNCH\"\) && [^\n]*tex_format == 0", src)
    assert len(defer) == 1 and int(defer[0][0]) << int(defer[0][1]) == fsc.CRC_DEFER_BYTES
    assert len(re.findall(r"total_blocks >= BU_ETC1S_STREAM_MIN_BLOCKS && !getenv\(\"BU_ETC1S_ONE_LAUNCH\"\)", src)) == 1
    # the band rule and the two-thread decode of a slice are functions now, each with one caller in the scheduler and the constant as its default: the host
    # build of the scheduler (tests/host_emul/bu_etc1s_stream_check.cpp) answers with the shipped defaults at both sides of the module's numbers
    assert len(re.findall(r"bu_etc1s_band_due\(avail, launched\[k\], finished, band_blocks\)", sched)) == 1
    assert len(re.findall(r"size_t band_blocks = BU_ETC1S_BAND_BLOCKS\)", sched)) == 2  # the rule's default and the scheduler's, which it hands down
    assert len(re.findall(r"bu_etc1s_slice_splits\(may_split, nblk, split_min\)", sched)) == 1  # (the job table; the token size asks per slice too)
    assert len(re.findall(r"size_t split_min = BU_ETC1S_STREAM_MIN_BLOCKS[,)]", sched)) == 3  # the rule, the token size and the scheduler
    he = os.path.join(ROOT, "tests", "host_emul")
    subprocess.run(["make", "-C", he, "bu_etc1s_stream_asan"], check=True, capture_output=True)

    def rule(*args):
        return int(subprocess.run([os.path.join(he, "bu_etc1s_stream_asan"), "--rule"] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout)

    band_units = fsc.BAND_BLOCKS // fsc.UNIT
    assert fsc.BAND_BLOCKS % fsc.UNIT == 0
    # unfinished image: a band from BAND_BLOCKS blocks on, wherever it starts; finished: whatever is left; nothing new: nothing
    assert [rule("band", 7 + band_units - 1, 7, 0), rule("band", 7 + band_units, 7, 0), rule("band", 8, 7, 1), rule("band", 7, 7, 1)] == [0, 1, 1, 0]
    assert [rule("split", fsc.STREAM_MIN_BLOCKS - 1), rule("split", fsc.STREAM_MIN_BLOCKS)] == [0, 1]


@pytest.mark.parametrize("name, alpha", CASES, ids=IDS)
def test_shape_takes_its_door_and_the_oracle_reads_it(oracle, name, alpha):
    fsc.check_door(name, alpha)
    f = fsc.etc1s_file(name, alpha)
    n_images, n_blocks = fsc.TOTALS[name]
    hdr, imgs = fsc.oracle_images(oracle, "rgba", f)
    assert len(imgs) == n_images and sum(len(d) for _, _, _, d in imgs) == 64 * n_blocks
    assert [(w, h) for w, h, _, _ in imgs] == [(4 * x, 4 * y) for x, y in fsc.dims_of(name)]
    _, etc1 = fsc.oracle_images(oracle, "etc1", f)  # every slice is an image of its own
    assert len(etc1) == n_images * (2 if alpha else 1) and sum(len(d) for _, _, _, d in etc1) == 8 * n_blocks * (2 if alpha else 1)
    want = fsc.want_blocks(oracle, f, alpha)
    assert [(w, h, nbx, rgba.shape) for w, h, nbx, rgba in want] == [(4 * x, 4 * y, x, (x * y, 64)) for x, y in fsc.dims_of(name)]


@pytest.mark.parametrize("target", list(ETC1S_TARGETS))
@pytest.mark.parametrize("name, alpha", CASES, ids=IDS)
def test_layout_and_unit_search(layout, name, alpha, target):  # noqa: F811
    dims = fsc.dims_of(name)
    got, unit_slice = check_etc1s_layout(layout, fsc.etc1s_file(name, alpha), dims, alpha, target)
    per_image = 2 if alpha and target == "etc1" else 1
    blocks = [x * y for x, y in dims for _ in range(per_image)]
    # units_of counts the partly filled tails, and consecutive entries never share a unit0
    assert got["units_of"] == [-(-n // fsc.UNIT) for n in blocks]
    table_unit0 = [d[0] for d in got["descs"]]
    assert all(a < b for a, b in zip(table_unit0, table_unit0[1:])) and table_unit0[0] == 0 and table_unit0[-1] == got["n_units"]
    # every unit of the file maps to the image that owns it: the owner by a linear walk over the images, not by the table
    owner = [image for image, n in enumerate(blocks) for _ in range(-(-n // fsc.UNIT))]
    assert [got["descs"][s][5] for s in unit_slice] == owner
    # the lanes the kernel accepts, (unit - unit0) * 64 + lane < n_blocks, are every block of every image exactly once
    live = [0] * len(blocks)
    for u, s in enumerate(unit_slice):
        unit0, n_blocks = got["descs"][s][:2]
        assert u >= unit0
        live[got["descs"][s][5]] += max(0, min(fsc.UNIT, n_blocks - (u - unit0) * fsc.UNIT))
    assert live == blocks
    if name == "array_240":
        assert set(got["units_of"]) == {4} and set(live) == {240} and got["n_units"] == 4 * len(blocks) and len(got["descs"]) == len(blocks) + 1
    if name == "cube_mips":
        assert len(got["descs"]) == 36 * per_image + 1 and sum(n < fsc.UNIT for n in blocks) == 18 * per_image
