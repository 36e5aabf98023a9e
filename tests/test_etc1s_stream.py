"""The scheduler of the streamed ETC1S front door (csrc/bu_etc1s_stream.hpp) on the CPU: tests/host_emul/bu_etc1s_stream_check.cpp runs the shipped text
with a recording sink in the device's place, under ASan / UBSan and under ThreadSanitizer.  The sink aborts on a call out of order, a band that is not
the next one of its image, or an index word of a launched unit that is not the sequential decode's at that moment; the harness then compares status and
index buffer with the sequential reading, fails a launch (which nobody may do to a real device) and reads the file again.  Every file goes through the
default thresholds, through every slice on two threads with bands of one unit, and without a token buffer, pristine and under bit flips."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import basis_builder as bb  # noqa: E402
import file_shape_cases as fsc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_EMUL = os.path.join(ROOT, "tests", "host_emul")
BUILDS = ("bu_etc1s_stream_asan", "bu_etc1s_stream_tsan")

SMALL = [(9, 7), (4, 4), (13, 2)]  # tests/test_container.py's multi-slice files
# name -> (dims, etc1s_file arguments, fuzz rounds of the ASan / UBSan build, of the ThreadSanitizer build)
FILES = {
    "plain": (SMALL, dict(n_codebook=70), 400, 40),
    "alpha_dpcm": (SMALL, dict(n_codebook=70, alpha=True, raw_selectors=False), 400, 40),
    "video": (SMALL, dict(n_codebook=70, is_video=True, history_size=3), 400, 40),
    "column": ([(1, 700)], dict(n_codebook=90), 300, 30),
    "row": ([(700, 1)], dict(n_codebook=90), 300, 30),
    "odd_alpha": ([(3, 301), (5, 3)], dict(n_codebook=90, alpha=True), 300, 30),
    # the first slice above the real threshold: the default path splits by itself
    "splits_by_itself": ([(192, 192), (33, 17), (1, 1)], dict(n_codebook=1024, alpha=True), 6, 1),
}


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", HOST_EMUL] + list(BUILDS), check=True, capture_output=True)
    return {b: os.path.join(HOST_EMUL, b) for b in BUILDS}


@pytest.mark.parametrize("name", list(FILES))
def test_scheduler_under_sanitizers(harness, tmp_path, name):
    dims, kw, rounds_asan, rounds_tsan = FILES[name]
    f = bb.etc1s_file(np.random.default_rng(17 + len(name)), dims, **kw)[0]
    if name == "splits_by_itself":
        assert dims[0][0] * dims[0][1] >= fsc.STREAM_MIN_BLOCKS
    path = tmp_path / "t.basis"
    path.write_bytes(f)
    for build, rounds in zip(BUILDS, (rounds_asan, rounds_tsan)):
        r = subprocess.run([harness[build], str(path), str(rounds)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr and "stream check done" in r.stdout, build + r.stdout + r.stderr[-3000:]


def test_pure_pieces_on_hand_made_inputs(harness):
    """item order, band rule, status order, token size and split rule, called directly"""
    for build in BUILDS:
        r = subprocess.run([harness[build], "--pure"], capture_output=True, text=True)
        assert r.returncode == 0 and "pure pieces ok" in r.stdout, build + r.stdout + r.stderr[-3000:]
