"""bu_blocks_decode_rgba_device against an independent truth: the ASTC blocks tests/astc_model.py builds from their fields,
with the texels the fields mean, and the BC7 blocks of tests/golden/bc7_third_party.bin with the texels Pillow's DDS reader gave them.  Neither
expectation passes through oracle/bu_decoders.c.  Guard bands, the poisoned image and the byte-for-byte image compare are those of
tests/test_gpu_decode_blocks.py."""
import numpy as np
import pytest

import astc_model as am
import decode_cases as dc
import test_gpu_decode_blocks as gdb
from test_decode_fields import CLASS, load_bc7_fixture

pytestmark = pytest.mark.gpu
BPR = 37  # no multiple or divisor of 64: waves straddle block rows


@pytest.fixture(scope="module")
def built():
    """(blocks, texels, statuses as the library numbers them, order grouped by (weight range, dual, partitions, endpoint mode))"""
    cases = am.case_set()
    blocks, texels, status = am.arrays()

    def key(i):  # the widest weight range first, void-extent and block-mode cases last: the first failing block is not block 0
        k = am.group_key(cases[i])
        return (k[0] == 99, -k[0]) + k[1:]

    grouped = np.array(sorted(range(len(cases)), key=key), dtype=np.int64)
    return blocks, texels, CLASS[status], grouped


def _whole_rows(order, bpr):
    """pads an order to a whole number of block rows by repeating its first blocks"""
    return np.concatenate([order, order[: -order.size % bpr]])


def _decode_and_check(ctx, fmt, blocks, texels, status, order, bpr, pitch, what):
    img, word = gdb._run(ctx, fmt, blocks[order], bpr, pitch)
    gdb._check_image(img, texels[order], bpr, what)
    assert word == gdb._expected_word(status[order], 0), (what, hex(word))
    assert word == gdb.CLEAR or word >> 8 > 0  # (the lowest failing index is not simply the first block)
    return word


def test_astc_field_built_blocks_grouped(ctx, built):
    """the whole set in one launch, whole waves sharing a configuration"""
    blocks, texels, status, grouped = built
    order = _whole_rows(grouped, BPR)
    assert order.size % BPR == 0 and order.size >= len(am.case_set()) and (status[order] != 0).any()
    _decode_and_check(ctx, "astc", blocks, texels, status, order, BPR, 0, "astc grouped")


def test_astc_field_built_blocks_scrambled(ctx, built):
    """the same set through a fixed multiplicative permutation: every wave mixes configurations, failing blocks and void extents; a padded pitch"""
    blocks, texels, status, grouped = built
    order = _whole_rows(grouped, BPR)
    n = order.size
    assert np.gcd(1597, n) == 1
    order = order[(np.arange(n, dtype=np.int64) * 1597 + 11) % n]
    assert np.array_equal(np.sort(order), np.sort(_whole_rows(grouped, BPR)))
    waves = status[order][: n - n % 64].reshape(-1, 64)
    assert ((waves != 0).any(axis=1) & (waves == 0).any(axis=1)).mean() > 0.9  # nearly every wave holds failing blocks beside good ones
    _decode_and_check(ctx, "astc", blocks, texels, status, order, BPR, 16 * BPR + 48, "astc scrambled")


def test_astc_field_built_good_blocks_leave_the_word_clear(ctx, built):
    blocks, texels, status, grouped = built
    order = _whole_rows(grouped[status[grouped] == 0], BPR)
    assert order.size > 5000
    word = _decode_and_check(ctx, "astc", blocks, texels, status, order, BPR, 16 * BPR + 48, "astc good blocks")
    assert word == gdb.CLEAR


@pytest.mark.parametrize("bpr", [64, 33])
def test_bc7_third_party_blocks(ctx, bpr):
    blocks, texels = load_bc7_fixture()
    order = _whole_rows(np.arange(1024, dtype=np.int64), bpr)
    word = _decode_and_check(ctx, "bc7", blocks, texels, np.zeros(1024, dtype=np.int64), order, bpr, 0, "bc7 third party, %d per row" % bpr)
    assert word == gdb.CLEAR
