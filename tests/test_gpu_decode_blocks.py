"""bu_blocks_decode_rgba_device / bu_blocks_decode_rgba on the GPU: the ten block formats -> RGBA8 images.

Expected bytes come from the witnesses of tests/decode_cases.py (oracle/bu_decoders.c and the numpy spec decoders), never from the code under test.
Per format ONE pool of blocks is modelled once per session -- the encoders' outputs for the golden UASTC blocks, random blocks, the edge blocks and,
for ASTC, blocks shaped onto the 4x4 grid; every case gathers its blocks from the pool.  Inputs and images lie between the guard bands of
tests/gpu_guard.py; images are pre-filled with a poison byte, so every image byte is compared and pitch padding must keep its poison."""
import numpy as np
import pytest

import decode_cases as dc
import etc1s_walk_cases as wc
import gpu_guard as gg
from basisu_rs_amd import BasisuError, _lib, synth
from oracle.pyoracle import Decoders
from test_roundtrip_decoders import BC7_BOUND, BC7_BOUND_DEFAULT

pytestmark = pytest.mark.gpu
NAMES = tuple(dc.FORMATS)
CLEAR = _lib.STATUS_WORD_CLEAR
POISON = 0xAB
SHAPES = ((1, 1), (63, 63), (64, 64), (65, 65), (130, 65), (192, 64), (35, 5), (1024, 128))  # (n_blocks, blocks_per_row)
NO_INVALID = ("bc4", "bc5", "r11", "rg11", "bc1", "bc3")  # with the OK-only pools of ETC1 / ETC2: the eight formats of the clear-word test


@pytest.fixture(scope="module")
def dec():
    return Decoders()


@pytest.fixture(scope="module")
def cu(ctx):
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


class Pool:
    """blocks [P, bytes] of one format, their expected texels [P, 64] and statuses [P]; `good` = indices of the blocks that decode"""

    def __init__(self, fmt, blocks, dec):
        self.fmt, self.blocks = fmt, np.ascontiguousarray(blocks)
        self.texels, self.status = dc.expected(dec, fmt, self.blocks)
        self.good = np.flatnonzero(self.status == 0)
        self.bad = {s: np.flatnonzero(self.status == s) for s in (dc.INVALID, dc.UNSUPPORTED)}


@pytest.fixture(scope="module")
def pools(oracle, golden, dec):
    enc, _ = dc.encoder_outputs(oracle, golden["uastc"])
    edges = dc.edge_blocks()
    out = {}
    for fmt in NAMES:
        parts = [enc[fmt], dc.random_blocks(fmt, 3000, seed=900 + dc.FORMATS[fmt]), edges[fmt]]
        if fmt == "astc":
            parts.append(dc.shaped_astc(6000, seed=77))
        out[fmt] = Pool(fmt, np.concatenate(parts), dec)
    assert len(out["astc"].good) > 1000 and len(out["bc7"].bad[dc.INVALID]) > 5 and len(out["etc1"].bad[dc.UNSUPPORTED]) > 100
    return out


def _pick(pool, n, salt=0, only_good=False):
    """n pool indices in a scrambled order"""
    src = pool.good if only_good else np.arange(pool.blocks.shape[0])
    return src[(np.arange(n, dtype=np.int64) * 7919 + 13 + 1009 * salt) % src.size]


def _expected_word(status, base):
    bad = np.flatnonzero(status != 0)
    return CLEAR if bad.size == 0 else ((base + int(bad[0])) << 8) | int(status[bad[0]])


def _run(ctx, fmt, blocks, bpr, pitch=0, base=0, with_status=True, src_offset=None):
    """one device call between guard bands -> (image [4 rows, pitch] uint8 as numpy, status word or None); bands checked"""
    import torch

    bb = dc.BLOCK_BYTES[fmt]
    n = blocks.shape[0]
    row = pitch if pitch else 16 * bpr
    src = gg.Arena("decode blocks in", max(n * bb, 1), gg.guard_bytes(bb), offsets=bb if src_offset is None else src_offset)
    dst = gg.Arena("decode image out", max(4 * (n // bpr) * row, 1), gg.guard_bytes(64), offsets=16)
    if n:
        src.data()[:] = torch.from_numpy(blocks.reshape(-1)).cuda()
    dst.data()[:] = POISON
    st = torch.full((1,), -1, dtype=torch.int64, device="cuda") if with_status else None
    ctx.decode_blocks_device(dc.FORMATS[fmt], src.ptr(), n, dst.ptr(), bpr, pitch, base, st)
    torch.cuda.synchronize()
    src.check()
    dst.check()
    img = dst.data().cpu().numpy().reshape(4 * (n // bpr), row) if n else np.zeros((0, row), dtype=np.uint8)
    return img, (int(st.item()) & CLEAR if with_status else None)


def _check_image(img, want_texels, bpr, what):
    want = dc.image(want_texels, bpr)
    got = img[:, : 16 * bpr]
    if not np.array_equal(got, want):
        y, x = np.argwhere(got != want)[0]
        raise AssertionError("%s: image differs at pixel row %d, byte %d (block %d): %d against %d" % (what, y, x, (y // 4) * bpr + x // 16, got[y, x], want[y, x]))
    assert (img[:, 16 * bpr:] == POISON).all(), what + ": pitch padding was written"


# ---- 1. all ten formats x shapes x pitches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", NAMES)
def test_every_shape_and_pitch(ctx, pools, fmt):
    pool = pools[fmt]
    for k, (n, bpr) in enumerate(SHAPES):
        for pitch in (0, 16 * bpr + 48):
            pick = _pick(pool, n, salt=k)
            img, word = _run(ctx, fmt, pool.blocks[pick], bpr, pitch, base=0)
            _check_image(img, pool.texels[pick], bpr, "%s %d x %d pitch %d" % (fmt, n, bpr, pitch))
            assert word == _expected_word(pool.status[pick], 0), (fmt, n, bpr, pitch)


# ---- 2. status ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,status", [("bc7", dc.INVALID), ("etc1", dc.UNSUPPORTED), ("etc2", dc.UNSUPPORTED), ("astc", dc.INVALID), ("astc", dc.UNSUPPORTED)])
def test_two_planted_bad_blocks_report_the_lower(ctx, pools, fmt, status):
    pool = pools[fmt]
    n, bpr, base = 640, 64, (5 << 32) + 12345
    pick = _pick(pool, n, salt=3, only_good=True)
    lo, hi = 257, 530
    pick[hi], pick[lo] = pool.bad[status][0], pool.bad[status][-1]
    assert (pool.status[pick] != 0).sum() == 2
    for with_status in (True, False):
        img, word = _run(ctx, fmt, pool.blocks[pick], bpr, base=base, with_status=with_status)
        _check_image(img, pool.texels[pick], bpr, "%s planted" % fmt)
        blocks = img.reshape(n // bpr, 4, bpr, 16).transpose(0, 2, 1, 3).reshape(n, 64)
        assert not blocks[lo].any() and not blocks[hi].any()
        assert all(blocks[i].any() == pool.texels[pick[i]].any() for i in (lo - 1, lo + 1, hi - 1, hi + 1))  # the neighbours are intact
        if with_status:
            assert word == ((base + lo) << 8) | status, (hex(word), fmt)
            with pytest.raises(BasisuError) as e:
                ctx.status_word_check(word)  # bu_status_word_decode knows both statuses of the decoders
            assert e.value.status == status


@pytest.mark.parametrize("fmt", NO_INVALID + ("etc1", "etc2"))
def test_the_word_stays_clear(ctx, pools, fmt):
    """the six formats without invalid encodings on random input; ETC1 / ETC2 on blocks that decode"""
    pool = pools[fmt]
    pick = _pick(pool, 4096, salt=9, only_good=fmt in ("etc1", "etc2"))
    if fmt in NO_INVALID:
        assert (pool.status == 0).all()
    img, word = _run(ctx, fmt, pool.blocks[pick], 64, base=77)
    _check_image(img, pool.texels[pick], 64, fmt)
    assert word == CLEAR


# ---- 3. grid-stride: two whole rounds of the grid and a ragged third -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,status", [("etc1", dc.UNSUPPORTED), ("bc7", dc.INVALID)])
def test_three_rounds_of_the_grid(ctx, pools, cu, fmt, status):
    """one case per block size, sized from the launcher's shape rule (bu_grid_for, restated in etc1s_walk_cases): the grid has 8 x cu workgroups of 256
    lanes; the array covers two whole rounds and a third that ends inside a workgroup.  Bad blocks in rounds three and one: the lowest is reported."""
    import torch

    pool = pools[fmt]
    B, bpr = wc.round_blocks(cu), 333
    n = -(-(2 * B + 1000) // bpr) * bpr
    while n % 256 == 0:
        n += bpr
    assert wc.grid_for(n, cu) * 256 == B and 2 * B < n < 3 * B and n % 256 != 0
    pick = _pick(pool, n, salt=5, only_good=True)
    third, first = 2 * B + 700, B - 300
    pick[third], pick[first] = pool.bad[status][0], pool.bad[status][1]
    base = 1 << 40
    bb = dc.BLOCK_BYTES[fmt]
    d_pick = torch.from_numpy(pick).cuda()
    src = gg.Arena("decode blocks in", n * bb, gg.guard_bytes(bb), offsets=bb)
    dst = gg.Arena("decode image out", 64 * n, gg.guard_bytes(64), offsets=16)
    src.data()[:] = torch.from_numpy(pool.blocks).cuda()[d_pick].reshape(-1)
    dst.data()[:] = POISON
    st = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ctx.decode_blocks_device(dc.FORMATS[fmt], src.ptr(), n, dst.ptr(), bpr, 0, base, st)
    torch.cuda.synchronize()
    src.check()
    dst.check()
    want = torch.from_numpy(pool.texels).cuda()[d_pick].reshape(n // bpr, bpr, 4, 16).permute(0, 2, 1, 3).reshape(-1)
    got = dst.data()
    if not torch.equal(got, want):
        k = int(torch.nonzero(got != want)[0, 0].item())
        raise AssertionError("%s: image differs first at byte %d (pixel row %d)" % (fmt, k, k // (16 * bpr)))
    assert int(st.item()) & CLEAR == ((base + first) << 8) | status


# ---- 4. host form ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bc7", "bc1", "astc", "rg11"])
def test_host_form_pageable_and_page_locked(ctx, pools, fmt):
    pool = pools[fmt]
    n, bpr = 2048 + 64, 64
    pick = _pick(pool, n, salt=11, only_good=True)
    blocks, want = pool.blocks[pick], dc.image(pool.texels[pick], bpr).reshape(-1)
    assert np.array_equal(ctx.decode_blocks(dc.FORMATS[fmt], blocks, bpr), want)
    hin, hout = ctx.host_alloc(blocks.size), ctx.host_alloc(64 * n)
    try:
        hin[:] = blocks.reshape(-1)
        hout[:] = POISON
        got = ctx.decode_blocks(dc.FORMATS[fmt], hin, bpr, out=hout)
        assert np.array_equal(got, want)
        assert np.array_equal(ctx.decode_blocks(dc.FORMATS[fmt], hin, bpr), want)  # page-locked in, pageable out
    finally:
        ctx.host_free(hin)
        ctx.host_free(hout)


def test_host_form_errors_leave_the_context_usable(ctx, pools):
    pool = pools["bc7"]
    n, bpr = 256, 16
    pick = _pick(pool, n, salt=13, only_good=True)
    good = pool.blocks[pick]
    want = dc.image(pool.texels[pick], bpr).reshape(-1)
    with pytest.raises(BasisuError) as e:
        ctx.decode_blocks(_lib.BC7, good.reshape(-1)[:-8], bpr)
    assert e.value.status == _lib.ERR_LENGTH
    with pytest.raises(BasisuError) as e:
        ctx.decode_blocks(_lib.BC7, good, bpr, out=np.empty(64 * n - 1, dtype=np.uint8))
    assert e.value.status == _lib.ERR_OUTPUT_SIZE
    for fmt, status in (("bc7", dc.INVALID), ("etc1", dc.UNSUPPORTED), ("astc", dc.UNSUPPORTED)):
        p = pools[fmt]
        pk = _pick(p, n, salt=14, only_good=True)
        pk[200], pk[77] = p.bad[status][0], p.bad[status][1]
        out = np.full(64 * n, POISON, dtype=np.uint8)
        with pytest.raises(BasisuError) as e:
            ctx.decode_blocks(dc.FORMATS[fmt], p.blocks[pk], bpr, out=out)
        assert e.value.status == status and e.value.first_bad_block == 77, (fmt, e.value.status, e.value.first_bad_block)
        assert np.array_equal(out, dc.image(p.texels[pk], bpr).reshape(-1))  # the image is complete, the failing blocks zero
    assert np.array_equal(ctx.decode_blocks(_lib.BC7, good, bpr), want)


# ---- 5. refusals launch nothing ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, pools):
    import torch

    pool = pools["bc7"]
    n, bpr = 128, 8
    blocks = pool.blocks[_pick(pool, n, only_good=True)]
    src = gg.Arena("decode blocks in", n * 16, gg.guard_bytes(16), offsets=16)
    dst = gg.Arena("decode image out", 64 * n + 4096, gg.guard_bytes(64), offsets=16)
    src.data()[:] = torch.from_numpy(blocks.reshape(-1)).cuda()
    dst.data()[:] = POISON
    st = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def refused(fmt=_lib.BC7, s=src.ptr(), count=n, d=dst.ptr(), row=bpr, pitch=0):
        with pytest.raises(BasisuError) as e:
            ctx.decode_blocks_device(fmt, s, count, d, row, pitch, 0, st)
        assert e.value.status == _lib.ERR_ARGUMENT

    for fmt in (4, 5, 10, 13):
        refused(fmt=fmt)
    refused(count=n - 1)
    refused(row=0)
    refused(s=src.ptr() + 8)
    refused(d=dst.ptr() + 8)
    refused(fmt=_lib.ETC1, s=src.ptr() + 4)
    for pitch in (16 * bpr - 16, 16 * bpr + 8, 8):
        refused(pitch=pitch)
    refused(s=0)
    refused(d=0)
    torch.cuda.synchronize()
    assert (dst.data() == POISON).all() and int(st.item()) & CLEAR == CLEAR
    src.check()
    dst.check()
    ctx.decode_blocks_device(_lib.BC7, 0, 0, 0, bpr, 0, 0, st)  # nothing to do: OK, nothing launched
    torch.cuda.synchronize()
    assert (dst.data() == POISON).all()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_transcode_then_decode_round_trip(ctx):
    """a 64 x 64-block UASTC slice -> ASTC -> pixels equals the slice's RGBA32 output exactly (UASTC is an ASTC subset); through BC7 it stays within the
    per-mode bounds of tests/test_roundtrip_decoders.py"""
    import torch

    n, bpr = 4096, 64
    blocks = synth.atlas_rand(n, seed=41)
    modes = synth.block_modes(blocks)
    d_in = torch.from_numpy(blocks.reshape(-1)).cuda()
    rgba = torch.full((64 * n,), POISON, dtype=torch.uint8, device="cuda")
    ctx.transcode_device(_lib.RGBA32, d_in, n, rgba, bpr)
    for fmt in (_lib.ASTC, _lib.BC7):
        mid = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        out = torch.full((64 * n,), POISON, dtype=torch.uint8, device="cuda")
        st = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        ctx.transcode_device(fmt, d_in, n, mid, bpr, 0, st)
        ctx.decode_blocks_device(fmt, mid, n, out, bpr, 0, 0, st)
        torch.cuda.synchronize()
        assert int(st.item()) & CLEAR == CLEAR
        if fmt == _lib.ASTC:
            assert torch.equal(out, rgba)
            continue
        err = np.abs(out.cpu().numpy().astype(int) - rgba.cpu().numpy().astype(int)).reshape(n // bpr, 4, bpr, 16).transpose(0, 2, 1, 3).reshape(n, 64).max(axis=1)
        for m in range(19):
            sel = modes == m
            if sel.any():
                assert err[sel].max() <= BC7_BOUND.get(m, BC7_BOUND_DEFAULT), (m, int(err[sel].max()))


# ---- 7. one linear graph capture ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_decode_replays(ctx, pools):
    """a 64-block BC7 decode captured on one stream (no parallel branches), replayed twice into a re-poisoned image: the same bytes as the direct call"""
    import torch

    pool = pools["bc7"]
    n, bpr = 64, 8
    pick = _pick(pool, n, salt=21, only_good=True)
    d_in = torch.from_numpy(pool.blocks[pick].reshape(-1)).cuda()
    want = torch.from_numpy(dc.image(pool.texels[pick], bpr).reshape(-1)).cuda()
    direct = torch.full((64 * n,), POISON, dtype=torch.uint8, device="cuda")
    ctx.decode_blocks_device(_lib.BC7, d_in, n, direct, bpr)
    torch.cuda.synchronize()
    assert torch.equal(direct, want)
    out = torch.full((64 * n,), POISON, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.decode_blocks_device(_lib.BC7, d_in, n, out, bpr, stream=s)
    for _ in range(2):
        out.fill_(POISON)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
