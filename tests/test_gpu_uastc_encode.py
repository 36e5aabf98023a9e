"""bu_rgba_encode_uastc / _device on the GPU: an RGBA8 image -> UASTC blocks.

The bytes are the numpy model's (tests/uastc_encode_model.py through tests/uastc_encode_cases.py, which the CPU tests judge by the oracle) on every shape
of the case list and on the layouts where the kernel can go wrong: unaligned bases and pitches (the 4-byte load path), padded outputs, a second
grid-stride step; on the edge families of the case list in waves of one block class and in waves that hold all four (a block's bytes must not depend
on its lane or its wave-mates); with guard bands around both buffers, refusals that must leave the output alone, the host form with pageable and page-locked
buffers, a graph capture, and the two compositions the encoder exists for: every transcode target of its blocks, and image -> .basis file -> read."""
import numpy as np
import pytest

import encode_cases as ec
import gpu_guard as gg
import uastc_encode_cases as uc
from basisu_rs_amd import BasisuError, _lib

pytestmark = pytest.mark.gpu

POISON = 0xA5
# (in_pad, out_pad_blocks, base_off): tight; an unaligned pitch (the fast path off) with a padded output; an aligned padded pitch; a base 4 bytes past
# 16-byte alignment (the fast path off with a tight pitch)
LAYOUTS = ((0, 0, 0), (4, 3, 0), (64, 0, 0), (0, 0, 4))
ALL_TARGETS = (_lib.ASTC, _lib.BC7, _lib.ETC1, _lib.ETC2, _lib.RGBA32, _lib.BC4_R, _lib.BC5_RG, _lib.EAC_R11, _lib.EAC_RG11, _lib.BC1_RGB, _lib.BC3_RGBA)


def _encode_device(ctx, img, in_pad=0, out_pad_blocks=0, base_off=0, pad_seed=0, stream=None):
    """blocks [nby, nbx, 16] of the device form; the layout arguments as in tests/test_gpu_encode_blocks.py"""
    import torch

    h, w, _ = img.shape
    nbx, nby = ec.blocks_of(w, h)
    in_pitch, out_pitch = 4 * w + in_pad, (nbx + out_pad_blocks) * 16
    fill = np.random.default_rng(pad_seed).integers(0, 256, size=ec.image_bytes(w, h, in_pitch), dtype=np.uint8)
    d_in = torch.zeros(base_off + fill.size, dtype=torch.uint8, device="cuda")
    d_in[base_off:] = torch.from_numpy(ec.pitched(img, in_pitch, fill)).cuda()
    d_out = torch.full((nby * out_pitch,), POISON, dtype=torch.uint8, device="cuda")
    ctx.encode_uastc_device(d_in[base_off:], w, h, d_out, in_pitch=in_pitch if in_pad else 0, out_pitch=out_pitch if out_pad_blocks else 0, stream=stream)
    torch.cuda.synchronize()
    rows = d_out.cpu().numpy().reshape(nby, out_pitch)
    assert (rows[:, nbx * 16:] == POISON).all(), "the out_pitch padding was written"
    return rows[:, : nbx * 16].reshape(nby, nbx, 16)


def _same(got, want, what):
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "%s: %d blocks differ, first (by, bx) %s: got %s, want %s" % (what, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])].tobytes().hex(),
                                                                                       want[tuple(bad[0])].tobytes().hex())


# ---- 1. the model on every case and layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.CASES, ids=uc.case_id)
def test_bytes_are_the_models(ctx, case):
    _, _, w, h = case
    want = uc.expected(*case)
    for in_pad, out_pad, off in LAYOUTS:
        got = _encode_device(ctx, uc.image(*case), in_pad, out_pad, off, pad_seed=in_pad + uc.CASES.index(case))
        _same(got, want, "%s layout %s" % (uc.case_id(case), (in_pad, out_pad, off)))


# ---- 1b. the edge families: waves of one class, waves of all four ---------------------------------------------------------------------------------
EDGE_LAYOUTS = LAYOUTS[:2]


def _strip_blocks(ctx, blocks, layout, seed):
    return _encode_device(ctx, uc.strip(blocks), *layout, pad_seed=seed)[0]


@pytest.fixture(scope="module")
def edge_gpu(ctx):
    """the device's blocks of edge_sorted and edge_mixed at the tight layout, encoded once"""
    return _strip_blocks(ctx, uc.edge_sorted()[0], EDGE_LAYOUTS[0], 1), _strip_blocks(ctx, uc.edge_mixed()[0], EDGE_LAYOUTS[0], 2)


def _family_of(i):
    return "%s[%d]" % (list(uc.EDGE_FAMILIES)[i // 64], i % 64)


def _same_strip(got, want, what, index=lambda i: i):
    bad = np.nonzero((got != want).any(-1))[0]
    assert bad.size == 0, "%s: %d blocks differ, first %d = %s: got %s, want %s" % (what, bad.size, bad[0], _family_of(int(index(bad[0]))), got[bad[0]].tobytes().hex(),
                                                                                   want[bad[0]].tobytes().hex())


def test_edge_blocks_are_the_models(ctx, edge_gpu):
    blocks, want = uc.edge_sorted()
    _same_strip(edge_gpu[0], want, "edge_sorted layout %s" % (EDGE_LAYOUTS[0],))
    _same_strip(_strip_blocks(ctx, blocks, EDGE_LAYOUTS[1], 3), want, "edge_sorted layout %s" % (EDGE_LAYOUTS[1],))


def test_mixed_class_waves_are_the_models(ctx, edge_gpu):
    """every wave of the strip holds lanes of all four classes (tests/test_uastc_encode.py asserts that of the strip).  Then without the model: block i
    of the mixed strip is block order[i] of the sorted one, encoded there in another lane beside blocks of its own family"""
    blocks, want, order = uc.edge_mixed()
    _same_strip(edge_gpu[1], want, "edge_mixed layout %s" % (EDGE_LAYOUTS[0],), lambda i: order[i])
    padded = _strip_blocks(ctx, blocks, EDGE_LAYOUTS[1], 4)
    _same_strip(padded, want, "edge_mixed layout %s" % (EDGE_LAYOUTS[1],), lambda i: order[i])
    _same_strip(edge_gpu[1], edge_gpu[0][order], "edge_mixed against the device's own edge_sorted", lambda i: order[i])
    _same_strip(padded, edge_gpu[0][order], "edge_mixed, padded, against the device's own edge_sorted", lambda i: order[i])


def test_class_rule_on_the_device(edge_gpu):
    """the class of a block's 16 texels against the mode in the device's bytes, no model between them"""
    for what, src, got in (("edge_sorted", uc.edge_sorted()[0], edge_gpu[0]), ("edge_mixed", uc.edge_mixed()[0], edge_gpu[1])):
        bad = uc.class_rule_violations(src, got)
        assert bad.size == 0, "%s: blocks %s" % (what, bad[:5].tolist())


@pytest.fixture(scope="module")
def formula_expected():
    import uastc_encode_model as um

    return {(w, h): um.encode(ec.to_blocks(uc.formula_image(w, h))).reshape(ec.blocks_of(w, h)[::-1] + (16,)) for (w, h) in ((255, 9), (12, 203))}


@pytest.mark.parametrize("shape", ((255, 9), (12, 203)), ids=lambda s: "%dx%d" % s)
def test_formula_image_with_partial_blocks(ctx, formula_expected, shape):
    """solid, opaque and RGBA classes change every 2 x 2 blocks, the last block column and row are partial"""
    w, h = shape
    img = uc.formula_image(w, h)
    assert len(set(uc.block_class(ec.to_blocks(img)).tolist())) >= 3
    for k, layout in enumerate(LAYOUTS):
        _same(_encode_device(ctx, img, *layout, pad_seed=50 + k), formula_expected[shape], "formula image %dx%d layout %s" % (w, h, layout))


# ---- 2. the host form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("plain", "random", 255, 9), ("opaque", "gradient", 257, 8), ("grey", "gradient", 12, 203)], ids=uc.case_id)
def test_host_form_pageable_and_page_locked(ctx, case):
    _, _, w, h = case
    want = uc.expected(*case)
    img = uc.image(*case)
    _same(ctx.encode_uastc(img, w, h).reshape(want.shape), want, "host form")
    pitch = 4 * w + 4
    buf = ec.pitched(img, pitch, np.full(ec.image_bytes(w, h, pitch), 0x3C, dtype=np.uint8))
    _same(ctx.encode_uastc(buf, w, h, in_pitch=pitch).reshape(want.shape), want, "host form, pitched")
    pin_in, pin_out = ctx.host_alloc(img.size), ctx.host_alloc(want.size)
    try:
        pin_in[:] = img.reshape(-1)
        pin_out[:] = POISON
        _same(ctx.encode_uastc(pin_in, w, h, out=pin_out).reshape(want.shape), want, "host form, page-locked")
    finally:
        ctx.host_free(pin_in)
        ctx.host_free(pin_out)


# ---- 3. a second grid-stride step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ("ag-gradient", "class-mixed"))
def test_second_grid_stride_step(ctx, pattern):
    """8 * CUs * 256 + 65 blocks or a little more: the grid is capped at 8 workgroups per CU, so some lanes take a second block; the image is a
    64 x 64-pixel pattern tiled, two pixels short of a multiple of four wide, on a 16-byte-aligned pitch (the 16-byte loads, the last column clamped).
    class-mixed: uc.mixed_pattern, whose block rows hold all four classes, and in the last 64 pixel rows -- the blocks of the second step -- the same
    pattern rolled by one 8 x 8 tile: the stride is a whole number of pattern heights, so without the roll a lane's second block would be its first
    again.  Asserted from the pixels: every lane that takes a second step gets a block of another class than its first, under a divergent mask"""
    import torch

    import uastc_encode_model as um

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    TX = 8
    TY = -(-(8 * cus * 256 + 65) // (256 * TX))
    w, h = 64 * TX - 2, 64 * TY
    nbx, nby = ec.blocks_of(w, h)
    assert nbx * nby >= 8 * cus * 256 + 65 and w % 4 != 0
    if pattern == "ag-gradient":
        pat, tile = uc.image("ag", "gradient", 64, 64), uc.expected("ag", "gradient", 64, 64)  # [16, 16, 16]
        last, last_tile = pat, tile
    else:
        pat, tile = uc.mixed_pattern(), uc.mixed_pattern_expected()
        last, last_tile = np.roll(pat, 8, axis=1), np.roll(tile, 2, axis=1)  # (one tile = two blocks to the right)
    # the partial last column: pattern columns 60, 61, 61, 61
    edge, last_edge = (um.encode(ec.to_blocks(p[:, 60:62])).reshape(16, 1, 16) for p in (pat, last))
    want = np.concatenate([np.tile(tile, (TY - 1, TX, 1)), np.tile(last_tile, (1, TX, 1))])
    want[:-16, -1:], want[-16:, -1:] = np.tile(edge, (TY - 1, 1, 1)), last_edge
    if pattern == "class-mixed":
        # a lane's blocks are i and i + stride; the stride is the whole grid, 8 workgroups per CU: TY - 1 pattern heights, so the second blocks are
        # exactly those of the last 64 pixel rows, above the same columns of the first 64
        stride = 8 * cus * 256
        assert stride == (TY - 1) * 16 * nbx and nbx * nby - stride == 16 * nbx
        first_cls, second_cls = (uc.block_class(ec.to_blocks(np.tile(p, (1, TX, 1))[:, :w])) for p in (pat, last))
        assert first_cls.size == 16 * nbx and (first_cls != second_cls).all()
        for s in range(0, first_cls.size, 64):
            assert len(set(first_cls[s:s + 64].tolist())) == 4 and len(set(second_cls[s:s + 64].tolist())) == 4
    d_img = torch.cat([torch.from_numpy(pat.copy()).cuda().repeat(TY - 1, TX, 1), torch.from_numpy(last.copy()).cuda().repeat(1, TX, 1)]).contiguous()
    assert tuple(d_img.shape) == (h, 64 * TX, 4)  # the pitch of the whole tiles, two columns unused
    d_out = torch.full((nbx * nby * 16,), POISON, dtype=torch.uint8, device="cuda")
    ctx.encode_uastc_device(d_img, w, h, d_out, in_pitch=4 * 64 * TX)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy().reshape(nby, nbx, 16), want, "second step, %s" % pattern)


# ---- 4. guard bands --------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_and_pitch_padding(ctx):
    """the image ends at its last pixel with a band right behind it; two runs whose bands and pitch padding hold different bytes give identical blocks,
    the output's bands and out_pitch padding keep their fill"""
    import torch

    for (case, in_pad, off) in ((("plain", "random", 255, 9), 64, 0), (("opaque", "random", 257, 8), 4, 4), (("plain", "gradient", 5, 3), 12, 8)):
        _, _, w, h = case
        nbx, nby = ec.blocks_of(w, h)
        in_pitch, out_pitch = 4 * w + in_pad, (nbx + 3) * 16
        n_in = ec.image_bytes(w, h, in_pitch)
        runs = []
        for r in range(2):
            a_in = gg.Arena("image run %d" % r, n_in, gg.GUARD_MIN + 4096 * r, offsets=off)
            a_out = gg.Arena("blocks run %d" % r, nby * out_pitch, gg.GUARD_MIN, offsets=0)
            reg = a_in.regions[0]
            fill = gg.fill_bytes(np, reg.start, reg.stop)  # the arena's own fill runs on through the padding
            if r:
                fill = fill ^ 0xFF
            a_in.data()[:] = torch.from_numpy(ec.pitched(uc.image(*case), in_pitch, fill)).cuda()
            oreg = a_out.regions[0]
            ofill = gg.fill_bytes(np, oreg.start, oreg.stop)
            a_out.data()[:] = torch.from_numpy(ofill).cuda()
            ctx.encode_uastc_device(a_in.ptr(), w, h, a_out.ptr(), in_pitch=in_pitch, out_pitch=out_pitch)
            torch.cuda.synchronize()
            a_in.check()
            a_out.check()
            rows = a_out.data().cpu().numpy().reshape(nby, out_pitch)
            assert (rows[:, nbx * 16:] == ofill.reshape(nby, out_pitch)[:, nbx * 16:]).all(), "%s: the out_pitch padding was written" % uc.case_id(case)
            runs.append(rows[:, : nbx * 16].reshape(nby, nbx, 16).copy())
        _same(runs[0], uc.expected(*case), "%s guarded" % uc.case_id(case))
        assert (runs[0] == runs[1]).all(), "%s: the blocks depend on bytes outside the image" % uc.case_id(case)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(ctx):
    import torch

    w, h = 32, 8
    d_in = torch.zeros(4 * w * h + 256, dtype=torch.uint8, device="cuda")
    d_out = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda")
    pi, po = d_in.data_ptr(), d_out.data_ptr()
    lib, handle = ctx._lib, ctx.handle

    def call(c=handle, src=pi, w=w, h=h, in_pitch=0, dst=po, out_pitch=0):
        return lib.bu_rgba_encode_uastc_device(c, src, w, h, in_pitch, dst, out_pitch, None)

    for row in (dict(c=None), dict(src=None), dict(dst=None), dict(src=pi + 2), dict(dst=po + 8), dict(dst=po + 4), dict(in_pitch=4 * w - 4),
                dict(in_pitch=4 * w + 2), dict(out_pitch=16 * 8 - 16), dict(out_pitch=16 * 8 + 8), dict(w=(1 << 30) + 1)):
        assert call(**row) == _lib.ERR_ARGUMENT, row
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())
    for row in (dict(w=0), dict(h=0), dict(w=0, h=0, src=None, dst=None)):  # an empty image is BU_OK and launches nothing
        assert call(**row) == _lib.OK, row
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())
    assert ctx.encode_uastc(np.zeros(0, dtype=np.uint8), 0, 7).size == 0
    with pytest.raises(BasisuError) as e:
        ctx.encode_uastc_device(d_in, w, h, d_out, in_pitch=4 * w + 2)
    assert e.value.status == _lib.ERR_ARGUMENT
    out = np.full(16 * 8 * 2 - 1, POISON, dtype=np.uint8)
    with pytest.raises(BasisuError) as e:
        ctx.encode_uastc(np.zeros(4 * w * h, dtype=np.uint8), w, h, out=out)
    assert e.value.status == _lib.ERR_OUTPUT_SIZE and (out == POISON).all()
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_equals_the_direct_call(ctx):
    import torch

    case = ("opaque", "random", 257, 8)
    _, _, w, h = case
    nbx, nby = ec.blocks_of(w, h)
    d_img = torch.from_numpy(uc.image(*case).copy()).cuda()
    direct = torch.zeros(nbx * nby * 16, dtype=torch.uint8, device="cuda")
    ctx.encode_uastc_device(d_img, w, h, direct)
    torch.cuda.synchronize()
    replay = torch.zeros_like(direct)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.encode_uastc_device(d_img, w, h, replay, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(direct, replay)
    _same(replay.cpu().numpy().reshape(nby, nbx, 16), uc.expected(*case), "graph")


# ---- 7. composition: every target, and image -> file -> read ---------------------------------------------------------------------------------------
ORACLE_TARGETS = {_lib.ASTC: "astc", _lib.BC7: "bc7", _lib.ETC1: "etc1", _lib.ETC2: "etc2"}


@pytest.mark.parametrize("case", [("plain", "random", 255, 9), ("opaque", "gradient", 64, 64), ("grey", "random", 12, 203), ("plain", "solid", 255, 9), "edge-mixed"],
                         ids=lambda c: c if isinstance(c, str) else uc.case_id(c))
def test_every_transcode_target_takes_the_blocks(ctx, oracle, case):
    """the encoder's own output transcodes without an error (one would raise) to all eleven targets -- ten through bu_uastc_transcode, RGBA32 through
    bu_uastc_decode_to_rgba, which is how the library spells that target -- the four targets the oracle has are the oracle's transcode of the same
    blocks, and the RGBA32 image is the oracle's decode"""
    if case == "edge-mixed":
        img = uc.strip(uc.edge_mixed()[0])
        h, w, _ = img.shape
    else:
        _, _, w, h = case
        img = uc.image(*case)
    nbx, nby = ec.blocks_of(w, h)
    blocks = ctx.encode_uastc(img, w, h).copy()
    for t in ALL_TARGETS:
        if t != _lib.RGBA32:
            got = ctx.transcode(t, blocks)
            assert got.size == nbx * nby * _lib.BLOCK_BYTES[t]
            if t in ORACLE_TARGETS:
                st, bad, want = oracle.transcode(ORACLE_TARGETS[t], blocks.tobytes())
                assert st == 0, (ORACLE_TARGETS[t], st, bad)
                assert np.array_equal(got, want), ORACLE_TARGETS[t]
    st, bad, want = oracle.decode_to_rgba(blocks.tobytes(), nbx)
    assert st == 0, (st, bad)
    assert (ctx.decode_to_rgba(blocks, nbx) == want).all()


def test_image_to_basis_file_and_back(ctx):
    import basisu_rs_amd as bu

    case = ("ag", "gradient", 64, 64)
    blocks = ctx.encode_uastc(uc.image(*case), 64, 64).copy()
    f = bu.write_uastc_file([dict(data=blocks.tobytes(), orig_w=64, orig_h=64, nbx=16, nby=16)])
    _, imgs = bu.read_to_rgba(f, ctx)
    assert len(imgs) == 1 and (imgs[0].w, imgs[0].h) == (64, 64)
    assert bytes(imgs[0].data) == ctx.decode_to_rgba(blocks, 16).tobytes()
    bc7 = bu.read_to_bc7(f, ctx)
    assert len(bc7) == 1 and bytes(bc7[0].data) == ctx.transcode(_lib.BC7, blocks).tobytes()
    # and the picture survives: the file's pixels are within the model's error of the source
    back = np.frombuffer(bytes(imgs[0].data), dtype=np.uint8).reshape(64, 64, 4).astype(np.int64)
    assert int(((back - uc.image(*case).astype(np.int64)) ** 2).sum()) == int(uc.fields(*case)["E"].sum())
