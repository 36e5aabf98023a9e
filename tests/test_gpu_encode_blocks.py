"""bu_rgba_encode_blocks / _device on the GPU: an RGBA8 image -> BC4, BC5, EAC R11, EAC RG11, BC1 or BC3 blocks.

The pinned yardstick is identity with the transcoder: encoding the RGBA32 unpack of a UASTC block gives the bytes the UASTC transcode to that format
gives.  Everything else is compared with the numpy models on images cut into blocks after replication padding (tests/encode_cases.py), on the shapes
where the kernel can go wrong: partial blocks, waves that straddle block rows, unaligned bases and pitches (the 4-byte load path), a second
grid-stride step; with guard bands around both buffers, refusals that must leave the output alone, an exact round trip, and a graph capture."""
import ctypes

import numpy as np
import pytest

import encode_cases as ec
import gpu_guard as gg
from basisu_rs_amd import BasisuError, _lib

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _encode_device(ctx, name, img, in_pad=0, out_pad_blocks=0, base_off=0, pad_seed=0, stream=None):
    """blocks [nby, nbx, bb] of the device form.  The image sits base_off bytes past an allocation's start with rows 4 w + in_pad apart, seeded random
    bytes in the padding; the output has out_pad_blocks blocks of padding per row, which must come back untouched"""
    import torch

    t, bb = ec.FORMATS[name]
    h, w, _ = img.shape
    nbx, nby = ec.blocks_of(w, h)
    in_pitch, out_pitch = 4 * w + in_pad, (nbx + out_pad_blocks) * bb
    fill = np.random.default_rng(pad_seed).integers(0, 256, size=ec.image_bytes(w, h, in_pitch), dtype=np.uint8)
    d_in = torch.zeros(base_off + fill.size, dtype=torch.uint8, device="cuda")
    d_in[base_off:] = torch.from_numpy(ec.pitched(img, in_pitch, fill)).cuda()
    d_out = torch.full((nby * out_pitch,), POISON, dtype=torch.uint8, device="cuda")
    ctx.encode_blocks_device(t, d_in[base_off:], w, h, d_out, in_pitch=in_pitch if in_pad else 0, out_pitch=out_pitch if out_pad_blocks else 0, stream=stream)
    torch.cuda.synchronize()
    rows = d_out.cpu().numpy().reshape(nby, out_pitch)
    assert (rows[:, nbx * bb:] == POISON).all(), "%s: the out_pitch padding was written" % name
    return rows[:, : nbx * bb].reshape(nby, nbx, bb)


def _same(got, want, what):
    bad = np.argwhere((got != want).any(-1))
    assert bad.size == 0, "%s: %d blocks differ, first (by, bx) %s: got %s, want %s" % (what, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])].tolist(),
                                                                                       want[tuple(bad[0])].tolist())


# ---- 1. identity with the transcoder ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_rows(ctx, golden):
    """the golden UASTC vectors, 64 blocks per row (the first 32 repeated to fill the tenth row), and their RGBA32 unpack [40, 256, 4]"""
    uastc = np.concatenate([golden["uastc"], golden["uastc"][:32]])
    assert uastc.shape == (640, 16)
    rgba = ctx.decode_to_rgba(uastc, 64).copy().reshape(40, 256, 4)
    return uastc, rgba


@pytest.mark.parametrize("name", list(ec.FORMATS))
def test_identity_with_the_transcoder(ctx, golden_rows, name):
    """encode_blocks(fmt, decode_to_rgba(uastc, 64)) == transcode(fmt, uastc), byte for byte: host form (pageable and page-locked) and device form"""
    uastc, rgba = golden_rows
    t, bb = ec.FORMATS[name]
    want = ctx.transcode(t, uastc).copy().reshape(10, 64, bb)
    _same(ctx.encode_blocks(t, rgba, 256, 40).reshape(10, 64, bb), want, name + " host form")
    pin_in, pin_out = ctx.host_alloc(rgba.size), ctx.host_alloc(640 * bb)
    try:
        pin_in[:] = rgba.reshape(-1)
        pin_out[:] = POISON
        _same(ctx.encode_blocks(t, pin_in, 256, 40, out=pin_out).reshape(10, 64, bb), want, name + " host form, page-locked")
    finally:
        ctx.host_free(pin_in)
        ctx.host_free(pin_out)
    _same(_encode_device(ctx, name, rgba), want, name + " device form")
    _same(_encode_device(ctx, name, rgba, in_pad=4, out_pad_blocks=3), want, name + " device form, 4-byte loads")


# ---- 2. the models on shapes where the kernel can go wrong -------------------------------------------------------------------------------------
# (in_pad, out_pad_blocks, base_off): tight; an unaligned pitch (the fast path off) with a padded output; an aligned padded pitch; a base 4 bytes
# past 16-byte alignment (the fast path off with a tight pitch -- what 1024 x 4 is listed for, run on every shape)
LAYOUTS = ((0, 0, 0), (4, 3, 0), (64, 0, 0), (0, 0, 4))


@pytest.mark.parametrize("shape", list(ec.SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(ec.FORMATS))
def test_models_on_the_shapes(ctx, name, shape):
    w, h = shape
    t, bb = ec.FORMATS[name]
    for k, kind in enumerate(ec.KINDS):
        want = ec.expected(name, kind, w, h)
        for in_pad, out_pad, off in LAYOUTS:
            got = _encode_device(ctx, name, ec.image(kind, w, h), in_pad, out_pad, off, pad_seed=10 * k + in_pad)
            _same(got, want, "%s %s %dx%d layout %s" % (name, kind, w, h, (in_pad, out_pad, off)))
    # the host form reads a pitched image too; its output is tight
    pitch = 4 * w + 4
    buf = ec.pitched(ec.image("random", w, h), pitch, np.full(ec.image_bytes(w, h, pitch), 0x3C, dtype=np.uint8))
    _same(ctx.encode_blocks(t, buf, w, h, in_pitch=pitch).reshape(want.shape), ec.expected(name, "random", w, h), "%s %dx%d host form" % (name, w, h))


# ---- 3. a second grid-stride step --------------------------------------------------------------------------------------------------------------
def _cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name", ["bc1", "rg11"])
def test_second_grid_stride_step(ctx, name):
    """8 * CUs * 256 + 65 blocks or a little more: the grid is capped at 8 workgroups per CU, so some lanes take a second block; the image is a
    64 x 64-pixel pattern tiled, two pixels short of a multiple of four wide, on a 16-byte-aligned pitch (the 16-byte loads, the last column clamped)"""
    import torch

    t, bb = ec.FORMATS[name]
    TX = 8
    TY = -(-(8 * _cu_count() * 256 + 65) // (256 * TX))
    w, h = 64 * TX - 2, 64 * TY
    nbx, nby = ec.blocks_of(w, h)
    assert nbx * nby >= 8 * _cu_count() * 256 + 65 and w % 4 != 0
    pat = ec.image("random", 64, 64, seed=3)
    tile = ec.expected(name, "random", 64, 64, seed=3)  # [16, 16, bb]
    edge = ec.model(name, ec.to_blocks(pat[:, 60:62])).reshape(16, 1, bb)  # the partial last column: pattern columns 60, 61, 61, 61
    want = np.tile(tile, (TY, TX, 1))
    want[:, -1:] = np.tile(edge, (TY, 1, 1))
    d_img = torch.from_numpy(pat.copy()).cuda().repeat(TY, TX, 1).contiguous()  # [h, 64 TX, 4]: the pitch of the whole tiles, two columns unused
    d_out = torch.full((nbx * nby * bb,), POISON, dtype=torch.uint8, device="cuda")
    ctx.encode_blocks_device(t, d_img, w, h, d_out, in_pitch=4 * 64 * TX)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy().reshape(nby, nbx, bb), want, name + " second step")


# ---- 4. guard bands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.FORMATS))
def test_guard_bands_and_pitch_padding(ctx, name):
    """the image ends at its last pixel with a band right behind it; two runs whose bands and pitch padding hold different bytes give identical blocks,
    the output's bands and out_pitch padding keep their fill"""
    import torch

    t, bb = ec.FORMATS[name]
    for (w, h, in_pad, off) in ((255, 9, 64, 0), (257, 8, 4, 4), (5, 3, 12, 8)):
        nbx, nby = ec.blocks_of(w, h)
        in_pitch, out_pitch = 4 * w + in_pad, (nbx + 3) * bb
        n_in = ec.image_bytes(w, h, in_pitch)
        img = ec.image("random", w, h)
        runs = []
        for r in range(2):
            a_in = gg.Arena("%s image run %d" % (name, r), n_in, gg.GUARD_MIN + 4096 * r, offsets=off)
            a_out = gg.Arena("%s blocks run %d" % (name, r), nby * out_pitch, gg.GUARD_MIN, offsets=0 if bb == 16 else 8)
            reg = a_in.regions[0]
            fill = gg.fill_bytes(np, reg.start, reg.stop)  # the arena's own fill runs on through the padding
            if r:
                fill = fill ^ 0xFF
            a_in.data()[:] = torch.from_numpy(ec.pitched(img, in_pitch, fill)).cuda()
            oreg = a_out.regions[0]
            ofill = gg.fill_bytes(np, oreg.start, oreg.stop)
            a_out.data()[:] = torch.from_numpy(ofill).cuda()
            ctx.encode_blocks_device(t, a_in.ptr(), w, h, a_out.ptr(), in_pitch=in_pitch, out_pitch=out_pitch)
            torch.cuda.synchronize()
            a_in.check()
            a_out.check()
            rows = a_out.data().cpu().numpy().reshape(nby, out_pitch)
            assert (rows[:, nbx * bb:] == ofill.reshape(nby, out_pitch)[:, nbx * bb:]).all(), "%s %dx%d: the out_pitch padding was written" % (name, w, h)
            runs.append(rows[:, : nbx * bb].reshape(nby, nbx, bb).copy())
        _same(runs[0], ec.expected(name, "random", w, h), "%s %dx%d guarded" % (name, w, h))
        assert (runs[0] == runs[1]).all(), "%s %dx%d: the blocks depend on bytes outside the image" % (name, w, h)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(ctx):
    import torch

    w, h = 32, 8
    d_in = torch.zeros(4 * w * h + 256, dtype=torch.uint8, device="cuda")
    d_out = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda")
    pi, po = d_in.data_ptr(), d_out.data_ptr()
    lib, handle = ctx._lib, ctx.handle

    def call(c=handle, fmt=_lib.BC3_RGBA, src=pi, w=w, h=h, in_pitch=0, dst=po, out_pitch=0):
        return lib.bu_rgba_encode_blocks_device(c, fmt, src, w, h, in_pitch, dst, out_pitch, None)

    rows = [dict(fmt=f) for f in ec.OTHER_FORMATS] + [dict(c=None), dict(src=None), dict(dst=None), dict(src=pi + 2), dict(dst=po + 8),
            dict(fmt=_lib.BC1_RGB, dst=po + 4), dict(in_pitch=4 * w - 4), dict(in_pitch=4 * w + 2), dict(out_pitch=16 * 8 - 16), dict(out_pitch=16 * 8 + 8),
            dict(w=(1 << 30) + 1)]
    for row in rows:
        assert call(**row) == _lib.ERR_ARGUMENT, row
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())
    # an empty image is BU_OK and launches nothing
    for row in (dict(w=0), dict(h=0), dict(w=0, h=0, src=None, dst=None)):
        assert call(**row) == _lib.OK, row
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())
    assert ctx.encode_blocks(_lib.BC1_RGB, np.zeros(0, dtype=np.uint8), 0, 7).size == 0
    # the Python layer raises what the library returns
    with pytest.raises(BasisuError) as e:
        ctx.encode_blocks_device(_lib.BC7, d_in, w, h, d_out)
    assert e.value.status == _lib.ERR_ARGUMENT
    img = np.zeros(4 * w * h, dtype=np.uint8)
    for fmt in ec.OTHER_FORMATS:
        with pytest.raises(BasisuError) as e:
            ctx.encode_blocks(fmt, img, w, h)
        assert e.value.status == _lib.ERR_ARGUMENT, fmt
    out = np.full(16 * 8 * 2 - 1, POISON, dtype=np.uint8)
    with pytest.raises(BasisuError) as e:
        ctx.encode_blocks(_lib.BC3_RGBA, img, w, h, out=out)
    assert e.value.status == _lib.ERR_OUTPUT_SIZE and (out == POISON).all()
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all())


# ---- 6. a round trip that is exact by derivation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bc4", "bc5"])
def test_solid_round_trip(ctx, name):
    """a solid block of value v is mx = mn = v with every selector 0, which decodes to v exactly"""
    t, bb = ec.FORMATS[name]
    for v in (0, 1, 127, 255):
        img = np.empty((8, 12, 4), dtype=np.uint8)
        img[..., 0], img[..., 1], img[..., 2], img[..., 3] = v, 77, 99, 255 - v
        blocks = ctx.encode_blocks(t, img, 12, 8)
        b = blocks.reshape(-1, 8)
        ch = [v] if name == "bc4" else [v, 255 - v]
        assert (b[:, 0] == np.tile(ch, b.shape[0] // len(ch))).all() and (b[:, 1] == b[:, 0]).all() and not b[:, 2:].any(), (name, v)
        back = ctx.decode_blocks(t, blocks, 3).reshape(8, 12, 4)
        assert (back[..., 0] == v).all() and (back[..., 3] == 255).all() and (back[..., 2] == 0).all(), (name, v)
        assert (back[..., 1] == (0 if name == "bc4" else 255 - v)).all(), (name, v)


# ---- 7. graph capture --------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_equals_the_direct_call(ctx):
    import torch

    t, bb = ec.FORMATS["bc1"]
    w, h = 257, 8
    nbx, nby = ec.blocks_of(w, h)
    d_img = torch.from_numpy(ec.image("random", w, h).copy()).cuda()
    direct = torch.zeros(nbx * nby * bb, dtype=torch.uint8, device="cuda")
    ctx.encode_blocks_device(t, d_img, w, h, direct)
    torch.cuda.synchronize()
    replay = torch.zeros_like(direct)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.encode_blocks_device(t, d_img, w, h, replay, stream=s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(direct, replay)
    _same(replay.cpu().numpy().reshape(nby, nbx, bb), ec.expected("bc1", "random", w, h), "bc1 graph")
