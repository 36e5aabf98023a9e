"""UASTC -> BC1 / BC3 on the device, bit for bit against the numpy model of tests/colour_model.py, whose input is the GPU's own RGBA32
output for the same blocks.  Every entry point that takes a bu_target: the host-pointer call, the device-pointer call under the exclusive,
shared and auto policies (slices around the shape changes), the blocking device call, the multi-run batch (mixed and mode-sorted), the
in-flight batch on four streams and the file level (several slices, with and without the alpha flag).  Run on the GPU box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import colour_model as col
import test_colour_targets as tcol
import test_gpu_channel_targets as tgc
from basisu_rs_amd import BasisuError, Decoder, TargetTextureFormat, _lib, synth

pytestmark = pytest.mark.gpu
NAMES = ("bc1", "bc3")
FMT = {"bc1": TargetTextureFormat.Bc1Rgb, "bc3": TargetTextureFormat.Bc3Rgba}
_same = tgc._same
_layout = tgc._layout


@pytest.fixture(scope="module")
def base(golden, oracle, ctx):
    """the CPU sets in one array, and the model's blocks for each target from the device's RGBA32 decode of them"""
    blocks = np.ascontiguousarray(np.concatenate(list(tcol.cpu_sets(golden, oracle).values())))
    rgba = ctx.decode_to_rgba(blocks, 1).reshape(-1, 64)
    want = {n: col.encode(n, rgba) for n in NAMES}
    return blocks, want


@pytest.mark.parametrize("name", NAMES)
def test_host_pointer_call(ctx, base, name):
    blocks, want = base
    got = Decoder(ctx).transcode(FMT[name], blocks).reshape(want[name].shape)
    _same(got, want[name], name)
    pinned = ctx.host_alloc(blocks.shape[0] * _lib.BLOCK_BYTES[int(FMT[name])])  # (page-locked output: the zero-copy launch)
    got = ctx.transcode(FMT[name], blocks, out=pinned).reshape(want[name].shape)
    _same(got, want[name], name + " zero-copy")
    ctx.host_free(pinned)


@pytest.mark.parametrize("name", NAMES)
def test_device_call_every_shape_and_policy(ctx, base, name):
    import torch

    blocks, want = base
    t, bb = int(FMT[name]), _lib.BLOCK_BYTES[int(FMT[name])]
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [1, 9, 1024 * cu, 1024 * cu + 1, 3 * 1024 * cu, 3 * 1024 * cu + 1, 1 << 20, (1 << 20) + 4321]
    g = torch.from_numpy(blocks).cuda()
    for policy in (False, True, "auto"):
        ctx.set_launch_policy(policy)
        for n in sizes:
            idx = _layout(n, blocks.shape[0], synth.block_modes(blocks), False, seed=n)
            d_in = g[torch.from_numpy(idx).cuda()].contiguous()
            d_out = torch.zeros((n, bb), dtype=torch.uint8, device="cuda")
            status = torch.empty(1, dtype=torch.int64, device="cuda")
            ctx.status_word_reset(status)
            ctx.transcode_device(t, d_in, n, d_out, d_status=status)
            torch.cuda.synchronize()
            ctx.status_word_check(int(status.item()))
            _same(d_out.cpu().numpy(), want[name][idx], "%s n=%d policy=%s" % (name, n, policy))
    ctx.set_launch_policy("auto")


@pytest.mark.parametrize("name", NAMES)
def test_device_sync_and_batches(ctx, base, name):
    import torch

    blocks, want = base
    lib = _lib.load()
    t, bb = int(FMT[name]), _lib.BLOCK_BYTES[int(FMT[name])]
    modes = synth.block_modes(blocks)
    g = torch.from_numpy(blocks).cuda()
    n = (1 << 20) + 77
    idx = _layout(n, blocks.shape[0], modes, False, seed=5)
    d_in = g[torch.from_numpy(idx).cuda()].contiguous()
    d_out = torch.zeros((n, bb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the blocking call runs on the context's own stream: d_in and d_out must be complete before it)
    assert ctx.transcode_device_sync(t, d_in, n, d_out) == _lib.STATUS_WORD_CLEAR
    _same(d_out.cpu().numpy(), want[name][idx], name + " sync")
    sizes = [600 * 1024 + 7, 4096, 301 * 1024, 70001, 1 << 19, 2047, 9, 1 << 20]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    VP, SZ = ctypes.c_void_p * len(sizes), ctypes.c_size_t * len(sizes)
    for sort in (False, True):
        idx = _layout(int(offs[-1]), blocks.shape[0], modes, sort, seed=91 + sort)
        d_idx = torch.from_numpy(idx).cuda()
        ins = [g[d_idx[offs[k]:offs[k + 1]]].contiguous() for k in range(len(sizes))]
        for in_flight in (False, True):
            outs = [torch.zeros((s, bb), dtype=torch.uint8, device="cuda") for s in sizes]
            status = torch.empty(1, dtype=torch.int64, device="cuda")
            ctx.status_word_reset(status)
            torch.cuda.synchronize()
            if in_flight:
                ctx.transcode_batch_in_flight(t, ins, sizes, outs, d_status=status, n_streams=4)
                ctx.synchronize()
            else:
                assert lib.bu_uastc_transcode_batch_device(ctx.handle, t, len(sizes), VP(*[x.data_ptr() for x in ins]), SZ(*sizes),
                                                           VP(*[x.data_ptr() for x in outs]), 0, None, ctypes.c_void_p(status.data_ptr()), None) == 0
            torch.cuda.synchronize()
            ctx.status_word_check(int(status.item()))
            _same(np.concatenate([o.cpu().numpy() for o in outs]), want[name][idx], "%s batch sort=%s in_flight=%s" % (name, sort, in_flight))


@pytest.mark.parametrize("alpha", [False, True])
def test_file_level(ctx, base, alpha):
    import basisu_rs_amd as bu

    blocks, want = base
    n0 = 96 * 64
    a, b = blocks[:n0], blocks[n0:n0 + 40 * 32]
    f = bu.write_uastc_file([dict(data=a.tobytes(), orig_w=384, orig_h=256, nbx=96, nby=64),
                             dict(data=b.tobytes(), orig_w=160, orig_h=128, nbx=40, nby=32, image_index=1)], header_flags=4 if alpha else 0)
    for name, fn in (("bc1", bu.read_to_bc1), ("bc3", bu.read_to_bc3)):
        imgs = fn(f, ctx)
        bb = _lib.BLOCK_BYTES[int(FMT[name])]
        assert len(imgs) == 2 and imgs[0].stride == bb * 96 and imgs[1].stride == bb * 40
        _same(np.asarray(imgs[0].data).reshape(-1, bb), want[name][:n0], name + " file slice 0")
        _same(np.asarray(imgs[1].data).reshape(-1, bb), want[name][n0:n0 + 40 * 32], name + " file slice 1")


def test_targets_10_and_13_name_no_target(ctx, golden):
    """the colour targets are 11 and 12: 10 and 13 are rejected at every entry point, and the per-block API has no colour member"""
    lib = _lib.load()
    blocks = np.ascontiguousarray(golden["uastc"][:64])
    out = np.zeros(64 * 64, dtype=np.uint8)
    bad = ctypes.c_uint64(0)
    w = ctypes.c_uint64(0)
    for t in (10, 13):
        assert lib.bu_uastc_transcode(ctx.handle, t, blocks.ctypes.data, blocks.size, out.ctypes.data, out.size, ctypes.byref(bad)) == _lib.ERR_ARGUMENT
        assert lib.bu_uastc_transcode_device(ctx.handle, t, None, 0, None, 0, 0, None, None) == _lib.ERR_ARGUMENT
        assert lib.bu_uastc_transcode_device_sync(ctx.handle, t, None, 0, None, 0, 0, ctypes.byref(w)) == _lib.ERR_ARGUMENT
    ns = ctypes.c_float(0)
    for t in (11, 12):
        assert lib.bu_time_block_api(ctx.handle, t, blocks.ctypes.data, 1, 1, out.ctypes.data, ctypes.byref(ns)) == _lib.ERR_ARGUMENT


@pytest.mark.parametrize("name", NAMES)
def test_invalid_blocks_report_the_lowest(ctx, golden, name):
    import torch

    t, bb = int(FMT[name]), _lib.BLOCK_BYTES[int(FMT[name])]
    e = synth.atlas_err(golden["uastc"], 4096, [3000, 77, 2048])
    with pytest.raises(BasisuError, match="block pattern is not valid|invalid mode index") as ex:
        Decoder(ctx).transcode(FMT[name], e)
    assert ex.value.first_bad_block == 77
    n = (1 << 20) + 5
    bad = [900001, 140001, 300000]
    e = synth.atlas_err(golden["uastc"], n, bad)
    d_in = torch.from_numpy(np.ascontiguousarray(e)).cuda()
    d_out = torch.full((n, bb), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    word = ctx.transcode_device_sync(t, d_in, n, d_out)
    assert word >> 8 == 140001 and (word & 0xFF) in (1, 2)
    out = d_out.cpu().numpy()
    assert (out[bad] == 0).all()
    keep = np.arange(150000, 150000 + 8192)  # (a window of valid blocks: the model over 2^20 blocks is slow on the host)
    rgba = ctx.decode_to_rgba(np.ascontiguousarray(e[keep]), 1).reshape(-1, 64)
    _same(out[keep], col.encode(name, rgba), name + " around invalid blocks")
