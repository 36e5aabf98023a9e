"""The ETC1 colour property of tests/etc_model.py on the device: the mined edge set (every edge class at least MINE_K times) through
UASTC -> ETC1 / ETC2 launches of every shape the dispatcher picks for ETC -- exclusive, shared and auto policies; slices of one and of
three 1024-block tiles per CU and one block more than each, and 2^20 blocks plus a ragged tail (one-tile workgroups); the multi-run
launch of bu_uastc_transcode_batch_device -- in a mixed layout and mode-sorted (whole waves of one mode: the sort's aggregated
atomics).  Every output block is checked by the property itself: the copies of a mined block must all equal one output, and that
output satisfies the property (and equals the oracle's).  Run on the GPU box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import etc_model as em
from basisu_rs_amd import _lib, synth
from oracle.pyoracle import Decoders

pytestmark = pytest.mark.gpu
TB = {"etc1": (_lib.ETC1, 8), "etc2": (_lib.ETC2, 16)}


@pytest.fixture(scope="module")
def dec():
    return Decoders()


@pytest.fixture(scope="module")
def mined(oracle, dec):
    blocks = em.mined_set(oracle, dec)
    rgba, st = oracle.batch("rgba", blocks)
    assert (st == 0).all()
    want = {t: oracle.batch(t, blocks)[0] for t in TB}
    return blocks, rgba, want


def _layout(n, m, modes, sort, seed):
    """indices into the mined set for a slice of n blocks: every mined block at least once, shuffled; sorted by mode if asked"""
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.concatenate([rng.permutation(m) for _ in range(-(-n // m))])[:n]
    if sort:
        idx = idx[np.argsort(modes[idx], kind="stable")]
    return idx


def _check(dec, mined, target, idx, got):
    """every copy of a mined block gave the same bytes, and those bytes satisfy the property (and are the oracle's)"""
    blocks, rgba, want = mined
    uniq, first = np.unique(idx, return_index=True)
    assert uniq.size == blocks.shape[0]
    rep = got[first]
    bad = (got != rep[np.searchsorted(uniq, idx)]).any(axis=1)
    assert not bad.any(), ("copies of one block differ", target, np.nonzero(bad)[0][:8])
    colour = np.ascontiguousarray(rep if target == "etc1" else rep[:, 8:])
    if target == "etc2":
        assert (colour == want["etc1"]).all()
    em.check(blocks, rgba, colour, dec)
    assert (rep == want[target]).all()


@pytest.mark.parametrize("target", ["etc1", "etc2"])
def test_mined_edges_every_policy_and_slice_shape(dec, mined, target):
    import torch

    from basisu_rs_amd import Context

    t, bb = TB[target]
    blocks = mined[0]
    modes = synth.block_modes(blocks)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [1024 * cu, 1024 * cu + 1, 3 * 1024 * cu, 3 * 1024 * cu + 1, (1 << 20) + 4321]
    ctx = Context(0)
    g = torch.from_numpy(blocks).cuda()
    for policy in (False, True, "auto"):
        ctx.set_launch_policy(policy)
        for n in sizes:
            for sort in (False, True):
                idx = _layout(n, blocks.shape[0], modes, sort, seed=n + sort)
                d_in = g[torch.from_numpy(idx).cuda()].contiguous()
                d_out = torch.zeros((n, bb), dtype=torch.uint8, device="cuda")
                status = torch.empty(1, dtype=torch.int64, device="cuda")
                ctx.status_word_reset(status)
                ctx.transcode_device(t, d_in, n, d_out, d_status=status)
                torch.cuda.synchronize()
                ctx.status_word_check(int(status.item()))
                _check(dec, mined, target, idx, d_out.cpu().numpy())
    ctx.close()


@pytest.mark.parametrize("target", ["etc1", "etc2"])
def test_mined_edges_multi_run_launch(ctx, dec, mined, target):
    """bu_uastc_transcode_batch_device: runs in separate allocations, large ones (2048-block tiles, persistent walk) and small ones"""
    import torch

    lib = _lib.load()
    t, bb = TB[target]
    blocks = mined[0]
    modes = synth.block_modes(blocks)
    sizes = [600 * 1024 + 7, 4096, 301 * 1024, 70001, 1 << 19, 2047, 9]
    g = torch.from_numpy(blocks).cuda()
    for sort in (False, True):
        idx = _layout(sum(sizes), blocks.shape[0], modes, sort, seed=91 + sort)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        d_idx = torch.from_numpy(idx).cuda()
        ins = [g[d_idx[offs[k]:offs[k + 1]]].contiguous() for k in range(len(sizes))]
        outs = [torch.zeros((n, bb), dtype=torch.uint8, device="cuda") for n in sizes]
        status = torch.empty(1, dtype=torch.int64, device="cuda")
        ctx.status_word_reset(status)
        torch.cuda.synchronize()
        VP, SZ = ctypes.c_void_p * len(sizes), ctypes.c_size_t * len(sizes)
        assert lib.bu_uastc_transcode_batch_device(ctx.handle, t, len(sizes), VP(*[x.data_ptr() for x in ins]), SZ(*sizes),
                                                   VP(*[x.data_ptr() for x in outs]), 0, None, ctypes.c_void_p(status.data_ptr()), None) == 0
        torch.cuda.synchronize()
        ctx.status_word_check(int(status.item()))
        _check(dec, mined, target, idx, np.concatenate([o.cpu().numpy() for o in outs]))
