"""The multi-run BC7 / ASTC persistent kernels issue a tile's result stores LAST in its iteration: the results wait in registers while the next tile's sort keys
and the drawn ticket are taken (bu_kernels.hpp, STORES_LAST).  What could go wrong is a result that crosses the loop edge into the wrong tile, or one lost at a
workgroup's first or last tile -- so every case is a walk of SEVERAL tiles per workgroup, sized from the device's CU count.  The one-slice kernels share the loop
and keep the plain tail: the same walks over one slice hold that they still do.

Inputs are gathered on the device from the 608 known-answer vectors by a seeded index, the expected bytes are the same gather of the golden results.
Every case runs in a child process (this file, run as a script): BU_TILE_TICKETS is read once per process, and the fixed walk needs it at 0."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024


def _setup(target):
    import torch

    from basisu_rs_amd import Context, _lib, synth

    golden = synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin"))
    gu, gt = torch.from_numpy(golden["uastc"]).cuda(), torch.from_numpy(golden[target]).cuda()
    ctx = Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return torch, ctx, {"bc7": _lib.BC7, "astc": _lib.ASTC}[target], gu, gt, cus


def _gather(torch, gu, n, seed):
    idx = torch.randint(0, 608, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    return idx, gu[idx].contiguous()


def case_one_slice(target, walk):
    """one slice: `walk` tiles per workgroup slot of the largest persistent shape (five per CU), once as whole rectangles of a 1024-block pitch and once as strips
    with a ragged last tile"""
    torch, ctx, t, gu, gt, cus = _setup(target)
    walk = float(walk)
    tiles = int(walk * 5 * cus) // 16 * 16  # (whole rows of 16 rectangular tiles)
    for n, bpr in ((tiles * TILE, 1024), (tiles * TILE - 37, 0)):
        idx, d_in = _gather(torch, gu, n, 5)
        out = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.transcode_device(t, d_in, n, out, blocks_per_row=bpr)
        torch.cuda.synchronize()
        assert torch.equal(out, gt[idx]), (target, n, bpr)
    ctx.close()


def _batch(torch, ctx, t, ins, sizes, outs, bpr, status, sp):
    n = len(sizes)
    VP, SZ = ctypes.c_void_p * n, ctypes.c_size_t * n
    st = ctx._lib.bu_uastc_transcode_batch_device(ctx.handle, t, n, VP(*[x.data_ptr() for x in ins]), SZ(*sizes), VP(*[x.data_ptr() for x in outs]), bpr, None,
                                                  ctypes.c_void_p(status.data_ptr()), sp)
    assert st == 0


def case_multi_run(target, walk, whole):
    """three runs in separate allocations, `walk` tiles per slot of a five-per-CU grid in all: whole rectangles / (mixed: smaller than a tile) / (mixed: a ragged end).
    Known answers; then the same launch twice back to back on one stream into different outputs; then failing blocks in two runs -- in the first tile a workgroup
    walks, in a middle one and in its last: the lowest one comes back, their outputs are zeros, every other block is right"""
    from basisu_rs_amd import BasisuError

    torch, ctx, t, gu, gt, cus = _setup(target)
    whole = whole == "whole"
    tiles = int(float(walk) * 5 * cus)
    a = tiles // 2 // 16 * 16
    sizes = [a * TILE, (tiles // 4 // 16 * 16) * TILE if whole else 700, (tiles - a) // 16 * 16 * TILE - (0 if whole else 333)]
    gathered = [_gather(torch, gu, n, 11 + k) for k, n in enumerate(sizes)]
    idxs, ins = [g[0] for g in gathered], [g[1] for g in gathered]
    outs = [[torch.zeros((n, 16), dtype=torch.uint8, device="cuda") for n in sizes] for _ in range(2)]
    status = torch.empty(1, dtype=torch.int64, device="cuda")
    ctx.status_word_reset(status)
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    _batch(torch, ctx, t, ins, sizes, outs[0], 1024, status, sp)
    _batch(torch, ctx, t, ins, sizes, outs[1], 1024, status, sp)  # back to back: the ticket counters were reset by the first launch's last workgroup
    torch.cuda.synchronize()
    ctx.status_word_check(int(status.item()))
    for o in outs:
        for k in range(3):
            assert torch.equal(o[k], gt[idxs[k]]), (target, k)
    # failing blocks (an invalid mode byte).  Run 0: tile `grid + 3` is some workgroup's second tile at the earliest, the last tile of the run is late in every walk;
    # run 2: its first block sits in the middle of the launch's tile sequence, its last block in the launch's last tile
    bad = [(0, 5), (0, (5 * cus + 3) * TILE + 17), (0, sizes[0] - 1), (2, 0), (2, sizes[2] - 1)]
    want = [gt[i].clone() for i in idxs]
    for k, b in bad:
        ins[k][b, 0] = 69
        want[k][b] = 0
    for o in outs[0]:
        o.fill_(0xEE)
    torch.cuda.synchronize()
    _batch(torch, ctx, t, ins, sizes, outs[0], 1024, status, sp)
    torch.cuda.synchronize()
    with pytest.raises(BasisuError) as e:
        ctx.status_word_check(int(status.item()))
    assert e.value.first_bad_block == 5
    for k in range(3):
        assert torch.equal(outs[0][k], want[k]), (target, k)
    # ... and with the lowest one healed the next lowest is reported: a failing block in a workgroup's later tiles
    ins[0][5] = gu[idxs[0][5]]
    want[0][5] = gt[idxs[0][5]]
    torch.cuda.synchronize()
    ctx.status_word_reset(status, stream=s)
    _batch(torch, ctx, t, ins, sizes, outs[1], 1024, status, sp)
    torch.cuda.synchronize()
    with pytest.raises(BasisuError) as e:
        ctx.status_word_check(int(status.item()))
    assert e.value.first_bad_block == (5 * cus + 3) * TILE + 17
    for k in range(3):
        assert torch.equal(outs[1][k], want[k]), (target, k)
    ctx.close()


CASES = {"one_slice": case_one_slice, "multi_run": case_multi_run}


def _child(case, *args, tickets=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    if not tickets:
        env["BU_TILE_TICKETS"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["bc7", "astc"])
def test_one_slice_fixed_walk_of_two_and_three_tiles(target):
    _child("one_slice", target, 2.5, tickets=False)


@pytest.mark.gpu
@pytest.mark.parametrize("target", ["bc7", "astc"])
def test_one_slice_just_over_the_ticket_threshold(target):
    _child("one_slice", target, 16.2)


@pytest.mark.gpu
@pytest.mark.parametrize("whole", ["whole", "mixed"])
@pytest.mark.parametrize("tickets", [False, True])
@pytest.mark.parametrize("target", ["bc7", "astc"])
def test_multi_run_first_middle_and_last_tiles(target, tickets, whole):
    # (mixed runs walk as four workgroups per CU: 16.2 x 5 tiles per CU is over their ticket threshold too)
    _child("multi_run", target, 16.2 if tickets else 2.5, whole, tickets=tickets)


if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
