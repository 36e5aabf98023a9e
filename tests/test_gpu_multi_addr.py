"""Multi-run launches whose workgroups walk from run to run: the kernels address every tile from its corner (a wave-uniform base) with 32-bit lane offsets that
hang on the run's width, keep the run they are walking in registers and look the table up only when a tile lies outside it (csrc/bu_multi_addr.hpp).  Each case
is ONE bu_uastc_transcode_batch_device call under the exclusive policy; inputs are the 608 known-answer vectors gathered by a seeded index, expected bytes the
same gather of the golden results, and every run sits between guard bands (tests/gpu_guard.py): invalid blocks around the inputs, a checked fill around the
outputs."""
import ctypes

import numpy as np
import pytest

import gpu_guard as gg
import guard_cases as gc

pytestmark = pytest.mark.gpu
CLEAR = 0xFFFFFFFFFFFFFFFF
SMALL = (65536, 4096, 8192, 16384)  # whole rectangles at the virtual pitches 1024, 256, 512, 1024: 64, 4, 8 and 16 tiles


@pytest.fixture(scope="module")
def env(golden, ctx):
    """the 608 vectors and the expected blocks of the three targets on the device (computed once, never written)"""
    import torch

    return dict(torch=torch, ctx=ctx, cus=torch.cuda.get_device_properties(0).multi_processor_count, gu=torch.from_numpy(golden["uastc"]).cuda(),
                want={k: torch.from_numpy(np.ascontiguousarray(golden[k])).cuda() for k in ("astc", "bc7", "etc1")})


def _tiles(sizes):
    return sum((n + 1023) // 1024 for n in sizes)


def _run_batch(e, name, sizes, offset16=False, plant=None):
    """runs of `sizes` blocks in one call; offset16: every run starts 16 bytes past a 256-byte boundary (inside the arena: no page alignment);
    plant = (run, block): an invalid mode code there -- the status word must name bases[run] + block and the block's result is zeros"""
    torch, ctx = e["torch"], e["ctx"]
    t, bb_ = gc.TARGETS[name]
    k = len(sizes)
    ofs = 16 if offset16 else 0
    ain = gg.Arena(name + " input", [16 * n for n in sizes], gg.POISON_BLOCKS * 16, [ofs] * k, fill="uastc")
    aout = gg.Arena(name + " output", [bb_ * n for n in sizes], gg.guard_bytes(bb_, 2048 if name in gc.ETC_FAMILY else 1024), [ofs] * k)
    assert not offset16 or all(ain.ptr(i) % 256 == 16 and aout.ptr(i) % 256 == 16 for i in range(k))
    idxs = []
    for i, n in enumerate(sizes):
        idx = torch.randint(0, 608, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(900 + i))
        ain.data(i).view(n, 16)[:] = e["gu"][idx]
        aout.data(i).fill_(0xEE)
        idxs.append(idx)
    bases = [(i + 1) << 33 for i in range(k)]  # far apart and above 2^32: base + index, in 64 bits
    if plant:
        ain.data(plant[0]).view(-1, 16)[plant[1], 0] = 69
    status = torch.empty(1, dtype=torch.int64, device="cuda")
    ctx.status_word_reset(status)
    VP, SZ, U64 = ctypes.c_void_p * k, ctypes.c_size_t * k, ctypes.c_uint64 * k
    ctx.set_launch_policy(False)  # exclusive
    try:
        torch.cuda.synchronize()
        st = ctx._lib.bu_uastc_transcode_batch_device(ctx.handle, t, k, VP(*[ain.ptr(i) for i in range(k)]), SZ(*sizes), VP(*[aout.ptr(i) for i in range(k)]), 0,
                                                      U64(*bases), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        ctx.set_launch_policy("auto")  # (the context is the session's)
    assert st == 0
    word = int(status.item()) & CLEAR
    if plant:
        assert word != CLEAR and word >> 8 == bases[plant[0]] + plant[1], (name, hex(word), hex(bases[plant[0]] + plant[1]))
    else:
        assert word == CLEAR, (name, hex(word))
    for i, n in enumerate(sizes):
        want = e["want"][name][idxs[i]]
        if plant and plant[0] == i:
            want[plant[1]] = 0
        assert torch.equal(aout.data(i), want.reshape(-1)), (name, i, n)
    ain.check()
    aout.check()


@pytest.mark.parametrize("name", ["bc7", "astc", "etc1"])
def test_fixed_walk_across_runs_of_different_widths(env, name):
    sizes = [SMALL[i % 4] for i in range(60)]
    assert _tiles(sizes) == 1380 and 5 * env["cus"] < 1380 < 16 * 4 * env["cus"]  # a second tile per workgroup, no tickets
    _run_batch(env, name, sizes)


@pytest.mark.parametrize("name", ["bc7", "astc"])
def test_ticketed_walk_over_unaligned_runs(env, name):
    sizes = []
    for i in range(20):
        sizes += [1 << 20, SMALL[i % 4]]
    assert _tiles(sizes) > 20480
    _run_batch(env, name, sizes, offset16=True)


@pytest.mark.parametrize("name", ["bc7", "astc"])
def test_a_different_run_for_nearly_every_tile(env, name):
    sizes = [4096] * 45 + [1 << 20] + [4096] * 45
    assert _tiles(sizes) == 1384
    _run_batch(env, name, sizes)


@pytest.mark.parametrize("name", ["bc7", "astc"])
def test_strips_with_ragged_ends(env, name):
    sizes = [5000, 70001, 1025, 262143] * 4
    assert _tiles(sizes) > 1024
    _run_batch(env, name, sizes)  # (the fill behind every run's output and the invalid blocks behind every input: the arenas' check)


@pytest.mark.parametrize("name", ["bc7", "astc"])
def test_a_failing_block_is_named_by_base_plus_index(env, name):
    sizes = [SMALL[i % 4] for i in range(60)]
    _run_batch(env, name, sizes, plant=(29, sizes[29] - 1))  # the last block of a middle run
