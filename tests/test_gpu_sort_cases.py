"""Chosen per-tile mode histograms through every mode-sorted kernel.  The other GPU tests feed the kernels a uniform mode mix or long single-mode stretches; here
every tile of every launch is laid out by a recipe of tests/sort_cases.py -- one key, run lengths of 63 / 64 / 65 blocks, all 20 runs, the largest chunk count,
whole waves of invalid mode codes, a uniform mix followed by a single key -- so that the counting sort's rank paths, its run and chunk map, run 19 and the
hand-over between the tiles of a walk are exercised on purpose (tests/test_sort_cases.py holds, without a GPU, that each recipe reaches its edge in the shape
the launch plan picks, and that the cases reach every kernel).

Inputs are gathers of a pool of blocks (the 608 known-answer vectors, invalid mode codes, out-of-range patterns), expected bytes the same gather of the pool's
expected blocks: the known answers, the numpy models of the known-answer RGBA32 (the six targets encoded after the unpack), zeros for failing blocks.  Every
case asserts every output byte and the exact status word: clear, or the lowest failing block and its status.  Run on the GPU box: pytest -m gpu.

The ticketed sizes also run in a child process (this file, run as a script) with BU_TILE_TICKETS=0: the variable is read once per process."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sort_cases as sc  # noqa: E402
import test_channel_targets as tct  # noqa: E402
import test_etc1s_targets as tet  # noqa: E402

BASE = 1000  # block_index_base of the blocking call
GAP = 4096   # bytes between two runs of a batch: runs that touch would be merged into one


def make_env(golden, ctx):
    """the pool and every target's expected pool blocks on the device (computed once, never written), the plan library, the targets' sort tables"""
    import torch

    lib = ctypes.CDLL(os.path.join(tct.HOST_EMUL, "libbu_emul.so"))
    I64P, U64P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)
    lib.bu_emul_launch_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_uint, I64P,
                                        ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    lib.bu_emul_launch_plan.restype = ctypes.c_size_t
    lib.bu_emul_runs_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, U64P, U64P, ctypes.POINTER(ctypes.c_size_t), U64P, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_uint, I64P, ctypes.c_size_t, I64P, ctypes.c_size_t]
    lib.bu_emul_runs_plan.restype = ctypes.c_size_t
    pool, pool_st = sc.pool_blocks(golden["uastc"])
    want = {name: sc.pool_expected(golden[name] if name in golden else tet.model(name, golden["rgba"])) for name in sc.ALL}
    return dict(torch=torch, ctx=ctx, lib=lib, cus=torch.cuda.get_device_properties(0).multi_processor_count, pool=torch.from_numpy(pool).cuda(), pool_host=pool,
                pool_st=pool_st, want={k: torch.from_numpy(v).cuda() for k, v in want.items()}, want_host=want, tables={name: sc.Tables(lib, name) for name in sc.ALL})


@pytest.fixture(scope="module")
def env(golden, ctx, emul):  # (emul: the host build exists)
    return make_env(golden, ctx)


def _rows(blocks, bpr):
    """RGBA32 blocks [n, 64] (four rows of 16 bytes each) -> the row-major image of bpr blocks per row, flat"""
    n = blocks.shape[0]
    return blocks.reshape(n // bpr, bpr, 4, 16).permute(0, 2, 1, 3).reshape(-1)


def _expected(e, name, d_idx, bpr):
    w = e["want"][name][d_idx]
    return _rows(w, bpr) if name == "rgba" else w.reshape(-1)


def _first_failure(e, d_idx):
    """(lowest failing block, its status) of blocks pool[d_idx], or None"""
    torch = e["torch"]
    if "pool_st_dev" not in e:
        e["pool_st_dev"] = torch.from_numpy(e["pool_st"]).cuda()
    bad = torch.nonzero(e["pool_st_dev"][d_idx])
    if bad.numel() == 0:
        return None
    i = int(bad[0, 0].item())
    return i, int(e["pool_st"][int(d_idx[i].item())])


def _word_of(first, base=0):
    return sc.CLEAR if first is None else ((base + first[0]) << 8) | first[1]


def _status_tensor(e):
    st = e["torch"].empty(1, dtype=e["torch"].int64, device="cuda")
    e["ctx"].status_word_reset(st)
    return st


def _index(e, name, c, n, tiles):
    """the pool indices of a case's blocks on the device: tiles laid out by their recipes on the host, the halves of a ticketed size by the device"""
    torch, tb = e["torch"], e["tables"][name]
    if c["content"][0] == "halves":
        return sc.halves_index(tb, c["content"], n, xp=torch, device="cuda")
    return torch.from_numpy(sc.fill_tiles(tb, tiles(), c["content"], c["last"], n)).cuda()


# ---- bu_uastc_transcode_device, bu_uastc_transcode_device_sync, host pointers ----------------------------------------------------------
def _healed(e, name, d_idx, d_in, first):
    """the lowest failing block replaced by a valid one"""
    good = int(e["tables"][name].cost_order[0]) * 32
    d_idx[first[0]] = good
    d_in[first[0]] = e["pool"][good]


def run_one_slice(e, name, c):
    torch, ctx, cus = e["torch"], e["ctx"], e["cus"]
    t, bb_ = sc.TARGETS[name]
    n, bpr = sc.size_of(c, name, cus), sc.pitch_of(c, name, cus)
    status = _status_tensor(e)
    for policy in c["policies"]:
        pol, auto = sc.POLICY_ARGS[policy]
        rows = tct._slice_plan(e["lib"], t, n, bpr, sc.grid_cap_of(c), pol, auto, cus)
        d_idx = _index(e, name, c, n, lambda: sc.slice_tiles(rows))
        d_in = e["pool"][d_idx]
        out = torch.empty(n * bb_, dtype=torch.uint8, device="cuda")
        ctx.set_launch_policy({sc.EXCL: False, sc.SHARED: True, sc.AUTO: "auto"}[policy])
        for step in range(2 if c["heal"] else 1):
            what = (name, c["id"], n, bpr, policy, step)
            first = _first_failure(e, d_idx)
            if step:
                assert first is not None, what
                _healed(e, name, d_idx, d_in, first)
                again = _first_failure(e, d_idx)
                assert again is not None and again[0] > first[0], what  # (another failure is left to report)
                first = again
            want = _expected(e, name, d_idx, bpr)
            out.fill_(0xEE)
            torch.cuda.synchronize()
            if c["entry"] == "sync":
                word = ctx.transcode_device_sync(t, d_in, n, out, bpr, BASE)
                assert word == _word_of(first, BASE), what + (hex(word),)
            else:
                ctx.status_word_reset(status)
                ctx.transcode_device(t, d_in, n, out, bpr, 0, status)
                torch.cuda.synchronize()
                word = int(status.item()) & sc.CLEAR
                assert word == _word_of(first), what + (hex(word),)
            assert torch.equal(out, want), what
    ctx.set_launch_policy("auto")


def run_pinned(e, name, c):
    """Context.transcode / decode_to_rgba into a page-locked out=: the kernels store over PCIe, 64 workgroups walking the tiles"""
    from basisu_rs_amd import BasisuError, _lib

    ctx, cus = e["ctx"], e["cus"]
    t, bb_ = sc.TARGETS[name]
    n, bpr = sc.size_of(c, name, cus), sc.pitch_of(c, name, cus)
    rows = tct._slice_plan(e["lib"], t, n, bpr, sc.grid_cap_of(c), 0, 0, cus)
    idx = sc.fill_tiles(e["tables"][name], sc.slice_tiles(rows), c["content"], c["last"], n)
    data = np.ascontiguousarray(e["pool_host"][idx])
    want = e["want_host"][name][idx]
    want = want.reshape(n // bpr, bpr, 4, 16).transpose(0, 2, 1, 3).reshape(-1) if name == "rgba" else want.reshape(-1)
    out = ctx.host_alloc(bb_ * n)
    try:
        out[:] = 0xEE
        word = sc.expected_word(e["pool_st"], idx)
        call = (lambda: ctx.decode_to_rgba(data, bpr, out=out)) if name == "rgba" else (lambda: ctx.transcode(t, data, out=out))
        if word == sc.CLEAR:
            assert (call() == want).all(), (name, c["id"])
        else:  # (the contents of `out` are unspecified after an error)
            with pytest.raises(BasisuError) as err:
                call()
            assert err.value.first_bad_block == word >> 8, (name, c["id"])
            assert err.value.status == {sc.ST_BAD_MODE: _lib.ERR_INVALID_MODE, sc.ST_BAD_PATTERN: _lib.ERR_INVALID_PATTERN}[word & 0xFF], (name, c["id"])
    finally:
        ctx.host_free(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.ALL)
def test_one_tile_of_every_recipe(env, name):
    cases = [c for c in sc.cases_for(name, "device", ticketed=False) if c["id"].startswith("one_tile")]
    assert len(cases) == len(sc.FULL) + len(sc.RAGGED)
    for c in cases:
        run_one_slice(env, name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.ALL)
def test_device_call_over_the_launch_shapes(env, name):
    cases = [c for c in sc.cases_for(name, "device", ticketed=False) if not c["id"].startswith("one_tile")]
    assert sum(c["heal"] for c in cases) == 1 and any(len(c["policies"]) == 3 for c in cases)
    try:
        for c in cases:
            run_one_slice(env, name, c)
    finally:  # (the context is the session's)
        env["ctx"].set_launch_policy("auto")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.ALL)
def test_blocking_device_call(env, name):
    cases = sc.cases_for(name, "sync")
    assert len(cases) == 1
    run_one_slice(env, name, cases[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.ALL)
def test_page_locked_out_walks_the_tiles_on_64_workgroups(env, name):
    cases = sc.cases_for(name, "pinned")
    assert len(cases) == 2
    for c in cases:
        run_pinned(env, name, c)


# ---- bu_uastc_transcode_batch_device ------------------------------------------------------------------------------------------------
def _carve(torch, sizes_bytes):
    """one allocation cut into regions GAP bytes apart, each 256-byte aligned"""
    starts, pos = [], 0
    for s in sizes_bytes:
        starts.append(pos)
        pos += -(-(s + GAP) // 256) * 256
    buf = torch.empty(pos, dtype=torch.uint8, device="cuda")
    return buf, [buf[a:a + s] for a, s in zip(starts, sizes_bytes)]


def run_batch(e, name, b):
    """every run a region of its own; one launch, then the same launch twice back to back on one stream into two sets of outputs"""
    torch, ctx, cus = e["torch"], e["ctx"], e["cus"]
    t, bb_ = sc.TARGETS[name]
    sizes, bpr = sc.batch_sizes(b, name, cus), b["bpr"]
    k, total = len(sizes), sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    launches = sc.runs_plan(e["lib"], t, sizes, bpr, cus)
    d_idx = _index(e, name, b, total, lambda: sc.runs_tiles(launches, starts[:-1]))
    _, ins = _carve(torch, [16 * n for n in sizes])
    outs = [_carve(torch, [bb_ * n for n in sizes])[1] for _ in range(2)]
    idxs = [d_idx[int(a):int(z)] for a, z in zip(starts, starts[1:])]
    for d, i in zip(ins, idxs):
        d.view(-1, 16)[:] = e["pool"][i]
    want = [_expected(e, name, i, bpr) for i in idxs]
    word = _word_of(_first_failure(e, d_idx))  # (runs are numbered back to back from 0)
    status = _status_tensor(e)
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    VP, SZ = ctypes.c_void_p * k, ctypes.c_size_t * k

    def call(o):
        st = ctx._lib.bu_uastc_transcode_batch_device(ctx.handle, t, k, VP(*[x.data_ptr() for x in ins]), SZ(*sizes), VP(*[x.data_ptr() for x in o]), bpr, None,
                                                      ctypes.c_void_p(status.data_ptr()), sp)
        assert st == 0, (name, b["id"])

    for twice in (False, True):
        for o in outs:
            for x in o:
                x.fill_(0xEE)
        ctx.status_word_reset(status)
        torch.cuda.synchronize()
        call(outs[0])
        if twice:
            call(outs[1])  # back to back: the first launch's last workgroup has reset the ticket counters, its status stands
        torch.cuda.synchronize()
        got = int(status.item()) & sc.CLEAR
        assert got == word, (name, b["id"], twice, hex(got), hex(word))
        for o in outs[:2 if twice else 1]:
            for i in range(k):
                assert torch.equal(o[i], want[i]), (name, b["id"], twice, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.ALL)
def test_batch_call_over_the_multi_run_kernels(env, name):
    batches = sc.batches_for(name, ticketed=False)
    assert len(batches) >= 2
    for b in batches:
        run_batch(env, name, b)


# ---- tile tickets ---------------------------------------------------------------------------------------------------------------
def run_ticketed(e, name):
    """the target's ticketed sizes: the first half of the blocks in the cheapest key, the second in the dearest"""
    cases, batches = sc.cases_for(name, ticketed=True), sc.batches_for(name, ticketed=True)
    assert len(cases) == 2 and len(batches) == 1
    for c in cases:
        run_one_slice(e, name, c)
        e["torch"].cuda.empty_cache()
    run_batch(e, name, batches[0])
    e["torch"].cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.TICKET_TARGETS)
def test_skewed_halves_through_the_ticket_draw(env, name):
    assert os.environ.get("BU_TILE_TICKETS", "1") != "0", "this process walks fixed shares: the ticketed run needs the default"
    run_ticketed(env, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.TICKET_TARGETS)
def test_skewed_halves_on_fixed_shares(name):
    """the same sizes with BU_TILE_TICKETS=0, in a fresh process"""
    env_ = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), BU_TILE_TICKETS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "ticketed", name], env=env_, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ticketed ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _main(what, name):
    from basisu_rs_amd import Context, synth

    assert what == "ticketed"
    ctx = Context(0)
    e = make_env(synth.load_golden(os.path.join(ROOT, "tests", "golden", "uastc_kat.bin")), ctx)
    run_ticketed(e, name)
    ctx.close()
    print("ticketed ok")


if __name__ == "__main__":
    _main(*sys.argv[1:])
