"""The case table of the mode-sort tests (tests/sort_cases.py) without a GPU.

1. The counting sort's bookkeeping restated in plain numpy -- histogram, every run's first slot and chunk count, the chunk list, and per wave whether the
   aggregated rank path is taken -- and with it, that every recipe reaches the edge it is named for at every tile size and workgroup shape it is used
   with.  Which path a tile took cannot be seen from its bytes: a recipe that stops reaching its edge fails here by name.
2. Every case planned with the launch plan the launchers use (csrc/bu_launch_plan.hpp through tests/host_emul), for 256 and 80 CUs: the cases reach every
   mode-sorted and multi-run kernel that the reference sweep of tests/test_guard_cases.py reaches, tile tickets included.
3. Every case's blocks through the host build of the block code: bytes, per-block status, lowest failing block and its status are what the case expects."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import guard_cases as gc
import sort_cases as sc
import test_channel_targets as tct
import test_etc1s_targets as tet
import test_guard_cases as tgc
from test_channel_targets import plan_lib  # noqa: F401  (fixture)

CUS = tgc.CUS
EMUL_EVERY_BLOCK = 300_000  # cases up to this size go through the host build block by block; above it, their distinct blocks (the block code is a pure function of the block)


# ---- 1. the bookkeeping, restated -------------------------------------------------------------------------------------------------
def book(keys, wgs, bpt, mask=None):
    """the sort of one tile of wgs x bpt blocks whose first len(keys) blocks hold sort keys `keys` (0..19), as bu_uastc_sorted_body does it: block l is lane
    l % 64 of wave (l % wgs) / 64 in load l / wgs; a wave ranks all its loads with one add of 64 per load when every load is of a single key and no lane lacks
    a block, else with one add of 1 per lane.  Run k = the blocks of key k; runs lie back to back in key order and are cut into chunks of up to 64 blocks.
    mask (a clipped tile of a rectangle): [T] bool, which lanes hold a block -- `keys` then names a key for every lane, and the lanes outside drop theirs"""
    T = wgs * bpt
    k = np.full(T, sc.NO_BLOCK, dtype=np.int64)
    if mask is None:
        k[:len(keys)] = keys
    else:
        k[mask] = np.asarray(keys)[mask]
        keys = k[mask]
    hist = np.bincount(k[k < 20], minlength=20)
    first = np.concatenate([[0], np.cumsum(hist)[:-1]])
    chunks = (hist + 63) // 64
    chunk_list = [(r, int(first[r]) + 64 * c, int(min(64, hist[r] - 64 * c))) for r in range(20) for c in range(chunks[r])]
    g = k.reshape(bpt, wgs // 64, 64)  # [load, wave, lane]
    single = (g == g[:, :, :1]).all(2) & (g[:, :, 0] < 20)
    full = (g < 20).all(2)
    uniform = single.all(0)
    adds64, adds1 = np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.int64)
    for w in range(wgs // 64):
        for j in range(bpt):
            if uniform[w]:
                adds64[g[j, w, 0]] += 1
            else:
                adds1 += np.bincount(g[j, w], minlength=32)
    assert ((64 * adds64 + adds1)[:20] == hist).all() and adds1[sc.NO_BLOCK] == T - len(keys)
    # the chunks cover the sorted tile exactly once
    assert sum(c for _, _, c in chunk_list) == len(keys) and [s for _, s, _ in chunk_list] == sorted(s for _, s, _ in chunk_list)
    return dict(T=T, hist=hist, first=first, chunks=chunks, nc=int(chunks.sum()), chunk_list=chunk_list, single=single, full=full, uniform=uniform,
                adds64=adds64, adds1=adds1, both=(adds64[:20] > 0) & (adds1[:20] > 0))


def test_book_on_a_hand_made_tile():
    # 256 x 2: wave 0 holds key 3 in both loads, wave 1 key 3 then key 19, wave 2 a mix in its first load, wave 3 runs out of blocks in its second
    keys = np.concatenate([np.full(128, 3), np.tile([5, 3], 32), np.full(64, 7), np.full(64, 3), np.full(64, 19), np.full(64, 7), np.full(10, 7)])
    b = book(keys, 256, 2)
    assert b["uniform"].tolist() == [True, True, False, False]
    assert b["hist"][[3, 5, 7, 19]].tolist() == [224, 32, 138, 64] and b["first"][[3, 5, 7, 19]].tolist() == [0, 224, 256, 394]
    assert b["nc"] == 4 + 1 + 3 + 1 and b["chunk_list"][3] == (3, 192, 32) and b["chunk_list"][-1] == (19, 394, 64)
    assert b["adds64"][[3, 19]].tolist() == [3, 1] and b["adds1"][[3, 5, 7, sc.NO_BLOCK]].tolist() == [32, 32, 138, 54]
    assert b["both"].nonzero()[0].tolist() == [3]


def _only(b, keys):
    return (b["hist"][list(keys)] > 0).all() and b["hist"].sum() == b["hist"][list(keys)].sum()


def _edge(rid, pk, b, T, bpt):
    """None, or what recipe `rid` (piece keys pk in a tile of nominally T blocks, book b) fails to reach"""
    name, _, layout = rid.partition("@")
    W, waves = T // 64, b["single"].shape[1]
    whole = b["uniform"][b["full"].all(0)]  # the waves that have a block in every lane of every load (all of them, but under a run-time tile size)
    every_wave_uniform = whole.size > 0 and whole.all()
    if name.startswith("single_") or name == "all_invalid":
        k = sc.INVALID if name == "all_invalid" else int(name[7:])
        return None if b["hist"][k] == T and every_wave_uniform and b["adds64"][k] >= 1 and b["nc"] == W and len(b["chunk_list"]) == W else "one run of whole uniform waves"
    if name.startswith("two_keys_"):
        c = int(name[9:])
        if not (b["hist"][5] == c and b["hist"][12] == T - c and b["chunks"][5] == -(-c // 64) and b["first"][12] == c):
            return "a first run of exactly %d blocks" % c
        if layout == sc.INTER:  # (2 c blocks alternate: where they reach into the first load of every wave -- 256 x 4 from c = 97 -- no wave is left uniform)
            return None if not b["uniform"][0] and b["adds1"][12] > 0 and (b["both"][12] or not b["uniform"].any()) else "key 12 ranked by 64-adds and by 1-adds"
        return None if every_wave_uniform == (c % 64 == 0) else "uniform waves exactly when the runs end on a wave"
    if name == "all_20_keys":
        return None if (b["hist"] > 0).all() and b["nc"] == 19 + -(-(T - 19) // 64) and b["both"][7] else "all 20 runs present"
    if name in ("max_chunks", "max_chunks_valid"):
        runs = 20 if name == "max_chunks" else 19
        ok = b["nc"] == W + runs - 1 and (b["hist"] > 0).sum() == runs and ((b["hist"][b["hist"] > 0] % 64 == 1).sum() == runs - 1)
        return None if ok else "nc == T / 64 + %d with %d runs of 1 (mod 64) blocks" % (runs - 1, runs - 1)
    if name == "keys_16_to_19":
        return None if _only(b, (16, 17, 18, 19)) and not b["uniform"].any() else "blocks in keys 16..19 only, no uniform wave"
    if name == "keys_0_to_3":
        return None if _only(b, (0, 1, 2, 3)) else "blocks in keys 0..3 only"
    if name == "keys_15_and_16":
        return None if _only(b, (15, 16)) and every_wave_uniform and b["adds64"][15] > 0 and b["adds64"][16] > 0 else "uniform waves of keys 15 and 16 only"
    if name == "waves_mod_20":
        return None if every_wave_uniform and (b["hist"] > 0).sum() == min(20, W) and (b["hist"] % 64 == 0).all() else "every wave uniform, key = wave mod 20"
    if name == "uniform_and_scattered":
        return None if b["both"][4] and b["adds1"][9] > 0 and b["adds64"][9] == 0 else "counter 4 takes 64-adds and 1-adds in one tile"
    if name == "first_load_uniform":
        if bpt == 1:
            return None
        ok = any(b["single"][j1, w] and b["full"][j2, w] and not b["single"][j2, w] for w in range(waves) for j1 in range(bpt) for j2 in range(bpt))
        return None if ok else "a wave uniform in one load and mixed in another"
    if name in ("half_invalid_a", "half_invalid_b"):
        if not (b["adds64"][sc.INVALID] >= 1 and all((pk == sc.BAD_PATTERN + m).sum() >= 2 for m in sc.PATTERN_MODES)):
            return "whole uniform waves of key 19 and scattered bad patterns"
        first = pk[np.nonzero(pk >= sc.INVALID)[0][0]]
        return None if (first >= sc.BAD_PATTERN) == (name == "half_invalid_a") and pk[0] >= sc.INVALID else "the lowest failing block of the right kind, at block 0"
    if name == "uniform_mix":
        return None if (b["hist"][:19] > 0).all() and b["hist"][19] == 0 and not b["uniform"].any() else "19 modes mixed, no uniform wave"
    if name in ("ragged_63", "ragged_1"):
        short = sc.RECIPES[name]["short"]
        ok = len(pk) % 64 == 64 - short and b["both"][3] and b["adds1"][sc.NO_BLOCK] >= short and b["hist"][3] == len(pk)
        return None if ok else "full waves of one key and a last wave of %d lanes" % (64 - short)
    return "no edge is written down for this recipe"


def all_plans(lib, name, cu):
    """[(case or batch id, policy, [tiles], ticketed launch?)] of every case of the target; a ("halves", ..) case has no tiles"""
    t = sc.TARGETS[name][0]
    out = []
    for c in sc.cases_for(name):
        n, bpr = sc.size_of(c, name, cu), sc.pitch_of(c, name, cu)
        assert 0 < n <= gc.MAX_BLOCKS and (name != "rgba" or n % bpr == 0), (c["id"], n, bpr)
        for p in c["policies"]:
            policy, auto = sc.POLICY_ARGS[p]
            rows = tct._slice_plan(lib, t, n, bpr, sc.grid_cap_of(c), policy, auto, cu)
            out.append((c, p, rows, None))
    for b in sc.batches_for(name):
        sizes = sc.batch_sizes(b, name, cu)
        assert sum(sizes) <= gc.MAX_BLOCKS and (name != "rgba" or all(n % b["bpr"] == 0 for n in sizes)), b["id"]
        out.append((b, sc.EXCL, None, sc.runs_plan(lib, t, sizes, b["bpr"], cu)))
    return out


def tiles_of(c, name, cu, rows, launches):
    if rows is not None:
        return sc.slice_tiles(rows)
    sizes = sc.batch_sizes(c, name, cu)
    return sc.runs_tiles(launches, np.concatenate([[0], np.cumsum(sizes)[:-1]]))


@pytest.mark.parametrize("cu", CUS)
def test_every_recipe_reaches_its_edge_wherever_it_is_used(plan_lib, cu):  # noqa: F811
    used = {}  # (recipe, T, wgs, bpt, count) -> a case that uses it
    named_last = set()
    for name in sc.ALL:
        for c, p, rows, launches in all_plans(plan_lib, name, cu):
            if c["content"][0] == "halves":
                continue
            tiles = tiles_of(c, name, cu, rows, launches)
            for _, t, grid, T, wgs, bpt, where in tiles:
                rid = sc.tile_recipe(c["content"], c["last"], t, grid, T, where.size)
                used.setdefault((rid, T, wgs, bpt, where.size), "%s / %s / %s" % (name, c["id"], p))
                if where.size < T and rid == c["last"]:
                    named_last.add((name, c["id"]))
            # a case that names a recipe for its ragged last tile has such a tile (RGBA32 under a power-of-two pitch has whole rows only)
            if c["last"] is not None and not (name == "rgba" and c["bpr"]):
                assert (name, c["id"]) in named_last, "%s / %s: no tile takes the ragged recipe %s" % (name, c["id"], c["last"])
    tb = sc.Tables(plan_lib, "bc7")
    failures, whole = [], set()
    for (rid, T, wgs, bpt, count), where in sorted(used.items()):
        full = T - sc.RECIPES[rid.partition("@")[0]]["short"]
        if count != full:
            continue  # (a recipe cut off by a ragged end: run, and counted for nothing)
        whole.add(rid)
        pk = sc.recipe_keys(rid, T)
        miss = _edge(rid, pk, book(tb.sort_keys(pk), wgs, bpt), T, bpt)
        if miss:
            failures.append("%s on %d x %d (tile %d, %s) does not reach: %s" % (rid, wgs, bpt, T, where, miss))
    assert not failures, "\n".join(failures)
    missing = sorted(set(sc.FULL + sc.RAGGED) - whole)
    assert not missing, "no case runs: " + ", ".join(missing)
    assert len(set(sc.FULL)) == len(sc.FULL) and {r.partition("@")[0] for r in sc.FULL + sc.RAGGED} == set(sc.RECIPES)
    shapes = {(wgs, bpt) for (_, _, wgs, bpt, _) in used}
    assert {(1024, 1), (512, 2), (256, 4), (512, 4), (1024, 4)} <= shapes, shapes
    assert {T for (_, T, _, _, _) in used} >= {1024, 2048}


@pytest.mark.parametrize("name", sc.ALL)
def test_bad_patterns_sort_under_their_own_mode(plan_lib, golden, name):  # noqa: F811
    """the key_lut of the host build puts the pool's blocks where the recipes say: vector 32 m + v under the key of mode m, code 69 under 19, an
    out-of-range pattern under its mode's key"""
    tb = sc.Tables(plan_lib, name)
    pool, st = sc.pool_blocks(golden["uastc"])
    got = tb.key_lut[pool[:, 0] & 127]
    for k in range(19):
        idx = tb.pool_index(np.full(1024, k), np.arange(1024))
        assert (got[idx] == k).all() and np.unique(idx).size == 32 and (st[idx] == 0).all()
    idx = tb.pool_index(np.full(1024, sc.INVALID), np.arange(1024))
    assert (got[idx] == 19).all() and (st[idx] == sc.ST_BAD_MODE).all() and np.unique(idx).size == sc.N_BAD_MODE
    for m in sc.PATTERN_MODES:
        idx = tb.pool_index(np.full(64, sc.BAD_PATTERN + m), np.arange(64))
        assert (got[idx] == tb.key_of_mode[m]).all() and (got[idx] < 19).all() and (st[idx] == sc.ST_BAD_PATTERN).all()
        assert (tb.sort_keys(np.full(3, sc.BAD_PATTERN + m)) == tb.key_of_mode[m]).all()


# ---- 2. plan coverage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("name", sc.ALL)
def test_cases_reach_every_sorted_kernel_of_the_sweep(plan_lib, name, cu):  # noqa: F811
    t = sc.TARGETS[name][0]
    want = {p for p in tgc.sweep_pairs(plan_lib, t, cu) if p[0] >= 0}  # (the one-lane-per-block kernel sorts nothing)
    got = {(r[sc.KERNEL], r[sc.TICKET]) for _, _, rows, _ in all_plans(plan_lib, name, cu) if rows is not None for r in rows}
    missing = sorted(want - got)
    assert not missing, "no sort case reaches: " + "; ".join(tgc.kernel_name(plan_lib, t, p) for p in missing)
    if name in sc.TICKET_TARGETS:
        ticketed = {c["id"] for c, _, rows, _ in all_plans(plan_lib, name, cu) if rows is not None and any(r[sc.TICKET] for r in rows)}
        assert ticketed >= {c["id"] for c in sc.cases_for(name, ticketed=True)} and ticketed, "no one-slice case draws tile tickets"
    # a walk: some workgroup goes from the uniform mix to a single key, from a single key to the mix, from an all-invalid tile to a valid one
    pairs = set()
    for c, p, rows, launches in all_plans(plan_lib, name, cu):
        if c["content"][0] != "walk":
            continue
        tiles = tiles_of(c, name, cu, rows, launches)
        count = {}
        for j, tile, *_ in tiles:
            count[j] = max(count.get(j, 0), tile + 1)
        for j, tile, grid, T, _, _, where in tiles:
            if tile + grid < count[j]:
                pairs.add((sc.tile_recipe(c["content"], None, tile, grid, T, T), sc.tile_recipe(c["content"], None, tile + grid, grid, T, T)))
    assert set(sc.WALK_PAIRS) <= pairs, "no workgroup walks: %s" % sorted(set(sc.WALK_PAIRS) - pairs)


@pytest.mark.parametrize("cu", CUS)
def test_batches_reach_every_multi_run_kernel(plan_lib, cu):  # noqa: F811
    want = set(tgc.MULTI_NAMES)  # (on 80 CUs too: the one-tile batch is sized for them)
    for name in sc.ALL:
        kernels, ticket = set(), False
        for b, _, _, launches in all_plans(plan_lib, name, cu):
            if launches is None:
                continue
            for l in launches:
                assert not l["plain"], (name, b["id"])
                kernels.add(l["kernel"])
                ticket = ticket or bool(l["ticket"])
                assert bool(l["ticket"]) == (b["id"] in sc.TICKETED_BATCHES), (name, b["id"], "tile tickets")
        family = {0, 1, 3} if name in sc.ETC_FAMILY else ({1, 3} if name == "rgba" else {1, 2, 3})
        missing = [tgc.MULTI_NAMES[k] for k in sorted(want & family - kernels)]
        assert not missing, "%s: no batch reaches %s" % (name, ", ".join(missing))
        assert ticket == (name in sc.TICKET_TARGETS), name


def test_removing_a_case_is_noticed(plan_lib, monkeypatch):  # noqa: F811
    monkeypatch.setattr(sc, "ONE_SLICE", [c for c in sc.ONE_SLICE if c["id"] != "tickets_astc_rect"])
    with pytest.raises(AssertionError, match="no sort case reaches: target 0, kernel 12 with tile tickets"):
        test_cases_reach_every_sorted_kernel_of_the_sweep(plan_lib, "astc", 256)


def test_a_recipe_that_misses_its_edge_is_named(plan_lib, monkeypatch):  # noqa: F811
    """two_keys_64 with its first run a block short: the census says which recipe, on which shape, misses what"""
    monkeypatch.setitem(sc.RECIPES, "two_keys_64", dict(sc.RECIPES["two_keys_64"], sections=lambda T: [(None, [(5, 63), (12, T - 63)])]))
    with pytest.raises(AssertionError, match=r"two_keys_64@contiguous on 1024 x 1 \(tile 1024, .*\) does not reach: a first run of exactly 64 blocks"):
        test_every_recipe_reaches_its_edge_wherever_it_is_used(plan_lib, 80)


# ---- 3. expectations, through the host build --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_build(emul):
    """name, blocks [n, 16] -> (bytes [n, bytes per block], status [n]) through the host build of the target's block code"""
    subprocess.run(["make", "-j2", "-C", tct.HOST_EMUL, "libbu_emul_channels.so", "libbu_emul_colour.so"], check=True, capture_output=True)
    libs = {k: ctypes.CDLL(os.path.join(tct.HOST_EMUL, "libbu_emul_%s.so" % k)) for k in ("channels", "colour")}

    def run(name, blocks):
        if name in ("astc", "bc7", "etc1", "etc2", "rgba"):
            return emul.batch(name, blocks)
        t, bb = sc.TARGETS[name]
        fn = libs["colour"].bu_emul_colour_batch if name in ("bc1", "bc3") else libs["channels"].bu_emul_channels_batch
        fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, 16)
        out, st = np.zeros((blocks.shape[0], bb), dtype=np.uint8), np.zeros(blocks.shape[0], dtype=np.uint8)
        assert fn(t, blocks.ctypes.data, blocks.shape[0], out.ctypes.data, st.ctypes.data) == 0
        return out, st
    return run


def good_blocks(golden, name):
    """the 608 expected blocks of a target: the known answers, or the numpy model of the known-answer RGBA32"""
    return golden[name] if name in golden else tet.model(name, golden["rgba"])


def case_index(lib, tb, c, name, cu, rows, launches):
    """the pool indices of a case's blocks (a batch: its runs back to back)"""
    n = sc.size_of(c, name, cu) if rows is not None else sum(sc.batch_sizes(c, name, cu))
    if c["content"][0] == "halves":
        return sc.halves_index(tb, c["content"], n)
    return sc.fill_tiles(tb, tiles_of(c, name, cu, rows, launches), c["content"], c["last"], n)


@pytest.mark.parametrize("name", sc.ALL)
def test_expectations_through_the_host_build(plan_lib, host_build, golden, name):  # noqa: F811
    cu = 80
    tb = sc.Tables(plan_lib, name)
    pool, pool_st = sc.pool_blocks(golden["uastc"])
    want = sc.pool_expected(good_blocks(golden, name))
    clear = failing = 0
    for c, p, rows, launches in all_plans(plan_lib, name, cu):
        idx = case_index(plan_lib, tb, c, name, cu, rows, launches)
        what = (name, c["id"], p)
        every = idx.size <= EMUL_EVERY_BLOCK
        sub = idx if every else np.unique(idx)
        out, st = host_build(name, pool[sub])
        assert (st == pool_st[sub]).all() and (out == want[sub]).all(), what
        assert (out[st != 0] == 0).all(), what
        bad = np.nonzero(st)[0] if every else np.nonzero(pool_st[idx])[0]
        word = sc.expected_word(pool_st, idx, 1000)
        if bad.size == 0:
            assert word == sc.CLEAR, what
            clear += 1
        else:
            assert word == ((1000 + int(bad[0])) << 8) | int(pool_st[idx[bad[0]]]) and word & 0xFF in (sc.ST_BAD_MODE, sc.ST_BAD_PATTERN), what
            failing += 1
        if c["id"] == "one_tile/half_invalid_a":
            assert word == (1000 << 8) | sc.ST_BAD_PATTERN
        if c["id"] == "one_tile/half_invalid_b":
            assert word == (1000 << 8) | sc.ST_BAD_MODE
        if c.get("heal"):  # the lowest failure healed: another one is left to report
            assert bad.size >= 2
    assert clear >= 20 and failing >= 10
