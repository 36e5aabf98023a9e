"""The case table of the rectangle-walk tests (tests/rect_walk_cases.py) without a GPU, on the launch plan and the lane mapping of the host build of
csrc/bu_rect_plan.hpp, for 256 and 128 CUs and both launch policies:

1. the tile-count conditions that make a workgroup walk (or not walk) hold for every target's grid, and no launch exceeds 2^21 blocks;
2. every source block of a case lies in exactly one lane of one tile, and every block's store address is its own place in its job's surface -- so every byte
   of a surface is the destination of exactly one block, or padding;
3. the walk edges t -> t + grid of `walk` join tiles of every ordered pair of widths, full and clipped tiles, different source and output pitches, the recipe
   pairs of sc.WALK_PAIRS, and some workgroup has a tile fewer than its neighbours;
4. every tile of `every_recipe` reaches the edge its recipe is named for under the rectangle kernel's lane order (512 threads x 2 blocks), checked with the
   numpy restatement of the sort's bookkeeping of tests/test_sort_cases.py under the tile's validity mask;
5. the lowest failing block of `walk` lies in a tile of a workgroup's third round or later, and healing it leaves a failure in another job.
This is the evidence that the GPU cases can tell consecutive tiles of a walk apart: no broken kernel is ever run."""
import itertools

import numpy as np
import pytest

import rect_walk_cases as rw
import sort_cases as sc
import test_sort_cases as tsc
from test_channel_targets import plan_lib  # noqa: F401  (fixture: the sort tables)
from test_rect_plan import lib  # noqa: F401  (fixture: the host build of the rectangle plan)

CUS = (256, 128)
POLICIES = (sc.EXCL, sc.SHARED)
GRID_CLASSES = ("bc7", "etc1")  # four and two workgroups per CU: the other targets plan as one of these


def planned(lib, c, cu, policy, name):  # noqa: F811
    geo = rw.geometry(lib, c, cu)
    return geo, rw.launches_of(lib, geo, name, policy)


def case_runs(c, name, policy):
    return name in c["targets"] and (policy in c["policies"] or c["policies"] == (sc.AUTO,))


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("cu", CUS)
def test_tile_counts_make_the_cases_walk(lib, cu, policy):  # noqa: F811
    for c in rw.CASES.values():
        seen = set()
        for name in sc.ALL:
            if not case_runs(c, name, policy):
                continue
            geo, launches = planned(lib, c, cu, policy, name)
            assert len(geo.jobs) > 0 and all(len(l["tiles"]) > 0 for l in launches)
            miss = rw.condition(c, launches, cu)
            assert miss is None, (c["id"], name, policy, cu, miss)
            for l in launches:
                assert sum(int(geo.tiles[j][lt][0].sum()) for _, j, lt in l["tiles"]) <= rw.MAX_BLOCKS, (c["id"], name)
            seen.add(tuple((l["n_tiles"], l["grid"]) for l in launches))
        if not seen:  # (sized for one policy only)
            assert c["policies"] == (sc.SHARED,) and policy == sc.EXCL
            continue
        if c["id"] == "walk":  # the largest grid: four workgroups per CU, and still over three rounds
            assert max(g for s in seen for _, g in s) == (4 if policy == sc.EXCL else 2) * cu
    geo = rw.geometry(lib, rw.CASES["walk"], cu)
    assert len(geo.jobs) <= rw.JOBS_PER_LAUNCH
    assert len(rw.geometry(lib, rw.CASES["three_launches"], cu).jobs) >= 130


def test_a_case_that_does_not_walk_is_named(lib, monkeypatch):  # noqa: F811
    monkeypatch.setitem(rw._GEOMETRY, ("walk", 256), rw.Geometry(lib, dict(rw.CASES["walk"], jobs=lambda cu: rw.walk_jobs(cu)[:40]), 256))
    geo, launches = planned(lib, rw.CASES["walk"], 256, sc.EXCL, "bc7")
    assert "fewer than 3 rounds" in rw.condition(rw.CASES["walk"], launches, 256)


@pytest.mark.parametrize("cu", CUS)
def test_every_block_in_one_tile_every_surface_byte_in_one_block_or_padding(lib, cu):  # noqa: F811
    has, src, dst, idx = np.zeros(rw.TILE, np.uint8), np.zeros(rw.TILE, np.uint64), np.zeros(rw.TILE, np.uint64), np.zeros(rw.TILE, np.uint64)
    for c in rw.CASES.values():
        geo = rw.geometry(lib, c, cu)
        used = {j["slice"] for j in geo.jobs}
        assert len(used) >= 3 and len({geo.slices[s][0] for s in used}) == len(used)
        pads = {j["pad"] for j in geo.jobs}
        assert 0 in pads and 1 in pads and max(pads) > 1
        bases = [j["base"] for j in geo.jobs]
        assert len(set(bases)) == len(bases) and bases != sorted(bases) and bases != sorted(bases, reverse=True) and min(bases) != bases[0]
        # source: a count per slice block
        count = [np.zeros(b * r, dtype=np.int32) for b, r in geo.slices]
        for j, tiles in zip(geo.jobs, geo.tiles):
            for m, sidx in tiles:
                np.add.at(count[j["slice"]], sidx[m], 1)
        assert all((k <= 1).all() for k in count), c["id"]
        for i, j in enumerate(geo.jobs):
            bpr, rows = geo.slices[j["slice"]]
            assert (count[j["slice"]].reshape(rows, bpr)[j["y0"]:j["y0"] + j["h"], j["x0"]:j["x0"] + j["w"]] == 1).all(), (c["id"], i)
        assert sum(int(k.sum()) for k in count) == sum(j["w"] * j["h"] for j in geo.jobs), c["id"]  # (no tile holds a block outside its job)
        # surfaces: block (x, y) of the job is stored at row y (RGBA32: pixel rows 4 y ..), byte x * row bytes: inside the row's w * row bytes, never the padding
        for name in ("bc7", "etc1", "rgba"):
            if name not in c["targets"]:
                continue
            rb, rpb = rw.row_bytes(name), rw.rows_per_block(name)
            table = rw.job_table(name, geo.jobs, geo.slices)
            ents = [e for _, es in rw.trp.plan(lib, sc.TARGETS[name][0], table, 0, cu) for e in es]
            for e, j, row, tiles in zip(ents, geo.jobs, table, geo.tiles):
                ew = np.array([e[k] for k in ("in", "out", "pitch", "base", "in_bpr", "w", "h", "tpr")], dtype=np.uint64)
                pitch = (j["w"] + j["pad"]) * rb
                assert row[7] == pitch and rw.surface_bytes(name, j) == rpb * j["h"] * pitch
                for lt, (m, sidx) in enumerate(tiles):
                    lib.bu_emul_rect_tile(sc.TARGETS[name][0], ew.ctypes.data_as(rw.trp.U64P), lt, has.ctypes.data, src.ctypes.data, dst.ctypes.data, idx.ctypes.data)
                    assert (has.astype(bool) == m).all()
                    y, x = np.divmod(sidx[m], row[1])
                    want = row[6] + (y - j["y0"]) * rpb * pitch + (x - j["x0"]) * rb
                    assert (dst[m].astype(np.int64) == want).all() and (idx[m].astype(np.int64) == j["base"] + sidx[m]).all(), (c["id"], name)


def shape_of(geo, job, lt):
    """(tile width, clipped?) of a tile"""
    m, _ = geo.tiles[job][lt]
    return rw.tile_width(geo.jobs[job]["w"]), not m.all()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", GRID_CLASSES)
@pytest.mark.parametrize("cu", CUS)
def test_walk_edges_join_tiles_that_differ_in_everything(lib, cu, name, policy):  # noqa: F811
    c = rw.CASES["walk"]
    geo, (l,) = planned(lib, c, cu, policy, name)
    grid, n = l["grid"], l["n_tiles"]
    widths, clips, recipes, in_bpr, pitch, same_job = set(), set(), set(), False, False, 0
    for t, job, lt in l["tiles"]:
        if t + grid >= n:
            continue
        _, job2, lt2 = l["tiles"][t + grid]
        same_job += job == job2
        (w1, c1), (w2, c2) = shape_of(geo, job, lt), shape_of(geo, job2, lt2)
        widths.add((w1, w2))
        clips.add((c1, c2))
        j1, j2 = geo.jobs[job], geo.jobs[job2]
        in_bpr = in_bpr or geo.slices[j1["slice"]][0] != geo.slices[j2["slice"]][0]
        pitch = pitch or j1["w"] + j1["pad"] != j2["w"] + j2["pad"]
        if job != job2:
            recipes.add((rw.recipe_of(c, geo, l, t, job, lt), rw.recipe_of(c, geo, l, t + grid, job2, lt2)))
    what = (cu, name, policy, grid, n)
    assert same_job == 0, what  # the tiles t, t + grid, t + 2 grid of a workgroup fall into different jobs
    missing = sorted(set(itertools.product(rw.WIDTHS, rw.WIDTHS)) - widths)
    assert not missing, what + ("no walk edge joins tiles of widths", missing)
    assert {(False, True), (True, False), (True, True), (False, False)} <= clips, what
    assert in_bpr and pitch, what
    assert set(sc.WALK_PAIRS) <= recipes, what + (sorted(set(sc.WALK_PAIRS) - recipes),)
    assert n >= 3 * grid + 1 and 0 < n % grid < grid  # workgroups n % grid .. grid - 1 walk one tile fewer than the ones in front of them
    kinds = {(j["w"], j["h"]) for j in geo.jobs}
    k = 4 * (cu // 16)
    assert {rw.shape(kind, k) for kind in ("col1", "col5", "full8", "w9", "full16", "pages", "w65", "strip", "full64")} <= kinds and (32, 32) in kinds and (1, 1) in kinds


def _clipped_edge(m, b, key):
    """None, or what a single-key tile under lane mask m misses: the uniform waves are exactly those whose lanes hold a block in both loads; every other lane
    with a block is ranked by an add of 1, every lane without one goes to the dummy counter"""
    inside = m.reshape(rw.BPT, rw.WGS // 64, 64).all(2).all(0)
    if (b["uniform"] != inside).any():
        return "uniform waves %s, lanes say %s" % (b["uniform"].nonzero()[0].tolist(), inside.nonzero()[0].tolist())
    if b["adds1"][sc.NO_BLOCK] != (~m).sum() or b["hist"][key] != m.sum() or b["hist"].sum() != m.sum():
        return "one key over the mask, the dummy counter for the rest"
    if b["adds64"][key] != rw.BPT * inside.sum():
        return "an add of 64 per load of a uniform wave"
    return None


def test_every_recipe_tile_reaches_its_edge_in_the_rectangle_lane_order(lib, plan_lib):  # noqa: F811
    c = rw.CASES["every_recipe"]
    geo = rw.geometry(lib, c, 256)
    tb = sc.Tables(plan_lib, "bc7")
    full, clipped, failures = set(), {}, []
    for j, tiles in zip(geo.jobs, geo.tiles):
        assert len(j["recipes"]) == len(tiles)
        for rid, (m, _) in zip(j["recipes"], tiles):
            pk = rw.lane_keys(rid)
            b = tsc.book(tb.sort_keys(pk), rw.WGS, rw.BPT, mask=m)
            tw = rw.tile_width(j["w"])
            if m.all():
                if rid in sc.RAGGED:
                    continue
                miss = tsc._edge(rid, sc.recipe_keys(rid, rw.TILE), b, rw.TILE, rw.BPT)
                full.add((tw, rid))
            else:
                assert rid in sc.RAGGED and (pk == pk[0]).all()
                miss = _clipped_edge(m, b, int(tb.sort_keys(pk[:1])[0]))
                lanes = np.arange(rw.TILE)[m]
                vc, vr = int((lanes % tw).max()) + 1, int((lanes // tw).max()) + 1
                assert m.sum() == vc * vr
                clipped[tw, vc, vr] = b
            if miss:
                failures.append("%s in a tile %d wide (job %d x %d) does not reach: %s" % (rid, tw, j["w"], j["h"], miss))
    assert not failures, "\n".join(failures)
    assert full == set(itertools.product(rw.WIDTHS, sc.FULL)), sorted(set(itertools.product(rw.WIDTHS, sc.FULL)) - full)
    # a row of 63 blocks and a row of one in the 64-wide shape; vc == 1 in the 8-wide one; vr == 1 (one whole wave of blocks, whose second load is empty: not uniform)
    assert {(64, 63, 16), (64, 1, 16), (8, 1, 128), (64, 64, 1), (64, 64, 15)} <= set(clipped), sorted(clipped)
    assert not clipped[64, 63, 16]["uniform"].any() and clipped[64, 63, 16]["adds1"][sc.NO_BLOCK] == 16
    assert not clipped[64, 1, 16]["uniform"].any() and clipped[64, 1, 16]["hist"].sum() == 16
    assert not clipped[8, 1, 128]["uniform"].any() and clipped[8, 1, 128]["hist"].sum() == 128
    assert not clipped[64, 64, 1]["uniform"].any() and clipped[64, 64, 1]["hist"].sum() == 64
    b = clipped[64, 64, 15]  # clipped in height only: seven waves keep both their rows and stay uniform, the eighth ranks its one row lane by lane
    assert b["uniform"].sum() == 7 and b["both"].any() and b["adds1"][sc.NO_BLOCK] == 64
    # the chunk count of max_chunks and all 20 runs, in every shape (through _edge above; said once more by number)
    for tw in rw.WIDTHS:
        j = next(j for j in geo.jobs if rw.tile_width(j["w"]) == tw and "max_chunks" in j["recipes"])
        m, _ = geo.tiles[geo.jobs.index(j)][j["recipes"].index("max_chunks")]
        b = tsc.book(tb.sort_keys(rw.lane_keys("max_chunks")), rw.WGS, rw.BPT, mask=m)
        assert b["nc"] == rw.TILE // 64 + 19 and (b["hist"] > 0).all()


def tile_of(geo, l, job, sidx):
    for t, j, lt in l["tiles"]:
        if j == job:
            m, s = geo.tiles[j][lt]
            if (s[m] == sidx).any():
                return t
    raise AssertionError("block %d of job %d is in no tile" % (sidx, job))


@pytest.mark.parametrize("cu", CUS)
def test_lowest_failure_late_in_a_walk_and_another_job_after_healing(lib, plan_lib, golden, cu):  # noqa: F811
    _, pool_st = sc.pool_blocks(golden["uastc"])
    late = 0
    for cid, name, policy in [("walk", n, p) for n in GRID_CLASSES for p in POLICIES] + [("three_launches", "etc1", sc.SHARED), ("every_recipe", "bc7", sc.EXCL)]:
        c = rw.CASES[cid]
        geo, launches = planned(lib, c, cu, policy, name)
        tb = sc.Tables(plan_lib, name)
        idx = rw.fill(c, geo, launches, tb)
        for i in range(len(geo.jobs)):
            assert (rw.job_region(geo, idx, i) >= 0).all()
        first = rw.lowest_failure(geo, idx, pool_st)
        assert first is not None and first[1] in (sc.ST_BAD_MODE, sc.ST_BAD_PATTERN) and first[2] != 0, (cid, name, policy)  # (not in the first job)
        assert rw.word_of(first) == ((geo.jobs[first[2]]["base"] + first[3]) << 8) | first[1]
        rw.heal(geo, idx, tb, first)
        again = rw.lowest_failure(geo, idx, pool_st)
        assert again is not None and again[0] > first[0], (cid, name, policy)
        if cid == "walk":
            (l,) = launches
            t = tile_of(geo, l, first[2], first[3])
            late += t >= 2 * l["grid"]
            assert t >= 2 * l["grid"], (name, policy, t, l["grid"])
            assert again[2] != first[2], (name, policy)  # the next failure is another job's
    assert late >= 1
