"""bu_uastc_transcode_rects_device on launches whose workgroups WALK: more tiles than the grid, so that a workgroup of the persistent rectangle kernel takes
tile t, t + grid, t + 2 grid, ... across jobs that differ in tile width, clipping, source pitch, output pitch and index base, with the next tile's descriptor
and blocks in flight during the current one -- and on tiles that hold the chosen histograms of tests/sort_cases.py (one key, runs of 63 / 64 / 65 blocks, all 20
runs, the largest chunk count, whole waves of invalid codes, a uniform mix followed by one key) in the lane geometry of 8 x 128, 16 x 64, 32 x 32, 64 x 16 and
clipped tiles.  tests/rect_walk_cases.py holds the cases; tests/test_rect_walk_cases.py holds without a GPU that they walk and reach what they are named for.

No call of the product supplies an expectation: inputs are gathers of the pool of sort_cases (known-answer vectors, invalid mode codes, out-of-range patterns),
expected bytes the same gather of the pool's expected blocks -- the reference's known answers for ASTC / BC7 / ETC1 / ETC2 / RGBA32, the numpy models of the
known-answer RGBA32 for the six other targets, zeros for failing blocks -- placed in each job's surface by numpy-style indexing of the rectangle, not by the
plan.  Slices sit between bands of invalid blocks, every surface is poisoned and sits between guard bands; every case compares every byte of every surface
(rectangle and padding) on the device, the guard bands, and the exact status word.  Before a launch the plan is recomputed for the device's own CU count and
the walk conditions are asserted for it: on a device where a case would not walk the test fails."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import rect_walk_cases as rw  # noqa: E402
import sort_cases as sc  # noqa: E402
import test_gpu_sort_cases as tgs  # noqa: E402
from test_rect_plan import lib  # noqa: E402,F401  (fixture: the host build of the rectangle plan)

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def env(golden, ctx, emul, lib):  # noqa: F811
    e = tgs.make_env(golden, ctx)
    e["rects"], e["built"] = lib, {}
    yield e
    e["built"].clear()


class Built:
    """the slices of a case in device memory between bands of invalid blocks, every tile laid out by its recipe for the grids of `launches`"""

    def __init__(self, e, c, geo, launches, name):
        from gpu_guard import Arena

        torch = e["torch"]
        self.idx = rw.fill(c, geo, launches, e["tables"][name])
        self.arena = Arena("slices", [max(16, 16 * a.size) for a in self.idx], 16 * 1024, fill="uastc")
        self.d_idx = []
        for s, a in enumerate(self.idx):  # the blocks no job takes: invalid mode codes
            a = np.where(a < 0, sc.POOL_BAD_MODE + np.arange(a.size) % sc.N_BAD_MODE, a)
            self.d_idx.append(torch.from_numpy(a).cuda())
            if a.size:
                self.arena.data(s).view(-1, 16)[:] = e["pool"][self.d_idx[s]]
        self.ptrs = [self.arena.ptr(s) for s in range(len(self.idx))]

    def put(self, e, s, sidx, pool_index):
        self.d_idx[s][sidx] = pool_index
        self.arena.data(s).view(-1, 16)[sidx] = e["pool"][pool_index]


def built(e, c, geo, launches, name):
    key = (c["id"], tuple(l["grid"] for l in launches) if c["content"][0] == "walk" else None, e["tables"][name].row)
    if key not in e["built"]:
        if len(e["built"]) >= 4:  # (a target's cases come one after another: the oldest is not needed again soon)
            e["built"].pop(next(iter(e["built"])))
        e["built"][key] = Built(e, c, geo, launches, name)
    return e["built"][key]


class Surfaces:
    """one poisoned surface per job, each between guard bands of one arena, every other one a block past 256-byte alignment"""

    def __init__(self, name, geo):
        from gpu_guard import Arena

        self.name, self.geo = name, geo
        self.arena = Arena("surfaces", [rw.surface_bytes(name, j) for j in geo.jobs], 64 * 1024, offsets=[rw.row_bytes(name) * (i % 2) for i in range(len(geo.jobs))])
        self.ptrs = [self.arena.ptr(i) for i in range(len(geo.jobs))]
        self.poison()

    def poison(self):
        for i in range(len(self.geo.jobs)):
            self.arena.data(i).fill_(POISON)

    def check(self, e, want, what):
        self.arena.check()
        for i, w in enumerate(want):
            assert e["torch"].equal(self.arena.data(i), w), what + ("job %d (%d x %d): the surface's bytes differ" % (i, self.geo.jobs[i]["w"], self.geo.jobs[i]["h"]),)


def expected(e, name, geo, b):
    """every job's surface as it must be left: the rectangle's blocks at the job's pitch, poison behind every row"""
    torch = e["torch"]
    rb, rpb, out = rw.row_bytes(name), rw.rows_per_block(name), []
    for j in geo.jobs:
        bpr, rows = geo.slices[j["slice"]]
        w, h = j["w"], j["h"]
        blocks = e["want"][name][b.d_idx[j["slice"]].view(rows, bpr)[j["y0"]:j["y0"] + h, j["x0"]:j["x0"] + w]]  # (h, w, block bytes)
        blocks = blocks.reshape(h, w, 4, 16).permute(0, 2, 1, 3).reshape(4 * h, 16 * w) if name == "rgba" else blocks.reshape(h, w * rb)
        s = torch.full((rpb * h, (w + j["pad"]) * rb), POISON, dtype=torch.uint8, device="cuda")
        s[:, :w * rb] = blocks
        out.append(s.reshape(-1))
    return out


def assert_walks(e, c, geo, name, policies):
    for p in policies:
        miss = rw.condition(c, rw.launches_of(e["rects"], geo, name, p), e["cus"])
        assert miss is None, "%s / %s / %s on %d CUs: %s" % (c["id"], name, p, e["cus"], miss)


def call(e, name, geo, b, surf, status, stream=None):
    e["ctx"].uastc_transcode_rects_device(sc.TARGETS[name][0], rw.job_table(name, geo.jobs, geo.slices, b.ptrs, surf.ptrs), d_status=status, stream=stream)


def run_case(e, c, name, policy, heal=False, twice=False):
    torch, ctx = e["torch"], e["ctx"]
    geo = rw.geometry(e["rects"], c, e["cus"])
    both = (sc.EXCL, sc.SHARED)
    assert_walks(e, c, geo, name, both if policy == sc.AUTO else (policy,))
    launches = rw.launches_of(e["rects"], geo, name, sc.EXCL if policy == sc.AUTO else policy)  # (AUTO: the same bytes whichever grid it resolves to)
    b = built(e, c, geo, launches, name)
    idx = [a.copy() for a in b.idx]
    surfs = [Surfaces(name, geo) for _ in range(2 if twice else 1)]
    status = tgs._status_tensor(e)
    ctx.set_launch_policy({sc.EXCL: False, sc.SHARED: True, sc.AUTO: "auto"}[policy])
    undo = None
    try:
        first = rw.lowest_failure(geo, idx, e["pool_st"])
        for step in range(2 if heal else 1):
            what = (c["id"], name, policy, e["cus"], step)
            if step:
                assert first is not None, what
                s = geo.jobs[first[2]]["slice"]
                undo = (s, first[3], int(idx[s][first[3]]))
                rw.heal(geo, idx, e["tables"][name], first)
                b.put(e, s, first[3], int(idx[s][first[3]]))
                again = rw.lowest_failure(geo, idx, e["pool_st"])
                assert again is not None and again[0] > first[0], what  # (another failure is left to report)
                assert c["id"] != "walk" or again[2] != first[2], what       # (walk: in another job)
                first = again
            want = expected(e, name, geo, b)
            for sf in surfs:
                sf.poison()
            ctx.status_word_reset(status)
            torch.cuda.synchronize()
            side = torch.cuda.Stream() if twice else None
            for sf in surfs:  # twice: back to back on one stream, nothing between -- the first launch's status stands, both sets are right
                call(e, name, geo, b, sf, status, side)
            torch.cuda.synchronize()
            got = int(status.item()) & sc.CLEAR
            assert got == rw.word_of(first), what + (hex(got), hex(rw.word_of(first)))
            for sf in surfs:
                sf.check(e, want, what)
            b.arena.check()
    finally:
        ctx.set_launch_policy("auto")
        if undo:
            b.put(e, *undo)
    return geo, launches


@pytest.mark.parametrize("name", sc.ALL)
def test_every_recipe_through_every_tile_shape(env, name):
    geo, launches = run_case(env, rw.CASES["every_recipe"], name, sc.AUTO)
    assert all(l["grid"] == l["n_tiles"] < env["cus"] for l in launches) and len(launches) >= 2  # no walk: the policy is not consulted


@pytest.mark.parametrize("policy", [sc.EXCL, sc.SHARED])
@pytest.mark.parametrize("name", sc.ALL)
def test_walk_across_jobs(env, name, policy):
    """over three rounds of the grid; then the lowest failing block -- in the last job, a tile of a late round -- healed: the next one, in another job"""
    geo, (l,) = run_case(env, rw.CASES["walk"], name, policy, heal=True)
    assert l["n_tiles"] >= 3 * l["grid"] + 1 and l["n_tiles"] % l["grid"] and l["grid"] == rw.per_cu(name, policy) * env["cus"]


@pytest.mark.parametrize("name", ["bc7", "etc1"])
def test_walk_under_the_auto_policy(env, name):
    run_case(env, rw.CASES["walk"], name, sc.AUTO)


@pytest.mark.parametrize("name", sc.ALL)
def test_walk_twice_back_to_back_into_two_sets_of_surfaces(env, name):
    run_case(env, rw.CASES["walk"], name, sc.EXCL, twice=True)


@pytest.mark.parametrize("name", ["etc1", "rgba"])
def test_three_walking_launches_in_one_call(env, name):
    geo, launches = run_case(env, rw.CASES["three_launches"], name, sc.SHARED)
    assert len(launches) == 3 and all(l["n_tiles"] >= 2 * l["grid"] + 1 and l["grid"] == env["cus"] for l in launches)


def test_a_walking_launch_is_captured_into_a_graph_and_replayed(env):
    """the pattern of tests/test_gpu_rects.py's three-job graph test on the walk case: recorded by stream capture, replayed twice into re-poisoned surfaces"""
    e, name, c = env, "bc7", rw.CASES["walk"]
    torch, ctx = e["torch"], e["ctx"]
    geo = rw.geometry(e["rects"], c, e["cus"])
    assert_walks(e, c, geo, name, (sc.EXCL, sc.SHARED))
    b = built(e, c, geo, rw.launches_of(e["rects"], geo, name, sc.EXCL), name)
    want, word = expected(e, name, geo, b), rw.word_of(rw.lowest_failure(geo, b.idx, e["pool_st"]))
    assert word != sc.CLEAR
    surf = Surfaces(name, geo)
    status = tgs._status_tensor(e)
    side = torch.cuda.Stream()

    def record():
        ctx.status_word_reset(status, stream=side)
        call(e, name, geo, b, surf, status, side)

    with torch.cuda.stream(side):
        record()  # (first use outside the capture)
    torch.cuda.synchronize()
    surf.check(e, want, ("graph", "eager"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        record()
    for replay in range(2):
        surf.poison()
        status.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        surf.check(e, want, ("graph", replay))
        assert int(status.item()) & sc.CLEAR == word, replay
    b.arena.check()
