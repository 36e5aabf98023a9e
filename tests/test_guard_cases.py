"""The case table of the guard-band tests (tests/guard_cases.py) against the launch plan (csrc/bu_launch_plan.hpp, compiled as it is into tests/host_emul): the
one-slice cases reach every (kernel, tile tickets) pair that a broad sweep of the plan reaches, the batch cases every multi-run kernel, and every kernel reached
has a case with a ragged end.  Which kernel ran cannot be seen from its bytes, so a case dropped from the table would go unnoticed on the GPU: here it
fails by naming the kernel that is no longer reached.  Also the guard helper's own check, on a host arena (no device needed)."""
import ctypes

import numpy as np
import pytest

import gpu_guard as gg
import guard_cases as gc
import test_channel_targets as tct
from test_channel_targets import plan_lib  # noqa: F401  (fixture)

I64P = ctypes.POINTER(ctypes.c_int64)
CUS = (256, 80)
SWEEP_POLICIES = ((0, 0), (1, 1), (2, 0), (2, 1), (2, 3))  # (the five of test_slice_plan_covers_every_block_once)
KERNEL, WGS, BPT, RECT, TILE_RT, TICKET = 2, 3, 4, 7, 10, 14  # columns of a bu_emul_launch_plan row
MULTI_NAMES = {0: "BU_MULTI_ETC_2048", 1: "BU_MULTI_ONE_TILE", 2: "BU_MULTI_WHOLE", 3: "BU_MULTI_PERSIST"}


def sweep_sizes(cu):
    return tct.SIZES + [9, 1023, 1025, 1024 * cu - 1, 1024 * cu + 1, 16384 * 17, 3 * 1024 * cu + 16384, 1 << 21, (1 << 21) + 5, (3 << 20) + 4096,
                        16 * 4 * cu * 1024, 16 * 5 * cu * 1024 + 77]


def kernel_name(lib, t, pair):
    k, ticket = pair
    return "target %d, kernel %d%s" % (t, k, " with tile tickets" if ticket else "") if k >= 0 else "target %d, the one-lane-per-block kernel" % t


def sweep_pairs(lib, t, cu):
    pairs = set()
    for n in sweep_sizes(cu):
        for bpr in (0, 1, 128, 1024, 4096):
            if t == gc.RGBA and bpr == 0:
                continue  # (RGBA32 without a pitch is BU_ERR_ARGUMENT at every entry point; the plan divides by it)
            for grid_cap in (0, 64):
                for policy, auto in SWEEP_POLICIES:
                    for r in tct._slice_plan(lib, t, n, bpr, grid_cap, policy, auto, cu):
                        pairs.add((r[KERNEL], r[TICKET]))
    return pairs


def case_plans(lib, name, cu):
    """[(case, policy, rows)] of every one-slice case of the target under each of its policies"""
    t = gc.TARGETS[name][0]
    out = []
    for c in gc.cases_for(name):
        n, bpr = gc.size_of(c, name, cu), gc.pitch_of(c, name, cu)
        assert 0 < n <= gc.MAX_BLOCKS, (c["id"], n)
        assert name != "rgba" or c["entry"] == "pageable" or n % bpr == 0, (c["id"], n, bpr)
        for p in c["policies"]:
            policy, auto = gc.POLICY_ARGS[p]
            out.append((c, p, tct._slice_plan(lib, t, n, bpr, gc.grid_cap_of(c), policy, auto, cu)))
    return out


def tile_of(r):
    return 256 if r[KERNEL] < 0 else (r[WGS] * r[BPT] if r[RECT] else r[TILE_RT])


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("name", gc.ALL)
def test_one_slice_cases_reach_every_kernel_of_the_sweep(plan_lib, name, cu):  # noqa: F811
    t = gc.TARGETS[name][0]
    want = sweep_pairs(plan_lib, t, cu)
    if cu == 256:  # (what the sweep reaches on an MI355X: the one-lane kernel included)
        assert len(want) == (9 if name in ("astc", "bc7") else 7), sorted(want)
    got = {(r[KERNEL], r[TICKET]) for _, _, rows in case_plans(plan_lib, name, cu) for r in rows}
    missing = sorted(want - got)
    assert not missing, "no case reaches: " + "; ".join(kernel_name(plan_lib, t, p) for p in missing)


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("name", gc.ALL)
def test_every_kernel_reached_has_a_ragged_case(plan_lib, name, cu):  # noqa: F811
    t = gc.TARGETS[name][0]
    plans = case_plans(plan_lib, name, cu)
    by_id = {}
    for c, p, rows in plans:
        by_id.setdefault(c["id"], []).append((p, rows))
    reached, ragged = set(), set()
    for c, p, rows in plans:
        for r in rows:
            pair = (r[KERNEL], r[TICKET])
            reached.add(pair)
            if r[KERNEL] < 0 or not r[RECT]:
                if r[1] % tile_of(r):
                    ragged.add(pair)
                continue
            # whole rectangles: a sibling case one block (RGBA32: one row) short, under the same policy, which the plan gives to a strip kernel
            for s in gc.cases_for(name):
                if s["ragged_of"] != c["id"]:
                    continue
                short = gc.size_of(c, name, cu) - gc.size_of(s, name, cu)
                assert short == (max(gc.pitch_of(c, name, cu), 1) if name == "rgba" or c["bpr"] else 1), (c["id"], s["id"], short)
                for sp, srows in by_id[s["id"]]:
                    if sp == p and all(x[KERNEL] >= 0 and not x[RECT] for x in srows):
                        ragged.add(pair)
    missing = sorted(reached - ragged)
    assert not missing, "no ragged case for: " + "; ".join(kernel_name(plan_lib, t, p) for p in missing)


def runs_plan(lib, t, sizes, bpr, cu, block_bytes, adjacent):
    """bu_plan_runs + bu_plan_multi_kernel (exclusive: what a lone batch call resolves to) over runs laid out as the GPU test lays them out:
    apart, or back to back and merged as bu_merge_runs merges them"""
    if adjacent:
        sizes = [sum(sizes)]
    k = len(sizes)
    U64 = ctypes.c_uint64 * k
    rows, ents = (ctypes.c_int64 * (10 * (k + 8)))(), (ctypes.c_int64 * (5 * (2 * k + 8)))()
    if k == 1:  # (bu_launch_runs: one run is the plain launch, nothing is planned)
        return [dict(plain=True, kernel=-1, ticket=0, entries=[])]
    m = lib.bu_emul_runs_plan(t, k, U64(*[(1 << 40) + (i << 34) for i in range(k)]), U64(*[(2 << 40) + (i << 34) for i in range(k)]),
                              (ctypes.c_size_t * k)(*sizes), U64(*[0] * k), bpr, 0, 0, cu, ctypes.cast(rows, I64P), k + 8, ctypes.cast(ents, I64P), 2 * k + 8)
    assert m > 0
    out = []
    for j in range(m):
        r = rows[10 * j:10 * j + 10]
        out.append(dict(plain=r[0] >= 0, kernel=r[5], ticket=r[8], entries=[ents[5 * e:5 * e + 5] for e in range(r[9], r[9] + r[1])]))
    return out


@pytest.mark.parametrize("cu", CUS)
def test_batch_cases_reach_every_multi_run_kernel(plan_lib, cu):  # noqa: F811
    kernels, ticket, plain, rgba_split = set(), False, False, False
    for b in gc.BATCHES:
        sizes = b["sizes"](cu)
        assert sum(sizes) <= gc.MAX_BLOCKS
        for name in b["targets"]:
            t, bb = gc.TARGETS[name]
            assert name != "rgba" or all(n % b["bpr"] == 0 for n in sizes), b["id"]
            for l in runs_plan(plan_lib, t, sizes, b["bpr"], cu, bb, b["adjacent"]):
                plain = plain or l["plain"]
                if l["plain"]:
                    continue
                kernels.add(l["kernel"])
                ticket = ticket or bool(l["ticket"])
                runs = [e[0] for e in l["entries"]]
                # an RGBA32 run as two entries: its whole prefix as rectangles (a shift), the rest as strips (0xFFFFFFFF)
                for a, c in zip(l["entries"], l["entries"][1:]):
                    if name == "rgba" and a[0] == c[0] and a[3] != 0xFFFFFFFF and c[3] == 0xFFFFFFFF:
                        rgba_split = True
                assert len(set(runs)) <= len(runs)
    if cu == 256:
        missing = [MULTI_NAMES[k] for k in MULTI_NAMES if k not in kernels]
        assert not missing, "no batch case reaches: " + ", ".join(missing)
    else:  # (on 80 CUs the small mix is already more tiles than CUs: no one-tile launch among these batches)
        assert {0, 2, 3} <= kernels
    assert ticket, "no batch case draws tile tickets"
    assert plain, "no batch case falls back to the plain launch"
    assert rgba_split, "no RGBA32 run is split into a whole prefix and strips"


def test_removing_a_case_is_noticed(plan_lib, monkeypatch):  # noqa: F811
    """the census names the kernel a dropped case was the only one to reach: ASTC's 256 x 4 rectangular shape with tile tickets"""
    monkeypatch.setattr(gc, "ONE_SLICE", [c for c in gc.ONE_SLICE if c["id"] != "astc_tickets_rect"])
    with pytest.raises(AssertionError, match="no case reaches: target 0, kernel 12 with tile tickets"):
        test_one_slice_cases_reach_every_kernel_of_the_sweep(plan_lib, "astc", 256)


# ---- the guard helper itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", gg.FILLS)
def test_fill_is_a_function_of_the_offset(fill):
    a = gg.fill_bytes(np, 0, 1 << 17, fill, phase=8)
    assert a.dtype == np.uint8 and (a[1000:5000] == gg.fill_bytes(np, 1000, 5000, fill, phase=8)).all()
    if fill in ("random", "uastc"):
        assert not (a.reshape(-1, 8) == 0).all(1).any(), "an aligned run of eight zero bytes"
        assert np.unique(a).size > 200
    if fill == "uastc":
        assert (a[8::16] == 69).all()
    if fill == "ones":
        assert (a.view("<u4") == 0xFFFFFFFF).all()


def test_host_arena_layout_and_check_names_the_offset():
    a = gg.Arena("self-check", [1000, 24, 4096], guard=1024 * 16, offsets=[16, 8, 0], where="pageable")
    assert len(a.regions) == 3 and len(a.bands) == 4
    for r, ofs in zip(a.regions, (16, 8, 0)):
        assert (a.addr + r.start) % 256 == ofs
    assert all(b - s >= gg.GUARD_MIN for s, b in a.bands)
    for i in range(3):
        a.data(i)[:] = 0  # the data regions are the caller's
    a.check()
    at = a.regions[1].stop + 5  # one byte, five bytes behind region 1
    a.buf[at] ^= 0x40
    assert a.violations() == [(2, at, 1)]
    with pytest.raises(AssertionError, match=r"self-check: guard band 2 changed at arena offset %d \(5 bytes past the end of region 1 " % at):
        a.check()
    a.buf[at] ^= 0x40
    a.buf[a.regions[0].start - 1] ^= 1  # the last byte in front of region 0
    with pytest.raises(AssertionError, match=r"guard band 0 changed at arena offset %d \(1 bytes in front of region 0\)" % (a.regions[0].start - 1)):
        a.check()
