"""The launch plan of the UASTC launchers (csrc/bu_launch_plan.hpp, compiled as it is into the test-only host build): which kernel, grid, tile size,
priorities, pitch and tile tickets every launch of bu_launch_uastc (one slice) and bu_launch_runs (several runs) gets.

Every shape produces the same bytes, so the GPU parity tests cannot see a wrong choice.  tests/golden/launch_plan_cases.json.gz holds the launches the
launchers made before the plan was split out of them -- kernel instantiation, grid, workgroup size and every argument, recorded through stubs for a matrix
of targets, sizes on both sides of each threshold, pitches, policies and CU counts -- and the plan must make exactly those, with one deliberate difference:
a launch draws its tiles by ticket only with a grid of at least 8 (the kernel numbers its tiles off eight counters)."""
import ctypes
import gzip
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "host_emul", "libbu_emul.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_cases.json.gz")
ASTC, BC7, ETC1, ETC2, RGBA = range(5)
EXCL, SHARED, AUTO, FEW = 0, 1, 2, 3
BLOCK_BYTES = [16, 16, 8, 16, 64]
IN, OUT, BASE = 1 << 40, 2 << 40, 1000  # the addresses and block numbering the recorded slices were launched with
MULTI = {0: (512, 4, 0, 0), 1: (1024, 1, 0, 0), 2: (256, 4, 1, 1), 3: (512, 2, 1, 0)}  # BU_MULTI_* -> bu_uastc_multi_kernel<T, WGS, BPT, PREFETCH, WHOLE>
I64P = ctypes.POINTER(ctypes.c_int64)
U64P = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-C", os.path.dirname(EMUL), "libbu_emul.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(EMUL)
    lib.bu_emul_launch_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_uint, I64P, ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_int)]
    lib.bu_emul_launch_plan.restype = ctypes.c_size_t
    lib.bu_emul_runs_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, U64P, U64P, ctypes.POINTER(ctypes.c_size_t), U64P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_uint, I64P, ctypes.c_size_t, I64P, ctypes.c_size_t]
    lib.bu_emul_runs_plan.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


FIELDS = ("offset", "n", "kernel", "wgs", "bpt", "minw", "prefetch", "rect", "grid", "block", "tile_rt", "rect_magic", "cus", "bpr", "ticket")


def slice_plan(lib, t, n, bpr, grid_cap=0, policy=EXCL, auto=EXCL, cu=256):
    """bu_plan_slice as bu_launch_uastc runs it (AUTO resolved to `auto` where the launcher asks bu_auto_policy): (list of dicts, needs_policy)"""
    cap = 256
    rows = (ctypes.c_int64 * (15 * cap))()
    needs = ctypes.c_int(0)
    k = lib.bu_emul_launch_plan(t, n, bpr, grid_cap, policy, auto, cu, rows, cap, ctypes.byref(needs))
    assert k <= cap
    return [dict(zip(FIELDS, rows[15 * i:15 * i + 15])) for i in range(k)], bool(needs.value)


def runs_plan(lib, t, runs, bpr, policy=EXCL, auto=EXCL, cu=256):
    """bu_plan_runs + bu_plan_multi_kernel as bu_launch_runs runs them, runs = [in, out, n, base]: list of (launch dict, its table entries)"""
    k = len(runs)
    A, O, B = [(ctypes.c_uint64 * k)(*[r[i] for r in runs]) for i in (0, 1, 3)]
    N = (ctypes.c_size_t * k)(*[r[2] for r in runs])
    cap, ecap = k + 8, 2 * k + 8
    rows, ents = (ctypes.c_int64 * (10 * cap))(), (ctypes.c_int64 * (5 * ecap))()
    m = lib.bu_emul_runs_plan(t, k, A, O, N, B, bpr, policy, auto, cu, rows, cap, ents, ecap)
    assert m > 0
    out = []
    for j in range(m):
        r = dict(zip(("plain_run", "k", "n_tiles", "tile", "needs_policy", "kernel", "grid", "block", "ticket", "first"), rows[10 * j:10 * j + 10]))
        out.append((r, [ents[5 * e:5 * e + 5] for e in range(r["first"], r["first"] + r["k"])]))
    return out


def slice_records(t, plan, in_addr, out_addr, base):
    """the plan as the recorded launches: ["P", target, grid, block, in, out, n, bpr, base] / ["S", target, WGS, BPT, MINW, PREFETCH, layout, grid, block, in, out, n,
    bpr, base, cus, tile_rt argument, ticket]"""
    out = []
    for l in plan:
        i, o, b = in_addr + 16 * l["offset"], out_addr + BLOCK_BYTES[t] * l["offset"], base + l["offset"]
        if l["kernel"] < 0:
            out.append(["P", t, l["grid"], l["block"], i, o, l["n"], l["bpr"], b])
        else:
            out.append(["S", t, l["wgs"], l["bpt"], l["minw"], l["prefetch"], l["rect"], l["grid"], l["block"], i, o, l["n"], l["bpr"], b, l["cus"],
                        l["rect_magic"] if l["rect"] else l["tile_rt"], l["ticket"]])
    return out


def expected(launches):
    """the recorded launches, with the one deliberate change: no tile tickets on a grid below 8"""
    out = []
    for l in launches:
        l = list(l)
        if l[0] == "S":
            l[16] = int(l[16] and l[7] >= 8)
        elif l[0] == "M":
            l[10] = int(l[10] and l[6] >= 8)
        out.append(l)
    return out


def test_slice_plans_match_recorded_launches(lib, golden):
    assert len(golden["slice"]) > 3000
    for t, n, bpr, grid_cap, policy, auto, cu, rec in golden["slice"]:
        plan, needs = slice_plan(lib, t, n, bpr, grid_cap, policy, auto, cu)
        case = (t, n, bpr, grid_cap, policy, auto, cu)
        assert slice_records(t, plan, IN, OUT, BASE) == expected(rec["launches"]), case
        # bu_auto_policy / bu_note_big_enqueue exactly where the launcher called them
        assert (rec["auto"], rec["note"]) == ((int(needs), 0) if policy == AUTO else (0, int(needs))), case


def test_runs_plans_match_recorded_launches(lib, golden):
    assert len(golden["runs"]) > 800
    for t, runs, bpr, policy, auto, cu, rec in golden["runs"]:
        case = (t, [r[2] for r in runs], bpr, policy, auto, cu)
        got, n_auto, n_note = [], 0, 0
        for l, entries in runs_plan(lib, t, runs, bpr, policy, auto, cu):
            if l["plain_run"] >= 0:
                r = runs[l["plain_run"]]
                plan, needs = slice_plan(lib, t, r[2], bpr, 0, policy, auto, cu)
                got += slice_records(t, plan, r[0], r[1], r[3])
                n_auto += needs and policy == AUTO
                n_note += needs and policy != AUTO
                continue
            n_auto += l["needs_policy"] and policy == AUTO
            table = [[runs[run][0] + 16 * off, runs[run][1] + BLOCK_BYTES[t] * off, runs[run][3] + off, n, vshift, first] for run, off, n, vshift, first in entries]
            got.append(["M", t, *MULTI[l["kernel"]], l["grid"], l["block"], l["n_tiles"], bpr, l["ticket"], table])
        want = [l[:-1] + [golden["tables"][l[-1]]] if l[0] == "M" else l for l in expected(rec["launches"])]
        assert got == want, case
        assert (n_auto, n_note) == (rec["auto"], rec["note"]), case


def check_slice_invariants(t, n, plan):
    """every block once, in order; grid <= tiles; a ticket launch has a grid of at least 8; every sorted launch names a compiled kernel"""
    done = 0
    for l in plan:
        assert l["offset"] == done and l["n"] > 0
        done += l["n"]
        tile = 256 if l["kernel"] < 0 else (l["wgs"] * l["bpt"] if l["rect"] else l["tile_rt"])
        assert 1 <= l["grid"] <= -(-l["n"] // tile)
        assert not l["ticket"] or l["grid"] >= 8
        assert (l["kernel"] < 0) == (n < 8) and (l["kernel"] < 0 or l["block"] == l["wgs"])
    assert done == n


def test_slice_invariants(lib, golden):
    for t, n, bpr, grid_cap, policy, auto, cu, _ in golden["slice"]:
        check_slice_invariants(t, n, slice_plan(lib, t, n, bpr, grid_cap, policy, auto, cu)[0])


def test_runs_invariants(lib, golden):
    for t, runs, bpr, policy, auto, cu, _ in golden["runs"]:
        covered = {i: 0 for i in range(len(runs))}
        for l, entries in runs_plan(lib, t, runs, bpr, policy, auto, cu):
            if l["plain_run"] >= 0:
                assert covered[l["plain_run"]] == 0
                covered[l["plain_run"]] = runs[l["plain_run"]][2]
                continue
            first = 0
            for run, off, n, vshift, first_tile in entries:
                assert off == covered[run] and n > 0
                covered[run] += n
                assert first_tile == first
                first += -(-n // l["tile"])
            assert l["n_tiles"] == first and 1 <= l["grid"] <= l["n_tiles"] and l["k"] <= 96
            assert not l["ticket"] or l["grid"] >= 8
        assert all(covered[i] == r[2] for i, r in enumerate(runs))


def test_documented_cases(lib):
    # BC7, 2^20 blocks on a 1024-block-wide grid, exclusive: sorted<BC7, 512, 2, 1, true, RECT> on one 64 x 16 rectangle per workgroup slot
    (l,), needs = slice_plan(lib, BC7, 1 << 20, 1024)
    assert needs and (l["wgs"], l["bpt"], l["minw"], l["prefetch"], l["rect"]) == (512, 2, 1, 1, 1)
    assert (l["grid"], l["block"], l["cus"], l["ticket"], l["bpr"]) == (1024, 512, 256, 0, 1024)
    # BC7, 2^25 blocks without a grid: the virtual pitch 1024, the same kernel, tile tickets (32 tiles per workgroup)
    (l,), _ = slice_plan(lib, BC7, 1 << 25, 0)
    assert (l["wgs"], l["bpt"], l["rect"], l["grid"], l["cus"], l["ticket"], l["bpr"]) == (512, 2, 1, 1024, 256, 1, 1024)
    # ETC1 from 2^20 blocks: one-tile workgroups of the shared shape (512 x 4 on 2048-block tiles), no priorities and no tickets under every policy
    for policy in (EXCL, SHARED):
        (l,), _ = slice_plan(lib, ETC1, 1 << 22, 0, policy=policy)
        assert (l["wgs"], l["bpt"], l["minw"], l["grid"], l["cus"], l["ticket"]) == (512, 4, 4, 2048, 0, 0)
    # below BU_SORT_MIN_BLOCKS the one-lane-per-block kernel; the zero-copy launches keep their 64 workgroups and never ask for a policy
    (l,), needs = slice_plan(lib, ASTC, 7, 0)
    assert (l["kernel"], l["grid"], l["block"], needs) == (-1, 1, 256, False)
    (l,), needs = slice_plan(lib, ASTC, 1 << 22, 1024, grid_cap=64)
    assert (l["wgs"], l["bpt"], l["rect"], l["grid"], l["ticket"], needs) == (256, 4, 0, 64, 0, False)


def test_no_tickets_on_a_grid_below_8(lib):
    """on one CU a 2^25-block BC7 launch has four persistent workgroups: long walks, but too few workgroups for the eight ticket counters"""
    for t, cu, grid in ((BC7, 1, 4), (ASTC, 1, 5), (RGBA, 2, 4), (BC7, 2, 8)):
        plan, _ = slice_plan(lib, t, 1 << 25, 1024, cu=cu)
        assert all(l["grid"] == grid and l["ticket"] == (grid >= 8) for l in plan)
        check_slice_invariants(t, 1 << 25, plan)
    # the same launch on 256 CUs does take them
    assert all(l["ticket"] for l in slice_plan(lib, BC7, 1 << 25, 1024)[0])
    # so does a persistent multi-run grid of ETC1 (96 short runs on 1024-block tiles, 60 tiles per workgroup), unlike ETC1's plain launches
    runs = [[IN + (i << 34), OUT + (i << 34), 5000, 5000 * i] for i in range(96)]
    (l, _), = runs_plan(lib, ETC1, runs, 0, cu=4)
    assert (l["kernel"], l["tile"], l["grid"], l["ticket"]) == (3, 1024, 8, 1)
    (l,), _ = slice_plan(lib, ETC1, 1 << 25, 0, cu=4)
    assert l["ticket"] == 0
    # below 8 workgroups it does not
    (l, _), = runs_plan(lib, ETC1, runs, 0, cu=2)
    assert (l["kernel"], l["grid"], l["ticket"]) == (3, 4, 0)
