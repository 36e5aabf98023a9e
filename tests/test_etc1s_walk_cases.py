"""The cases of the ETC1S walk tests (tests/etc1s_walk_cases.py) without a GPU, for 256 and 128 CUs: that every launch they describe is larger than its grid in
the way the GPU test relies on, so that a case which stops walking fails HERE and does not pass quietly on the device.

1. The rectangle tables go through the host build of the launch plan (bu_emul_etc1s_rects_plan, tests/host_emul/bu_emul_etc1s_rects.cpp, with plan, units_of
   and grid_for of tests/test_etc1s_rect_plan.py): the launches and first-unit numbers the cases restate in numpy are the plan's; three_rounds is one launch of
   two whole rounds and a ragged third that ends inside a workgroup; wave slot WALK_SLOT steps through three jobs that differ in unit shape,
   in_blocks_per_row and pitch; a clipped unit lies in the last round; the planted bad blocks lie in rounds 2, 0 and 1 and the third-round one has the lowest
   status index; two_launches is two launches of more than a round each; and every block of every rectangle lies in exactly one lane of one unit of one launch.
2. The file cases: the one-launch door's unit count (ceil(blocks / 64) per non-empty image), restated, is above two rounds, ragged, within the block budget.
3. The slice cases: sizes, the alignment-independent arithmetic of chunks and rounds, and the rounds of the planted blocks.
No broken kernel is ever run: these are properties of the tables."""
import numpy as np
import pytest

import etc1s_walk_cases as wc
import test_etc1s_rect_plan as trp
from test_etc1s_rect_plan import lib  # noqa: F401  (fixture: the host build of the rectangle plan)

CUS = (256, 128)


def planned(lib, case, cu, name="rgba"):  # noqa: F811
    jobs, slices = wc.RECT_CASES[case](cu)
    return jobs, slices, trp.plan(lib, wc.job_table(name, jobs, slices), cu)


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("case", list(wc.RECT_CASES))
def test_the_restated_plan_is_the_launchers(lib, case, cu):  # noqa: F811
    jobs, slices, launches = planned(lib, case, cu)
    mine = wc.launches_of(jobs)
    assert len(mine) == len(launches)
    for m, (l, ents) in zip(mine, launches):
        assert (m["n_jobs"], m["n_units"]) == (l["k"], l["n_units"])
        assert [e["job"] for e in ents] == list(range(m["first_job"], m["first_job"] + m["n_jobs"]))
        assert [e["first_unit"] for e in ents] == m["first_unit"].tolist()
        assert l["grid"] == trp.grid_for(l["n_units"] * trp.UNIT, cu) == wc.grid_for(l["n_units"] * wc.UNIT, cu) == 8 * cu and l["block"] == 256
        for e in ents:
            j = jobs[e["job"]]
            assert trp.units_of(j["w"], j["h"]) == wc.units_of(j["w"], j["h"]) and trp.unit_shape(j["w"]) == wc.unit_shape(j["w"])
    assert wc.round_units(cu) == launches[0][0]["grid"] * launches[0][0]["block"] // 64


@pytest.mark.parametrize("cu", CUS)
def test_three_rounds_walks_three_ragged_rounds(lib, cu):  # noqa: F811
    jobs, slices, ((l, ents),) = planned(lib, "three_rounds", cu)
    U, n = wc.round_units(cu), l["n_units"]
    assert wc.rect_condition("three_rounds", cu) is None
    # the same, literally, on the launcher's plan
    assert l["k"] == 64 and 2 * U < n < 3 * U and -(-n // U) == 3
    assert n % U != 0 and n % 4 != 0          # the last round ends inside a workgroup: its last workgroup has 1 .. 3 units
    first = np.array([e["first_unit"] for e in ents])
    steps = [int(np.searchsorted(first, u, side="right")) - 1 for u in range(wc.WALK_SLOT, n, U)]
    assert steps == [0, 24, 48] == wc.slot_steps(wc.launches_of(jobs)[0], jobs, cu)
    es = [ents[k] for k in steps]
    assert [trp.unit_shape(e["w"]) for e in es] == [(4, 16), (32, 2), (64, 1)]
    assert [e["in_bpr"] for e in es] == [65, 33, 200]
    assert [jobs[k]["pitch"] for k in steps] == ["tight", "padded", "4096"]
    for name in wc.TARGETS:
        (_, ents_n), = trp.plan(lib, wc.job_table(name, jobs, slices), cu)
        assert len({ents_n[k]["pitch"] for k in steps}) == 3 and [ents_n[k]["pitch"] for k in steps] == [wc.pitch_of(name, jobs[k]) for k in steps]
    # every width, every pitch, alpha on every other job (the ETC1 table has none), clipping to the right and to the bottom
    assert {e["w"] for e in ents} == set(wc.WIDTHS) and {j["pitch"] for j in jobs} == set(wc.PITCHES)
    assert [e["aidx"] != 0 for e in ents] == [i % 2 == 1 for i in range(64)]
    assert all(row[1] == 0 for row in wc.job_table("etc1", jobs, slices))
    assert any(j["h"] % wc.unit_shape(j["w"])[1] for j in jobs) and any(j["w"] % wc.unit_shape(j["w"])[0] for j in jobs)
    # a clipped unit in the last round, by the kernel's own mapping: a unit whose lanes do not all hold a block
    has, shape = np.zeros(64, np.uint8), np.zeros(4, np.uint32)
    a = [np.zeros(64, np.uint64) for _ in range(4)]
    clipped = 0
    for u in range(2 * U, n):
        r = int(np.searchsorted(first, u, side="right")) - 1
        ew = np.array([ents[r][k] for k in trp.ENTRY], dtype=np.uint64)
        lib.bu_emul_etc1s_rect_unit(trp.RGBA, ew.ctypes.data_as(trp.U64P), u - int(first[r]), has.ctypes.data, *(x.ctypes.data for x in a), shape.ctypes.data)
        clipped += int(has.sum()) < 64
        assert (int(has.sum()) < 64) == wc.unit_is_clipped(jobs[r], u - int(first[r]))
    assert clipped >= 1
    # bases fall against the job order
    assert [j["base"] for j in jobs] == sorted((j["base"] for j in jobs), reverse=True)


@pytest.mark.parametrize("cu", CUS)
def test_two_launches_both_walk(lib, cu):  # noqa: F811
    jobs, slices, launches = planned(lib, "two_launches", cu)
    assert wc.rect_condition("two_launches", cu) is None
    assert [l["k"] for l, _ in launches] == [64, 3]
    assert all(l["n_units"] > wc.round_units(cu) and l["grid"] == 8 * cu for l, _ in launches)


@pytest.mark.parametrize("cu", CUS)
def test_the_planted_blocks_lie_in_rounds_2_0_and_1(lib, cu):  # noqa: F811
    jobs, slices, ((l, ents),) = planned(lib, "three_rounds", cu)
    assert wc.status_condition(cu) is None
    sb, U = wc.status_blocks(jobs, slices), wc.round_units(cu)
    rounds, index = {}, {}
    for key in ("endpoint", "selector", "alpha"):
        job, x, y = sb[key + "_at"]
        e = ents[job]
        s, sidx = sb[key]
        assert s == jobs[job]["slice"] and e["in_bpr"] == slices[s][0]
        # the block's status index from the entry the kernel reads: base (index_base + origin) + its offset inside the rectangle
        index[key] = e["base"] + y * e["in_bpr"] + x
        assert index[key] == jobs[job]["base"] + sidx
        uw, uh = trp.unit_shape(e["w"])
        rounds[key] = (e["first_unit"] + (y // uh) * e["upr"] + x // uw) // U
    assert rounds == dict(endpoint=2, selector=0, alpha=1)
    assert index["endpoint"] < index["alpha"] < index["selector"]
    assert ents[wc.BAD_ALPHA[0]]["aidx"] != 0
    assert wc.lowest_status_index("rgba", jobs, slices, sb) == wc.lowest_status_index("etc1", jobs, slices, sb) == index["endpoint"]
    assert wc.job_of_block(jobs, slices, *sb["outside"]) is None


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("case,name", [("three_rounds", "rgba"), ("three_rounds", "etc1"), ("two_launches", "bc3")])
def test_every_block_in_exactly_one_lane_of_one_unit_of_one_launch(lib, case, name, cu):  # noqa: F811
    jobs, slices = wc.RECT_CASES[case](cu)
    table = wc.job_table(name, jobs, slices)
    assert all(lib.bu_emul_etc1s_rect_job_ok(wc.TARGETS[name], trp.words([row])[0].ctypes.data_as(trp.U64P)) for row in table)
    trp.check_plan(lib, wc.TARGETS[name], table, cu)
    # no source block in two jobs, and the surfaces planned apart
    for s, (bpr, rows) in enumerate(slices):
        count = np.zeros((rows, bpr), np.int32)
        for j in jobs:
            if j["slice"] == s:
                count[j["y0"]:j["y0"] + j["h"], j["x0"]:j["x0"] + j["w"]] += 1
        assert count.max() == 1 and count.min() == 0
    assert all(wc.surface_bytes(name, j) <= 1 << 34 for j in jobs)


def test_a_table_that_does_not_walk_is_named(monkeypatch):
    """lowered to one round, every case is refused by its condition (tried by hand on the tables themselves; kept here so that it stays tried)"""
    with monkeypatch.context() as m:
        m.setattr(wc, "THREE_ROUNDS", tuple((w, 3 if w == 130 else 1) for w, _ in wc.THREE_ROUNDS))   # 77 q units
        assert "not three rounds" in wc.rect_condition("three_rounds", 256)
    with monkeypatch.context() as m:
        m.setattr(wc, "SECOND_LAUNCH", ((65, 2), (33, 24), (130, 12)))
        assert "launch 1" in wc.rect_condition("two_launches", 256)   # (38 q units: less than a round, the grid not even full)
    with monkeypatch.context() as m:
        m.setattr(wc, "file_dims", lambda cu, f=wc.file_dims: f(cu)[:len(f(cu)) // 3])   # a third of the images: less than a round
        assert "not three ragged rounds" in wc.file_condition(256)
    with monkeypatch.context() as m:
        m.setattr(wc, "staged_case", lambda cu, f=wc.staged_case: dict(f(cu), chunks=f(cu)["W"] + 3, n=(f(cu)["W"] + 3) * 256 + 77))
        assert "no ragged third step" in wc.staged_condition(256)
    with monkeypatch.context() as m:
        m.setattr(wc, "gather_case", lambda cu, name="bc1", f=wc.gather_case: dict(f(cu, name), n=f(cu, name)["B"] + 77 * wc.RGBA_NBX))
        assert "not two rounds" in wc.gather_condition(256) and "not two rounds" in wc.gather_condition(256, "rgba")
    assert wc.rect_condition("three_rounds", 256) is None and wc.file_condition(256) is None


# ---- whole files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", CUS)
def test_file_cases_hold_more_than_two_rounds_of_units(cu):
    dims = wc.file_dims(cu)
    assert wc.file_condition(cu) is None
    U = wc.round_units(cu)
    n_units = sum((w * h + 63) // 64 for w, h in dims if w * h)   # the one-launch door's rule, restated: ceil(blocks / 64) per non-empty image
    assert n_units == wc.file_units(dims) and 2 * U < n_units < 3 * U and n_units % U != 0
    assert abs(n_units - (2 * U + U // 3)) <= 3
    assert sum(w * h for w, h in dims) <= wc.FILE_MAX_BLOCKS
    assert trp.grid_for(n_units * 64, cu) == 8 * cu
    special = [d for d in dims if d != (1, 1)]
    assert set(special) == set(wc.SPECIAL) and 16 * len(special) >= len(dims) and 2 * len(special) < len(dims)
    # images of one to three units that end mid-unit, and one that fills its unit
    assert {(-(-w * h // 64), (w * h) % 64 != 0) for w, h in wc.SPECIAL} == {(1, True), (2, True), (1, False), (3, True)}
    # a unit of the third round belongs to a multi-unit image and one to a 1 x 1 image
    unit0 = np.concatenate([[0], np.cumsum([-(-w * h // 64) for w, h in dims])])
    late = [d for d, u in zip(dims, unit0) if u >= 2 * U]
    assert (1, 1) in late and any(w * h > 64 for w, h in late)


# ---- slice kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", CUS)
def test_slice_cases_take_a_ragged_third_round(cu):
    assert wc.staged_condition(cu) is None
    c = wc.staged_case(cu)
    W = 16 * cu                                    # waves of the staged launch: cu workgroups of 1024 threads
    assert c["W"] == W and c["n"] == (2 * W + W // 2 + 3) * 256 + 77 and c["n"] >= 1 << 19
    assert c["n"] // 256 > 2 * W and (c["n"] // 256) % W != 0 and c["n"] % 256 == 77
    assert (wc.STAGED_EP + wc.STAGED_SEL) * 4 <= wc.LDS_MAX
    lo, hi = c["bad_endpoint"], c["bad_selector"]
    assert (lo // 256) // W == 1 and (hi // 256) // W == 2 and (lo // 256) % W == (hi // 256) % W and lo < hi
    assert hi % 256 == 2 * 9 + 129 and lo % 256 == 2 * 20   # the fourth block of lane 9 (i0 + 129), the first of lane 20
    for name in ("bc1", "rgba"):
        assert wc.gather_condition(cu, name) is None
        g = wc.gather_case(cu, name)
        B = 8 * cu * 256
        assert g["B"] == B and 2 * B < g["n"] < 3 * B and g["n"] % B != 0
        assert g["early"] // B == 1 and g["late"] // B == 2 and g["early"] < g["late"] < g["n"]
        assert trp.grid_for(g["n"], cu) == 8 * cu
    assert wc.gather_case(cu)["n"] == 2 * B + B // 2 + 77
    assert wc.gather_case(cu, "rgba")["n"] % wc.RGBA_NBX == 0 and B % wc.RGBA_NBX != 0
    assert (wc.N_EP + wc.N_SEL + 256) * 4 == 193024 > wc.LDS_MAX == 155648
