"""The launch plan and the address mapping of bu_etc1s_transcode_rects_device (csrc/bu_etc1s_rect_plan.hpp), without a GPU.

tests/host_emul/bu_emul_etc1s_rects.cpp compiles the header as it is -- the plan, and the functions the kernel itself calls to find a unit's job and to place a
unit and a lane -- and this file checks, against offsets computed independently in numpy: every block of every rectangle lies in exactly one lane of exactly one
unit of exactly one launch, no lane holds a block outside its rectangle, launches respect the argument-space and unit-count limits, and unit shapes follow the
rule (2^k blocks wide, the smallest power of two not below min(w, 64); 64 >> k high).  The fixed jobs are also walked by a stand-alone build under
-fsanitize=undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_emul", "bu_emul_etc1s_rects.cpp")
ETC1, RGBA, BC4, BC5, R11, RG11, BC1, BC3 = 2, 4, 6, 7, 8, 9, 11, 12
TARGETS = (ETC1, RGBA, BC4, BC5, R11, RG11, BC1, BC3)
ROW_BYTES = {ETC1: 8, RGBA: 16, BC4: 8, BC5: 16, R11: 8, RG11: 16, BC1: 8, BC3: 16}   # bytes a block takes of one output row
ROWS = {t: 4 if t == RGBA else 1 for t in TARGETS}                                     # output rows per block row
UNIT, MAX_UNITS, KERNARG_BYTES = 64, (1 << 31) - 1, 4096
U64P, U32P = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
IDX, AIDX, OUT = 1 << 40, 3 << 40, 1 << 42


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("etc1s_rects") / "libbu_emul_etc1s_rects.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), SRC], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_etc1s_rect_job_ok.argtypes = [ctypes.c_int, U64P]
    lib.bu_emul_etc1s_rect_job_ok.restype = ctypes.c_int
    lib.bu_emul_etc1s_rects_plan.argtypes = [ctypes.c_size_t, U64P, ctypes.c_uint, U64P, ctypes.c_size_t, U64P, ctypes.c_size_t, U64P]
    lib.bu_emul_etc1s_rects_plan.restype = ctypes.c_size_t
    lib.bu_emul_etc1s_rect_unit.argtypes = [ctypes.c_int, U64P, ctypes.c_uint32] + [ctypes.c_void_p] * 6
    lib.bu_emul_etc1s_rect_unit.restype = None
    lib.bu_emul_etc1s_rect_units.argtypes = [ctypes.c_int, U64P, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    lib.bu_emul_etc1s_rect_units.restype = None
    lib.bu_emul_etc1s_rect_unit_job.argtypes = [U32P, ctypes.c_size_t, ctypes.c_uint32]
    lib.bu_emul_etc1s_rect_unit_job.restype = ctypes.c_uint32
    lib.bu_emul_etc1s_rect_ushift.argtypes = [ctypes.c_uint32]
    lib.bu_emul_etc1s_rect_ushift.restype = ctypes.c_uint32
    lib.bu_emul_etc1s_rect_table_bytes.restype = lib.bu_emul_etc1s_rect_other_arg_bytes.restype = lib.bu_emul_etc1s_rect_jobs_per_launch.restype = ctypes.c_size_t
    lib.bu_emul_etc1s_rect_max_units.restype = lib.bu_emul_etc1s_rect_max_job_units.restype = ctypes.c_uint64
    return lib


def words(jobs):
    """jobs: (idx, aidx, in_bpr, x0, y0, w, h, out, pitch, index_base)"""
    return np.ascontiguousarray(np.array(jobs, dtype=np.uint64).reshape(-1, 10))


ENTRY = ("idx", "aidx", "out", "pitch", "base", "in_bpr", "w", "h", "upr")


def plan(lib, jobs, cu=256):
    """[(launch dict, [entry dict])] of bu_plan_etc1s_rects"""
    w = words(jobs)
    lcap, ecap = len(jobs) + 8, len(jobs) + 8
    L, E, T = np.zeros(4 * lcap, np.uint64), np.zeros(11 * ecap, np.uint64), np.zeros(lcap, np.uint64)
    n = lib.bu_emul_etc1s_rects_plan(len(jobs), w.ctypes.data_as(U64P), cu, L.ctypes.data_as(U64P), lcap, E.ctypes.data_as(U64P), ecap, T.ctypes.data_as(U64P))
    assert n <= lcap
    out, e = [], 0
    for i in range(n):
        l = dict(zip(("k", "n_units", "grid", "block"), (int(x) for x in L[4 * i:4 * i + 4])), tail=int(T[i]))
        ents = [dict(zip(ENTRY + ("first_unit", "job"), (int(x) for x in E[11 * (e + k):11 * (e + k) + 11]))) for k in range(l["k"])]
        e += l["k"]
        out.append((l, ents))
    return out


def unit_shape(w):
    """the rule, spelled out here: width = the smallest power of two not below min(w, 64), height = 64 / width"""
    uw = next(1 << k for k in range(7) if (1 << k) >= min(w, 64))
    return uw, UNIT // uw


def units_of(w, h):
    uw, uh = unit_shape(w)
    return -(-w // uw) * -(-h // uh)


def grid_for(n_blocks, cu):
    """the grid of the whole-file ETC1S launches for the same number of blocks: 256-thread workgroups, at most eight per CU"""
    return max(1, min(-(-n_blocks // 256), 8 * cu))


def expected(target, job):
    """index address, alpha index address, store address and status index of every block of the rectangle, computed here: arrays of shape (h, w)"""
    d_idx, d_aidx, bpr, x0, y0, w, h, d_out, pitch, base = job
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    sl = (np.uint64(y0) + y) * np.uint64(bpr) + np.uint64(x0) + x
    a = np.uint64(d_aidx) + np.uint64(4) * sl if d_aidx else np.zeros_like(sl)
    return np.uint64(d_idx) + np.uint64(4) * sl, a, np.uint64(d_out) + y * np.uint64(ROWS[target] * pitch) + x * np.uint64(ROW_BYTES[target]), np.uint64(base) + sl


def check_launch_limits(lib, launches, cu):
    jpl = lib.bu_emul_etc1s_rect_jobs_per_launch()
    for l, ents in launches:
        assert 1 <= l["k"] <= jpl and len(ents) == l["k"]
        assert 1 <= l["n_units"] <= MAX_UNITS
        assert l["block"] == 256 and l["grid"] == grid_for(l["n_units"] * UNIT, cu)
        assert l["tail"] == 0xFFFFFFFF
        u = 0
        for e in ents:
            uw, _ = unit_shape(e["w"])
            assert e["upr"] == -(-e["w"] // uw)
            assert e["first_unit"] == u
            u += units_of(e["w"], e["h"])
        assert u == l["n_units"]


def walk_entry(lib, target, e):
    """every lane of every unit of a table entry: (has, src, asrc, dst, idx), each of shape (units, 64)"""
    n = units_of(e["w"], e["h"])
    ew = np.array([e[k] for k in ENTRY], dtype=np.uint64)
    has = np.zeros((n, UNIT), np.uint8)
    src, asrc, dst, idx = (np.zeros((n, UNIT), np.uint64) for _ in range(4))
    lib.bu_emul_etc1s_rect_units(target, ew.ctypes.data_as(U64P), 0, n, has.ctypes.data, src.ctypes.data, asrc.ctypes.data, dst.ctypes.data, idx.ctypes.data)
    return has.astype(bool), src, asrc, dst, idx


def check_plan(lib, target, jobs, cu=256):
    launches = plan(lib, jobs, cu)
    check_launch_limits(lib, launches, cu)
    got = {j: [] for j in range(len(jobs))}
    order = []
    for l, ents in launches:
        for e in ents:
            order.append(e["job"])
            has, src, asrc, dst, idx = walk_entry(lib, target, e)
            # the unit shape of the rule: lane l is row l // uw, column l % uw of unit (uy, ux), units numbered row by row
            uw, uh = unit_shape(e["w"])
            lu, lanes = np.meshgrid(np.arange(has.shape[0]), np.arange(UNIT), indexing="ij")
            col, row = (lu % e["upr"]) * uw + lanes % uw, (lu // e["upr"]) * uh + lanes // uw
            assert (has == ((col < e["w"]) & (row < e["h"]))).all()   # no lane holds a block outside its rectangle, and none inside is missing
            got[e["job"]].append(np.stack([src[has], asrc[has], dst[has], idx[has]], axis=1))
    assert order == list(range(len(jobs)))  # one entry per job, in order
    for j, job in enumerate(jobs):
        g = np.concatenate(got[j])
        es, ea, ed, ei = expected(target, job)
        assert g.shape[0] == job[5] * job[6], "job %d: %d blocks in units, %d in the rectangle" % (j, g.shape[0], job[5] * job[6])
        o, eo = np.argsort(g[:, 2], kind="stable"), np.argsort(ed.ravel(), kind="stable")
        g = g[o]
        # every store address of the rectangle exactly once (so: every block in exactly one lane, none outside), with its own load addresses and index
        assert (g[:, 2] == ed.ravel()[eo]).all()
        assert (g[:, 0] == es.ravel()[eo]).all() and (g[:, 1] == ea.ravel()[eo]).all()
        assert (g[:, 3] == ei.ravel()[eo]).all()
    return launches


def fixed_jobs(target, pad=0, alpha=True):
    """w x h over all the sizes at which the unit shape or the clipping changes; every other job with an alpha slice; each in a surface region of its own"""
    rb, jobs, out = ROW_BYTES[target], [], OUT
    for w in SIZES:
        for h in SIZES:
            pitch = w * rb + pad * rb
            jobs.append((IDX + 4 * len(jobs), AIDX if alpha and len(jobs) % 2 else 0, 300, 3 + (w % 5), 2 + (h % 3), w, h, out, pitch, 1000 * len(jobs)))
            out += ROWS[target] * h * pitch + 4096
    return jobs


@pytest.mark.parametrize("pad", [0, 3], ids=["tight", "padded"])
@pytest.mark.parametrize("target", [ETC1, RGBA, BC1, BC3])
def test_every_block_in_exactly_one_lane(lib, target, pad):
    launches = check_plan(lib, target, fixed_jobs(target, pad=pad, alpha=target != ETC1))
    assert [l["k"] for l, _ in launches] == [64, 64, 64, 64]  # 256 jobs
    # a 32 x 32-block page is 16 full units; a one-block-wide column fills its lanes
    (l, ents), = check_plan(lib, target, [(IDX, 0, 1024, 64, 96, 32, 32, OUT, 4096, 0)])
    assert l["n_units"] == 16 and ents[0]["upr"] == 1 and walk_entry(lib, target, ents[0])[0].all()
    (l, ents), = check_plan(lib, target, [(IDX, 0, 1024, 5, 0, 1, 128, OUT, 16, 0)])
    assert l["n_units"] == 2 and walk_entry(lib, target, ents[0])[0].all()


def test_unit_shapes_follow_the_rule(lib):
    for w in list(range(1, 70)) + [127, 128, 129, 1000, (1 << 32) - 1]:
        k = lib.bu_emul_etc1s_rect_ushift(w)
        assert 0 <= k <= 6 and (1 << k) >= min(w, 64) and (k == 0 or (1 << (k - 1)) < min(w, 64))
        assert unit_shape(w) == (1 << k, 64 >> k)
    has, shape = np.zeros(UNIT, np.uint8), np.zeros(4, np.uint32)
    a = [np.zeros(UNIT, np.uint64) for _ in range(4)]
    for w in list(range(1, 70)) + [127, 128, 129, 1000]:
        (l, ents), = plan(lib, [(IDX, 0, 2048, 0, 0, w, 130, OUT, 16 * w, 0)])
        uw, uh = unit_shape(w)
        assert ents[0]["upr"] == -(-w // uw) and l["n_units"] == -(-w // uw) * -(-130 // uh)
        ew = np.array([ents[0][k] for k in ENTRY], dtype=np.uint64)
        # the last unit: clipped to what is left of the rectangle
        lib.bu_emul_etc1s_rect_unit(BC3, ew.ctypes.data_as(U64P), l["n_units"] - 1, has.ctypes.data, *(x.ctypes.data for x in a), shape.ctypes.data)
        assert tuple(shape) == (uw.bit_length() - 1, w - (ents[0]["upr"] - 1) * uw, 130 - (-(-130 // uh) - 1) * uh, uh)
        assert has.sum() == shape[1] * shape[2]


def test_the_table_fits_the_argument_space(lib):
    jpl = lib.bu_emul_etc1s_rect_jobs_per_launch()
    assert jpl >= 32
    # five 64-bit and four 32-bit values per job and its first-unit number; beside it a unit count, two codebook pointers with their sizes, the status word and
    # the tables: 4 + (4) + 8 + 4 + (4) + 8 + 4 + (4) + 8 + 8 = 48 bytes with alignment padding after a table aligned to 8
    assert lib.bu_emul_etc1s_rect_table_bytes() == jpl * (5 * 8 + 4 * 4 + 4) and lib.bu_emul_etc1s_rect_table_bytes() % 8 == 0
    assert lib.bu_emul_etc1s_rect_other_arg_bytes() >= 48
    assert lib.bu_emul_etc1s_rect_table_bytes() + lib.bu_emul_etc1s_rect_other_arg_bytes() <= KERNARG_BYTES
    assert lib.bu_emul_etc1s_rect_max_units() == MAX_UNITS < 1 << 31


def small_jobs(n, seed):
    rng = np.random.default_rng(seed)
    jobs, out = [], OUT
    for i in range(n):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        jobs.append((IDX, AIDX if i % 3 == 0 else 0, 4096, int(rng.integers(0, 4096 - w)), int(rng.integers(0, 4000)), w, h, out, 16 * w + 16 * int(rng.integers(0, 3)), 1 << 33))
        out += jobs[-1][8] * h
    return jobs


def test_unit_to_job_search(lib):
    """tables of one job, the full table, and the full table + 1 job (two launches, in order): every unit finds its entry, first and last unit of every entry
    included"""
    jpl = lib.bu_emul_etc1s_rect_jobs_per_launch()
    for n, want_k in ((1, [1]), (jpl, [jpl]), (jpl + 1, [jpl, 1])):
        launches = check_plan(lib, BC3, small_jobs(n, seed=n))
        assert [l["k"] for l, _ in launches] == want_k
        assert [e["job"] for _, ents in launches for e in ents] == list(range(n))
        for l, ents in launches:
            first = np.array([e["first_unit"] for e in ents], dtype=np.uint32)
            want = np.searchsorted(first, np.arange(l["n_units"]), side="right") - 1
            got = [lib.bu_emul_etc1s_rect_unit_job(first.ctypes.data_as(U32P), len(ents), u) for u in range(l["n_units"])]
            assert (np.array(got) == want).all()
            assert got[0] == 0 and got[-1] == len(ents) - 1
    # the largest unit number a launch can hold, in a full table and in a table of one job
    first = np.arange(jpl, dtype=np.uint32) * 1000
    assert lib.bu_emul_etc1s_rect_unit_job(first.ctypes.data_as(U32P), jpl, MAX_UNITS - 1) == jpl - 1
    assert lib.bu_emul_etc1s_rect_unit_job(first.ctypes.data_as(U32P), 1, MAX_UNITS - 1) == 0


def test_300_jobs_in_one_call(lib):
    launches = check_plan(lib, RGBA, small_jobs(300, seed=300))
    assert [l["k"] for l, _ in launches] == [64, 64, 64, 64, 44]


def test_wide_slice(lib):
    """in_blocks_per_row = 2^21: the slice index of a block needs all 32 bits, its byte offset more"""
    bpr = 1 << 21
    jobs = [(IDX, AIDX, bpr, bpr - 70, 2047 - 20, 70, 21, OUT, 4096, 5), (IDX, 0, bpr, 0, 0, 9, 9, 1 << 43, 160, 0), (IDX, AIDX, bpr, bpr - 1, 2047, 1, 1, 1 << 44, 16, 0)]
    for t in (BC1, RGBA, BC5):
        check_plan(lib, t, jobs)
        assert all(lib.bu_emul_etc1s_rect_job_ok(t, words(jobs)[i].ctypes.data_as(U64P)) for i in range(3))


def test_seeded_random_job_lists(lib):
    rng = np.random.default_rng(20250102)
    for case in range(200):
        target = TARGETS[case % 8]
        rb = ROW_BYTES[target]
        jobs, out = [], OUT + 16 * int(rng.integers(0, 64))
        for _ in range(int(rng.integers(1, 9))):
            bpr = int(rng.choice([1, 5, 64, 200, 257, 4096]))
            w = int(rng.integers(1, min(bpr, 150) + 1))
            h = int(rng.integers(1, 70))
            x0, y0 = int(rng.integers(0, bpr - w + 1)), int(rng.integers(0, 100))
            pitch = w * rb + rb * int(rng.choice([0, 1, 7, 100]))
            aidx = AIDX + 4 * int(rng.integers(0, 1000)) if target != ETC1 and rng.integers(0, 2) else 0
            jobs.append((IDX + 4 * int(rng.integers(0, 1000)), aidx, bpr, x0, y0, w, h, out, pitch, int(rng.integers(0, 1 << 40))))
            out += ROWS[target] * h * pitch + rb * int(rng.integers(0, 5))
        check_plan(lib, target, jobs, cu=(256, 64, 8)[case % 3])


def sampled_units(lib, target, job, e, units):
    """units of an entry too large to walk: every lane against the numpy offsets of the whole job"""
    d_idx, d_aidx, bpr, x0, y0, w, h, d_out, pitch, base = job
    uw, uh = unit_shape(w)
    ew = np.array([e[k] for k in ENTRY], dtype=np.uint64)
    has, shape, lanes = np.zeros(UNIT, np.uint8), np.zeros(4, np.uint32), np.arange(UNIT)
    src, asrc, dst, idx = (np.zeros(UNIT, np.uint64) for _ in range(4))
    for lu in units:
        lib.bu_emul_etc1s_rect_unit(target, ew.ctypes.data_as(U64P), lu, has.ctypes.data, src.ctypes.data, asrc.ctypes.data, dst.ctypes.data, idx.ctypes.data, shape.ctypes.data)
        x, y = (lu % e["upr"]) * uw + lanes % uw, (lu // e["upr"]) * uh + lanes // uw
        m = (x < w) & (y < h)
        assert (has.astype(bool) == m).all() and m.any()
        sl = [(y0 + int(b)) * bpr + x0 + int(a) for a, b in zip(x[m], y[m])]   # (python integers: no wrap-around to hide one)
        assert [int(v) for v in src[m]] == [d_idx + 4 * s for s in sl] and [int(v) for v in idx[m]] == [base + s for s in sl]
        assert [int(v) for v in asrc[m]] == [d_aidx + 4 * s if d_aidx else 0 for s in sl]
        assert [int(v) for v in dst[m]] == [d_out + int(b) * ROWS[target] * pitch + int(a) * ROW_BYTES[target] for a, b in zip(x[m], y[m])]


@pytest.mark.parametrize("target", [BC1, RGBA, BC3])
def test_extreme_legal_jobs(lib, target):
    """the largest jobs the argument rules allow are planned, not walked: their unit counts against the bound the header derives (one job never passes the
    launch limit, so no job is cut into bands), and sampled units -- first, last, around the middle -- against the numpy offsets.  (h is a 32-bit field: the
    tallest one-block-wide column is h = 2^32 - 1 from y0 = 1, whose last block row is row 2^32 - 1 of the slice.)"""
    rb = ROW_BYTES[target]
    bound = lib.bu_emul_etc1s_rect_max_job_units()
    assert bound <= MAX_UNITS
    tall = (IDX, AIDX, 1, 0, 1, 1, (1 << 32) - 1, OUT, rb, (1 << 40) + 9)
    wide = (IDX + 4, 0, 1 << 20, 0, 0, 1 << 20, 4096, OUT + rb, (1 << 20) * rb + 3 * rb, 7)
    narrow = (IDX, AIDX, 33, 0, 0, 33, (1 << 32) // 33, OUT, 40 * rb, 0)  # 64 x 1 units over 33 columns: the most units per block
    two = (IDX, 0, 65, 0, 10, 65, (1 << 32) // 65 - 10, OUT, 65 * rb + rb, 7)
    for job in (tall, wide, narrow, two):
        assert lib.bu_emul_etc1s_rect_job_ok(target, words([job])[0].ctypes.data_as(U64P))
        (l, (e,)), = plan(lib, [job])
        check_launch_limits(lib, [(l, [e])], 256)
        n = units_of(job[5], job[6])
        assert l["n_units"] == n <= bound and l["grid"] == 8 * 256
        sampled_units(lib, target, job, e, sorted({0, 1, e["upr"] - 1, e["upr"], n // 2, n - e["upr"] - 1, n - 2, n - 1}))
    assert units_of(*tall[5:7]) == 1 << 26 and units_of(*wide[5:7]) == 1 << 26 and units_of(*narrow[5:7]) > 1 << 26
    # a launch is closed in front of the job that would take it past the limit: 2^31 / 2^26 = 32 such jobs are one unit too many
    launches = plan(lib, [tall] * 40)
    check_launch_limits(lib, launches, 256)
    assert [l["k"] for l, _ in launches] == [31, 9]


def test_argument_rules(lib):
    ok = [IDX, AIDX, 200, 7, 3, 65, 17, OUT, 4096, 0]
    names = ("d_idx", "d_aidx", "bpr", "x0", "y0", "w", "h", "d_out", "pitch", "base")

    def judged(target, **kw):
        j = list(ok)
        if target == ETC1:
            j[1] = 0
        for k, v in kw.items():
            j[names.index(k)] = v
        return bool(lib.bu_emul_etc1s_rect_job_ok(target, words([j])[0].ctypes.data_as(U64P)))

    for t in TARGETS:
        assert judged(t) and judged(t, d_aidx=0)
        assert not judged(t, d_idx=0) and not judged(t, d_out=0)
        assert not judged(t, w=0) and not judged(t, h=0) and not judged(t, bpr=0, x0=0)
        assert judged(t, x0=135) and not judged(t, x0=136)          # x0 + w <= in_blocks_per_row
        assert not judged(t, x0=(1 << 32) - 1)                      # (no wrap-around in x0 + w)
        assert not judged(t, d_idx=IDX + 2) and not judged(t, d_idx=IDX + 1) and judged(t, d_idx=IDX + 4)   # d_idx 4-byte aligned
        if t != ETC1:
            assert not judged(t, d_aidx=AIDX + 2) and judged(t, d_aidx=AIDX + 4)
        rb = ROW_BYTES[t]
        assert judged(t, pitch=65 * rb) and not judged(t, pitch=65 * rb - rb)   # pitch >= w * row bytes (RGBA32: 16 w)
        assert not judged(t, pitch=4096 + rb // 2) and not judged(t, d_out=OUT + rb // 2)
        assert judged(t, pitch=4096 + rb, d_out=OUT + rb)
    # ETC1 has no alpha
    assert not judged(ETC1, d_aidx=AIDX)
    # the other values of bu_target are refused whatever the job
    for t in (0, 1, 3, 5, 10, 13, -1, 1 << 20):
        assert not judged(t) and not judged(t, d_aidx=0)
    # (y0 + h) * in_blocks_per_row <= 2^32, one past it refused
    assert judged(BC1, bpr=1 << 21, x0=0, y0=2048 - 17) and not judged(BC1, bpr=1 << 21, x0=0, y0=2048 - 16)
    assert judged(BC1, bpr=1, x0=0, w=1, y0=1, h=(1 << 32) - 1, pitch=8) and not judged(BC1, bpr=1, x0=0, w=1, y0=2, h=(1 << 32) - 1, pitch=8)
    assert not judged(BC1, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=65, x0=0)
    # (a product past 2^64 must not wrap back under the bound: this one is 2^64 + 2^32 - 2)
    assert not judged(BC1, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=(1 << 31) + 1, x0=0)
    assert not judged(BC1, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=(1 << 32) - 1, x0=0, w=1)
    assert judged(BC1, y0=0, h=1, bpr=(1 << 32) - 1, x0=0, w=1 << 28, pitch=1 << 32) and not judged(BC1, y0=1, h=1, bpr=(1 << 32) - 1, x0=0)


def test_no_context_is_refused_by_the_library():
    """the one refusal the built library can show without a device (the per-job rules go through the same bu_etc1s_rect_job_ok: tests/test_gpu_etc1s_rects.py)"""
    from basisu_rs_amd import _lib

    lib = _lib.load()
    job = _lib.Etc1sRectJob(1 << 40, None, 64, 0, 0, 1, 1, 1 << 41, 16, 0)
    assert lib.bu_etc1s_transcode_rects_device(None, _lib.BC1_RGB, 1, ctypes.byref(job), 1 << 42, 1, 1 << 43, 1, None, None) == _lib.ERR_ARGUMENT


def test_address_mapping_under_ubsan(tmp_path):
    """the stand-alone build walks every unit of the fixed jobs under -fsanitize=undefined (a report aborts it) and reproduces the numpy offsets"""
    exe = tmp_path / "bu_emul_etc1s_rects"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                    "-DBU_EMUL_ETC1S_RECTS_MAIN", "-I" + CSRC, "-o", str(exe), SRC], check=True)
    bpr = 1 << 21
    jpl = 64
    for target in (ETC1, RGBA, BC3):
        jobs = fixed_jobs(target, pad=1, alpha=target != ETC1) + [(IDX, 0 if target == ETC1 else AIDX, bpr, bpr - 70, 2047 - 20, 70, 21, 1 << 45, 4096, (1 << 56) - 1)]
        jf, of = tmp_path / ("jobs%d.bin" % target), tmp_path / ("out%d.bin" % target)
        words(jobs).tofile(jf)
        r = subprocess.run([str(exe), str(target), str(jf), str(of)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "clean 5 launches" in r.stdout, (r.returncode, r.stderr[-2000:])
        rec = np.fromfile(of, dtype=np.uint64).reshape(-1, 6)
        assert (np.diff(rec[:, 0].astype(np.int64)) >= 0).all() and (rec[:, 0] == rec[:, 1] // jpl).all()  # 64 jobs per launch, in order
        for j, job in enumerate(jobs):
            g = rec[rec[:, 1] == j]
            es, ea, ed, ei = expected(target, job)
            assert g.shape[0] == es.size
            o, eo = np.argsort(g[:, 4], kind="stable"), np.argsort(ed.ravel(), kind="stable")
            assert (g[o, 4] == ed.ravel()[eo]).all() and (g[o, 2] == es.ravel()[eo]).all() and (g[o, 3] == ea.ravel()[eo]).all() and (g[o, 5] == ei.ravel()[eo]).all()
