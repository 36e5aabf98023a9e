"""The launch plan and the address mapping of bu_uastc_transcode_rects_device (csrc/bu_rect_plan.hpp), without a GPU.

tests/host_emul/bu_emul_rects.cpp compiles the header as it is -- the plan, and the functions the kernel itself calls to place a tile and a block -- and
this file checks, against offsets computed independently in numpy: every block of every rectangle lies in exactly one tile of exactly one launch, no tile
holds a block outside its rectangle, launches respect the argument-space limit, and tile shapes follow the rule (2^k blocks wide, the smallest of 8 / 16 /
32 / 64 not below min(w, 64); 1024 / width high).  The fixed jobs are also walked by a stand-alone build under -fsanitize=undefined."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "basisu_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_emul", "bu_emul_rects.cpp")
ASTC, BC7, ETC1, ETC2, RGBA, BC4 = 0, 1, 2, 3, 4, 6
ROW_BYTES = {ASTC: 16, BC7: 16, ETC1: 8, ETC2: 16, RGBA: 16, BC4: 8}   # bytes a block takes of one output row
ROWS = {ASTC: 1, BC7: 1, ETC1: 1, ETC2: 1, RGBA: 4, BC4: 1}            # output rows per block row
TILE, JOBS_PER_LAUNCH, MAX_TILES = 1024, 64, (1 << 32) // 1024 - 1
KERNARG_BYTES = 4096
U64P = ctypes.POINTER(ctypes.c_uint64)
SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("rects") / "libbu_emul_rects.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(so), SRC], check=True)
    lib = ctypes.CDLL(str(so))
    lib.bu_emul_rect_job_ok.argtypes = [ctypes.c_int, U64P]
    lib.bu_emul_rect_job_ok.restype = ctypes.c_int
    lib.bu_emul_rects_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, U64P, ctypes.c_int, ctypes.c_uint, U64P, ctypes.c_size_t, U64P, ctypes.c_size_t, U64P]
    lib.bu_emul_rects_plan.restype = ctypes.c_size_t
    lib.bu_emul_rect_tile.argtypes = [ctypes.c_int, U64P, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.bu_emul_rect_tile.restype = None
    lib.bu_emul_rect_table_bytes.restype = lib.bu_emul_rect_jobs_per_launch.restype = ctypes.c_size_t
    return lib


def words(jobs):
    """jobs: (in, in_bpr, x0, y0, w, h, out, pitch, index_base)"""
    return np.ascontiguousarray(np.array(jobs, dtype=np.uint64).reshape(-1, 9))


def plan(lib, target, jobs, policy=0, cu=256):
    """[(launch dict, [entry dict])] of bu_plan_rects + bu_plan_rects_grid"""
    w = words(jobs)
    lcap, ecap = len(jobs) + 64, len(jobs) + 256
    L, E, T = np.zeros(4 * lcap, np.uint64), np.zeros(10 * ecap, np.uint64), np.zeros(lcap, np.uint64)
    n = lib.bu_emul_rects_plan(target, len(jobs), w.ctypes.data_as(U64P), policy, cu, L.ctypes.data_as(U64P), lcap, E.ctypes.data_as(U64P), ecap, T.ctypes.data_as(U64P))
    assert n <= lcap
    out, e = [], 0
    for i in range(n):
        l = dict(zip(("k", "n_tiles", "grid", "block"), (int(x) for x in L[4 * i:4 * i + 4])), tail=int(T[i]))
        ents = [dict(zip(("in", "out", "pitch", "base", "in_bpr", "w", "h", "tpr", "first_tile", "job"), (int(x) for x in E[10 * (e + k):10 * (e + k) + 10])))
                for k in range(l["k"])]
        e += l["k"]
        assert e <= ecap
        out.append((l, ents))
    return out


def tile_shape(w):
    tw = next(t for t in (8, 16, 32, 64) if t >= min(w, 64))
    return tw, TILE // tw


def expected(target, job):
    """load address, store address and status index of every block of the rectangle, computed here: arrays of shape (h, w)"""
    d_in, bpr, x0, y0, w, h, d_out, pitch, base = job
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    sl = (np.uint64(y0) + y) * np.uint64(bpr) + np.uint64(x0) + x
    return np.uint64(d_in) + np.uint64(16) * sl, np.uint64(d_out) + y * np.uint64(ROWS[target] * pitch) + x * np.uint64(ROW_BYTES[target]), np.uint64(base) + sl


def check_launch_limits(lib, target, launches, policy, cu):
    per_cu = {ASTC: 4, BC7: 4}.get(target, 2) // (2 if policy == 1 else 1)
    # the table as the header lays it out and the kernel's three other arguments (a tile count, two pointers: 24 bytes) share the kernel-argument space
    assert lib.bu_emul_rect_jobs_per_launch() == JOBS_PER_LAUNCH
    assert lib.bu_emul_rect_table_bytes() >= JOBS_PER_LAUNCH * 52 and lib.bu_emul_rect_table_bytes() + 24 <= KERNARG_BYTES
    for l, ents in launches:
        assert 1 <= l["k"] <= JOBS_PER_LAUNCH and len(ents) == l["k"]
        assert 1 <= l["n_tiles"] <= MAX_TILES and l["n_tiles"] * TILE < 1 << 32
        assert l["block"] == 512 and l["grid"] == min(l["n_tiles"], per_cu * cu)
        assert l["tail"] == 0xFFFFFFFF
        t = 0
        for e in ents:
            tw, th = tile_shape(e["w"])
            assert e["tpr"] == -(-e["w"] // tw)
            assert e["first_tile"] == t
            t += e["tpr"] * -(-e["h"] // th)
        assert t == l["n_tiles"]


def check_plan(lib, target, jobs, policy=0, cu=256):
    launches = plan(lib, target, jobs, policy, cu)
    check_launch_limits(lib, target, launches, policy, cu)
    has, src, dst, idx = np.zeros(TILE, np.uint8), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64)
    got = {j: [] for j in range(len(jobs))}
    order = []
    for l, ents in launches:
        for e in ents:
            order.append(e["job"])
            ew = np.array([e[k] for k in ("in", "out", "pitch", "base", "in_bpr", "w", "h", "tpr")], dtype=np.uint64)
            tw, th = tile_shape(e["w"])
            for lt in range(e["tpr"] * -(-e["h"] // th)):
                lib.bu_emul_rect_tile(target, ew.ctypes.data_as(U64P), lt, has.ctypes.data, src.ctypes.data, dst.ctypes.data, idx.ctypes.data)
                m = has.astype(bool)
                # the tile shape of the rule: lane l is row l // tw, column l % tw of the tile
                ty, tx = divmod(lt, e["tpr"])
                lanes = np.arange(TILE)
                want = ((tx * tw + lanes % tw) < e["w"]) & ((ty * th + lanes // tw) < e["h"])
                assert (m == want).all()
                got[e["job"]].append(np.stack([src[m], dst[m], idx[m]], axis=1))
    assert order == sorted(order) and sorted(set(order)) == list(range(len(jobs)))  # jobs go out in order, every one of them
    for j, job in enumerate(jobs):
        g = np.concatenate(got[j])
        es, ed, ei = expected(target, job)
        assert g.shape[0] == job[4] * job[5], "job %d: %d blocks in tiles, %d in the rectangle" % (j, g.shape[0], job[4] * job[5])
        o = np.argsort(g[:, 1], kind="stable")
        g = g[o]
        eo = np.argsort(ed.ravel(), kind="stable")
        # every store address of the rectangle exactly once (so: every block in exactly one tile, none outside), with its own load address and index
        assert (g[:, 1] == ed.ravel()[eo]).all()
        assert (g[:, 0] == es.ravel()[eo]).all()
        assert (g[:, 2] == ei.ravel()[eo]).all()
    return launches


def fixed_jobs(target, pad=0):
    """w x h over the sizes at which the tile shape or the clipping changes, h = 1 / 16 / 17 among them; each in a surface region of its own"""
    rb, jobs, out = ROW_BYTES[target], [], 1 << 41
    for w in SIZES:
        for h in SIZES + (16, 17):
            pitch = w * rb + pad * rb
            jobs.append((1 << 40, 300, 3 + (w % 5), 2 + (h % 3), w, h, out, pitch, 1000 * len(jobs)))
            out += ROWS[target] * h * pitch + 4096
    return jobs


@pytest.mark.parametrize("target", [BC7, ETC1, RGBA])
def test_fixed_sizes(lib, target):
    launches = check_plan(lib, target, fixed_jobs(target, pad=1))
    assert len(launches) == 2  # 120 jobs
    # a 32 x 32-block page is exactly one whole tile
    l, ents = check_plan(lib, target, [(1 << 40, 1024, 64, 96, 32, 32, 1 << 41, 4096, 0)])[0]
    assert l["n_tiles"] == 1 and ents[0]["tpr"] == 1


def test_tile_shapes_follow_the_rule(lib):
    for w in list(range(1, 70)) + [127, 128, 129, 1000]:
        (l, ents), = plan(lib, BC7, [(1 << 40, 2048, 0, 0, w, 130, 1 << 41, 16 * w, 0)])
        tw, th = tile_shape(w)
        assert tw == (8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64) and tw * th == TILE
        assert ents[0]["tpr"] == -(-w // tw) and l["n_tiles"] == -(-w // tw) * -(-130 // th)


def test_300_jobs_in_one_call(lib):
    rng = np.random.default_rng(300)
    jobs, out = [], 1 << 41
    for i in range(300):
        w, h = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        jobs.append((1 << 40, 4096, int(rng.integers(0, 4096 - w)), int(rng.integers(0, 4000)), w, h, out, 16 * w + 16 * int(rng.integers(0, 3)), 1 << 33))
        out += jobs[-1][7] * h
    launches = check_plan(lib, BC7, jobs)
    assert [l["k"] for l, _ in launches] == [64, 64, 64, 64, 44]


def test_wide_slice(lib):
    """in_blocks_per_row = 2^21: the slice index of a block needs all 32 bits, its byte offset more"""
    bpr = 1 << 21
    jobs = [(1 << 40, bpr, bpr - 70, 2047 - 20, 70, 21, 1 << 41, 4096, 5), (1 << 40, bpr, 0, 0, 9, 9, 1 << 42, 160, 0), (1 << 40, bpr, bpr - 1, 2047, 1, 1, 1 << 43, 16, 0)]
    check_plan(lib, BC7, jobs)
    check_plan(lib, RGBA, jobs)
    w = words(jobs)
    assert all(lib.bu_emul_rect_job_ok(BC7, w[i].ctypes.data_as(U64P)) for i in range(3))


def test_seeded_random_job_lists(lib):
    rng = np.random.default_rng(20250101)
    for case in range(300):
        target = (ASTC, BC7, ETC1, ETC2, RGBA, BC4)[case % 6]
        rb = ROW_BYTES[target]
        jobs, out = [], (1 << 41) + 16 * int(rng.integers(0, 64))
        for _ in range(int(rng.integers(1, 9))):
            bpr = int(rng.choice([1, 5, 64, 200, 257, 4096]))
            w = int(rng.integers(1, min(bpr, 150) + 1))
            h = int(rng.integers(1, 70))
            x0, y0 = int(rng.integers(0, bpr - w + 1)), int(rng.integers(0, 100))
            pitch = w * rb + rb * int(rng.choice([0, 1, 7, 100]))
            jobs.append(((1 << 40) + 16 * int(rng.integers(0, 1000)), bpr, x0, y0, w, h, out, pitch, int(rng.integers(0, 1 << 40))))
            out += ROWS[target] * h * pitch + rb * int(rng.integers(0, 5))
        check_plan(lib, target, jobs, policy=case % 2, cu=(256, 64, 8)[case % 3])


def test_a_job_of_more_tiles_than_a_launch_holds_goes_out_as_bands(lib):
    """65 blocks wide = two tiles per row, 16 rows each: (2^32 / 65) rows are more tiles than one launch may number"""
    h = (1 << 32) // 65 - 10
    job = (1 << 40, 65, 0, 10, 65, h, 1 << 50, 65 * 16 + 16, 7)
    w = words([job])
    assert lib.bu_emul_rect_job_ok(BC7, w[0].ctypes.data_as(U64P))
    launches = plan(lib, BC7, [job])
    check_launch_limits(lib, BC7, launches, 0, 256)
    assert len(launches) >= 2
    y = 0
    for l, (e,) in launches:  # whole tile rows each, one behind the other, the same addresses as the job cut at that row
        assert (e["in"], e["out"], e["base"]) == (job[0] + 16 * 65 * (10 + y), job[6] + y * job[7], 7 + 65 * (10 + y))
        assert (e["w"], e["in_bpr"], e["pitch"]) == (65, 65, job[7])
        y += e["h"]
        assert y == h or e["h"] % 16 == 0
    assert y == h


@pytest.mark.parametrize("target", [BC7, ETC1, RGBA])
@pytest.mark.parametrize("w", [(1 << 28) - 64, (1 << 28) - 63, (1 << 28) - 57, (1 << 28) + 5, 3 * ((1 << 28) - 64) + 33, (1 << 32) - 1])
def test_a_tile_row_of_more_tiles_than_a_launch_holds_goes_out_as_column_bands(lib, target, w):
    """w >= 2^28 - 63: one row of 64-wide tiles is more tiles than a launch may number (the rule (y0 + h) * in_blocks_per_row <= 2^32 leaves such a job
    at most 16 block rows).  It goes out as column bands, each an entry of its own with the tile shape of its own width; the blocks are too many to walk, so
    the bands are checked to tile the columns, and the first and last tile of each is mapped and compared with the numpy offsets of the whole job."""
    y0 = 2
    h = ((1 << 32) // w) - y0 if w < 1 << 31 else 1
    if w >= 1 << 31:
        y0 = 0
    assert 1 <= h <= 14
    rb, rows = ROW_BYTES[target], ROWS[target]
    job = ((1 << 40) + 48, w, 0, y0, w, h, (1 << 50) + rb, w * rb + 3 * rb, (1 << 40) + 9)
    assert lib.bu_emul_rect_job_ok(target, words([job])[0].ctypes.data_as(U64P))
    launches = plan(lib, target, [job])
    check_launch_limits(lib, target, launches, 0, 256)
    ents = [e for _, es in launches for e in es]
    assert len(ents) == -(-w // (MAX_TILES * 64)) and all(e["job"] == 0 for e in ents)
    has, src, dst, idx = np.zeros(TILE, np.uint8), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64)
    c0, lanes = 0, np.arange(TILE)
    for e in ents:
        first = y0 * w + c0
        assert (e["in"], e["out"], e["base"]) == (job[0] + 16 * first, job[6] + c0 * rb, job[8] + first)
        assert (e["in_bpr"], e["pitch"], e["h"]) == (w, job[7], h)
        tw, th = tile_shape(e["w"])
        assert th >= h and e["tpr"] == -(-e["w"] // tw) <= MAX_TILES
        ew = np.array([e[k] for k in ("in", "out", "pitch", "base", "in_bpr", "w", "h", "tpr")], dtype=np.uint64)
        for lt in sorted({0, e["tpr"] // 2, e["tpr"] - 1}):
            lib.bu_emul_rect_tile(target, ew.ctypes.data_as(U64P), lt, has.ctypes.data, src.ctypes.data, dst.ctypes.data, idx.ctypes.data)
            x, y = c0 + lt * tw + lanes % tw, lanes // tw   # column and row inside the whole job
            m = (x < c0 + e["w"]) & (y < h)
            assert (has.astype(bool) == m).all() and m.any()
            sl = (y0 + y[m]) * w + x[m]
            assert (src[m] == np.array(job[0] + 16 * sl, dtype=np.uint64)).all() and (idx[m] == np.array(job[8] + sl, dtype=np.uint64)).all()
            assert (dst[m] == np.array(job[6] + y[m] * rows * job[7] + x[m] * rb, dtype=np.uint64)).all()
        c0 += e["w"]
    assert c0 == w


def test_argument_rules(lib):
    ok = [1 << 40, 200, 7, 3, 65, 17, 1 << 41, 4096, 0]

    def judged(target, **kw):
        j = list(ok)
        for k, v in kw.items():
            j[("d_in", "bpr", "x0", "y0", "w", "h", "d_out", "pitch", "base").index(k)] = v
        return bool(lib.bu_emul_rect_job_ok(target, words([j])[0].ctypes.data_as(U64P)))

    for t in (ASTC, BC7, ETC1, ETC2, RGBA, BC4):
        assert judged(t)
        assert not judged(t, d_in=0) and not judged(t, d_out=0)
        assert not judged(t, w=0) and not judged(t, h=0) and not judged(t, bpr=0)
        assert judged(t, x0=135) and not judged(t, x0=136)          # x0 + w <= in_blocks_per_row
        assert not judged(t, x0=(1 << 32) - 1)                      # (no wrap-around in x0 + w)
        assert not judged(t, d_in=(1 << 40) + 8)                    # d_in 16-byte aligned
        rb = ROW_BYTES[t]
        assert judged(t, pitch=65 * rb) and not judged(t, pitch=65 * rb - rb)   # pitch >= w * block bytes (RGBA32: 16 w)
        assert not judged(t, pitch=4096 + rb // 2) and not judged(t, d_out=(1 << 41) + rb // 2)
        assert judged(t, pitch=4096 + rb, d_out=(1 << 41) + rb)
    # (y0 + h) * in_blocks_per_row <= 2^32
    assert judged(BC7, bpr=1 << 21, x0=0, y0=2048 - 17) and not judged(BC7, bpr=1 << 21, x0=0, y0=2048 - 16)
    assert not judged(BC7, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=65, x0=0)
    # (a product past 2^64 must not wrap back under the bound: this one is 2^64 + 2^32 - 2)
    assert not judged(BC7, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=(1 << 31) + 1, x0=0)
    assert not judged(BC7, y0=(1 << 32) - 1, h=(1 << 32) - 1, bpr=(1 << 32) - 1, x0=0, w=1)
    assert judged(BC7, y0=0, h=1, bpr=(1 << 32) - 1, x0=0, w=1 << 28, pitch=1 << 32) and not judged(BC7, y0=1, h=1, bpr=(1 << 32) - 1, x0=0)
    assert judged(BC7, y0=(1 << 32) - 2, h=1, bpr=1, x0=0, w=1, pitch=16) and judged(BC7, y0=(1 << 32) - 1, h=1, bpr=1, x0=0, w=1, pitch=16)
    assert not judged(BC7, y0=(1 << 32) - 1, h=2, bpr=1, x0=0, w=1, pitch=16)


def test_no_context_is_refused_by_the_library():
    """the one refusal the built library can show without a device (the per-job rules go through the same bu_rect_job_ok: tests/test_gpu_rects.py)"""
    from basisu_rs_amd import _lib

    lib = _lib.load()
    job = _lib.RectJob(1 << 40, 64, 0, 0, 1, 1, 1 << 41, 16, 0)
    assert lib.bu_uastc_transcode_rects_device(None, _lib.BC7, 1, ctypes.byref(job), None, None) == _lib.ERR_ARGUMENT


def test_address_mapping_under_ubsan(tmp_path):
    """the stand-alone build walks every tile of the fixed jobs under -fsanitize=undefined (a report aborts it) and reproduces the numpy offsets"""
    exe = tmp_path / "bu_emul_rects"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas",
                    "-DBU_EMUL_RECTS_MAIN", "-I" + CSRC, "-o", str(exe), SRC], check=True)
    bpr = 1 << 21
    for target in (BC7, ETC1, RGBA):
        jobs = fixed_jobs(target) + [(1 << 40, bpr, bpr - 70, 2047 - 20, 70, 21, 1 << 45, 4096, (1 << 56) - 1)]
        jf, of = tmp_path / ("jobs%d.bin" % target), tmp_path / ("out%d.bin" % target)
        words(jobs).tofile(jf)
        r = subprocess.run([str(exe), str(target), str(jf), str(of)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "clean" in r.stdout, (r.returncode, r.stderr[-2000:])
        rec = np.fromfile(of, dtype=np.uint64).reshape(-1, 5)
        assert (np.diff(rec[:, 0].astype(np.int64)) >= 0).all() and (rec[:, 0] == rec[:, 1] // JOBS_PER_LAUNCH).all()  # 64 jobs per launch, in order
        for j, job in enumerate(jobs):
            g = rec[rec[:, 1] == j]
            es, ed, ei = expected(target, job)
            assert g.shape[0] == es.size
            o, eo = np.argsort(g[:, 3], kind="stable"), np.argsort(ed.ravel(), kind="stable")
            assert (g[o, 3] == ed.ravel()[eo]).all() and (g[o, 2] == es.ravel()[eo]).all() and (g[o, 4] == ei.ravel()[eo]).all()
