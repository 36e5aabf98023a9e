"""The cases of tests/test_gpu_rect_walks.py as data: job tables of bu_uastc_transcode_rects_device whose launches hold more tiles than the grid, so that a
workgroup of the persistent rectangle kernel (layout RECTS of bu_uastc_sorted_body, 512 threads x 2 blocks) walks tile t, t + grid, t + 2 grid, ... ACROSS jobs
-- tiles that differ in width (8 / 16 / 32 / 64 blocks), clipping, source pitch, output pitch and index base -- and whose tiles hold the chosen histograms of
tests/sort_cases.py.  tests/test_rect_walk_cases.py (no GPU) holds that the tables do what they are built for, on the plan the launcher itself uses.

A case is a list of jobs (a function of the CU count) and the content rule of its tiles.  Tiles are never restated here: which tiles a job makes, which launch
and tile number each gets, and which block every lane of a tile holds come from the host build of csrc/bu_rect_plan.hpp (bu_emul_rects_plan, bu_emul_rect_tile:
tests/host_emul/bu_emul_rects.cpp through tests/test_rect_plan.py).  A recipe's key for lane l goes to the block lane l holds; lanes outside the rectangle drop
their keys (a recipe shorter than the tile is continued in its last key).  So a tile clipped only in height keeps its whole uniform waves where both of a wave's
loads are inside, and a tile clipped in width has none: its missing lanes carry key 31.

The jobs of a case cut DISJOINT regions out of three or four slices of different blocks-per-row (a shelf packing: every source block lies in at most one tile; the blocks no
job takes are invalid ones).  Every job has a surface of its own, a pitch of its own (tight, one block of padding, larger ones) and an index base of its own; the
bases fall against the job order in swapped pairs, the LAST job has the lowest.

    every_recipe    no walk (fewer tiles per launch than CUs): every recipe of sc.FULL through a full tile of each shape 8 x 128, 16 x 64, 32 x 32, 64 x 16; the
                    ragged ideas of sc.RAGGED through clipped tiles (a single key over the tile's lane mask)
    walk            one launch of 12 CUs + 38 tiles: three whole rounds and a few tiles more on the largest grid (BC7 / ASTC, exclusive: 4 x CUs), twelve on the
                    smallest; 48 jobs of CUs / 4 tiles each in the order of MATRIX, small jobs in front and behind, the last one a single block
    three_launches  136 jobs: three launches of the shared grid of the 2-per-CU targets, each over two rounds
The content of the walking cases is ("walk", sc.WALKS) through sc.tile_recipe: it depends on the grid, so an input is built per grid."""
import numpy as np

import sort_cases as sc
import test_rect_plan as trp

TILE, WGS, BPT = trp.TILE, 512, 2
WIDTHS = (8, 16, 32, 64)
JOBS_PER_LAUNCH = trp.JOBS_PER_LAUNCH
MAX_BLOCKS = 1 << 21        # blocks of one launch
POLICY_ARG = {sc.EXCL: 0, sc.SHARED: 1}
PADS = (0, 1, 0, 7, 1, 3)   # blocks of padding behind a surface row, by job number
BASE_STEP = 1 << 22         # between two index bases: more than a slice holds
SLICE_BPR = (97, 200, 1037)  # blocks per row of the slices of the narrow (tiles 8 / 16 wide), the 32-wide and the 64-wide jobs; the one-row strips have a fourth
TAIL = 38                   # tiles of `walk` beyond twelve per CU: no multiple of a grid, and the last tile is walk 37 % 5 = 2 (all_invalid) in round 0 of every grid


def row_bytes(name):
    """bytes a block takes of one surface row (RGBA32: of one of its four pixel rows)"""
    return 16 if name == "rgba" else sc.TARGETS[name][1]


def rows_per_block(name):
    return 4 if name == "rgba" else 1


def per_cu(name, policy):
    """workgroups per CU of a rectangle launch (bu_plan_rects_grid)"""
    return (4 if name in ("bc7", "astc") else 2) // (2 if policy == sc.SHARED else 1)


def tile_width(w):
    return next(t for t in WIDTHS if t >= min(w, 64))


def tiles_of(w, h):
    tw = tile_width(w)
    return -(-w // tw) * -(-h // (TILE // tw))


# ---- jobs -------------------------------------------------------------------------------------------------------------------------
def shape(kind, k):
    """(w, h) of a job of `kind` that makes k tiles (w65: k rounded up to even)"""
    if kind == "col1":    # 8 x 128 tiles of one column; the last one five rows short
        return 1, 128 * k - 5
    if kind == "col5":
        return 5, 128 * k
    if kind == "full8":
        return 8, 128 * k
    if kind == "w9":      # 16 x 64 tiles of nine columns; the last one a row short
        return 9, 64 * k - 1
    if kind == "w12":
        return 12, 64 * k
    if kind == "full16":
        return 16, 64 * k
    if kind == "w17":     # 32 x 32 tiles of 17 columns; the last one holds one row
        return 17, 32 * k - 31
    if kind == "pages":   # whole 32 x 32 pages, one below the other
        return 32, 32 * k
    if kind == "w65":     # tiles alternate between 64 x 16 and one column
        return 65, 16 * ((k + 1) // 2)
    if kind == "w40":
        return 40, 16 * k
    if kind == "strip":   # one row of blocks: 64-block tiles, the last one of five
        return 64 * (k - 1) + 5, 1
    assert kind == "full64"
    a = 4 if k % 4 == 0 else 2 if k % 2 == 0 else 1
    return 64 * a, 16 * (k // a)


KINDS = {8: ("col1", "col5", "col1", "full8"), 16: ("w9", "w12", "w9", "full16"), 32: ("w17", "w17", "pages"), 64: ("strip", "w65", "full64", "w65", "strip")}
# tile widths of the 48 main jobs of `walk`, four jobs (= one CU count of tiles) per row: over the rows a -> a + 1, a + 2 and a + 4 (the walk edges of the grids
# of 1, 2 and 4 workgroups per CU) every ordered pair of widths occurs
MATRIX = ((32, 64, 64, 16), (16, 8, 16, 8), (64, 64, 64, 16), (16, 8, 16, 32), (32, 16, 8, 32), (8, 64, 8, 32), (64, 8, 32, 16), (16, 8, 64, 8), (16, 8, 64, 32),
          (32, 8, 8, 32), (64, 32, 64, 64), (16, 16, 32, 32))


def _job(w, h, recipes=None):
    return dict(w=w, h=h, recipes=recipes)


def _place(jobs):
    """slice, origin, padding and index base of every job; returns (jobs, slices [(blocks per row, rows)])"""
    strips = [j["w"] for j in jobs if j["h"] == 1 and j["w"] > 64]
    bpr = list(SLICE_BPR) + [max(strips) + 3 if strips else 67]
    for i, j in enumerate(jobs):
        tw = tile_width(j["w"])
        j["slice"] = 3 if (j["h"] == 1 and j["w"] > 64) else 0 if tw <= 16 else 1 if tw == 32 else 2
        assert j["w"] <= bpr[j["slice"]]
        j["pad"] = PADS[i % len(PADS)]
        r = len(jobs) - 1 - i
        j["base"] = BASE_STEP * (r if r == 0 else ((r - 1) ^ 1) + 1) + 77 * i
    x, y, sh = [0] * 4, [0] * 4, [0] * 4
    for i in sorted(range(len(jobs)), key=lambda i: (jobs[i]["slice"], -jobs[i]["h"], -jobs[i]["w"], i)):  # shelves: the tall jobs first
        j = jobs[i]
        s = j["slice"]
        if x[s] + j["w"] > bpr[s]:
            x[s], y[s], sh[s] = 0, y[s] + sh[s], 0
        j["x0"], j["y0"] = x[s], y[s]
        x[s] += j["w"]
        sh[s] = max(sh[s], j["h"])
    slices = [(bpr[s], y[s] + sh[s]) for s in range(4)]
    assert all(b * r <= BASE_STEP for b, r in slices)
    return jobs, slices


def every_recipe_jobs(cu):
    """jobs of one or two tiles: a shape's full tiles one below the other (64 wide: every other pair side by side), then the clipped ones"""
    jobs = []
    for tw in WIDTHS:
        th, i, two = TILE // tw, 0, False
        while i < len(sc.FULL):
            rs = sc.FULL[i:i + (2 if two else 1)]
            i += len(rs)
            beside = tw == 64 and len(rs) == 2 and len(jobs) % 4 == 0
            jobs.append(_job(tw * (2 if beside else 1), th * (1 if beside else len(rs)), rs))
            two = not two
    r63, r1 = sc.RAGGED
    jobs += [_job(63, 16, (r63,)),                  # 64 x 16: every row -- the last one too -- holds 63 blocks
             _job(65, 16, ("uniform_mix", r1)),      # the second tile holds one block per row
             _job(1, 128, (r1,)),                    # 8 x 128, width-clipped: vc == 1
             _job(64, 17, ("single_5", r63)),        # height-clipped: vr == 1, one whole wave of blocks
             _job(64, 15, (r63,)),                   # vr == 15: seven waves keep both loads
             _job(7, 128, (r63,)), _job(9, 65, (r1, r63)), _job(32, 33, ("single_9", r1)), _job(31, 32, (r63,)), _job(16, 63, (r63,)), _job(8, 127, (r63,))]
    return jobs


def walk_jobs(cu):
    u = cu // 16
    assert u >= 3, "too few CUs for this table"
    k = 4 * u
    used = {tw: 0 for tw in WIDTHS}
    main = []
    for tw in [t for row in MATRIX for t in row]:
        kind = KINDS[tw][used[tw] % len(KINDS[tw])]
        used[tw] += 1
        main.append(_job(*shape(kind, k)))
    rest = 12 * cu - sum(tiles_of(j["w"], j["h"]) for j in main)  # (a CU count that is no multiple of 16)
    front = [_job(32, 32), _job(*shape("w65", 4)), _job(*shape("strip", 6)), _job(32, 32), _job(*shape("w9", 3))]
    back = [_job(*shape("full64", 4)), _job(17, 33), _job(*shape("full8", 3)), _job(*shape("col5", 4)), _job(32, 32), _job(*shape("w40", 5)), _job(1, 257), _job(1, 1)]
    jobs = front + main + ([_job(*shape("col1", rest))] if rest else []) + back
    assert sum(tiles_of(j["w"], j["h"]) for j in front + back) == TAIL
    return jobs


THREE_KINDS = ("col1", "w9", "strip", "w17", "w65", "col5", "w12", "w40", "full8", "pages")


def three_launches_jobs(cu):
    """two launches of 64 jobs and one of eight, each over two rounds of the shared grid of the 2-per-CU targets (one workgroup per CU)"""
    k1, k2 = cu // 32 + 1, cu // 4 + 1
    return [_job(*shape(THREE_KINDS[i % len(THREE_KINDS)], k1)) for i in range(128)] + [_job(*shape(THREE_KINDS[(3 * i) % len(THREE_KINDS)], k2)) for i in range(8)]


WALK_CONTENT = ("walk", sc.WALKS)
CASES = {
    "every_recipe": dict(id="every_recipe", jobs=every_recipe_jobs, content=("jobs",), targets=sc.ALL, policies=(sc.AUTO,)),
    "walk": dict(id="walk", jobs=walk_jobs, content=WALK_CONTENT, targets=sc.ALL, policies=(sc.EXCL, sc.SHARED)),
    "three_launches": dict(id="three_launches", jobs=three_launches_jobs, content=WALK_CONTENT, targets=("etc1", "rgba"), policies=(sc.SHARED,)),
}


# ---- a case on the plan -----------------------------------------------------------------------------------------------------------
IN_AT, OUT_AT = 1 << 40, 1 << 44  # the addresses a table is planned with where no device is at hand


def job_table(name, jobs, slices, in_ptrs=None, out_ptrs=None):
    """the call's job list: (in, in_bpr, x0, y0, w, h, out, pitch, index_base)"""
    rb = row_bytes(name)
    return [(in_ptrs[j["slice"]] if in_ptrs else IN_AT + (j["slice"] << 36), slices[j["slice"]][0], j["x0"], j["y0"], j["w"], j["h"],
             out_ptrs[i] if out_ptrs else OUT_AT + (i << 32), (j["w"] + j["pad"]) * rb, j["base"]) for i, j in enumerate(jobs)]


def surface_bytes(name, j):
    return rows_per_block(name) * j["h"] * (j["w"] + j["pad"]) * row_bytes(name)


_GEOMETRY = {}


class Geometry:
    """the jobs of a case placed for a CU count, and per job the lanes of its tiles as the kernel maps them: tiles[job][local tile] = (has [1024] bool, slice index
    [1024]); the same for every target and policy"""

    def __init__(self, lib, c, cu):
        self.case, self.cu = c, cu
        self.jobs, self.slices = _place(c["jobs"](cu))
        table = job_table("etc1", self.jobs, self.slices)
        self.tiles = []
        has, src, dst, idx = np.zeros(TILE, np.uint8), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64), np.zeros(TILE, np.uint64)
        ents = [e for _, es in trp.plan(lib, sc.TARGETS["etc1"][0], table, 0, cu) for e in es]
        assert [e["job"] for e in ents] == list(range(len(self.jobs))), "one table entry per job"
        for e, j, row in zip(ents, self.jobs, table):
            ew = np.array([e[k] for k in ("in", "out", "pitch", "base", "in_bpr", "w", "h", "tpr")], dtype=np.uint64)
            out = []
            for lt in range(tiles_of(j["w"], j["h"])):
                lib.bu_emul_rect_tile(sc.TARGETS["etc1"][0], ew.ctypes.data_as(trp.U64P), lt, has.ctypes.data, src.ctypes.data, dst.ctypes.data, idx.ctypes.data)
                m = has.astype(bool)
                sidx = (idx - np.uint64(j["base"])).astype(np.int64)
                assert (src[m] == np.uint64(row[0]) + np.uint64(16) * sidx[m].astype(np.uint64)).all()
                out.append((m, np.where(m, sidx, -1)))
            self.tiles.append(out)


def geometry(lib, c, cu):
    if (c["id"], cu) not in _GEOMETRY:
        _GEOMETRY[c["id"], cu] = Geometry(lib, c, cu)
    return _GEOMETRY[c["id"], cu]


def launches_of(lib, geo, name, policy):
    """the plan of the case's one call for a target under a policy (sc.EXCL / sc.SHARED): [dict(n_tiles, grid, tiles [(tile number, job, local tile)])]"""
    out = []
    for l, ents in trp.plan(lib, sc.TARGETS[name][0], job_table(name, geo.jobs, geo.slices), POLICY_ARG[policy], geo.cu):
        tiles = []
        for e in ents:
            n = tiles_of(e["w"], e["h"])
            assert (e["w"], e["h"]) == (geo.jobs[e["job"]]["w"], geo.jobs[e["job"]]["h"]) and n == len(geo.tiles[e["job"]])
            tiles += [(e["first_tile"] + lt, e["job"], lt) for lt in range(n)]
        assert [t for t, _, _ in tiles] == list(range(l["n_tiles"])) and l["grid"] == min(l["n_tiles"], per_cu(name, policy) * geo.cu)
        out.append(dict(n_tiles=l["n_tiles"], grid=l["grid"], tiles=tiles))
    return out


def walks(launches, rounds):
    """None, or why a launch does not walk: every one holds at least rounds x grid + 1 tiles"""
    for i, l in enumerate(launches):
        if l["n_tiles"] < rounds * l["grid"] + 1:
            return "launch %d: %d tiles on a grid of %d, fewer than %d rounds and a tile" % (i, l["n_tiles"], l["grid"], rounds)
    return None


def condition(c, launches, cu):
    """None, or which tile-count condition of case c its planned launches miss"""
    if c["id"] == "every_recipe":
        bad = [l["n_tiles"] for l in launches if l["n_tiles"] >= cu or l["grid"] != l["n_tiles"]]
        return "a launch of %d tiles on %d CUs walks" % (bad[0], cu) if bad else None
    if c["id"] == "walk":
        (l,) = launches
        return walks(launches, 3) or ("%d tiles are whole rounds of the grid %d" % (l["n_tiles"], l["grid"]) if l["n_tiles"] % l["grid"] == 0 else None)
    return walks(launches, 2) or (None if len(launches) == 3 else "%d launches" % len(launches))


_KEYS = {}


def lane_keys(rid):
    """the recipe's piece key of every lane of a 1024-block tile (a recipe that is short of the tile continued in its last key)"""
    if rid not in _KEYS:
        k = sc.recipe_keys(rid, TILE)
        _KEYS[rid] = np.concatenate([k, np.full(TILE - k.size, k[-1], dtype=k.dtype)])
    return _KEYS[rid]


def recipe_of(c, geo, l, t, job, lt):
    if c["content"][0] == "jobs":
        return geo.jobs[job]["recipes"][lt]
    return sc.tile_recipe(c["content"], None, t, l["grid"], TILE, TILE)


def fill(c, geo, launches, tb):
    """pool indices of every slice's blocks, [rows x blocks per row] each: every tile laid out by its recipe over the lanes that hold a block; -1: in no tile"""
    idx = [np.full(b * r, -1, dtype=np.int64) for b, r in geo.slices]
    for l in launches:
        for t, job, lt in l["tiles"]:
            m, sidx = geo.tiles[job][lt]
            s = geo.jobs[job]["slice"]
            where = sidx[m]
            assert (idx[s][where] == -1).all(), "job %d, tile %d: a block of another tile" % (job, lt)
            idx[s][where] = tb.pool_index(lane_keys(recipe_of(c, geo, l, t, job, lt))[m], where + (s << 24))
    return idx


def job_region(geo, idx, job):
    """the pool indices of a job's rectangle, (h, w): a view of its slice"""
    j = geo.jobs[job]
    bpr, rows = geo.slices[j["slice"]]
    return idx[j["slice"]].reshape(rows, bpr)[j["y0"]:j["y0"] + j["h"], j["x0"]:j["x0"] + j["w"]]


def lowest_failure(geo, idx, pool_st):
    """None, or (status index, status, job, slice index) of the failing block with the lowest index_base + slice index"""
    best = None
    for i, j in enumerate(geo.jobs):
        reg = job_region(geo, idx, i)
        bad = np.nonzero(pool_st[reg].reshape(-1))[0]
        if bad.size:
            y, x = divmod(int(bad[0]), j["w"])
            sidx = (j["y0"] + y) * geo.slices[j["slice"]][0] + j["x0"] + x
            if best is None or j["base"] + sidx < best[0]:
                best = (j["base"] + sidx, int(pool_st[reg[y, x]]), i, sidx)
    return best


def word_of(first):
    return sc.CLEAR if first is None else (first[0] << 8) | first[1]


def heal(geo, idx, tb, first):
    """the failing block `first` replaced by a valid one"""
    idx[geo.jobs[first[2]]["slice"]][first[3]] = int(tb.cost_order[0]) * 32
