"""The cases of tests/test_gpu_etc1s_walks.py as data: ETC1S launches whose waves take a second and a third step of their grid-stride loop.  Pure numpy, shared
with tests/test_etc1s_walk_cases.py (no GPU), which holds on the host build of the launch plan that the tables do what they are built for.  It mirrors
tests/rect_walk_cases.py.

Every case is a function of the CU count `cu`; a ROUND is what one step of a whole grid covers (bu_grid_for: at most 8 x cu workgroups of 256 threads):
    U = 8 cu x 4      units of 64 blocks: the wave-per-unit kernels (bu_etc1s_rects_kernel, bu_etc1s_file_kernel, bu_etc1s_file_target_kernel)
    B = 8 cu x 256    blocks: the L2-gather slice kernels (bu_etc1s_etc1_kernel, bu_etc1s_rgba_kernel, bu_etc1s_target_kernel<T, false>)
    W = cu x 16       chunks of 256 blocks: the four-blocks-per-lane path of bu_etc1s_staged_kernel<false> (cu workgroups of 16 waves)

1. Rectangle job tables (bu_etc1s_transcode_rects_device).  A job is w x h blocks cut from one of three slices of 65, 33 and 200 blocks per row; the jobs of a
   slice lie one below the other (every source block in at most one job; the rows between two jobs belong to none), each job has a surface of its own, one of
   three pitches, an alpha slice if its number is odd, and an index base of its own -- the bases fall against the job order, so a late job has a low base.
   Sizes are multiples of q = cu / 2 units:
       three_rounds   64 jobs, 149 q + 7 (or 6) units: two whole rounds and a ragged third that ends inside a workgroup.  Wave slot 0 (WALK_SLOT) takes unit 0 in
                      job 0 (3 wide: units of 4 x 16, slice of 65), unit U in job 24 (17 wide: 32 x 2, slice of 33) and unit 2 U in job 48 (130 wide: 64 x 1,
                      slice of 200), at three pitches
       two_launches   the same 64 jobs and three more of 68 q units: a second launch of three table entries over more than a round
   status_blocks plants a bad endpoint index in a third-round unit of a late job, a bad selector index in a first-round unit of an early one (a higher index
   base), a bad alpha index in a second-round unit, and a bad index in a row no job takes.
2. Whole files (the one-launch door of bu_read_to / bu_read_file_to): file_dims(cu), images of mostly 1 x 1 blocks -- a unit never spans images -- with one in
   sixteen out of SPECIAL, about 2 U + U / 3 units in at most FILE_MAX_BLOCKS blocks.
3. Slice kernels: staged_case(cu) for the staged ETC1 kernel, gather_case(cu) for the gather kernels: sizes and the blocks that get a bad index.

The content of every large index array is a pool of POOL distinct colour / alpha index pairs in a scrambled order (pool_order): expected bytes are modelled once
per pool and gathered."""
import numpy as np

UNIT, WAVES_PER_WG, JOBS_PER_LAUNCH = 64, 4, 64
TARGETS = {"etc1": 2, "rgba": 4, "bc1": 11, "bc3": 12, "bc4": 6, "bc5": 7, "r11": 8, "rg11": 9}   # bu_target numbers
BLOCK_BYTES = {"etc1": 8, "rgba": 64, "bc1": 8, "bc3": 16, "bc4": 8, "bc5": 16, "r11": 8, "rg11": 16}
POOL = 16384
N_EP = N_SEL = 24000  # the codebooks of the rectangle and the gather cases
LDS_MAX, STAGED_MIN = 155648, 1 << 19   # BU_ETC1S_LDS_MAX, BU_ETC1S_STAGED_MIN
STAGED_EP, STAGED_SEL = 4096, 8192      # the codebooks of the staged ETC1 case: 48 KiB of LDS


def round_units(cu):
    return 8 * cu * WAVES_PER_WG


def round_blocks(cu):
    return 8 * cu * 256


def round_chunks(cu):
    return cu * 16


def grid_for(n_blocks, cu):
    """bu_grid_for, restated"""
    return max(1, min(-(-n_blocks // 256), 8 * cu))


def pool_order(n, salt=0):
    """pool entry of block i of an array of n blocks"""
    return (np.arange(n, dtype=np.int64) * 7919 + 13 + 1009 * salt) % POOL


# ---- 1. rectangles ----------------------------------------------------------------------------------------------------------------
SLICE_BPR = (65, 33, 200)
PITCHES = ("tight", "padded", "4096")
BASE_STEP = 1 << 24   # between two index bases: more than a slice holds
WALK_SLOT = 0         # the wave slot whose three steps the tables are built around
# (w, units / q) of the first 63 jobs of three_rounds: 24 jobs of 62 q units, job 24 over unit U = 64 q, 23 jobs up to 126 q, job 48 over unit 2 U = 128 q and
# 14 jobs of 20 q.  (130-wide jobs have three units per row and 65-wide ones two: their multiples make whole rows.)
_NINE_A = ((3, 2), (1, 1), (2, 1), (9, 3), (33, 3), (64, 3), (65, 4), (130, 3), (17, 3))
_ROUND0 = _NINE_A + _NINE_A + ((3, 2), (9, 3), (33, 3), (64, 3), (65, 2), (130, 3))
_NINE_B = ((1, 1), (2, 1), (33, 3), (64, 3), (65, 4), (130, 3), (9, 3), (3, 2), (17, 3))
_ROUND1 = _NINE_B + _NINE_B + ((33, 3), (64, 3), (9, 3), (65, 4), (2, 1))
_ROUND2 = ((33, 2), (1, 1), (65, 2), (2, 1), (64, 1), (9, 1), (17, 1), (3, 1), (33, 2), (130, 3), (1, 1), (65, 2), (64, 1), (9, 1))
THREE_ROUNDS = _ROUND0 + ((17, 4),) + _ROUND1 + ((130, 3),) + _ROUND2
SECOND_LAUNCH = ((65, 32), (33, 24), (130, 12))
WIDTHS = (1, 2, 3, 9, 17, 33, 64, 65, 130)
assert len(THREE_ROUNDS) == 63 and sum(m for _, m in _ROUND0) == 62 and sum(m for _, m in _ROUND1) == 60 and sum(m for _, m in THREE_ROUNDS) == 149
assert {w for w, _ in THREE_ROUNDS} == set(WIDTHS)


def unit_shape(w):
    """blocks a unit is wide and high: the smallest power of two not below min(w, 64), and 64 over it"""
    uw = next(1 << k for k in range(7) if (1 << k) >= min(w, 64))
    return uw, UNIT // uw


def units_of(w, h):
    uw, uh = unit_shape(w)
    return -(-w // uw) * -(-h // uh)


def row_bytes(name):
    """bytes a block takes of one surface row (RGBA32: of one of its four pixel rows)"""
    return 16 if name == "rgba" else BLOCK_BYTES[name]


def rows_per_block(name):
    return 4 if name == "rgba" else 1


def pitch_of(name, j):
    rb, w = row_bytes(name), j["w"]
    return {"tight": w * rb, "padded": -(-(w * rb + rb + 48) // rb) * rb, "4096": max(4096, w * rb)}[j["pitch"]]


def surface_bytes(name, j):
    return rows_per_block(name) * j["h"] * pitch_of(name, j)


def _place(sized):
    """the jobs of [(w, units)], placed: the slice by width, one job below the other with i % 3 rows between, left / middle / right in the slice, the bottom row
    of units of every other job clipped where a unit is more than a row high; returns (jobs, slices [(blocks per row, rows)])"""
    jobs, rows = [], [0, 0, 0]
    for i, (w, units) in enumerate(sized):
        uw, uh = unit_shape(w)
        upr = -(-w // uw)
        assert units > 0 and units % upr == 0, (w, units)
        h = (units // upr) * uh - ((5 * i + 1) % uh if i % 2 else 0)
        s = 2 if w > 65 else 0 if w in (64, 65, 1, 3, 9) else 1
        y0 = rows[s] + i % 3
        rows[s] = y0 + h
        jobs.append(dict(w=w, h=h, slice=s, x0=(SLICE_BPR[s] - w) * (i % 3) // 2, y0=y0, alpha=i % 2 == 1, pitch=PITCHES[(i % 3 + i // 24) % 3]))
        assert units_of(w, h) == units
    for i, j in enumerate(jobs):
        j["base"] = (len(jobs) - 1 - i) * BASE_STEP + 77 * i
    slices = [(SLICE_BPR[s], rows[s] + 2) for s in range(3)]
    assert all(b * r <= BASE_STEP for b, r in slices)
    return jobs, slices


def _sized(cu):
    q = max(cu // 2, 1)
    total = 149 * q
    return [(w, m * q) for w, m in THREE_ROUNDS] + [(33, 7 if (total + 7) % 4 else 6)]


def three_rounds_jobs(cu):
    return _place(_sized(cu))


def two_launches_jobs(cu):
    q = max(cu // 2, 1)
    return _place(_sized(cu) + [(w, m * q) for w, m in SECOND_LAUNCH])


RECT_CASES = {"three_rounds": three_rounds_jobs, "two_launches": two_launches_jobs}
IDX_AT, AIDX_AT, OUT_AT = 1 << 40, 3 << 40, 1 << 44   # the addresses a table is planned with where no device is at hand


def job_table(name, jobs, slices, idx_ptrs=None, aidx_ptrs=None, out_ptrs=None):
    """the call's job list: (d_idx, d_alpha_idx or 0, in_blocks_per_row, x0, y0, w, h, d_out, pitch, index_base); ETC1 takes no alpha slice"""
    rows = []
    for i, j in enumerate(jobs):
        s = j["slice"]
        aidx = 0 if name == "etc1" or not j["alpha"] else (aidx_ptrs[s] if aidx_ptrs else AIDX_AT + (s << 36))
        rows.append((idx_ptrs[s] if idx_ptrs else IDX_AT + (s << 36), aidx, slices[s][0], j["x0"], j["y0"], j["w"], j["h"],
                     out_ptrs[i] if out_ptrs else OUT_AT + (i << 34), pitch_of(name, j), j["base"]))
    return rows


def launches_of(jobs):
    """the plan, restated: up to 64 jobs per launch in order, a job's units behind those of the jobs in front of it: [dict(first_job, n_jobs, first_unit [per
    job], n_units)]"""
    out = []
    for a in range(0, len(jobs), JOBS_PER_LAUNCH):
        units = [units_of(j["w"], j["h"]) for j in jobs[a:a + JOBS_PER_LAUNCH]]
        first = np.concatenate([[0], np.cumsum(units)]).astype(np.int64)
        out.append(dict(first_job=a, n_jobs=len(units), first_unit=first[:-1], n_units=int(first[-1])))
    return out


def unit_job(l, unit):
    """the job (number in the call) that holds a launch's unit, and the unit's number inside it"""
    r = int(np.searchsorted(l["first_unit"], unit, side="right")) - 1
    return l["first_job"] + r, unit - int(l["first_unit"][r])


def unit_is_clipped(j, lu):
    uw, uh = unit_shape(j["w"])
    upr = -(-j["w"] // uw)
    uy, ux = divmod(lu, upr)
    return (ux + 1) * uw > j["w"] or (uy + 1) * uh > j["h"]


def unit_of_block(l, jobs, job, x, y):
    """the launch's unit number of block (x, y) of a job"""
    j = jobs[job]
    uw, uh = unit_shape(j["w"])
    return int(l["first_unit"][job - l["first_job"]]) + (y // uh) * -(-j["w"] // uw) + x // uw


def slot_steps(l, jobs, cu, slot=WALK_SLOT):
    """the jobs (numbers in the call) of the units a wave slot takes: slot, slot + U, slot + 2 U, ..."""
    return [unit_job(l, u)[0] for u in range(slot, l["n_units"], round_units(cu))]


def slot_facts(jobs, slices, steps):
    """what must change from step to step of a wave slot, per step: the job, its unit shape, its slice's blocks per row, its pitch kind and pitch in bytes"""
    a = [jobs[k] for k in steps]
    facts = {"job": list(steps), "unit shape": [unit_shape(j["w"]) for j in a], "in_blocks_per_row": [slices[j["slice"]][0] for j in a],
             "pitch kind": [j["pitch"] for j in a]}
    for name in TARGETS:
        facts["pitch of " + name] = [pitch_of(name, j) for j in a]
    return facts


def rect_condition(case, cu):
    """None, or what the case's table misses of what it is built for on `cu` CUs"""
    jobs, slices = RECT_CASES[case](cu)
    ls, U = launches_of(jobs), round_units(cu)
    for i, l in enumerate(ls):
        if grid_for(l["n_units"] * UNIT, cu) != 8 * cu:
            return "launch %d: %d units do not fill the grid" % (i, l["n_units"])
    if case == "two_launches":
        if len(ls) != 2 or ls[1]["n_jobs"] >= 8:
            return "%d launches, the last of %d jobs" % (len(ls), ls[-1]["n_jobs"])
        return next(("launch %d: %d units, no more than a round of %d" % (i, l["n_units"], U) for i, l in enumerate(ls) if l["n_units"] <= U), None)
    (l,) = ls
    n = l["n_units"]
    if not (len(jobs) == JOBS_PER_LAUNCH and 2 * U < n < 3 * U):
        return "%d jobs, %d units: not three rounds of %d in one launch" % (len(jobs), n, U)
    if n % U == 0 or n % WAVES_PER_WG == 0:
        return "%d units end with a workgroup" % n
    steps = slot_steps(l, jobs, cu)
    if len(steps) != 3:
        return "wave slot %d takes %d steps" % (WALK_SLOT, len(steps))
    facts = slot_facts(jobs, slices, steps)
    for key, values in facts.items():
        if len(set(values)) != 3:  # (three different values: every step changes it)
            return "the steps of wave slot %d do not differ in %s: %s" % (WALK_SLOT, key, values)
    if not any(unit_is_clipped(jobs[k], lu) for k, lu in (unit_job(l, u) for u in range(2 * U, n))):
        return "no clipped unit in the last round"
    if {j["w"] for j in jobs} != set(WIDTHS) or {j["pitch"] for j in jobs} != set(PITCHES):
        return "widths or pitches are missing"
    return None


# the blocks of three_rounds that get a bad index: (job, x, y) -- the last block of a job of the third round, a block of an early job, a block of a
# second-round job that has an alpha slice -- and (slice, row offset below job 1's rectangle start, x): a block of a row between two jobs
BAD_ENDPOINT, BAD_SELECTOR, BAD_ALPHA = (57, 32, -1), (3, 5, 7), (31, 8, 2)


def status_blocks(jobs, slices):
    """dict(endpoint, selector, alpha, outside) -> (slice, slice index) of the planted blocks, with their (job, x, y) under the same keys + "_at" """
    out = {}
    for key, (job, x, y) in (("endpoint", BAD_ENDPOINT), ("selector", BAD_SELECTOR), ("alpha", BAD_ALPHA)):
        j = jobs[job]
        y = y % j["h"]
        assert x < j["w"]
        out[key] = (j["slice"], (j["y0"] + y) * slices[j["slice"]][0] + j["x0"] + x)
        out[key + "_at"] = (job, x, y)
    j = jobs[1]  # (its i % 3 = 1: one row above it belongs to no job)
    out["outside"] = (j["slice"], (j["y0"] - 1) * slices[j["slice"]][0] + j["x0"])
    return out


def job_of_block(jobs, slices, s, sidx):
    """None, or the job whose rectangle holds block sidx of slice s"""
    y, x = divmod(sidx, slices[s][0])
    hits = [i for i, j in enumerate(jobs) if j["slice"] == s and j["x0"] <= x < j["x0"] + j["w"] and j["y0"] <= y < j["y0"] + j["h"]]
    assert len(hits) <= 1
    return hits[0] if hits else None


def status_condition(cu):
    """None, or what the planted blocks of three_rounds miss on `cu` CUs: their rounds, and the order of their status indices"""
    jobs, slices = three_rounds_jobs(cu)
    (l,), U, sb = launches_of(jobs), round_units(cu), status_blocks(*three_rounds_jobs(cu))
    rounds, index = {}, {}
    for key in ("endpoint", "selector", "alpha"):
        job, x, y = sb[key + "_at"]
        if job_of_block(jobs, slices, *sb[key]) != job:
            return "the %s block is not in job %d" % (key, job)
        rounds[key] = unit_of_block(l, jobs, job, x, y) // U
        index[key] = jobs[job]["base"] + sb[key][1]
    if rounds != dict(endpoint=2, selector=0, alpha=1):
        return "rounds %s" % rounds
    if not (index["endpoint"] < index["alpha"] < index["selector"]):
        return "status indices %s" % index
    if not jobs[BAD_ALPHA[0]]["alpha"]:
        return "job %d has no alpha slice" % BAD_ALPHA[0]
    if job_of_block(jobs, slices, *sb["outside"]) is not None:
        return "the outside block lies in a job"
    return None


def lowest_status_index(name, jobs, slices, sb):
    """index_base + slice index of the failing block the status word names (ETC1 reads no alpha slice)"""
    keys = ("endpoint", "selector") + (() if name == "etc1" else ("alpha",))
    return min(jobs[sb[k + "_at"][0]]["base"] + sb[k][1] for k in keys)


# ---- 2. whole files ---------------------------------------------------------------------------------------------------------------
SPECIAL = ((3, 2), (13, 5), (65, 1), (1, 64), (9, 15))   # blocks: 6 (one unit), 65 (two, one block in the second), 65, 64 (one whole unit), 135 (three)
FILE_MAX_BLOCKS = 100000
FILE_CODEBOOK = 512


def file_dims(cu):
    """(blocks wide, blocks high) per image: 1 x 1, image 5 of every sixteen (and image 6 of every 1024, next to it) out of SPECIAL in turn, until the units
    -- ceil(blocks / 64) per image -- reach 2 U + U / 3"""
    want = 2 * round_units(cu) + round_units(cu) // 3
    dims, units, k = [], 0, 0
    while units < want:
        i = len(dims)
        if i % 16 == 5 or i % 1024 == 6:
            dims.append(SPECIAL[k % len(SPECIAL)])
            k += 1
        else:
            dims.append((1, 1))
        units += -(-dims[-1][0] * dims[-1][1] // UNIT)
    return dims


def file_units(dims):
    """units of the one-launch door: ceil(blocks / 64) per non-empty image"""
    return sum(-(-w * h // UNIT) for w, h in dims if w * h)


def file_condition(cu):
    dims = file_dims(cu)
    n, U = file_units(dims), round_units(cu)
    if not (2 * U < n < 3 * U and n % U):
        return "%d units: not three ragged rounds of %d" % (n, U)
    if grid_for(n * UNIT, cu) != 8 * cu:
        return "the grid is not full"
    special = [d != (1, 1) for d in dims]
    if sum(special) * 16 < len(dims) or {d for d in dims if d != (1, 1)} != set(SPECIAL):
        return "fewer than one image in sixteen out of SPECIAL"
    if not any(a and b for a, b in zip(special, special[1:])):
        return "no two multi-unit images next to each other"
    return None


# ---- 3. slice kernels -------------------------------------------------------------------------------------------------------------
def staged_case(cu):
    """the staged ETC1 kernel, four blocks per lane: 2 W + W / 2 + 3 chunks of 256 blocks and 77 more (at least 2^19 blocks: the launcher stages from there).
    Chunk c is step c // W of wave c % W.  bad_selector: lane 9's fourth block (+129) of a third-step chunk; bad_endpoint: lane 20's first block of the
    second-step chunk of the SAME wave -- the lower block"""
    W = round_chunks(cu)
    chunks = max(2 * W + W // 2 + 3, STAGED_MIN // 256 + 3)
    return dict(n=chunks * 256 + 77, chunks=chunks, W=W, bad_selector=(2 * W + 5) * 256 + 2 * 9 + 129, bad_endpoint=(W + 5) * 256 + 2 * 20)


def staged_condition(cu):
    c = staged_case(cu)
    W, n = c["W"], c["n"]
    if n < STAGED_MIN or (STAGED_EP + STAGED_SEL) * 4 > LDS_MAX:
        return "%d blocks are not staged" % n
    if not (c["chunks"] > 2 * W and c["chunks"] % W and n % 256):
        return "%d chunks: no ragged third step on %d waves" % (c["chunks"], W)
    lo, hi = c["bad_endpoint"], c["bad_selector"]
    if not (lo < hi < c["chunks"] * 256 and lo // 256 // W == 1 and hi // 256 // W == 2 and (lo // 256) % W == (hi // 256) % W and hi % 256 == 2 * 9 + 129):
        return "the bad blocks are not in steps 1 and 2 of one wave"
    return None


RGBA_NBX = 1037   # blocks per row of the RGBA32 gather case: no power of two, no divisor of a round, so block rows straddle rounds


def gather_case(cu, name="bc1"):
    """the gather kernels: 2 B + B / 2 + 77 blocks (RGBA32: the next multiple of RGBA_NBX).  late: a block of the last, partial round; early: one of round one"""
    B = round_blocks(cu)
    n = 2 * B + B // 2 + 77
    if name == "rgba":
        n = -(-n // RGBA_NBX) * RGBA_NBX
    return dict(n=n, B=B, late=2 * B + B // 4 + 33, early=B + 3 * (B // 4) + 130)


def gather_condition(cu, name="bc1"):
    c = gather_case(cu, name)
    n, B = c["n"], c["B"]
    if (N_EP + N_SEL + 256) * 4 <= LDS_MAX:
        return "the codebooks fit LDS"
    if not (2 * B < n < 3 * B and n % B and grid_for(n, cu) == 8 * cu):
        return "%d blocks: not two rounds of %d and a ragged third" % (n, B)
    if not (c["early"] // B == 1 and c["late"] // B == 2 and c["late"] < n):
        return "the bad blocks are not in rounds 1 and 2"
    if name == "rgba" and (B % RGBA_NBX == 0 or RGBA_NBX & (RGBA_NBX - 1) == 0 or n % RGBA_NBX):
        return "block rows do not straddle rounds"
    return None
