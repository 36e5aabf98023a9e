"""The cases of tests/test_gpu_sort_cases.py as data: what every TILE of a launch holds, chosen on purpose.  The mode-sorted kernel
(csrc/bu_kernels.hpp, bu_uastc_sorted_body, phases A-D) is the one piece of orchestration whose control flow depends on the data: a counting sort by
mode whose rank path, run / chunk map and switch depend on the tile's histogram of sort keys.  tests/guard_cases.py chooses the launch shapes and feeds
them a uniform mode mix; here a RECIPE says which keys a tile holds and where, and a CASE is a launch shape plus the recipes of its tiles.
tests/test_sort_cases.py (no GPU) restates the sort's bookkeeping in numpy, holds that every recipe reaches the edge it is named for at every tile
size it is used with, that the cases reach every kernel the launch plan can choose, and that the host build of the block code gives the expected bytes.

A recipe is a list of sections, each an ordered list of (key, count) pieces and a layout:
    contiguous   the pieces back to back (counts that are multiples of 64 make whole waves uniform)
    interleaved  round-robin over the pieces until each is used up (no wave is uniform while two pieces last)
    shuffled     the pieces in a fixed pseudo-random order
A key is a position in the target's row of BU_COST_ORDER (0 = the dearest code path, 18 the cheapest, 19 = the invalid mode codes): the row and the
key_lut come from the host build (bu_emul_sort_tables), nothing here copies them.  BAD_PATTERN + m stands for a block of UASTC mode m whose pattern
index is out of range: it sorts under its own mode's key and fails inside the block code.

Blocks come from a POOL: the 608 known-answer vectors (32 per mode: vector 32 m + v is of mode m), 64 blocks of mode code 69 with random bits behind
it, 16 out-of-range patterns each for modes 3 and 7.  A case's input is a gather of the pool, its expected bytes the same gather of the pool's
expected blocks (golden results / the numpy models of the golden RGBA32; zeros for the failing ones), its status word the lowest failing block."""
import numpy as np

import guard_cases as gc
from basisu_rs_amd import synth

TARGETS, ALL, ETC_FAMILY, BLOCK_LINEAR = gc.TARGETS, gc.ALL, gc.ETC_FAMILY, gc.BLOCK_LINEAR
EXCL, SHARED, AUTO, EVERY_POLICY, POLICY_ARGS = gc.EXCL, gc.SHARED, gc.AUTO, gc.EVERY_POLICY, gc.POLICY_ARGS
TILE, TICKET_WALK, PER_CU = gc.TILE, gc.TICKET_WALK, gc.PER_CU
TICKET_TARGETS = ("bc7", "astc", "rgba")
INVALID, NO_BLOCK = 19, 31  # the run of the invalid mode codes; the key of a lane without a block
BAD_PATTERN = 100           # piece key BAD_PATTERN + m
PATTERN_MODES = (3, 7)
CONT, INTER, SHUF = "contiguous", "interleaved", "shuffled"
CLEAR = 0xFFFFFFFFFFFFFFFF
ST_BAD_MODE, ST_BAD_PATTERN = 1, 2

# ---- the pool -------------------------------------------------------------------------------------------------------------------
N_GOLD, N_BAD_MODE, N_BAD_PAT = 608, 64, 16
POOL_BAD_MODE = N_GOLD
POOL_BAD_PAT = {m: N_GOLD + N_BAD_MODE + i * N_BAD_PAT for i, m in enumerate(PATTERN_MODES)}
N_POOL = N_GOLD + N_BAD_MODE + N_BAD_PAT * len(PATTERN_MODES)


def bad_pattern_blocks(mode, n, rng):
    """blocks of `mode` with the pattern field at or above the mode's pattern count, random bits behind it (synth.atlas_err builds mode 3 / pattern 15 so)"""
    code_size, tf_bits, pat_bits, pat_count = synth._PATTERN_FIELD[mode]
    code = [c for c in range(1 << code_size) if synth._mode_lut()[c] == mode][0]
    blocks = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    lo = blocks[:, :8].copy().view("<u8").reshape(-1)
    pos = np.uint64(code_size + tf_bits)
    pat = rng.integers(pat_count, 1 << pat_bits, size=n).astype(np.uint64)
    lo &= ~np.uint64((1 << code_size) - 1) & ~(np.uint64((1 << pat_bits) - 1) << pos)
    lo |= np.uint64(code) | (pat << pos)
    blocks[:, :8] = lo.view(np.uint8).reshape(-1, 8)
    return blocks


def pool_blocks(golden_uastc):
    """[N_POOL, 16] input blocks and their statuses (0 / ST_BAD_MODE / ST_BAD_PATTERN)"""
    assert golden_uastc.shape == (N_GOLD, 16)
    assert (synth.block_modes(golden_uastc) == np.repeat(np.arange(19), 32)).all()
    rng = np.random.default_rng(0x50F7)
    bad_mode = rng.integers(0, 256, size=(N_BAD_MODE, 16), dtype=np.uint8)
    bad_mode[:, 0] = (bad_mode[:, 0] & 0x80) | 69
    parts = [golden_uastc, bad_mode] + [bad_pattern_blocks(m, N_BAD_PAT, rng) for m in PATTERN_MODES]
    st = np.zeros(N_POOL, dtype=np.uint8)
    st[POOL_BAD_MODE:POOL_BAD_MODE + N_BAD_MODE] = ST_BAD_MODE
    st[POOL_BAD_MODE + N_BAD_MODE:] = ST_BAD_PATTERN
    return np.ascontiguousarray(np.concatenate(parts)), st


def pool_expected(good):
    """the pool's expected blocks from the 608 expected blocks of the known-answer vectors: failing blocks are written as zeros"""
    return np.ascontiguousarray(np.concatenate([good, np.zeros((N_POOL - N_GOLD, good.shape[1]), dtype=np.uint8)]))


# ---- recipes --------------------------------------------------------------------------------------------------------------------
RECIPES = {}


def recipe(id, sections, short=0, layout_free=False):
    """sections: T -> [(layout, [(key, count), ...]), ...] for a tile of T blocks (a multiple of 64); short: blocks the recipe leaves off the tile's end (the
    ragged last tile of a slice or run); layout_free: one section whose layout the case table names ("id@contiguous", "id@interleaved")"""
    assert id not in RECIPES
    RECIPES[id] = dict(id=id, sections=sections, short=short, layout_free=layout_free)


def _lay(layout, pieces, T):
    keys = np.concatenate([np.full(c, k, dtype=np.int64) for k, c in pieces if c > 0])
    if layout == CONT:
        return keys
    if layout == INTER:  # the j-th block of piece i goes out in round j, after the j-th blocks of the pieces before it
        rounds = np.concatenate([np.arange(c, dtype=np.int64) for _, c in pieces if c > 0])
        return keys[np.argsort(rounds, kind="stable")]
    assert layout == SHUF
    return keys[np.random.default_rng(T).permutation(keys.size)]


def recipe_keys(rid, T):
    """the piece keys of recipe `rid` ("id" or "id@layout") in a tile of T blocks, in the tile's own block order: [T - short] of 0..19 / BAD_PATTERN + m"""
    name, _, layout = rid.partition("@")
    r = RECIPES[name]
    assert T % 64 == 0 and bool(layout) == r["layout_free"], rid
    out = np.concatenate([_lay(layout or lay, pieces, T) for lay, pieces in r["sections"](T)])
    assert out.size == T - r["short"], (rid, T, out.size)
    return out


def _even(keys, total):
    """`total` blocks over `keys` as evenly as they go"""
    q, rem = divmod(total, len(keys))
    return [(k, q + (i < rem)) for i, k in enumerate(keys)]


def _max_chunks(keys):
    """every run but the last of `keys` holds 1 (mod 64) blocks -- alternately 65 and 1 --, the last one the rest: len(keys) - 1 more chunks than T / 64"""
    def sections(T):
        pieces = [(k, 65 if i % 2 == 0 else 1) for i, k in enumerate(keys[:-1])]
        return [(INTER, pieces + [(keys[-1], T - sum(c for _, c in pieces))])]
    return sections


for _k in range(19):
    recipe("single_%d" % _k, lambda T, k=_k: [(CONT, [(k, T)])])
recipe("all_invalid", lambda T: [(CONT, [(INVALID, T)])])
TWO_KEY_COUNTS = (63, 64, 65, 127, 128, 129)
for _c in TWO_KEY_COUNTS:  # run lengths around one and two chunks; interleaved, the waves that hold both keys are mixed and the rest is uniform in the second
    recipe("two_keys_%d" % _c, lambda T, c=_c: [(None, [(5, c), (12, T - c)])], layout_free=True)
recipe("all_20_keys", lambda T: [(CONT, [(k, 1) for k in range(20)] + [(7, T - 20)])])
recipe("max_chunks", _max_chunks([k for k in range(20) if k != 18] + [18]))
recipe("max_chunks_valid", _max_chunks(list(range(19))))
recipe("keys_16_to_19", lambda T: [(INTER, _even([16, 17, 18, 19], T))])
recipe("keys_0_to_3", lambda T: [(CONT, _even([0, 1, 2, 3], T // 2)), (INTER, _even([0, 1, 2, 3], T - T // 2))])
recipe("keys_15_and_16", lambda T: [(CONT, [(15 + (w & 1), 64) for w in range(T // 64)])])
recipe("waves_mod_20", lambda T: [(CONT, [(w % 20, 64) for w in range(T // 64)])])


def _per_four_waves(whole, mixed, rest):
    """per 256 blocks two 64-block groups of `whole` (one key: contiguous) and two of `mixed` (interleaved pieces of 128 blocks in all), in the order given by
    which is named first; a tile's last T % 256 blocks in key `rest`.  Block l of a tile is lane l % 64 of wave (l / 64) % (WGS / 64), load l / WGS, and WGS / 64 is
    4, 8 or 16: waves 0, 1 (mod 4) hold the first kind in EVERY load and waves 2, 3 the second, so whole waves stay uniform whatever the shape"""
    def sections(T):
        out = []
        for _ in range(T // 256):
            out += [whole, mixed] if whole[2] == 0 else [mixed, whole]
        return [(lay, pieces) for lay, pieces, _ in out] + ([(CONT, [(rest, T % 256)])] if T % 256 else [])
    return sections


# key 4 from whole uniform waves and from single blocks among keys 9 and 13 in the mixed waves beside them: its counter takes 64-adds and 1-adds
recipe("uniform_and_scattered", _per_four_waves((CONT, [(4, 128)], 0), (INTER, [(4, 16), (9, 48), (13, 64)], 1), 4))
# BPT > 1: the first half of the tile (the waves' first loads) one key per wave, the second half (their later loads) mixed
recipe("first_load_uniform", lambda T: [(CONT, [((2, 6, 11)[w % 3], 64) for w in range(T // 128)]), (INTER, _even([2, 6], T - 64 * (T // 128)))])
# half a tile of invalid mode codes in whole uniform waves, out-of-range patterns scattered through the valid half.  _a: the valid waves first, their first
# block a bad pattern (the lowest failing block is bad-pattern); _b: the invalid waves first (bad-mode)
recipe("half_invalid_a", _per_four_waves((CONT, [(INVALID, 128)], 1), (INTER, [(BAD_PATTERN + 3, 2), (BAD_PATTERN + 7, 2), (10, 124)], 0), 10))
recipe("half_invalid_b", _per_four_waves((CONT, [(INVALID, 128)], 0), (INTER, [(10, 124), (BAD_PATTERN + 7, 2), (BAD_PATTERN + 3, 2)], 1), INVALID))
recipe("uniform_mix", lambda T: [(SHUF, _even(list(range(19)), T))])
# the ragged last tile: every full wave one key, the last wave 63 lanes / one lane of it
recipe("ragged_63", lambda T: [(CONT, [(3, T - 1)])], short=1)
recipe("ragged_1", lambda T: [(CONT, [(3, T - 63)])], short=63)

TWO_KEYS = tuple("two_keys_%d@%s" % (c, lay) for c in TWO_KEY_COUNTS for lay in (CONT, INTER))
FULL = tuple(["single_%d" % k for k in range(19)] + ["all_invalid"] + list(TWO_KEYS) + [
    "all_20_keys", "max_chunks", "max_chunks_valid", "keys_16_to_19", "keys_0_to_3", "keys_15_and_16", "waves_mod_20", "uniform_and_scattered",
    "first_load_uniform", "half_invalid_a", "half_invalid_b", "uniform_mix"])  # every full-tile recipe, once
RAGGED = ("ragged_63", "ragged_1")


def fails(rid):
    name = rid.partition("@")[0]
    return any(k >= INVALID for _, pieces in RECIPES[name]["sections"](TILE) for k, _ in pieces)


VALID = tuple(r for r in FULL if not fails(r))
# the tiles a workgroup walks one after another (tile t, t + grid, t + 2 grid, ...: workgroup b takes WALKS[b % len(WALKS)]): the uniform mix followed by a
# single key and the reverse, an all-invalid tile followed by a valid one, the cheapest key followed by the dearest
WALKS = (("uniform_mix", "single_18", "uniform_mix"), ("single_18", "uniform_mix", "single_0"), ("all_invalid", "uniform_mix", "all_invalid"),
         ("single_0", "single_18", "first_load_uniform"), ("max_chunks_valid", "keys_15_and_16", "waves_mod_20"))
WALKS_VALID = tuple(w for w in WALKS if not any(fails(r) for r in w))
WALK_PAIRS = (("uniform_mix", "single_18"), ("single_18", "uniform_mix"), ("all_invalid", "uniform_mix"))  # (what test_sort_cases.py looks for in a planned walk)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def case(id, n, content, bpr=0, policies=(EXCL,), entry="device", targets=ALL, last=None, rgba_n=None, heal=False):
    """n: blocks as a function of the CU count (rgba_n: what RGBA32 takes instead, whole rows of its pitch).  content: ("seq", recipes) -- tile t of a launch
    holds recipes[t % len]; ("walk", walks) -- tile t of a launch of `grid` workgroups holds walks[(t % grid) % len][(t // grid) % 3]; ("halves", k0, k1) -- the
    first half of the blocks in key k0, the second in k1 (the ticketed sizes: no tile is laid out).  last: the recipe of the ragged last tile.  entry: "device",
    "sync", "pinned" (Context.transcode / decode_to_rgba into a page-locked out=: the zero-copy kernels).  heal: after the run the lowest failing block is
    replaced by a valid one and the next-lowest must be reported"""
    assert content[0] in ("seq", "walk", "halves")
    return dict(id=id, n=n, content=content, bpr=bpr, policies=tuple(policies), entry=entry, targets=tuple(targets), last=last, rgba_n=rgba_n, heal=heal,
                min_align=False, ragged_of=None)


def _up(n, q):
    return -(-n // q) * q


N_FULL = _up(len(FULL), 16)  # tiles of a launch that holds every full-tile recipe: whole rows of 16 rectangular tiles
CHEAP, DEAR = 18, 0
_HALVES = ("halves", CHEAP, DEAR)

ONE_SLICE = [case("one_tile/" + r, lambda cu: TILE, ("seq", (r,))) for r in FULL] + [
    case("one_tile_1023", lambda cu: TILE - 1, ("seq", ("ragged_63",)), last="ragged_63"),
    case("one_tile_961", lambda cu: TILE - 63, ("seq", ("ragged_1",)), last="ragged_1"),
    # one tile per workgroup: every recipe in one launch (1024 threads on a tile); then with the lowest failure healed
    case("tile_per_workgroup", lambda cu: TILE * len(FULL) + TILE - 63, ("seq", FULL), last="ragged_1", heal=True),
    case("tile_per_workgroup_valid", lambda cu: TILE * len(VALID) + TILE - 1, ("seq", VALID), last="ragged_63"),
    # whole rectangles at one tile per workgroup (BC7 / ASTC: the one-tile RECT kernel; RGBA32: 1024 x 1 RECT), the recipe in the rectangle's own block order
    case("rect_bpr128", lambda cu: TILE * N_FULL, ("seq", FULL), bpr=128, targets=("astc", "bc7", "rgba")),
    case("rect_bpr1024", lambda cu: TILE * N_FULL, ("seq", FULL), bpr=1024, targets=("astc", "bc7", "rgba")),
    case("rect_virtual_pitch", lambda cu: TILE * N_FULL, ("seq", VALID), targets=("astc", "bc7")),
    # just over one tile per CU: the large shapes of BC7 / ASTC / RGBA32, the mid shape of the ETC family (every tile still has a workgroup of its own)
    case("over_one_per_cu", lambda cu: TILE * cu + TILE - 63, ("seq", FULL), policies=EVERY_POLICY, last="ragged_1"),
    # a persistent walk: six tiles per CU and a few (below the 2^21 blocks from which ASTC changes shape).  The workgroups of the exclusive shapes walk one or
    # two tiles (BC7 / ASTC, four per CU) / three (RGBA32, two per CU), those of the shared shapes three and more; strips with a ragged end, and rectangles
    case("walk", lambda cu: TILE * (6 * cu + 5) - 63, ("walk", WALKS), policies=EVERY_POLICY, last="ragged_1", targets=("astc", "bc7", "rgba")),
    case("walk_valid", lambda cu: TILE * (6 * cu + 5) - 1, ("walk", WALKS_VALID), last="ragged_63", targets=("astc", "bc7", "rgba")),
    case("walk_rect", lambda cu: _up(TILE * (6 * cu + 5), 16384), ("walk", WALKS), bpr=1024, policies=(EXCL, SHARED), targets=("astc", "bc7", "rgba")),
    # the ETC family beyond three tiles per CU: the run-time tile balanced over the workgroups (exclusive; one tile each), the shared 512 x 4 shape (a walk)
    case("etc_balanced_tile", lambda cu: 3 * TILE * cu + 4 * TILE + 1, ("walk", WALKS), policies=EVERY_POLICY, targets=ETC_FAMILY),
    case("etc_balanced_tile_rect", lambda cu: _up(3 * TILE * cu + 1, 64 * 1024), ("seq", FULL), bpr=1024, policies=(EXCL, SHARED), targets=ETC_FAMILY),
    # from 2^20 blocks the ETC family runs one-tile workgroups on 2048-block tiles; with a grid, rectangles of 64 x 32
    case("etc_2048", lambda cu: (1 << 20) + 2048 * len(FULL) - 63, ("seq", FULL), last="ragged_1", targets=ETC_FAMILY),
    case("etc_2048_rect", lambda cu: (1 << 20) + 32 * 1024, ("seq", FULL), bpr=1024, targets=ETC_FAMILY),
    # ASTC from 2^21 blocks: 256 x 4, five workgroups per CU
    case("astc_256x4", lambda cu: (1 << 21) + TILE - 63, ("walk", WALKS), last="ragged_1", targets=("astc",)),
    case("astc_256x4_rect", lambda cu: 1 << 21, ("walk", WALKS_VALID), targets=("astc",)),
    # RGBA32 above 3 * 2^20 blocks: 512 x 2
    case("rgba_512x2", lambda cu: _up((3 << 20) + 1, 1000), ("walk", WALKS), bpr=1000, policies=(EXCL, SHARED), targets=("rgba",)),
    case("rgba_512x2_rect", lambda cu: (3 << 20) + 16 * 1024, ("walk", WALKS), bpr=1024, policies=(EXCL, SHARED), targets=("rgba",)),
    # the blocking call: one case per target, a non-zero block_index_base
    case("sync", lambda cu: TILE * cu + TILE + 333, ("seq", FULL[::-1]), entry="sync"),
    # a page-locked out=: 64 workgroups walk the tiles (256 x 4; RGBA32 512 x 2) and store over PCIe
    case("pinned_valid", lambda cu: TILE * 133 - 1, ("walk", WALKS_VALID), entry="pinned", last="ragged_63"),
    case("pinned_failing", lambda cu: TILE * 133 - 63, ("walk", WALKS), entry="pinned", last="ragged_1"),
    # tile tickets: just over 16 tiles per workgroup of the exclusive large shape, the first half of the slice all in the cheapest key, the second all in the
    # dearest -- the workgroups that drew cheap tiles run ahead.  Strips with a ragged end, and whole rectangles: the plan keeps a kernel of its own for each.
    # The only large cases (with their multi-run siblings below); run once more in a child process with BU_TILE_TICKETS=0
    case("tickets_bc7", lambda cu: TICKET_WALK * PER_CU["bc7"] * cu * TILE + 77, _HALVES, targets=("bc7",)),
    case("tickets_bc7_rect", lambda cu: TICKET_WALK * PER_CU["bc7"] * cu * TILE + 16384, _HALVES, targets=("bc7",)),
    case("tickets_astc", lambda cu: TICKET_WALK * PER_CU["astc"] * cu * TILE + 77, _HALVES, targets=("astc",)),
    case("tickets_astc_rect", lambda cu: TICKET_WALK * PER_CU["astc"] * cu * TILE + 16384, _HALVES, targets=("astc",)),
    case("tickets_rgba", lambda cu: _up(TICKET_WALK * PER_CU["rgba"] * cu * TILE + 77, 1000), _HALVES, bpr=1000, targets=("rgba",)),
    case("tickets_rgba_rect", lambda cu: TICKET_WALK * PER_CU["rgba"] * cu * TILE + 16384, _HALVES, bpr=1024, targets=("rgba",)),
]
TICKETED = tuple(c["id"] for c in ONE_SLICE if c["content"][0] == "halves")


# ---- batches: runs of bu_uastc_transcode_batch_device, each run an allocation of its own ------------------------------------------
def batch(id, sizes, content, bpr=0, targets=ALL, last=None):
    """sizes: the runs' blocks as a function of the CU count (RGBA32: whole rows of bpr); content: as case(), over the launch's tile numbers; last: the recipe
    of every run's ragged last tile"""
    return dict(id=id, sizes=sizes, content=content, bpr=bpr, targets=tuple(targets), last=last)


BATCHES = [
    # no more tiles than CUs (on 80 CUs too): 1024 threads on every tile (BU_MULTI_ONE_TILE); a whole-rectangle run among strips
    batch("multi_one_tile", lambda cu: [16 * TILE, 20 * TILE + TILE - 63, TILE - 63, 30 * TILE + TILE - 63], ("seq", FULL), last="ragged_1", targets=BLOCK_LINEAR),
    batch("multi_one_tile_rgba", lambda cu: [16 * TILE, 21 * TILE, 128, 30 * TILE + 896], ("seq", FULL), bpr=128, targets=("rgba",)),
    # a persistent grid that walks: over two tiles per workgroup (BC7 / ASTC four per CU, 512 x 2, stores last for BC7), ragged runs, a run smaller than a tile
    batch("multi_persist", lambda cu: [TILE * (4 * cu + 3) - 63, TILE - 63, TILE * 4 * cu + TILE - 63], ("walk", WALKS), last="ragged_1", targets=("astc", "bc7")),
    batch("multi_persist_valid", lambda cu: [TILE * (4 * cu + 3) - 1, TILE - 1, TILE * 4 * cu + TILE - 1], ("walk", WALKS_VALID), last="ragged_63", targets=("astc", "bc7")),
    batch("multi_persist_rgba", lambda cu: [TILE * (2 * cu + 3) + 896, 640, TILE * 2 * cu], ("walk", WALKS), bpr=128, targets=("rgba",)),
    # the ETC family walks two per CU on 1024-block tiles below 2^20 blocks in all
    batch("multi_persist_etc", lambda cu: [TILE * (cu + 3) - 63, TILE - 63, TILE * 2 * cu - 63], ("walk", WALKS), last="ragged_1", targets=ETC_FAMILY),
    # whole rectangles only: BC7 / ASTC 256 x 4 without validity tests, five per CU, stores last (BU_MULTI_WHOLE)
    batch("multi_whole", lambda cu: [3 * 4096, 16384, _up(TILE * 5 * cu, 16384), _up(TILE * 5 * cu, 16384) + 4096], ("walk", WALKS), targets=("astc", "bc7")),
    # 2^20 blocks and more in long runs: the ETC family on 2048-block one-tile workgroups (BU_MULTI_ETC_2048)
    batch("multi_etc_2048", lambda cu: [(1 << 19) + 3 * 2048 - 63, 1 << 19, (1 << 18) + 2048 - 63], ("seq", FULL), last="ragged_1", targets=ETC_FAMILY),
    # tile tickets: 16 tiles per workgroup of the persistent grid and more, the first two runs in the cheapest key, the last two in the dearest
    batch("tickets_multi", lambda cu: [TICKET_WALK * cu * TILE + 5] * 4, _HALVES, targets=("bc7", "astc")),
    batch("tickets_multi_rgba", lambda cu: [TICKET_WALK * cu * TILE + 128] * 2, _HALVES, bpr=128, targets=("rgba",)),
]
TICKETED_BATCHES = tuple(b["id"] for b in BATCHES if b["content"][0] == "halves")
MULTI_SHAPES = {0: (512, 4), 1: (1024, 1), 2: (256, 4), 3: (512, 2)}  # WGS x BPT of BU_MULTI_ETC_2048 / _ONE_TILE / _WHOLE / _PERSIST


def size_of(c, target, cu):
    return gc.size_of(c, target, cu)


def pitch_of(c, target, cu):
    return gc.pitch_of(c, target, cu)


def grid_cap_of(c):
    return gc.ZEROCOPY_GRID if c["entry"] == "pinned" else 0


def cases_for(target, entry=None, ticketed=None):
    return [c for c in ONE_SLICE if target in c["targets"] and (entry is None or c["entry"] == entry) and (ticketed is None or (c["id"] in TICKETED) == ticketed)]


def batches_for(target, ticketed=None):
    return [b for b in BATCHES if target in b["targets"] and (ticketed is None or (b["id"] in TICKETED_BATCHES) == ticketed)]


def batch_sizes(b, target, cu):
    return b["sizes"](cu)


# ---- tiles of a planned launch ----------------------------------------------------------------------------------------------------
KERNEL, WGS, BPT, RECT, GRID, TILE_RT, BPR, TICKET = 2, 3, 4, 7, 8, 10, 13, 14  # columns of a bu_emul_launch_plan row


def _rect_tile(t, T, width, origin=0):
    """blocks of rectangular tile t (64 wide, T / 64 high) of a grid `width` blocks wide, in the tile's own order"""
    tpr = width // 64
    ty, tx = divmod(t, tpr)
    l = np.arange(T, dtype=np.int64)
    return origin + ((T // 64) * ty + l // 64) * width + 64 * tx + l % 64


def slice_tiles(rows):
    """the tiles of a one-slice plan (rows of bu_emul_launch_plan): [(launch, tile number, grid, T, WGS, BPT, block indices in the tile's order)]"""
    out = []
    for j, r in enumerate(rows):
        assert r[KERNEL] >= 0, "the one-lane-per-block kernel sorts nothing"
        off, n = r[0], r[1]
        if r[RECT]:
            T = r[WGS] * r[BPT]
            assert n % T == 0 and off % (T // 64 * r[BPR]) == 0
            for t in range(n // T):
                out.append((j, t, r[GRID], T, r[WGS], r[BPT], _rect_tile(t, T, r[BPR], off)))
        else:
            T = r[TILE_RT]
            for t in range(-(-n // T)):
                out.append((j, t, r[GRID], T, r[WGS], r[BPT], off + np.arange(t * T, min(n, (t + 1) * T), dtype=np.int64)))
    return out


def runs_plan(lib, t, sizes, bpr, cu):
    """bu_plan_runs + bu_plan_multi_kernel (exclusive: what a lone batch call resolves to) over runs of `sizes` blocks in allocations of their own (addresses far
    apart: nothing merges): [dict(plain, kernel (BU_MULTI_*), grid, n_tiles, tile, ticket, entries [(run, offset, n, vshift, first_tile)])] per launch"""
    import ctypes

    k = len(sizes)
    U64, I64P = ctypes.c_uint64 * k, ctypes.POINTER(ctypes.c_int64)
    rows, ents = (ctypes.c_int64 * (10 * (k + 8)))(), (ctypes.c_int64 * (5 * (2 * k + 8)))()
    m = lib.bu_emul_runs_plan(t, k, U64(*[(1 << 40) + (i << 34) for i in range(k)]), U64(*[(2 << 40) + (i << 34) for i in range(k)]),
                              (ctypes.c_size_t * k)(*sizes), U64(*[0] * k), bpr, 0, 0, cu, ctypes.cast(rows, I64P), k + 8, ctypes.cast(ents, I64P), 2 * k + 8)
    assert m > 0
    out = []
    for j in range(m):
        r = rows[10 * j:10 * j + 10]
        out.append(dict(plain=r[0] >= 0, n_tiles=r[2], tile=r[3], kernel=r[5], grid=r[6], ticket=r[8], entries=[tuple(ents[5 * e:5 * e + 5]) for e in range(r[9], r[9] + r[1])]))
    return out


def runs_tiles(launches, starts):
    """the tiles of a batch plan (test_guard_cases.runs_plan), block indices counted over the runs back to back (starts[run] = the run's first block)"""
    out = []
    for j, l in enumerate(launches):
        assert not l["plain"]
        wgs, bpt = MULTI_SHAPES[l["kernel"]]
        T, t = wgs * bpt, 0
        assert T == l["tile"]
        for run, off, n, vshift, first in l["entries"]:
            assert first == t
            for lt in range(-(-n // T)):
                if vshift == 0xFFFFFFFF:
                    idx = starts[run] + off + np.arange(lt * T, min(n, (lt + 1) * T), dtype=np.int64)
                else:
                    assert T == TILE and n % (16 * (64 << vshift)) == 0
                    idx = _rect_tile(lt, T, 64 << vshift, starts[run] + off)
                out.append((j, t, l["grid"], T, wgs, bpt, idx))
                t += 1
        assert t == l["n_tiles"]
    return out


def tile_recipe(content, last, t, grid, T, count):
    """the recipe of tile t (of `count` blocks, nominally T) of a launch of `grid` workgroups.  A ragged tile takes the case's `last` recipe where its size
    is the one that recipe is written for (tests/test_sort_cases.py holds that it is, wherever a case names one); any other ragged tile is its own recipe cut off"""
    if count < T and last is not None and count == T - RECIPES[last]["short"]:
        return last
    if content[0] == "seq":
        return content[1][t % len(content[1])]
    walk = content[1][(t % grid) % len(content[1])]
    return walk[(t // grid) % len(walk)]


class Tables:
    """a target's row of BU_COST_ORDER and key_lut, from the host build"""

    def __init__(self, lib, target):
        import ctypes

        co, kl = np.zeros(20, dtype=np.uint8), np.zeros(128, dtype=np.uint8)
        lib.bu_emul_sort_tables.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.bu_emul_sort_tables.restype = ctypes.c_int
        self.row = lib.bu_emul_sort_tables(TARGETS[target][0], co.ctypes.data, kl.ctypes.data)
        self.cost_order, self.key_lut = co.astype(np.int64), kl.astype(np.int64)
        assert sorted(self.cost_order) == list(range(20)) and self.cost_order[19] == 19
        self.key_of_mode = np.argsort(self.cost_order)

    def sort_keys(self, piece_keys):
        """piece keys -> the kernel's sort keys (a bad pattern sorts under its mode)"""
        pk = np.asarray(piece_keys)
        return np.where(pk >= BAD_PATTERN, self.key_of_mode[np.clip(pk - BAD_PATTERN, 0, 19)], pk)

    def pool_index(self, piece_keys, where):
        """the pool block of every piece key: a hash of the block's index `where` picks among the key's 32 vectors / 64 / 16 failing blocks"""
        pk = np.asarray(piece_keys)
        h = synth.hash32(where, 0x50F7).astype(np.int64)
        idx = self.cost_order[np.clip(pk, 0, 19)] * 32 + h % 32
        idx = np.where(pk == INVALID, POOL_BAD_MODE + h % N_BAD_MODE, idx)
        for m, base in POOL_BAD_PAT.items():
            idx = np.where(pk == BAD_PATTERN + m, base + h % N_BAD_PAT, idx)
        assert ((pk <= INVALID) | np.isin(pk, [BAD_PATTERN + m for m in PATTERN_MODES])).all(), "a key no pool block stands for"
        return idx


def fill_tiles(tb, tiles, content, last, n):
    """pool indices [n] of a launch sequence's blocks: every tile laid out by its recipe"""
    idx = np.full(n, -1, dtype=np.int64)
    memo = {}
    for _, t, grid, T, _, _, where in tiles:
        rid = tile_recipe(content, last, t, grid, T, where.size)
        if (rid, T) not in memo:
            memo[rid, T] = recipe_keys(rid, T)
        idx[where] = tb.pool_index(memo[rid, T][:where.size], where)
    assert (idx >= 0).all(), "the tiles do not cover the blocks"
    return idx


def halves_index(tb, content, n, xp=np, **kw):
    """pool indices of a ("halves", k0, k1) case, with numpy or on the device with torch: the 32 vectors of each key in turn"""
    i = xp.arange(n, **kw)
    m0, m1 = int(tb.cost_order[content[1]]), int(tb.cost_order[content[2]])
    return xp.where(i < n // 2, m0 * 32 + i % 32, m1 * 32 + i % 32)


def expected_word(pool_st, idx, base=0):
    """the status word of blocks idx: clear, or the lowest failing block and its status"""
    bad = np.nonzero(pool_st[idx])[0]
    return CLEAR if bad.size == 0 else ((base + int(bad[0])) << 8) | int(pool_st[idx[bad[0]]])
