"""The cases of tests/test_gpu_guard_bands.py as data: sizes as functions of the device's CU count, blocks_per_row, launch policy and entry point.
tests/test_guard_cases.py (no GPU) plans every case with the launch plan the launchers use (csrc/bu_launch_plan.hpp through tests/host_emul) and
holds that the table reaches every kernel a broad sweep of the plan reaches, each with a ragged end.

Sizes come from the tile sizes of bu_launch_plan.hpp: 1024-block tiles (BU_HOST_TILE), 64 x 16-block rectangles (a whole tile row is 16 x pitch
blocks: 16 384 at the virtual pitch 1024), one tile per CU, three per CU for the ETC family, 2^20 / 2^21 / 3 * 2^20 blocks for the ETC, ASTC and RGBA32
large shapes, 16 tiles per workgroup for tile tickets."""

ASTC, BC7, ETC1, ETC2, RGBA = 0, 1, 2, 3, 4
TARGETS = {"astc": (0, 16), "bc7": (1, 16), "etc1": (2, 8), "etc2": (3, 16), "rgba": (4, 64), "bc4": (6, 8), "bc5": (7, 16), "r11": (8, 8),
           "rg11": (9, 16), "bc1": (11, 8), "bc3": (12, 16)}
ALL = tuple(TARGETS)
BLOCK_LINEAR = tuple(t for t in ALL if t != "rgba")
ETC_FAMILY = tuple(t for t in ALL if t not in ("astc", "bc7", "rgba"))  # planned in the shapes of ETC1 (8-byte) / ETC2 (16-byte): bu_shape_target
EXCL, SHARED, AUTO = "exclusive", "shared", "auto"
POLICY_ARGS = {EXCL: (0, 0), SHARED: (1, 1), AUTO: (2, 0)}  # (policy, what AUTO resolves to: a lone launch on a caller's stream is exclusive)
EVERY_POLICY = (EXCL, SHARED, AUTO)
ZEROCOPY_GRID = 64  # BU_ZEROCOPY_GRID: the grid cap of a launch that reads or writes page-locked host memory
MAX_BLOCKS = 1 << 25
TILE = 1024
# tiles per workgroup from which a launch draws tickets x workgroups per CU of the exclusive large shape: BC7 512 x 2 four per CU, ASTC 256 x 4 five
# per CU (from 2^21 blocks), RGBA32 two per CU
TICKET_WALK = 16
PER_CU = {"bc7": 4, "astc": 5, "rgba": 2}


def rgba_pitch(n):
    """a blocks_per_row for an RGBA32 slice of n blocks whose case names none: RGBA32 takes whole block rows only, so the smallest divisor of n
    from 2 up that is no multiple of 64 (no rectangular tiles), n itself for a prime"""
    d = 2
    while d * d <= n:
        if n % d == 0 and d % 64:
            return d
        d += 1
    return n


def case(id, n, bpr=0, policies=EVERY_POLICY, entry="device", targets=ALL, ragged_of=None, min_align=False, rgba_n=None):
    """n: blocks as a function of the CU count.  entry: "device" (bu_uastc_transcode_device), "sync" (bu_uastc_transcode_device_sync),
    "pinned" / "pageable" (transcode / decode_to_rgba with a page-locked / pageable out=).  ragged_of: the id of the whole-rectangle case this one is
    the ragged sibling of -- one block (RGBA32: one block row) short, where the plan must flip to the strip kernel.  min_align: buffers at the smallest
    alignment include/basisu_hip.h allows.  rgba_n: the size RGBA32 takes instead where n is no whole number of rows of bpr."""
    return dict(id=id, n=n, bpr=bpr, policies=tuple(policies), entry=entry, targets=tuple(targets), ragged_of=ragged_of, min_align=min_align, rgba_n=rgba_n)


def _up(n, q):
    return -(-n // q) * q


ONE_SLICE = [
    # the one-lane-per-block kernel (below BU_SORT_MIN_BLOCKS = 8) and the one-tile shape
    case("n1", lambda cu: 1),
    case("n7", lambda cu: 7, min_align=True),
    case("n8", lambda cu: 8),
    case("n9", lambda cu: 9, min_align=True),
    case("n1023", lambda cu: 1023),
    case("n1025", lambda cu: 1025, min_align=True),
    case("last_cu_one_block", lambda cu: TILE * (cu - 1) + 1),
    # whole rectangles at no more than one tile per CU: ASTC / BC7 take the one-tile RECT kernel (a virtual pitch of 256: 16 x 256 blocks); a block less: strips
    case("one_tile_rect", lambda cu: 4096, targets=("astc", "bc7")),
    case("one_tile_rect_short", lambda cu: 4095, targets=("astc", "bc7"), ragged_of="one_tile_rect"),
    # a real grid of 128 / 1024 blocks per row, whole and one row short
    case("bpr128_whole", lambda cu: 16 * 128 * 3, bpr=128),
    case("bpr128_row_short", lambda cu: 16 * 128 * 3 - 128, bpr=128, ragged_of="bpr128_whole"),
    case("bpr1024_whole", lambda cu: 16 * 1024 * 2, bpr=1024),
    case("bpr1024_row_short", lambda cu: 16 * 1024 * 2 - 1024, bpr=1024, ragged_of="bpr1024_whole"),
    # beyond one tile per CU: the large shapes of BC7 / ASTC / RGBA32, the mid shape of the ETC family
    case("over_one_per_cu", lambda cu: TILE * cu + 1),
    # the first multiple of 16 384 above one tile per CU: the virtual pitch 1024 of BC7 / ASTC (RECT) against strips one block short
    case("virtual_pitch", lambda cu: _up(TILE * cu + 1, 16384), targets=BLOCK_LINEAR),
    case("virtual_pitch_short", lambda cu: _up(TILE * cu + 1, 16384) - 1, targets=BLOCK_LINEAR, ragged_of="virtual_pitch"),
    case("big_bpr1024_whole", lambda cu: _up(TILE * cu + 1, 16384), bpr=1024, targets=("astc", "bc7", "rgba")),
    case("big_bpr1024_row_short", lambda cu: _up(TILE * cu + 1, 16384) - 1024, bpr=1024, targets=("astc", "bc7", "rgba"), ragged_of="big_bpr1024_whole"),
    # the ETC family beyond three tiles per CU: a run-time tile balanced over the workgroups (exclusive), the shared 512 x 4 shape
    case("etc_balanced_tile", lambda cu: 3 * TILE * cu + 1, targets=ETC_FAMILY),
    # from 2^20 blocks the ETC family runs one-tile workgroups on 2048-block tiles under every policy; with a grid, whole rectangles of 64 x 32
    case("etc_2048", lambda cu: (1 << 20) + 4321, targets=ETC_FAMILY + ("bc7",)),
    case("etc_2048_rect", lambda cu: (1 << 20) + 32 * 1024, bpr=1024, targets=ETC_FAMILY),
    case("etc_2048_rect_row_short", lambda cu: (1 << 20) + 31 * 1024, bpr=1024, targets=ETC_FAMILY, ragged_of="etc_2048_rect"),
    # ASTC from 2^21 blocks: 256 x 4, five workgroups per CU, strips and (at the virtual pitch) rectangles
    case("astc_256x4", lambda cu: (1 << 21) + 5, targets=("astc",), policies=(EXCL, AUTO)),
    case("astc_256x4_rect", lambda cu: (1 << 21), targets=("astc",), policies=(EXCL,)),
    case("astc_256x4_rect_short", lambda cu: (1 << 21) - 1, targets=("astc",), policies=(EXCL,), ragged_of="astc_256x4_rect"),
    # RGBA32 above 3 * 2^20 blocks: 512 x 2
    case("rgba_512x2", lambda cu: _up((3 << 20) + 1, 1000), bpr=1000, targets=("rgba",), policies=(EXCL, SHARED)),
    case("rgba_512x2_rect", lambda cu: (3 << 20) + 16 * 1024, bpr=1024, targets=("rgba",), policies=(EXCL, SHARED)),
    case("rgba_512x2_rect_row_short", lambda cu: (3 << 20) + 15 * 1024, bpr=1024, targets=("rgba",), policies=(EXCL, SHARED), ragged_of="rgba_512x2_rect"),
    # just over the ticket threshold (16 tiles per workgroup of the exclusive large shape), ragged; and whole rectangles at it, with the sibling
    case("bc7_tickets", lambda cu: TICKET_WALK * PER_CU["bc7"] * cu * TILE + 77, targets=("bc7",), policies=(EXCL,)),
    case("bc7_tickets_rect", lambda cu: TICKET_WALK * PER_CU["bc7"] * cu * TILE + 16384, targets=("bc7",), policies=(EXCL,)),
    case("bc7_tickets_rect_short", lambda cu: TICKET_WALK * PER_CU["bc7"] * cu * TILE + 16383, targets=("bc7",), policies=(EXCL,), ragged_of="bc7_tickets_rect"),
    case("astc_tickets", lambda cu: TICKET_WALK * PER_CU["astc"] * cu * TILE + 77, targets=("astc",), policies=(EXCL,)),
    case("astc_tickets_rect", lambda cu: TICKET_WALK * PER_CU["astc"] * cu * TILE + 16384, targets=("astc",), policies=(EXCL,)),
    case("astc_tickets_rect_short", lambda cu: TICKET_WALK * PER_CU["astc"] * cu * TILE + 16383, targets=("astc",), policies=(EXCL,), ragged_of="astc_tickets_rect"),
    case("rgba_tickets", lambda cu: _up(TICKET_WALK * PER_CU["rgba"] * cu * TILE + 77, 1000), bpr=1000, targets=("rgba",), policies=(EXCL,)),
    case("rgba_tickets_rect", lambda cu: TICKET_WALK * PER_CU["rgba"] * cu * TILE + 16384, bpr=1024, targets=("rgba",), policies=(EXCL,)),
    case("rgba_tickets_rect_row_short", lambda cu: TICKET_WALK * PER_CU["rgba"] * cu * TILE + 15 * 1024, bpr=1024, targets=("rgba",), policies=(EXCL,),
         ragged_of="rgba_tickets_rect"),
    # bu_uastc_transcode_device_sync: one ragged case per target (exclusive, a non-zero block_index_base)
    case("sync_ragged", lambda cu: TILE * cu + 333, entry="sync", policies=(EXCL,)),
    # host pointers: a page-locked out= is written by the kernels over PCIe on the zero-copy shape (64 workgroups, each walking tiles), a pageable one
    # is copied back
    case("pinned_ragged", lambda cu: 70001, entry="pinned", policies=(EXCL,)),
    case("pageable_ragged", lambda cu: 5003, entry="pageable", policies=(EXCL,)),
]

# ---- batches: run sizes of bu_uastc_transcode_batch_device / transcode_batch_in_flight; every run in one arena with a guard band between two runs ----
MIX = (1, 7, 9, 700, 1024, 1025, 2047, 4096, 16384, 16385, 70001)


def batch(id, sizes, bpr=0, targets=ALL, adjacent=False, in_flight=True):
    """sizes: the runs' blocks as a function of the CU count; adjacent: the runs sit back to back in one region (bu_merge_runs joins them: the plain
    launch), guards at the two ends only"""
    return dict(id=id, sizes=sizes, bpr=bpr, targets=tuple(targets), adjacent=adjacent, in_flight=in_flight)


def _rows(sizes, bpr):
    return [_up(n, bpr) for n in sizes]


BATCHES = [
    # no more tiles than CUs on an MI355X: 1024 threads on every tile (BU_MULTI_ONE_TILE)
    batch("mix", lambda cu: list(MIX), targets=BLOCK_LINEAR),
    # more tiles than CUs, ragged runs among them: the persistent grid (BU_MULTI_PERSIST)
    batch("mix_persist", lambda cu: list(MIX) + [TILE * cu + 333], targets=BLOCK_LINEAR),
    # whole rectangles only: BC7 / ASTC take the variant without validity tests (BU_MULTI_WHOLE); the sibling has one run a block short
    batch("all_whole", lambda cu: [4096, 16384, _up(TILE * cu, 16384), 4096], targets=BLOCK_LINEAR),
    batch("all_whole_but_one", lambda cu: [4096, 16384, _up(TILE * cu, 16384) - 1, 4096], targets=BLOCK_LINEAR),
    # 2^20 blocks and more in long runs: the ETC family on 2048-block tiles (BU_MULTI_ETC_2048), ragged ends
    batch("long_runs", lambda cu: [(1 << 19) + 3 * 2048 + 77, 1 << 19, (1 << 18) + 5], targets=BLOCK_LINEAR),
    # RGBA32, 128 blocks per row: whole images, a ragged run of eight tile rows and more (its whole prefix as rectangles, the rest as strips), small ones
    batch("rgba_rows", lambda cu: [128, 16 * 128, 16384 + 3 * 128, 128 * 7, 8 * 16384 + 128, TILE * cu], bpr=128, targets=("rgba",)),
    # 16 tiles per workgroup of the persistent grid and more: tile tickets (BC7 / ASTC four workgroups per CU, ragged runs)
    batch("tickets", lambda cu: [TICKET_WALK * cu * TILE + 5] * 4, targets=("bc7", "astc"), in_flight=False),
    # adjacent runs: merged into one run, which goes out as the plain launch
    batch("adjacent", lambda cu: [700, 1024, 16385, 9], targets=BLOCK_LINEAR, adjacent=True),
    batch("adjacent_rgba", lambda cu: [128 * 3, 128, 128 * 130], bpr=128, targets=("rgba",), adjacent=True),
]

# transcode_batch_in_flight cutting ONE contiguous array into pieces: (n as a function of the CU count, blocks_per_row)
IN_FLIGHT_ARRAYS = [
    dict(id="array_bpr0", n=lambda cu: (1 << 21) + 4097, bpr=0, targets=BLOCK_LINEAR),
    dict(id="array_bpr1024", n=lambda cu: (1 << 21) + 3 * 1024, bpr=1024, targets=ALL),
]


def size_of(c, target, cu):
    n = c["n"](cu)
    if target == "rgba" and c["rgba_n"] is not None:
        n = c["rgba_n"](cu)
    return n


def pitch_of(c, target, cu):
    """the blocks_per_row a case runs with for this target"""
    if target == "rgba" and c["bpr"] == 0:
        return rgba_pitch(size_of(c, target, cu))
    return c["bpr"]


def grid_cap_of(c):
    return ZEROCOPY_GRID if c["entry"] == "pinned" else 0


def cases_for(target, entry=None):
    return [c for c in ONE_SLICE if target in c["targets"] and (entry is None or c["entry"] == entry)]
