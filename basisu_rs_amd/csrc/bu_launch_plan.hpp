// The launch plan of the UASTC launchers (bu_uastc_launch.hpp bu_launch_uastc: one slice; bu_capi_slice.hpp bu_launch_runs: several runs): which
// instantiation of the mode-sorted kernel runs, on which grid, with which tile size, priorities, pitch and tile tickets.  No HIP in here: the
// test-only host build (tests/host_emul) compiles it as it is and tests/test_launch_plan.py checks it case by case without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bu_batch_plan.hpp"      // BuRun
#include "bu_uastc_dispatch.hpp"  // BU_TGT_*

constexpr int BU_WG = 256;            // 4 waves
// Below this the plain one-lane-per-block kernel is used.  It runs one mode path per DISTINCT mode present, so it only
// wins for a handful of blocks (BC7: 1 block 2.3 vs 3.3 us, 8 blocks 4.2 vs 3.7 us, 64 blocks 7.8 vs 4.4 us,
// 1024 blocks 16.1 vs 4.8 us; ETC1 at 128 blocks 38.6 vs 15.0 us).
constexpr int BU_SORT_MIN_BLOCKS = 8;
// shapes of the mode-sorted kernel whose tile size is a run-time argument (bu_balanced_tile): the ETC family on 4096-block tiles
constexpr bool bu_dyn_tile(int target, int tile) { return bu_etc_family(target) && tile == 4096; }
constexpr unsigned BU_RECT_W = 64;  // width of a rectangular tile (bu_kernels.hpp, layout RECT)
constexpr unsigned BU_MULTI_RUNS = 96;  // runs per multi-run launch (bu_kernels.hpp, BuRunTable)
constexpr uint32_t BU_RUN_STRIPS = 0xFFFFFFFFu;
// The widest grid a run of a multi-run launch is tiled on as rectangles (bu_plan_runs).  The kernel keeps a lane's distance from its tile's corner as a 32-bit byte
// offset: at most (31 rows x this width + 63 blocks) x 16 bytes < 2^29 (bu_multi_addr.hpp asserts it)
constexpr size_t BU_MULTI_MAX_WIDTH = (size_t)1 << 20;
// RGBA32: the widest image (blocks per row) whose runs share a multi-run launch -- there the lane offset spans pixel rows of the image (bu_lane_off_rgba);
// runs of wider images go out one by one as plain launches
constexpr size_t BU_MULTI_RGBA_MAX_BPR = (size_t)1 << 24;
// a launch that draws its tiles by ticket needs a grid of at least this many workgroups: the kernel numbers its tiles off eight counters
constexpr unsigned BU_TICKET_MIN_GRID = 8;

inline unsigned bu_grid_for(size_t n_blocks, unsigned cu_count)
{
    // enough workgroups to fill the chip several times over, capped so every workgroup amortises its
    // table copy over >= 2 batches on large inputs (guide: grid ~ CUs x 8 for memory-bound kernels)
    size_t wgs = (n_blocks + BU_WG - 1) / BU_WG;
    const size_t cap = (size_t)cu_count * 8;
    if (wgs > cap) wgs = cap;
    if (wgs == 0) wgs = 1;
    return (unsigned)wgs;
}

// workgroups of the zero-copy launches: enough loads in flight to cover PCIe latency, few enough that every workgroup
// walks many tiles and reads overlap writes (measured on a 4096^2 atlas: 16 -> 0.52 ms, 64 -> 0.47, 256 -> 0.54, 1024 -> 0.56)
constexpr unsigned BU_ZEROCOPY_GRID = 64;

// Blocks per tile of a launch whose kernel takes its tile size at run time (bu_uastc_sorted_kernel, DYN_TILE): the smallest
// number of rounds the full tile allows, then equal tiles (a multiple of 64 blocks) so that every workgroup slot gets the
// same share.  1.5 Mi blocks on 256 slots of up to 4096: two rounds of 3072 instead of 4096 + 2048.
inline size_t bu_balanced_tile(size_t max_tile, size_t n_blocks, size_t slots, bool dynamic)
{
    if (!dynamic || slots == 0) return max_tile;
    const size_t per_slot = (n_blocks + slots - 1) / slots, rounds = (per_slot + max_tile - 1) / max_tile;
    size_t t = ((per_slot + rounds - 1) / rounds + 63) & ~(size_t)63;
    return t < 64 ? 64 : (t > max_tile ? max_tile : t);
}

// ---- shapes of the mode-sorted kernel ------------------------------------------------------------------------------------------
// One BuShape = one compiled instantiation of bu_uastc_sorted_kernel (strip layout, plus the rectangular layout where RECT is set):
// WGS threads x BPT blocks per thread = one tile; MINW = waves per SIMD the register allocation leaves room for; PER_CU = how many
// workgroups of ONE launch may be resident on a CU (the grid of a large launch is min(tiles, PER_CU x CUs); workgroups walk the
// remaining tiles, with the next tile's loads in flight where PREFETCH is set).
struct BuShape {
    int wgs, bpt, minw;
    bool prefetch, rect;
    int per_cu;
    constexpr size_t tile() const { return (size_t)wgs * bpt; }
};
// The shape of a LARGE launch (more than one 1024-block tile per CU; ETC: more than three) per target and launch policy.
//
// BU_LAUNCH_EXCLUSIVE -- the launch is alone on the chip and must fill it by itself (rounds 1-4; every figure an A/B inside one run
// on a 4096^2 atlas = 4096 blocks per CU, DESIGN_HISTORY.md section 4 and profiles/r04_ab_bc7_tile_shapes_and_upfront_loads.txt):
//   BC7 / ASTC  512 x 2, four workgroups per CU = 32 waves, <= 64 VGPRs.  Four INDEPENDENT sort chains per CU hide each other's
//               barriers and LDS round trips; 2048-block tiles +10 %, 4096 +35 %, 256 x 4 four per CU +18 %.
//   ETC1 / ETC2 one 1024-thread workgroup per CU on a tile of up to 4096 blocks (99 / 121 VGPRs: 16 waves are all that fit);
//               73 chunks per 4096 blocks where two 2048-block tiles have 83.
//               (Only below 2^20 blocks since the end of round 6: from there on ETC launches are one-tile workgroups of the SHARED shape, bu_plan_slice.)
//   RGBA32      1024-block tiles (64 KiB of LDS for the four pixel rows), two workgroups per CU, 1024 x 1 up to 3 Mi blocks then 512 x 2.
// BU_LAUNCH_SHARED -- several launches from different streams are in flight and should run SIDE BY SIDE on every CU, so that one
// launch's load phase (3.4 us with the vector ALUs idle when it is alone) lies under another one's chunk phase (ALUs saturated, HBM
// idle).  A launch takes at most half of a CU's wave slots, registers and LDS (round 5, profiles/r05_ab_bc7_two_launches_in_flight.txt,
// r05_ab_etc_shared_shapes_x_streams.txt, r05_ab_wave_priorities_with_launches_in_flight.txt;
// us per 4096^2 atlas with 1 / 2 / 3 / 4 launches in flight):
//   BC7 / ASTC  256 x 4, two per CU (8 waves, 56 KiB), no wave priorities   11.8 / 6.8 / 6.0 / 5.45-5.55   (exclusive shape: 8.4 / 6.7 / 6.2 / 6.2)
//   ETC1        512 x 4, one per CU (8 waves, <= 128 VGPRs, 63 KiB) 20.1 / 13.1 / 12.1 / 12.2   (17.7 / 15.5 / 15.2 / 15.7)
//   ETC2        the same without the prefetch (115 VGPRs)           25.4 / 16.3 / 15.0 / 15.0   (22.1 / 19.7 / 19.3 / 20.4)
//   RGBA32      1024 x 1, one per CU (16 waves, 69 KiB)             19.6 / 14.7 / 13.4 / 13.1   (14.7 / 14.2 / 13.8 / 13.6)
// Alone on the chip a shared-policy launch is 15-40 % slower than an exclusive one: the policy is for callers that keep >= 2
// streams busy (bu_context_set_launch_policy).
enum { BU_POLICY_EXCLUSIVE = 0, BU_POLICY_SHARED = 1, BU_POLICY_AUTO = 2,
       BU_POLICY_SHARED_FEW = 3 };  // (internal, picked by bu_auto_policy only: the shared kernels on one-tile workgroups, for one or two other launches in flight)
constexpr BuShape BuBigShape(int target, int policy)
{
    if (target == BU_TGT_BC7 || target == BU_TGT_ASTC)
        return policy == BU_POLICY_SHARED ? BuShape{256, 4, 1, true, true, 2}
                                          : BuShape{512, 2, target == BU_TGT_ASTC ? 8 : 1, true, true, 4};  // (ASTC MINW 8: the strip form took 65 VGPRs = three per CU: a ragged 2^20-block slice 12.5 -> 9.5 us)
    return policy == BU_POLICY_SHARED ? BuShape{512, 4, 4, target == BU_TGT_ETC1, true, 1} : BuShape{1024, 4, 1, true, true, 1};  // ETC1 / ETC2
}
// BC7 / ASTC use their large shape from the first tile beyond one per CU (8 waves on a 1024-block tile beat 4: 2^16 blocks 7.5 -> 5.7 us,
// 2^18 8.1 -> 6.3 us); ETC1 / ETC2 keep every tile of the 512 x 2 shape resident up to three 1024-block tiles per CU (2^19 blocks:
// 12.7 against 18.2 us for the 4096-block shape, 786 432: 16.7 / 18.6) and switch beyond it (917 504 blocks: 21.5 against 18.9 us)
constexpr bool bu_big_from_one_tile_per_cu(int target) { return target == BU_TGT_BC7 || target == BU_TGT_ASTC; }
// the shapes below the large ones, the same under both policies:
//   at most one 1024-block tile per CU: 16 waves on it (BC7 1 Ki blocks 4.32 -> 3.92 us, 2^16 5.16 -> 4.80, 2^18 5.70 -> 5.41; ETC1 6.76 -> 6.47, 7.95 -> 7.64, 8.82 -> 8.54)
constexpr BuShape BuOneTileShape(int target) { return BuShape{1024, 1, 1, false, target == BU_TGT_BC7 || target == BU_TGT_ASTC, 1}; }
//   ETC, up to three tiles per CU: 8 waves per tile, every tile resident (ETC1 at 2^16 blocks: 14.1 -> 11.3 us)
constexpr BuShape BuEtcMidShape{512, 2, 1, false, false, 3};
//   zero-copy launches over PCIe (grid_cap): 256 x 4 on a small persistent grid
constexpr BuShape BuZeroCopyShape{256, 4, 1, true, false, 1};
constexpr int BU_HOST_TILE = 1024;  // the tile the launcher counts in where the shape does not say otherwise

// The compiled instantiations of bu_uastc_sorted_kernel<target, WGS, BPT, MINW, PREFETCH, RECT ? layout RECT : STRIP> (bu_uastc_launch.hpp launches entry i):
// every shape above in the strip layout, and in the rectangular one where it has RECT.  (Never planned, compiled all the same: the ETC mid shape for BC7 /
// ASTC, the 256 x 4 RECT shape for ETC1 / ETC2.)
struct BuSortedKey { int target, wgs, bpt, minw; bool prefetch, rect; };
constexpr BuSortedKey BU_SORTED_KERNELS[] = {
    {BU_TGT_BC7, 1024, 1, 1, false, false}, {BU_TGT_BC7, 1024, 1, 1, false, true}, {BU_TGT_BC7, 512, 2, 1, true, false}, {BU_TGT_BC7, 512, 2, 1, true, true},
    {BU_TGT_BC7, 256, 4, 1, true, false}, {BU_TGT_BC7, 256, 4, 1, true, true}, {BU_TGT_BC7, 512, 2, 1, false, false},
    {BU_TGT_ASTC, 1024, 1, 1, false, false}, {BU_TGT_ASTC, 1024, 1, 1, false, true}, {BU_TGT_ASTC, 512, 2, 8, true, false}, {BU_TGT_ASTC, 512, 2, 8, true, true},
    {BU_TGT_ASTC, 256, 4, 1, true, false}, {BU_TGT_ASTC, 256, 4, 1, true, true}, {BU_TGT_ASTC, 512, 2, 1, false, false},
    {BU_TGT_ETC1, 1024, 1, 1, false, false}, {BU_TGT_ETC1, 512, 2, 1, false, false}, {BU_TGT_ETC1, 1024, 4, 1, true, false}, {BU_TGT_ETC1, 1024, 4, 1, true, true},
    {BU_TGT_ETC1, 512, 4, 4, true, false}, {BU_TGT_ETC1, 512, 4, 4, true, true}, {BU_TGT_ETC1, 256, 4, 1, true, false}, {BU_TGT_ETC1, 256, 4, 1, true, true},
    {BU_TGT_ETC2, 1024, 1, 1, false, false}, {BU_TGT_ETC2, 512, 2, 1, false, false}, {BU_TGT_ETC2, 1024, 4, 1, true, false}, {BU_TGT_ETC2, 1024, 4, 1, true, true},
    {BU_TGT_ETC2, 512, 4, 4, false, false}, {BU_TGT_ETC2, 512, 4, 4, false, true}, {BU_TGT_ETC2, 256, 4, 1, true, false}, {BU_TGT_ETC2, 256, 4, 1, true, true},
    {BU_TGT_RGBA, 1024, 1, 1, true, false}, {BU_TGT_RGBA, 1024, 1, 1, true, true}, {BU_TGT_RGBA, 512, 2, 1, true, false}, {BU_TGT_RGBA, 512, 2, 1, true, true},
// the targets encoded after the RGBA32 unpack (one- and two-channel, then colour): the ETC shapes they are planned in (bu_shape_target) -- one
// tile per CU, the mid shape, the exclusive and the shared large shapes (strips and rectangles), the zero-copy shape
#define BU_CHANNEL_SHAPES(T, SHARED_PREFETCH)                                                                                                   \
    {T, 1024, 1, 1, false, false}, {T, 512, 2, 1, false, false}, {T, 1024, 4, 1, true, false}, {T, 1024, 4, 1, true, true},                     \
    {T, 512, 4, 4, SHARED_PREFETCH, false}, {T, 512, 4, 4, SHARED_PREFETCH, true}, {T, 256, 4, 1, true, false}
    BU_CHANNEL_SHAPES(BU_TGT_BC4, true), BU_CHANNEL_SHAPES(BU_TGT_BC5, false), BU_CHANNEL_SHAPES(BU_TGT_R11, true), BU_CHANNEL_SHAPES(BU_TGT_RG11, false),
    BU_CHANNEL_SHAPES(BU_TGT_BC1, true), BU_CHANNEL_SHAPES(BU_TGT_BC3, false),
#undef BU_CHANNEL_SHAPES
};
constexpr int bu_sorted_kernel(int target, const BuShape& s, bool rect)
{
    int i = 0;
    for (const BuSortedKey& k : BU_SORTED_KERNELS) {
        if (k.target == target && k.wgs == s.wgs && k.bpt == s.bpt && k.minw == s.minw && k.prefetch == s.prefetch && k.rect == rect) return i;
        i++;
    }
    return -1;
}

// Tile tickets (kernel, `ticket`): tiles per workgroup from which an exclusive BC7 / ASTC / RGBA32 launch draws its tiles by ticket (ETC1 / ETC2 are bound by
// vector-ALU issue on every CU alike: nothing to balance, +0.7 % with tickets)
constexpr size_t BU_TICKET_MIN_WALK = 16;
constexpr bool bu_ticket_target(int target) { return target == BU_TGT_BC7 || target == BU_TGT_ASTC || target == BU_TGT_RGBA; }

// ---- the plain launch: one slice -----------------------------------------------------------------------------------------------
// one launch of bu_launch_uastc: blocks [offset, offset + n) of the slice, numbered from its base + offset
struct BuSliceLaunch {
    size_t offset, n;
    int kernel;           // BU_SORTED_KERNELS[kernel]; -1: the one-lane-per-block kernel (bu_uastc_kernel)
    unsigned grid, block;
    unsigned tile_rt;     // blocks per tile (layout STRIP)
    unsigned rect_magic;  // ceil(2^32 / tiles per row): the kernel's tile -> (row, column) reciprocal, its `tile_rt` argument under RECT
    unsigned cus;         // generation priorities (kernel, `cus`); 0: none
    size_t bpr;           // the pitch the kernel is given: the caller's, or a virtual one
    bool wants_ticket;    // the launch draws its tiles by ticket (bu_ticket_for)
};

// BU_LAUNCH_AUTO is decided per call, and only where the shapes differ (a launch of more than one tile per CU): bu_plan_slice reads the policy
// only then, and the launcher resolves AUTO (bu_auto_policy) or notes an explicit policy's enqueue (bu_note_big_enqueue) exactly for these launches
inline bool bu_slice_needs_policy(size_t n_blocks, unsigned grid_cap, unsigned cu_count)
{
    return n_blocks >= (size_t)BU_SORT_MIN_BLOCKS && grid_cap == 0 && n_blocks > (size_t)BU_HOST_TILE * cu_count;
}

// The launches of one slice of n_blocks blocks (blocks_per_row: the caller's block grid, 0 = unknown) under the resolved `policy` (BU_POLICY_*, not AUTO).
// grid_cap > 0 (zero-copy over PCIe): 1024-block tiles on at most grid_cap workgroups.
// (kernel_target: the slice's target, whose kernels run; every shape decision is its family's, bu_shape_target)
inline void bu_plan_slice(int kernel_target, size_t n_blocks, size_t bpr, unsigned grid_cap, int policy, unsigned cu_count, std::vector<BuSliceLaunch>& out)
{
    const int target = bu_shape_target(kernel_target);
    out.clear();
    if (n_blocks == 0) return;
    if (n_blocks < (size_t)BU_SORT_MIN_BLOCKS) {
        out.push_back(BuSliceLaunch{0, n_blocks, -1, bu_grid_for(n_blocks, cu_count), (unsigned)BU_WG, 0u, 0u, 0u, bpr, false});
        return;
    }
    // mode-sorted kernel.  The kernel indexes with 32 bits, so very large slices are cut into launches of <= 2^26 blocks
    // (1 GiB in); RGBA32 pieces end on whole block rows so the image addressing stays launch-relative.
    size_t piece = (size_t)1 << 26;
    if (target == BU_TGT_RGBA) piece = bpr <= piece ? (piece / bpr) * bpr : bpr;
    constexpr size_t RW = BU_RECT_W;
    // blocks_per_row allows rectangular tiles at all: a multiple of 64, at least two tiles wide, below 2^21
    // (one tile per row, blocks_per_row == 64: the strip IS the rectangle)
    bool rect_rows = grid_cap == 0 && bpr >= 2 * RW && bpr % RW == 0 && bpr < ((size_t)1 << 21);
    // every piece of the slice is a multiple of (rows per tile x blocks_per_row) for rows per tile dividing this
    const size_t rect_quantum = n_blocks <= piece ? 0 : piece;
    // A VIRTUAL pitch for BC7 / ASTC when the caller gave no usable block grid (blocks_per_row 0, or no multiple of 64): for a block-linear target the
    // grid never changes a byte, it only decides which 1024 blocks form a tile -- and a tile that is 16 segments of 1 KiB at a pitch of 4 KiB or more
    // loads and stores measurably faster than 16 KiB in a row (its 16 segments sit on 16 different HBM channel groups; the workgroup waits for ALL of its
    // tile at barrier 1): strips 8.94 / 5.77 / 187.5 us against 8.45 / 5.56 / 177.7 for a lone 2^20-block launch / four in flight / one 2^25-block launch
    // (profiles/r06_tile_pitch_sweep.txt).  Needs whole tiles: the slice a multiple of 16 x pitch blocks.  (A real grid is kept whatever its pitch:
    // on texture-like content rectangles of the IMAGE keep regions of one mode whole, which is worth more.)
    if (!rect_rows && grid_cap == 0 && (target == BU_TGT_BC7 || target == BU_TGT_ASTC)) {
        for (const size_t v : {(size_t)1024, (size_t)2048, (size_t)512, (size_t)256}) {
            if (n_blocks % (16 * v) == 0) {
                bpr = v;
                rect_rows = true;
                break;
            }
        }
    }
    const unsigned rect_magic = rect_rows ? (unsigned)((((unsigned long long)1 << 32) + bpr / RW - 1) / (bpr / RW)) : 0u;  // ceil(2^32 / tiles per row)
    const bool etc = target == BU_TGT_ETC1 || target == BU_TGT_ETC2;
    if (target == BU_TGT_RGBA && policy == BU_POLICY_SHARED_FEW) policy = BU_POLICY_SHARED;
    for (size_t done = 0; done < n_blocks; done += piece) {
        const size_t nb = n_blocks - done < piece ? n_blocks - done : piece;
        const size_t tiles = (nb + BU_HOST_TILE - 1) / BU_HOST_TILE;
        auto go = [&](const BuShape& S, size_t grid, unsigned cus, size_t tile_rt, bool ticket) {
            // Rectangular tiles (kernel, RECT): the caller told us the block grid, it is a multiple of 64 wide and the piece -- and every
            // other piece of the slice -- is whole rows of tiles `rows` blocks high
            const size_t rows = S.tile() / RW;
            const bool rect_ok = rect_rows && nb % (rows * bpr) == 0 && (rect_quantum == 0 || rect_quantum % (rows * bpr) == 0);
            // (a shape that sizes its tile at run time is rectangular only when that size is the full tile)
            const bool rect = S.rect && rect_ok && (!bu_dyn_tile(target, (int)S.tile()) || tile_rt == S.tile());
            ticket = ticket && grid_cap == 0 && grid >= BU_TICKET_MIN_GRID;
            out.push_back(BuSliceLaunch{done, nb, bu_sorted_kernel(kernel_target, S, rect), (unsigned)grid, (unsigned)S.wgs, (unsigned)tile_rt, rect_magic, cus, bpr, ticket});
        };
        // a large launch in shape S: persistent workgroups, PER_CU per CU, walking equal shares of the tiles.  `priorities`: the static wave
        // priorities by residency generation (kernel, `cus`).  They serve a launch that is ALONE on the chip (BC7 8.57 -> 8.37 us) and hurt as
        // soon as launches of several streams share the CUs -- the generations of different launches then compete through the same four levels:
        // shared shape, four in flight 5.72-5.79 -> 5.44-5.56 us per atlas without them (the exclusive shape on two streams 6.70 -> 5.97:
        // profiles/r05_ab_wave_priorities_with_launches_in_flight.txt) -- so the shared policy launches without.
        auto go_big = [&](const BuShape& S, bool priorities) {
            const size_t slots = (size_t)cu_count * S.per_cu;
            const size_t tile_rt = bu_balanced_tile(S.tile(), nb, slots, bu_dyn_tile(target, (int)S.tile()));
            const size_t big_tiles = (nb + tile_rt - 1) / tile_rt;
            // generation priorities (kernel, `cus`) only when every workgroup walks the same number of tiles: with 1.25 tiles per
            // slot the one-tile generations run ahead of the two-tile ones (1.25 Mi blocks BC7 13.06 -> 11.57 us, ASTC 13.5 -> 11.0)
            const unsigned cus = (priorities && (big_tiles <= slots || big_tiles % slots == 0)) ? cu_count : 0u;
            // Tile tickets (kernel, `ticket`) for the LONG walks of a launch that has the chip to itself: with a fixed share of 32 tiles per workgroup
            // a 2^25-block BC7 launch takes 188.5 us, with tickets 174 (ASTC 201 -> 184.5; the launch ends when the tiles do, not when the slowest share
            // does; 16 tiles per workgroup: BC7 -2.8 %, ASTC -5 %, RGBA32 -4 %; 8: +-0); a walk of 2-4 tiles loses to the atomics' round trips at its head
            // and tail (2^22 blocks: 26.7 -> 32.2 us), and launches that share the chip fill each other's tails anyway (four 2^25-block launches in flight
            // 167 -> 171): profiles/r06_ab_tile_tickets.txt
            const bool ticket = priorities && bu_ticket_target(target) && big_tiles >= BU_TICKET_MIN_WALK * slots;
            go(S, big_tiles < slots ? big_tiles : slots, cus, tile_rt, ticket);
        };
        if (target == BU_TGT_RGBA) {
            // RGBA32, 64 B of output per block: results return through a 64 KiB LDS tile (1024 blocks x 4 rows, the input tile aliased
            // into row 0) so the image rows leave as coalesced 1 KiB stores; persistent workgroups walk their tiles with prefetch, two per
            // CU (one under the shared policy).  Up to 3 Mi blocks 1024 threads per tile (32 waves per CU: 2^18 blocks 7.8 -> 7.2 us,
            // 2^20 17.95 -> 16.9, 2^21 35.0 -> 33.75), above that 512 threads x 2 blocks (2^22 blocks 62.7 against 64.4 us, 2^24 252
            // against 265).  The zero-copy launches (grid_cap) keep the 512 x 2 shape.
            const size_t cap = grid_cap ? (size_t)grid_cap : (size_t)cu_count * (policy == BU_POLICY_SHARED ? 1 : 2);
            const size_t grid = tiles < cap ? tiles : cap;
            // generation priorities only when every workgroup walks at least two tiles (2^19 blocks 10.7 -> 10.3 us and
            // 786 432 blocks 15.75 -> 14.24 without them, 2^20 blocks 16.7 against 18.7 with them)
            const unsigned cus = (policy != BU_POLICY_SHARED && tiles >= 2 * grid) ? cu_count : 0u;
            const bool ticket = policy != BU_POLICY_SHARED && tiles >= BU_TICKET_MIN_WALK * grid;  // (tile tickets for long walks, as go_big)
            const bool wide = grid_cap == 0 && nb <= ((size_t)3 << 20);
            go(wide ? BuShape{1024, 1, 1, true, true, 2} : BuShape{512, 2, 1, true, true, 2}, grid, cus, BU_HOST_TILE, ticket);
        } else if (grid_cap) {
            go(BuZeroCopyShape, tiles < grid_cap ? tiles : grid_cap, cu_count, BuZeroCopyShape.tile(), false);
        } else if (nb <= (size_t)BU_HOST_TILE * cu_count) {
            go(BuOneTileShape(target), tiles, cu_count, BU_HOST_TILE, false);
        } else if (bu_big_from_one_tile_per_cu(target) || nb > (size_t)3 * BU_HOST_TILE * cu_count) {
            // BU_POLICY_SHARED_FEW (BC7 / ASTC, from bu_auto_policy when one or two other launches are in flight): the shared policy's kernel with the grid at four
            // workgroups per CU -- 1024 one-tile workgroups dealt by the hardware dispatcher instead of 512 persistent ones walking two tiles each.  With two /
            // three launches in flight 6.07 / 5.7 us per 2^20-block atlas against 6.95 / 6.1 (shared) and 6.85 / 6.3 (exclusive); with four the persistent form wins
            // (5.60 against 5.77): profiles/r06_ab_bc7_shared_one_tile_workgroups.txt
            const BuShape shared = BuBigShape(target, BU_POLICY_SHARED);
            if (etc && nb >= ((size_t)1 << 20))
                // ETC1 / ETC2 from 2^20 blocks on, under EVERY policy: ONE-TILE workgroups of the shared shape (512 x 4 on a 2048-block tile, two resident per CU) dealt by the
                // hardware dispatcher instead of a persistent grid -- the form in which four launches in flight reach 12.2 / 15.1 us per 2^20 blocks, in ONE launch.  Exclusive (was
                // 1024 x 4, one per CU): 2^20 blocks 17.8 / 22.2 -> 17.5 / 20.6 us, 1.5 x 2^20 28.2 / 33.9 -> 23.8 / 28.1, 2^22 59.5 / 75.6 -> 54.1 / 65.1, 2^25 433 / 556 -> 394 / 479
                // (12.3 / 15.0 per 2^20); shared (was 512 x 4 persistent, one per CU): one launch at a time 20.2 / 25.0 -> 17.6 / 20.6, two in flight 13.2 / 16.3 -> 12.1 / 15.0, three
                // and four +-1 %.  Below 2^20 blocks the persistent grids stay ahead (0.8 x 2^20 exclusive: 16.2 / 19.4 against 17.8 / 21.0).  Walking 2 / 4 / 8 tiles per workgroup
                // gives the gain back step by step (profiles/r06_ab_etc_one_tile_workgroups.txt; the copies of profiles/r06_copy_ceiling_by_size.txt behave the same way).
                // (No tile tickets for plain ETC launches, persistent or not; the multi-run launch's persistent ETC grids do take them: bu_plan_multi_kernel.)
                go(shared, (nb + shared.tile() - 1) / shared.tile(), 0u, shared.tile(), false);
            else if (policy == BU_POLICY_SHARED_FEW && bu_big_from_one_tile_per_cu(target))
                go_big(BuShape{shared.wgs, shared.bpt, shared.minw, shared.prefetch, shared.rect, 4}, false);
            else if (policy == BU_POLICY_SHARED || policy == BU_POLICY_SHARED_FEW) go_big(shared, false);
            else if (target == BU_TGT_ASTC && nb >= ((size_t)1 << 21))
                // ASTC from 2^21 blocks on: 256 x 4, five per CU (79 VGPRs, 24 KiB) -- 2^21 / 2^22 / 2^23 / 2^25 blocks 15.2 / 28.3 / 53.6 / 183.3 -> 14.3 / 27.5 / 51.2 / 179.9 us,
                // 2^24 level (97.5 / 98.0), a lone 2^20-block atlas 8.9 -> 9.9: profiles/r06_ab_astc_large_launch_256x4.txt.  (BC7 loses 0-5 % in that shape at every size.)
                go_big(BuShape{256, 4, 1, true, true, 5}, true);
            else go_big(BuBigShape(target, BU_POLICY_EXCLUSIVE), true);
        } else {
            go(BuEtcMidShape, tiles, cu_count, BU_HOST_TILE, false);
        }
    }
}

// ---- the multi-run launch: several runs at unrelated addresses in one launch (kernel layout MULTI) --------------------------------
// a table entry: blocks [offset, offset + n) of runs[run], tiled as strips (BU_RUN_STRIPS) or as whole rectangles of a 64 << vshift-block-wide grid
struct BuRunEntry { size_t run, offset, n; uint32_t vshift, first_tile; };
// the instantiations of bu_uastc_multi_kernel: <T, 512, 4> (ETC1 / ETC2, 2048-block tiles), <T, 1024, 1>, <T, 256, 4, true, true> (BC7 / ASTC), <T, 512, 2, true>
enum { BU_MULTI_ETC_2048 = 0, BU_MULTI_ONE_TILE = 1, BU_MULTI_WHOLE = 2, BU_MULTI_PERSIST = 3 };
struct BuRunsLaunch {
    size_t plain_run = SIZE_MAX;  // SIZE_MAX: a multi-run launch of entries[0 .. k); else the plain launch of runs[plain_run]
    BuRunEntry entries[BU_MULTI_RUNS];
    size_t k = 0, n_tiles = 0;
    unsigned tile = 1024;       // 1024, or 2048 (ETC1 / ETC2 large batches)
    bool all_whole = true;      // every entry is tiled as whole rectangles
    bool needs_policy = false;  // the kernel depends on the launch policy: BU_LAUNCH_AUTO is resolved for this launch (bu_auto_policy)
    int kernel = BU_MULTI_PERSIST;  // bu_plan_multi_kernel: BU_MULTI_*, grid, workgroup size, tile tickets
    unsigned grid = 0, block = 0;
    bool wants_ticket = false;
};

// runs[0 .. n_runs) on ONE stream: one run is the plain launch; several runs at unrelated addresses are ONE launch per BU_MULTI_RUNS runs,
// the run table in the kernel arguments (kernel layout MULTI).  The kernels of the multi-run launches are left to bu_plan_multi_kernel.
// Launching the runs one by one is bound by the ~4 us of host time per launch whatever the number of streams (64 slices
// of 65 536 blocks: 290 us on one stream, 230-260 us on 2-8, profiles/r03_small_slices_streams_vs_one_launch.txt).
// (a run too long for the table's 32-bit fields -- 2^32 blocks or more -- never enters it: it goes out as the plain launch
// below, which cuts it into pieces of 2^26 blocks, exactly as it would on its own)
inline void bu_plan_runs(int kernel_target, const BuRun* runs, size_t n_runs, size_t blocks_per_row, unsigned cu_count, std::vector<BuRunsLaunch>& out)
{
    const int target = bu_shape_target(kernel_target);  // (as bu_plan_slice)
    out.clear();
    // BC7 / ASTC / RGBA32: a run that is whole 64 x 16-block rectangles of a power-of-two grid is tiled that way -- the caller's blocks_per_row if it is one, else (block-
    // linear targets; RGBA32 is an image and has only its real pitch) a virtual pitch (bu_plan_slice has the story: 16 segments of 1 KiB at >= 4 KiB pitch load faster than
    // 16 KiB in a row; multi-run launch over 32 slices of 2^20 blocks 6.0 -> 5.6 us per slice; RGBA32 14.8 -> 12.9: profiles/r06_ab_rgba_multi_run_rectangles.txt).
    // whole_pitch = the pitch n blocks are whole rectangles of (0: none); prefix_pitch = the largest pitch of the list with at least eight tile rows in n (ragged runs: their
    // whole PREFIX goes out as an entry of its own, the remainder as strips -- RGBA32 only: 64 ragged images of 1021 x 1024 blocks 15.0 -> 13.1 us per image, BC7 / ASTC unmoved:
    // profiles/r06_ab_rgba_multi_run_rectangles.txt)
    const bool rect_target = target == BU_TGT_BC7 || target == BU_TGT_ASTC || target == BU_TGT_RGBA;
    const size_t real = (blocks_per_row >= 128 && (blocks_per_row & (blocks_per_row - 1)) == 0 && blocks_per_row <= BU_MULTI_MAX_WIDTH) ? blocks_per_row : 0;
    const size_t virt = target == BU_TGT_RGBA ? 0 : 1;
    const size_t pitches[5] = {real, virt * 1024, virt * 2048, virt * 512, virt * 256};
    auto shift_of = [](size_t v) {
        uint32_t sh = 0;
        while (((size_t)BU_RECT_W << sh) < v) sh++;
        return sh;
    };
    for (size_t r0 = 0; r0 < n_runs;) {
        if (target == BU_TGT_RGBA && blocks_per_row > BU_MULTI_RGBA_MAX_BPR) {  // (the kernel's 32-bit lane offsets: bu_multi_addr.hpp)
            out.emplace_back().plain_run = r0++;
            continue;
        }
        BuRunsLaunch l;
        // ETC1 / ETC2 batches of 2^20 blocks or more in runs long enough for them: 2048-block tiles, ONE tile per workgroup, dealt by the hardware dispatcher (512 x 4 under the
        // shared shape's launch bounds, two resident per CU) -- what the plain launch does from 2^20 blocks on (bu_plan_slice): 64 slices of 2^20 blocks in separate
        // allocations 13.8 / 17.5 -> see profiles/r06_ab_etc_one_tile_workgroups.txt.  (Many short runs keep 1024-block tiles: a run's last tile is partly empty.)
        if (target == BU_TGT_ETC1 || target == BU_TGT_ETC2) {
            size_t total = 0, tiles2 = 0;
            for (size_t i = r0; i < n_runs && i < r0 + BU_MULTI_RUNS; i++) {
                total += runs[i].n;
                tiles2 += (runs[i].n + 2047) / 2048;
            }
            if (total >= ((size_t)1 << 20) && tiles2 * 2048 <= total + total / 8) l.tile = 2048;
        }
        auto emit = [&](size_t run, size_t offset, size_t n, uint32_t vshift) {
            l.all_whole = l.all_whole && vshift != BU_RUN_STRIPS;
            l.entries[l.k++] = BuRunEntry{run, offset, n, vshift, (uint32_t)l.n_tiles};
            l.n_tiles += (n + l.tile - 1) / l.tile;
        };
        size_t used = 0;
        for (; r0 + used < n_runs && l.k < BU_MULTI_RUNS; used++) {
            const size_t ri = r0 + used, n = runs[ri].n;
            const size_t t = (n + l.tile - 1) / l.tile;
            if (l.n_tiles + t + 1 >= (((size_t)1 << 32) / l.tile)) break;  // (tiles x tile size is the launch's 32-bit block count)
            size_t whole_pitch = 0, prefix_pitch = 0;
            if (rect_target) {
                for (const size_t v : pitches)
                    if (v && n % (16 * v) == 0) {
                        whole_pitch = v;
                        break;
                    }
                if (!whole_pitch && target == BU_TGT_RGBA && l.k + 2 <= BU_MULTI_RUNS)  // (BC7 / ASTC gain nothing from the split: 5.95 / 6.3 us per slice either way)
                    for (const size_t v : pitches)
                        if (v && n >= 8 * 16 * v) {  // (at least eight tile rows of rectangles, or the split is not worth an entry)
                            prefix_pitch = v;
                            break;
                        }
            }
            if (whole_pitch) {
                emit(ri, 0, n, shift_of(whole_pitch));
            } else if (prefix_pitch) {
                const size_t prefix = n / (16 * prefix_pitch) * (16 * prefix_pitch);
                emit(ri, 0, prefix, shift_of(prefix_pitch));
                emit(ri, prefix, n - prefix, BU_RUN_STRIPS);
            } else {
                emit(ri, 0, n, BU_RUN_STRIPS);
            }
        }
        if (used <= 1) {  // a run on its own (the last one of a long batch, or one of 2^32 blocks): the plain launch
            out.emplace_back().plain_run = r0++;
            continue;
        }
        // (the one-tile-per-CU shape is the same under both policies: AUTO is not resolved for it, and the multi-run launch never reports an
        // explicit policy's enqueue to bu_auto_policy as the plain launch does)
        l.needs_policy = !(l.tile == 1024 && l.n_tiles <= (size_t)cu_count);
        out.push_back(l);
        r0 += used;
    }
}

// The kernel of a multi-run launch under the resolved `policy` (BU_POLICY_*, not AUTO).
// Shapes, as the plain launcher picks them by size (bu_plan_slice): at most one tile per CU 1024 threads on it; beyond that 512 x 2.
// BC7 / ASTC / RGBA32 batches of more tiles than fit the chip at once run as a PERSISTENT grid (four / four / two workgroups per CU)
// whose workgroups walk the tiles of all runs with the next tile's loads in flight -- a batch of large slices in separate
// allocations is then one long launch that overlaps its own loads and compute (two 2^20-block slices 7.9 us each, eight 6.4, against
// 8.4 for plain launches one after another and 9.2-10.2 through the round-4 table kernel without the prefetch).  ETC1 / ETC2 walk the same way with
// TWO workgroups per CU (97 / 119 VGPRs: 16 waves are what fits): 64 slices of 2^20 blocks in separate allocations 15.4 / 19.4 -> 13.8 / 17.5 us per
// slice against one-tile workgroups dealt by the dispatcher (tools/exp/etc_multi_persist.sh; their plain large shape sorts 4096-block tiles, the
// table numbers 1024-block ones: 13.4 / 17.1 when the slices are adjacent and merge into one run).
// Launch policy of a grouped launch.  Under the shared policy (launches of other streams run beside this one: bu_uastc_transcode_batch_in_flight
// with groups of small runs) the PERSISTENT grid is capped at about half of every CU -- two workgroups of 512 threads for BC7 / ASTC (16 of the 32 wave
// slots, 56 of the 160 KiB; four of 256 in the whole-tile shape below), one for RGBA32 -- so that two such launches fit side by side (ETC1 / ETC2: one of the two that fit; 64 slices of
// 65 536 blocks on four streams 66.3 / 80.2 -> 65.0 / 78.0 us, tools/exp/etc_small_slices.sh); the one-tile-per-CU shape is the same under both
// policies (a tile's 1024 threads cannot be halved).
inline void bu_plan_multi_kernel(int kernel_target, int policy, unsigned cu_count, BuRunsLaunch& l)
{
    const int target = bu_shape_target(kernel_target);  // (as bu_plan_slice)
    const bool half = policy == BU_POLICY_SHARED || policy == BU_POLICY_SHARED_FEW;
    const bool etc = target == BU_TGT_ETC1 || target == BU_TGT_ETC2;
    // BC7 / ASTC batches whose runs are all whole rectangular tiles (the variant without validity tests): 256 x 4, FIVE workgroups per CU (63 / 76 VGPRs, 31 / 27 KiB),
    // four under the shared policy.  ASTC's 512 x 2 form of that variant sits at exactly 64 VGPRs -- the compiler gets there by serialising -- and ran 64 atlases in
    // separate allocations at 5.95-6.0 us per atlas where the plain kernel does 5.5: 5.59-5.63 in this shape (64 / 512 slices of 65 536 blocks 32.8 / 243 -> 30.6 / 219 us);
    // BC7 5.57-5.75 -> 5.52-5.57, 512 small slices 224 -> 215 (in flight 202 -> 191): profiles/r06_ab_multi_run_256x4.txt.  Everything else 512 x 2, four / two per CU.
    const bool whole = (target == BU_TGT_BC7 || target == BU_TGT_ASTC) && l.all_whole;
    const size_t cap = (size_t)cu_count * (target == BU_TGT_RGBA ? (half ? 1 : 2) : etc ? (half ? 1 : 2) : whole ? (half ? 4 : 5) : (half ? 2 : 4));
    const size_t grid = l.n_tiles < cap ? l.n_tiles : cap;
    l.kernel = (etc && l.tile == 2048) ? BU_MULTI_ETC_2048 : (l.tile == 1024 && l.n_tiles <= (size_t)cu_count) ? BU_MULTI_ONE_TILE : whole ? BU_MULTI_WHOLE : BU_MULTI_PERSIST;
    l.grid = (unsigned)(l.kernel == BU_MULTI_ETC_2048 ? l.n_tiles : grid);  // (one-tile workgroups dealt by the dispatcher)
    l.block = l.kernel == BU_MULTI_ONE_TILE ? 1024 : l.kernel == BU_MULTI_WHOLE ? 256 : 512;
    // tile tickets for the long walks of a persistent grid that has the chip to itself, as bu_plan_slice (a batch of 64 slices of 2^20 blocks in
    // separate allocations: 64 tiles per workgroup); ETC1 / ETC2 included here, unlike their plain launches
    l.wants_ticket = (l.kernel == BU_MULTI_WHOLE || l.kernel == BU_MULTI_PERSIST) && !half && l.n_tiles >= BU_TICKET_MIN_WALK * grid &&
                     l.grid >= BU_TICKET_MIN_GRID;
}
