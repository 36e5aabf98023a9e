// Addresses of the multi-run launch (kernel layouts MULTI and MULTI_WHOLE of bu_uastc_sorted_body): which tiles the run a workgroup is walking holds, where a
// tile's corner block lies, and how far from that corner a lane's block is -- ONE copy, compiled into the kernel and into the test-only host build.
// No HIP in here: tests/test_multi_addr.py checks the arithmetic without a GPU.
//
// Every access of a tile is  (wave-uniform 64-bit address of the tile's corner block) + (32-bit byte offset of the lane's block from that corner):
//   * the corner moves with the tile and is scalar arithmetic on the run's record (bu_tile_of);
//   * the lane offset depends on the thread and on the run's WIDTH only (bu_lane_off): it is the same for every tile of a run, the same for a tile's loads and its
//     stores, and is recomputed only when the walk reaches a run of another width.
// A run may hold up to 2^32 - 1 blocks; nothing but the lane offset ever sits in 32 bits.
#pragma once
#include <stdint.h>

#include "bu_launch_plan.hpp"  // BU_RECT_W, BU_RUN_STRIPS, BU_MULTI_MAX_WIDTH, BU_MULTI_RGBA_MAX_BPR

// a run as the kernel's table holds it (BuRunDesc of bu_kernels.hpp, addresses as integers)
struct BuRunRec {
    uint64_t in, out, base;  // the run's first block, its output, its block-index base (status words)
    uint32_t n;              // blocks
    uint32_t vshift;         // BU_RUN_STRIPS, or whole 64 x (tile / 64)-block rectangles of a grid 64 << vshift blocks wide
};
// the run a workgroup is walking, in wave-uniform registers: a tile inside [first_tile, first_tile + n_tiles) needs no look-up in the table
struct BuRunCursor {
    BuRunRec run;
    uint32_t first_tile, n_tiles;
};
// the tile a workgroup loads or writes back
struct BuMultiTile {
    uint64_t in;     // address of the tile's corner block (strips: its first block)
    uint64_t out;    // address the corner block's result goes to (RGBA32: the start of the corner's row of blocks in the image; the column is in the lane offset)
    uint64_t base;   // block-index base of the run
    uint32_t first;  // the corner's block index inside its run.  Strips: tile number x tile size; rectangles: (tile / 64 * tile row) * width + 64 * tile column
    uint32_t n;      // blocks the tile holds
    uint32_t width;  // rectangles: blocks per row of the run's (virtual) grid; 0: strips
    uint32_t bx0;    // RGBA32: the corner block's column in the image
};

BU_DEV BuRunCursor bu_no_run() { return BuRunCursor{BuRunRec{0, 0, 0, 0u, BU_RUN_STRIPS}, 0u, 0u}; }
// (n / tile + 1 for a ragged end, not (n + tile - 1) / tile: n may be 2^32 - 1)
BU_DEV BuRunCursor bu_run_cursor(const BuRunRec& r, uint32_t first_tile, uint32_t tile) { return BuRunCursor{r, first_tile, r.n / tile + (r.n % tile ? 1u : 0u)}; }
BU_DEV bool bu_cursor_holds(const BuRunCursor& c, uint32_t t) { return t - c.first_tile < c.n_tiles; }  // (one unsigned compare; an empty cursor holds nothing)

// Tile t of the cursor's run (bu_cursor_holds(c, t)).  `tile`: blocks per tile; `out_bytes`: bytes per block of the output (8 or 16; RGBA32: 16, one pixel row);
// `rgba_bpr`: 0, or RGBA32's blocks per image row (block idx of a run goes to pixel rows 4 * (idx / bpr) .. + 3, 16 bytes at column idx % bpr)
BU_DEV BuMultiTile bu_tile_of(const BuRunCursor& c, uint32_t t, uint32_t tile, uint32_t out_bytes, uint32_t rgba_bpr)
{
    const BuRunRec& r = c.run;
    const uint32_t lt = t - c.first_tile;  // the tile's number inside its run
    BuMultiTile d;
    if (r.vshift != BU_RUN_STRIPS) {
        // a 64 x (tile / 64)-block rectangle of the run's grid (tiles per row a power of two): segments of 1 KiB at the grid's pitch
        const uint32_t ty = lt >> r.vshift, tx = lt & ((1u << r.vshift) - 1u);
        d.width = (uint32_t)BU_RECT_W << r.vshift;
        d.first = (tile / (uint32_t)BU_RECT_W) * ty * d.width + (uint32_t)BU_RECT_W * tx;  // a block of the run: below n < 2^32
        d.n = tile;
    } else {
        d.width = 0u;
        d.first = lt * tile;
        d.n = r.n - d.first < tile ? r.n - d.first : tile;
    }
    d.in = r.in + (uint64_t)d.first * 16u;
    d.base = r.base;
    if (rgba_bpr) {
        const uint32_t by0 = d.first / rgba_bpr;
        d.bx0 = d.first - by0 * rgba_bpr;
        d.out = r.out + (uint64_t)by0 * rgba_bpr * 64u;  // four pixel rows of bpr x 16 bytes per row of blocks
    } else {
        d.bx0 = 0u;
        d.out = r.out + (uint64_t)d.first * out_bytes;
    }
    return d;
}

// Byte offset of block l of a tile from the tile's corner block, in the INPUT (16 bytes per block) -- and in the output of a 16-byte target; an 8-byte target
// stores at half of it.  `whole`: the layout knows every run is rectangles (width != 0).  l < 2048 and width <= BU_MULTI_MAX_WIDTH:
// ((2048 / 64 - 1) * 2^20 + 63) * 16 < 2^29.
BU_DEV uint32_t bu_lane_off(bool whole, uint32_t width, uint32_t l)
{
    return ((whole || width) ? (l / (uint32_t)BU_RECT_W) * width + (l % (uint32_t)BU_RECT_W) : l) * 16u;
}
static_assert((uint64_t)((2048 / BU_RECT_W - 1) * (uint64_t)BU_MULTI_MAX_WIDTH + BU_RECT_W - 1) * 16u < ((uint64_t)1 << 32), "a lane offset fits 32 bits");
// block index inside its run of the block `off` bytes from the corner of tile d (status words: d.base + this)
BU_DEV uint64_t bu_lane_block(const BuMultiTile& d, uint32_t off) { return (uint64_t)d.first + (off >> 4); }

// RGBA32: byte offset, from d.out, of pixel row 0 of the block `off` input bytes from the corner of tile d; the block's pixel row r lies r * bpr * 16 bytes further.
// The block is c = bx0 + off / 16 blocks from the start of the corner's row of blocks, dy = c / bpr rows of blocks down, at column c - dy * bpr: pixel row 4 * dy,
// ((4 dy) bpr + c - dy bpr) * 16 = (3 dy bpr + c) * 16 bytes.  With pixel row 3 that is at most (4 c + 3 bpr) * 16 < (7 bpr + 4 off / 16) * 16 <= 7 * 2^28 + 2^31
// for bpr <= BU_MULTI_RGBA_MAX_BPR: 32 bits hold it (the planner sends wider images out as plain launches).
BU_DEV uint32_t bu_lane_off_rgba(const BuMultiTile& d, uint32_t off, uint32_t bpr)
{
    const uint32_t c = d.bx0 + (off >> 4), dy = c / bpr;
    return (3u * dy * bpr + c) * 16u;
}
static_assert((7 * (uint64_t)BU_MULTI_RGBA_MAX_BPR + 4 * ((2048 / BU_RECT_W) * (uint64_t)BU_MULTI_MAX_WIDTH)) * 16u < ((uint64_t)1 << 32), "an RGBA32 lane offset fits 32 bits");

// the run of tile t: the last entry of `first_tile` (ascending, unused entries ~0) that is <= t.  The kernel finds it with one ballot per 64 entries; this is
// the same count, for the host.
inline uint32_t bu_run_of_tile(const uint32_t* first_tile, uint32_t entries, uint32_t t)
{
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < entries; i++) cnt += first_tile[i] <= t;
    return cnt - 1u;
}
