// Rectangles of UASTC slices into pitched surfaces (bu_uastc_transcode_rects_device): the job table the kernel reads, the address mapping of a tile
// and of a block inside it -- ONE copy, compiled into the kernel (layout RECTS of bu_uastc_sorted_body) and into the test-only host build -- and the
// launch plan (bu_plan_rects).  No HIP in here: tests/test_rect_plan.py checks the plan and the mapping without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bu_launch_plan.hpp"

// ---- tiles -----------------------------------------------------------------------------------------------------------------------
// Every job is cut into tiles of BU_RECTS_TILE blocks whose shape is chosen per job: 2^tshift blocks wide with 2^tshift the smallest of 8 / 16 / 32 / 64 not
// below min(w, 64), and BU_RECTS_TILE >> tshift blocks high (a 64 x 16 tile wastes half its lanes on a 32-wide page; a 32 x 32-block page is exactly one
// tile).  Tiles are numbered row by row; those at the right and bottom edge are clipped, their missing lanes sit out as lanes past the end of a strip do.
constexpr unsigned BU_RECTS_TILE = 1024;
constexpr unsigned BU_RECT_JOBS = 64;  // jobs per launch: one ballot over the first-tile numbers finds a tile's job
constexpr uint64_t BU_RECTS_MAX_TILES = ((uint64_t)1 << 32) / BU_RECTS_TILE - 1;  // tiles per launch: tiles x tile size is the kernel's 32-bit block count
BU_DEV uint32_t bu_rect_tshift(uint32_t w) { return w > 32u ? 6u : w > 16u ? 5u : w > 8u ? 4u : 3u; }

// one job as the kernel reads it (bu_rect_job with the rectangle's origin folded into the addresses)
struct BuRectDesc {
    uint64_t in;      // address of the rectangle's block (0, 0): d_in + 16 * (y0 * in_bpr + x0)
    uint64_t out;     // address its result goes to
    uint64_t pitch;   // bytes from one block row of the output to the next (RGBA32: from one pixel row to the next)
    uint64_t base;    // status-word index of the rectangle's block (0, 0): index_base + y0 * in_bpr + x0
    uint32_t in_bpr;  // blocks per row of the slice the rectangle is cut from
    uint32_t w, h;    // blocks
    uint32_t tpr;     // tiles per row of tiles, ceil(w / tile width)
};
struct BuRectTable {
    BuRectDesc job[BU_RECT_JOBS];
    uint32_t first_tile[BU_RECT_JOBS];  // ascending; entries past the last job hold 0xFFFFFFFF
};
static_assert(sizeof(BuRectDesc) == 48 && sizeof(BuRectTable) % 16 == 0 && sizeof(BuRectTable) <= 3968,
              "the job table must fit the 4 KiB of kernel arguments beside the other parameters");

// tile `lt` of a job: where its corner block is loaded from and stored to, how much of it lies inside the rectangle
struct BuRectTile {
    uint64_t in, out;  // addresses of the tile's block (0, 0)
    uint64_t pitch, base;
    uint32_t in_bpr, tshift;
    uint32_t vc, vr;   // block columns / rows of the tile inside the rectangle (the rest is clipped)
};
// (row_bytes: bytes one block takes of an output row -- the block size, RGBA32: 16; rows_per_block: output rows a block row takes -- 1, RGBA32: 4)
BU_DEV BuRectTile bu_rect_tile(const BuRectDesc& j, uint32_t lt, uint32_t row_bytes, uint32_t rows_per_block)
{
    const uint32_t tshift = bu_rect_tshift(j.w), th = BU_RECTS_TILE >> tshift;
    const uint32_t ty = lt / j.tpr, tx = lt - ty * j.tpr;
    const uint32_t c0 = tx << tshift, r0 = ty * th;
    // r0 * in_bpr + c0 is a block of the rectangle, relative to its origin: below (y0 + h) * in_bpr <= 2^32 (the argument rule), so 32 bits hold it
    const uint32_t first = r0 * j.in_bpr + c0;
    BuRectTile t;
    t.in = j.in + (uint64_t)first * 16u;
    t.out = j.out + (uint64_t)r0 * rows_per_block * j.pitch + (uint64_t)c0 * row_bytes;
    t.pitch = j.pitch;
    t.base = j.base + first;
    t.in_bpr = j.in_bpr;
    t.tshift = tshift;
    t.vc = j.w - c0 < (1u << tshift) ? j.w - c0 : (1u << tshift);
    t.vr = j.h - r0 < th ? j.h - r0 : th;
    return t;
}
// block l of a tile: its row and column inside the tile, whether the rectangle holds it, and (only then meaningful) its offsets
BU_DEV uint32_t bu_rect_row(const BuRectTile& t, uint32_t l) { return l >> t.tshift; }
BU_DEV uint32_t bu_rect_col(const BuRectTile& t, uint32_t l) { return l & ((1u << t.tshift) - 1u); }
BU_DEV bool bu_rect_has(const BuRectTile& t, uint32_t l) { return bu_rect_col(t, l) < t.vc && bu_rect_row(t, l) < t.vr; }
BU_DEV uint32_t bu_rect_idx(const BuRectTile& t, uint32_t l) { return bu_rect_row(t, l) * t.in_bpr + bu_rect_col(t, l); }  // blocks from the tile's corner, in the slice
BU_DEV uint64_t bu_rect_src(const BuRectTile& t, uint32_t l) { return t.in + (uint64_t)bu_rect_idx(t, l) * 16u; }
BU_DEV uint64_t bu_rect_dst(const BuRectTile& t, uint32_t l, uint32_t row_bytes, uint32_t rows_per_block)
{
    return t.out + (uint64_t)(bu_rect_row(t, l) * rows_per_block) * t.pitch + bu_rect_col(t, l) * row_bytes;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// the caller's job (bu_rect_job of include/basisu_hip.h, addresses as integers)
struct BuRectJobIn {
    uint64_t in;
    uint32_t in_bpr, x0, y0, w, h;
    uint64_t out, pitch, index_base;
};
// bytes one block takes of an output row, output rows per block row
constexpr uint32_t bu_rect_row_bytes(int target) { return target == BU_TGT_RGBA ? 16u : (uint32_t)bu_out_words(target) * 4u; }
constexpr uint32_t bu_rect_rows_per_block(int target) { return target == BU_TGT_RGBA ? 4u : 1u; }

// The argument rules of one job (include/basisu_hip.h)
inline bool bu_rect_job_ok(int target, const BuRectJobIn& j)
{
    const uint32_t rb = bu_rect_row_bytes(target);
    if (!j.in || !j.out || !j.w || !j.h || !j.in_bpr) return false;
    if ((uint64_t)j.x0 + j.w > j.in_bpr) return false;
    if ((uint64_t)j.y0 + j.h > ((uint64_t)1 << 32) / j.in_bpr) return false;  // (y0 + h) * in_bpr <= 2^32, without the product: it can pass 2^64
    if (j.in % 16u || j.out % rb || j.pitch % rb) return false;
    return j.pitch >= (uint64_t)j.w * rb;
}

struct BuRectsLaunch {
    BuRectTable table;
    size_t k = 0;                      // entries of the table in use
    size_t job_of[BU_RECT_JOBS] = {};  // the job of the call every entry was cut from
    size_t n_tiles = 0;
    unsigned grid = 0, block = 512;
};

// jobs[0 .. n_jobs) (every one passed bu_rect_job_ok) as launches of bu_uastc_rects_kernel<target>: up to BU_RECT_JOBS table entries and BU_RECTS_MAX_TILES tiles
// per launch, in order.  A job is one entry, unless it holds more tiles than a launch may: then it goes out as bands of whole tile rows, an entry each, and where
// one tile row alone is too many (w >= 2^28) as column bands of BU_RECTS_MAX_TILES tiles first.  An entry is a rectangle of its own to the kernel (the addresses in
// the table are folded), so a band takes the tile shape of its own width.  The grid is left to bu_plan_rects_grid.
constexpr uint64_t BU_RECTS_MAX_COLS = BU_RECTS_MAX_TILES << 6;  // block columns of one entry: a row of 64-wide tiles that a launch can still number
inline void bu_plan_rects(int kernel_target, const BuRectJobIn* jobs, size_t n_jobs, std::vector<BuRectsLaunch>& out)
{
    const uint32_t rpb = bu_rect_rows_per_block(kernel_target), rb = bu_rect_row_bytes(kernel_target);
    out.clear();
    auto close = [&] {
        BuRectsLaunch& l = out.back();
        for (size_t i = l.k; i < BU_RECT_JOBS; i++) {
            l.table.job[i] = BuRectDesc{0, 0, 0, 0, 1u, 1u, 1u, 1u};
            l.table.first_tile[i] = 0xFFFFFFFFu;
        }
    };
    for (size_t ji = 0; ji < n_jobs; ji++) {
        const BuRectJobIn& j = jobs[ji];
        for (uint64_t c0 = 0; c0 < j.w;) {  // c0: the column band's first block column inside the rectangle (one band, unless w > BU_RECTS_MAX_COLS)
            const uint32_t bw = (uint32_t)(j.w - c0 < BU_RECTS_MAX_COLS ? j.w - c0 : BU_RECTS_MAX_COLS);
            const uint32_t tshift = bu_rect_tshift(bw), th = BU_RECTS_TILE >> tshift;
            const uint64_t tpr = ((uint64_t)bw + (1u << tshift) - 1) >> tshift;  // 1 .. BU_RECTS_MAX_TILES
            const uint64_t band_rows = BU_RECTS_MAX_TILES / tpr;                   // tile rows of the band one launch may hold, >= 1
            for (uint64_t r0 = 0; r0 < j.h;) {                                     // r0: the row band's first block row inside the rectangle
                const uint64_t rows_left = (j.h - r0 + th - 1) / th, rows = rows_left < band_rows ? rows_left : band_rows;
                const uint64_t tiles = rows * tpr;
                if (out.empty() || out.back().k == BU_RECT_JOBS || out.back().n_tiles + tiles > BU_RECTS_MAX_TILES) {
                    if (!out.empty()) close();
                    out.emplace_back();
                }
                BuRectsLaunch& l = out.back();
                const uint64_t h = rows * th < j.h - r0 ? rows * th : j.h - r0;
                const uint64_t first = ((uint64_t)j.y0 + r0) * j.in_bpr + j.x0 + c0;
                l.table.job[l.k] = BuRectDesc{j.in + first * 16u, j.out + r0 * rpb * j.pitch + c0 * rb, j.pitch, j.index_base + first, j.in_bpr, bw, (uint32_t)h, (uint32_t)tpr};
                l.table.first_tile[l.k] = (uint32_t)l.n_tiles;
                l.job_of[l.k] = ji;
                l.k++;
                l.n_tiles += (size_t)tiles;
                r0 += h;
            }
            c0 += bw;
        }
    }
    if (!out.empty()) close();
}

// The grid of a rectangle launch under the resolved `policy` (BU_POLICY_*, not AUTO).  The kernel is the multi-run launch's persistent shape (512 threads, two blocks
// each, the next tile's loads in flight) for every target, on the grid that shape gets there (bu_plan_multi_kernel): min(tiles, per-CU cap x CUs) -- four workgroups
// per CU for BC7 / ASTC, two for the others, halved under the shared policy.  No tile tickets.
inline bool bu_rects_needs_policy(const BuRectsLaunch& l, unsigned cu_count) { return l.n_tiles > (size_t)cu_count; }
inline void bu_plan_rects_grid(int kernel_target, int policy, unsigned cu_count, BuRectsLaunch& l)
{
    const int target = bu_shape_target(kernel_target);
    const bool half = policy == BU_POLICY_SHARED || policy == BU_POLICY_SHARED_FEW;
    const size_t cap = (size_t)cu_count * ((target == BU_TGT_BC7 || target == BU_TGT_ASTC) ? (half ? 2 : 4) : (half ? 1 : 2));
    l.grid = (unsigned)(l.n_tiles < cap ? l.n_tiles : cap);
}
