// Rectangles of ETC1S slices into pitched surfaces (bu_etc1s_transcode_rects_device): the job table the kernel reads, the address mapping of a unit and of a
// lane inside it -- ONE copy, compiled into the kernel (bu_etc1s_rects_kernel, bu_etc1s_kernels.hpp) and into the test-only host build
// (tests/host_emul/bu_emul_etc1s_rects.cpp) -- and the launch plan (bu_plan_etc1s_rects).  No HIP in here: tests/test_etc1s_rect_plan.py checks the plan and the
// mapping without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "bu_rect_plan.hpp"  // bu_rect_row_bytes, bu_rect_rows_per_block; bu_launch_plan.hpp: BU_WG, bu_grid_for

// ---- units ------------------------------------------------------------------------------------------------------------------------
// ETC1S has no mode sort, so the unit of work is the wave: every job is cut into units of BU_ETC1S_UNIT blocks, one lane each, 2^k blocks wide with 2^k the
// smallest power of two not below min(w, 64) (k = 0 .. 6) and BU_ETC1S_UNIT >> k high: a one-block-wide column fills its lanes, a 32 x 32-block page is 16 full
// units.  Units are numbered row by row per job; those at the right and bottom edge are clipped, their missing lanes sit out.
constexpr unsigned BU_ETC1S_UNIT = 64;
constexpr unsigned BU_ETC1S_RECT_JOBS = 64;                           // jobs per launch
constexpr uint64_t BU_ETC1S_RECTS_MAX_UNITS = ((uint64_t)1 << 31) - 1;  // units per launch: the kernel's unit number stays 32-bit, its grid stride cannot wrap it
BU_DEV uint32_t bu_etc1s_rect_ushift(uint32_t w)
{
    uint32_t k = 0;
    while (k < 6u && (1u << k) < w) k++;
    return k;
}
// The most units ONE legal job can have.  Its rules give w <= in_bpr and (y0 + h) * in_bpr <= 2^32, so w * h <= 2^32.
//   w >= 64: units are 64 x 1, ceil(w / 64) * h <= (w / 64 + 1) * h <= (w / 32) * h <= 2^27.
//   2 <= w < 64: 2^k <= 2 (w - 1), so a unit is 64 / 2^k >= 32 / (w - 1) rows high and the job's one column of units holds ceil(h / rows) <= h (w - 1) / 32 + 1
//   <= 2^27 units.   w = 1: 64 rows per unit, ceil(h / 64) <= 2^26.
// A job therefore never passes BU_ETC1S_RECTS_MAX_UNITS on its own and is never cut into bands (bu_plan_rects has to: its tiles x 1024 is the 32-bit quantity);
// a launch is closed in front of a job that would take its unit count past the limit.
constexpr uint64_t BU_ETC1S_RECT_MAX_JOB_UNITS = (uint64_t)1 << 27;
static_assert(BU_ETC1S_RECT_MAX_JOB_UNITS <= BU_ETC1S_RECTS_MAX_UNITS, "one job fits one launch");

// one job as the kernel reads it (bu_etc1s_rect_job with the rectangle's origin folded into the addresses)
struct BuEtc1sRectDesc {
    uint64_t idx;     // address of the index word of the rectangle's block (0, 0): d_idx + 4 * (y0 * in_bpr + x0)
    uint64_t aidx;    // the same of the alpha slice, 0 = none (A = 255)
    uint64_t out;     // address its result goes to
    uint64_t pitch;   // bytes from one block row of the output to the next (RGBA32: from one pixel row to the next)
    uint64_t base;    // status-word index of the rectangle's block (0, 0): index_base + y0 * in_bpr + x0
    uint32_t in_bpr;  // blocks per row of the slice the rectangle is cut from
    uint32_t w, h;    // blocks
    uint32_t upr;     // units per row of units, ceil(w / unit width)
};
struct BuEtc1sRectTable {
    BuEtc1sRectDesc job[BU_ETC1S_RECT_JOBS];
    uint32_t first_unit[BU_ETC1S_RECT_JOBS];  // ascending, first_unit[0] = 0; entries past the last job hold 0xFFFFFFFF
};
// the kernel's other parameters: the unit count, both codebooks with their sizes, the status word and the tables -- 48 bytes with their alignment
constexpr size_t BU_ETC1S_RECTS_OTHER_ARGS = 48;
static_assert(sizeof(BuEtc1sRectDesc) == 56 && sizeof(BuEtc1sRectTable) % 8 == 0 && BU_ETC1S_RECT_JOBS >= 32 &&
                  sizeof(BuEtc1sRectTable) + BU_ETC1S_RECTS_OTHER_ARGS <= 4096,
              "the job table must fit the 4 KiB of kernel arguments beside the other parameters");

// The entry that holds `unit`: the largest r with first_unit[r] <= unit (first_unit[0] = 0: there is one; unused entries are ~0 and unit < 2^31).  On the device
// `unit` is wave-uniform and the array is read through the scalar cache.  Two counts, over the first entry of every group of eight and then over the group:
// two rounds of loads that do not depend on each other, where a binary search is a chain of six, and sixteen values in scalar registers, where a count over
// all 64 takes more registers than a wave has (DESIGN.md section 4.8 has the three measured).
BU_DEV uint32_t bu_etc1s_rect_unit_job(const uint32_t* first_unit, uint32_t unit)
{
    static_assert(BU_ETC1S_RECT_JOBS == 64, "eight groups of eight");
    uint32_t g = 0, n = 0;
    BU_UNROLL
    for (uint32_t i = 1; i < 8; i++) g += first_unit[8 * i] <= unit ? 1u : 0u;
    BU_UNROLL
    for (uint32_t i = 0; i < 8; i++) n += first_unit[8 * g + i] <= unit ? 1u : 0u;
    return 8 * g + n - 1u;  // (n >= 1: the group's first entry is <= unit)
}

// unit `lu` of a job: where its corner block is loaded from and stored to, how much of it lies inside the rectangle
struct BuEtc1sRectUnit {
    uint64_t idx, aidx, out;  // addresses of the unit's block (0, 0); aidx 0 = no alpha slice
    uint64_t pitch, base;
    uint32_t in_bpr, ushift;
    uint32_t vc, vr;          // block columns / rows of the unit inside the rectangle (the rest is clipped)
};
// (row_bytes: bytes one block takes of an output row -- the block size, RGBA32: 16; rows_per_block: output rows a block row takes -- 1, RGBA32: 4)
BU_DEV BuEtc1sRectUnit bu_etc1s_rect_unit(const BuEtc1sRectDesc& j, uint32_t lu, uint32_t row_bytes, uint32_t rows_per_block)
{
    const uint32_t ushift = bu_etc1s_rect_ushift(j.w), uh = BU_ETC1S_UNIT >> ushift;
    const uint32_t uy = lu / j.upr, ux = lu - uy * j.upr;
    const uint32_t c0 = ux << ushift, r0 = uy * uh;
    // r0 * in_bpr + c0 is a block of the rectangle, relative to its origin: below (y0 + h) * in_bpr <= 2^32 (the argument rule), so 32 bits hold it
    const uint32_t first = r0 * j.in_bpr + c0;
    BuEtc1sRectUnit u;
    u.idx = j.idx + (uint64_t)first * 4u;
    u.aidx = j.aidx ? j.aidx + (uint64_t)first * 4u : 0u;
    u.out = j.out + (uint64_t)r0 * rows_per_block * j.pitch + (uint64_t)c0 * row_bytes;
    u.pitch = j.pitch;
    u.base = j.base + first;
    u.in_bpr = j.in_bpr;
    u.ushift = ushift;
    u.vc = j.w - c0 < (1u << ushift) ? j.w - c0 : (1u << ushift);
    u.vr = j.h - r0 < uh ? j.h - r0 : uh;
    return u;
}
// lane l of a unit: its row and column inside the unit, whether the rectangle holds its block, and (only then meaningful) its offsets
BU_DEV uint32_t bu_etc1s_rect_row(const BuEtc1sRectUnit& u, uint32_t l) { return l >> u.ushift; }
BU_DEV uint32_t bu_etc1s_rect_col(const BuEtc1sRectUnit& u, uint32_t l) { return l & ((1u << u.ushift) - 1u); }
BU_DEV bool bu_etc1s_rect_has(const BuEtc1sRectUnit& u, uint32_t l) { return bu_etc1s_rect_col(u, l) < u.vc && bu_etc1s_rect_row(u, l) < u.vr; }
// index words from the unit's corner, in the slice; added to u.base: the block's status index
BU_DEV uint32_t bu_etc1s_rect_idx(const BuEtc1sRectUnit& u, uint32_t l) { return bu_etc1s_rect_row(u, l) * u.in_bpr + bu_etc1s_rect_col(u, l); }
BU_DEV uint64_t bu_etc1s_rect_src(const BuEtc1sRectUnit& u, uint32_t l) { return u.idx + (uint64_t)bu_etc1s_rect_idx(u, l) * 4u; }
BU_DEV uint64_t bu_etc1s_rect_asrc(const BuEtc1sRectUnit& u, uint32_t l) { return u.aidx + (uint64_t)bu_etc1s_rect_idx(u, l) * 4u; }
BU_DEV uint64_t bu_etc1s_rect_dst(const BuEtc1sRectUnit& u, uint32_t l, uint32_t row_bytes, uint32_t rows_per_block)
{
    return u.out + (uint64_t)(bu_etc1s_rect_row(u, l) * rows_per_block) * u.pitch + bu_etc1s_rect_col(u, l) * row_bytes;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// the caller's job (bu_etc1s_rect_job of include/basisu_hip.h, addresses as integers)
struct BuEtc1sRectJobIn {
    uint64_t idx, aidx;
    uint32_t in_bpr, x0, y0, w, h;
    uint64_t out, pitch, index_base;
};
// the targets of the call: ETC1, RGBA32 and the six of bu_etc1s_targets.hpp
constexpr bool bu_etc1s_rects_target_ok(int target)
{
    return target == BU_TGT_ETC1 || target == BU_TGT_RGBA || (target >= BU_TGT_BC4 && target <= BU_TGT_RG11) || target == BU_TGT_BC1 || target == BU_TGT_BC3;
}

// The argument rules of one job (include/basisu_hip.h)
inline bool bu_etc1s_rect_job_ok(int target, const BuEtc1sRectJobIn& j)
{
    if (!bu_etc1s_rects_target_ok(target)) return false;
    const uint32_t rb = bu_rect_row_bytes(target);
    if (!j.idx || !j.out || !j.w || !j.h || !j.in_bpr) return false;
    if (target == BU_TGT_ETC1 && j.aidx) return false;  // ETC1 has no alpha
    if ((uint64_t)j.x0 + j.w > j.in_bpr) return false;
    if ((uint64_t)j.y0 + j.h > ((uint64_t)1 << 32) / j.in_bpr) return false;  // (y0 + h) * in_bpr <= 2^32, without the product: it can pass 2^64
    if (j.idx % 4u || j.aidx % 4u || j.out % rb || j.pitch % rb) return false;
    return j.pitch >= (uint64_t)j.w * rb;
}

// units of a rectangle of w x h blocks
inline uint64_t bu_etc1s_rect_units(uint32_t w, uint32_t h)
{
    const uint32_t ushift = bu_etc1s_rect_ushift(w), uh = BU_ETC1S_UNIT >> ushift;
    return (((uint64_t)w + (1u << ushift) - 1) >> ushift) * (((uint64_t)h + uh - 1) / uh);
}

struct BuEtc1sRectsLaunch {
    BuEtc1sRectTable table;
    size_t k = 0;                            // entries of the table in use
    size_t job_of[BU_ETC1S_RECT_JOBS] = {};  // the job of the call every entry was cut from
    size_t n_units = 0;
    unsigned grid = 0, block = BU_WG;        // four waves per workgroup, a unit each per step
};

// jobs[0 .. n_jobs) (every one passed bu_etc1s_rect_job_ok) as launches of bu_etc1s_rects_kernel<target>: up to BU_ETC1S_RECT_JOBS table entries and
// BU_ETC1S_RECTS_MAX_UNITS units per launch, in order, one entry per job (BU_ETC1S_RECT_MAX_JOB_UNITS: no job needs cutting).  The grid is the one the whole-file
// ETC1S launches take for the same number of units: bu_grid_for over units x 64 blocks.
inline void bu_plan_etc1s_rects(const BuEtc1sRectJobIn* jobs, size_t n_jobs, unsigned cu_count, std::vector<BuEtc1sRectsLaunch>& out)
{
    out.clear();
    auto close = [&] {
        BuEtc1sRectsLaunch& l = out.back();
        for (size_t i = l.k; i < BU_ETC1S_RECT_JOBS; i++) {
            l.table.job[i] = BuEtc1sRectDesc{0, 0, 0, 0, 0, 1u, 1u, 1u, 1u};
            l.table.first_unit[i] = 0xFFFFFFFFu;
        }
        l.grid = bu_grid_for(l.n_units * BU_ETC1S_UNIT, cu_count);
    };
    for (size_t ji = 0; ji < n_jobs; ji++) {
        const BuEtc1sRectJobIn& j = jobs[ji];
        const uint64_t units = bu_etc1s_rect_units(j.w, j.h);
        if (out.empty() || out.back().k == BU_ETC1S_RECT_JOBS || out.back().n_units + units > BU_ETC1S_RECTS_MAX_UNITS) {
            if (!out.empty()) close();
            out.emplace_back();
        }
        BuEtc1sRectsLaunch& l = out.back();
        const uint64_t first = (uint64_t)j.y0 * j.in_bpr + j.x0;
        const uint32_t ushift = bu_etc1s_rect_ushift(j.w);
        l.table.job[l.k] = BuEtc1sRectDesc{j.idx + first * 4u, j.aidx ? j.aidx + first * 4u : 0u, j.out, j.pitch, j.index_base + first, j.in_bpr, j.w, j.h,
                                           (uint32_t)(((uint64_t)j.w + (1u << ushift) - 1) >> ushift)};
        l.table.first_unit[l.k] = (uint32_t)l.n_units;
        l.job_of[l.k] = ji;
        l.k++;
        l.n_units += (size_t)units;
    }
    if (!out.empty()) close();
}
