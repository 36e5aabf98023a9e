// test-only host build of csrc/bu_etc1s_rect_plan.hpp as it is: the launch plan of bu_etc1s_transcode_rects_device and the address mapping its kernel runs
// (tests/test_etc1s_rect_plan.py builds it twice: as a shared library for the plan, and -- with -DBU_EMUL_ETC1S_RECTS_MAIN -fsanitize=undefined -- as a
// stand-alone program that walks every unit of a job list and writes out every block's load addresses, store address and status index)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bu_uastc_dispatch.hpp"
#include "bu_etc1s_rect_plan.hpp"

// jobs: n x 10 words (idx, aidx, in_bpr, x0, y0, w, h, out, pitch, index_base)
static std::vector<BuEtc1sRectJobIn> jobs_of(const uint64_t* w, size_t n)
{
    std::vector<BuEtc1sRectJobIn> j(n);
    for (size_t i = 0; i < n; i++, w += 10)
        j[i] = BuEtc1sRectJobIn{w[0], w[1], (uint32_t)w[2], (uint32_t)w[3], (uint32_t)w[4], (uint32_t)w[5], (uint32_t)w[6], w[7], w[8], w[9]};
    return j;
}
static BuEtc1sRectDesc desc_of(const uint64_t* e)
{
    return BuEtc1sRectDesc{e[0], e[1], e[2], e[3], e[4], (uint32_t)e[5], (uint32_t)e[6], (uint32_t)e[7], (uint32_t)e[8]};
}

extern "C" {

size_t bu_emul_etc1s_rect_table_bytes() { return sizeof(BuEtc1sRectTable); }  // the kernel argument the job table travels in
size_t bu_emul_etc1s_rect_other_arg_bytes() { return BU_ETC1S_RECTS_OTHER_ARGS; }
size_t bu_emul_etc1s_rect_jobs_per_launch() { return BU_ETC1S_RECT_JOBS; }
uint64_t bu_emul_etc1s_rect_max_units() { return BU_ETC1S_RECTS_MAX_UNITS; }
uint64_t bu_emul_etc1s_rect_max_job_units() { return BU_ETC1S_RECT_MAX_JOB_UNITS; }
uint32_t bu_emul_etc1s_rect_ushift(uint32_t w) { return bu_etc1s_rect_ushift(w); }

int bu_emul_etc1s_rect_job_ok(int target, const uint64_t* job) { return bu_etc1s_rect_job_ok(target, jobs_of(job, 1)[0]) ? 1 : 0; }

// launches: per launch 4 words (entries, units, grid, block); entries: per table entry 11 words (idx, aidx, out, pitch, base, in_bpr, w, h, upr, first_unit,
// job); tails: per launch the AND of the unused first-unit numbers.  Returns the number of launches (when larger than launch_cap, or the entries do not fit
// entry_cap, nothing is complete).
size_t bu_emul_etc1s_rects_plan(size_t n_jobs, const uint64_t* job_words, unsigned cu_count, uint64_t* launches, size_t launch_cap, uint64_t* entries,
                                size_t entry_cap, uint64_t* tails)
{
    const std::vector<BuEtc1sRectJobIn> jobs = jobs_of(job_words, n_jobs);
    std::vector<BuEtc1sRectsLaunch> plan;
    bu_plan_etc1s_rects(jobs.data(), n_jobs, cu_count, plan);
    size_t e = 0;
    for (size_t i = 0; i < plan.size() && i < launch_cap; i++) {
        const BuEtc1sRectsLaunch& l = plan[i];
        launches[4 * i] = l.k, launches[4 * i + 1] = l.n_units, launches[4 * i + 2] = l.grid, launches[4 * i + 3] = l.block;
        for (size_t k = 0; k < l.k && e < entry_cap; k++, e++) {
            const BuEtc1sRectDesc& d = l.table.job[k];
            const uint64_t row[11] = {d.idx, d.aidx, d.out, d.pitch, d.base, d.in_bpr, d.w, d.h, d.upr, l.table.first_unit[k], l.job_of[k]};
            for (int c = 0; c < 11; c++) entries[11 * e + c] = row[c];
        }
        uint32_t tail = 0xFFFFFFFFu;
        for (size_t k = l.k; k < BU_ETC1S_RECT_JOBS; k++) tail &= l.table.first_unit[k];
        tails[i] = tail;
    }
    return plan.size();
}

// the kernel's search over a table's first-unit array (n <= jobs per launch numbers, the rest filled with ~0 as the plan does)
uint32_t bu_emul_etc1s_rect_unit_job(const uint32_t* first_unit, size_t n, uint32_t unit)
{
    uint32_t f[BU_ETC1S_RECT_JOBS];
    for (size_t i = 0; i < BU_ETC1S_RECT_JOBS; i++) f[i] = i < n ? first_unit[i] : 0xFFFFFFFFu;
    return bu_etc1s_rect_unit_job(f, unit);
}

// one unit of one table entry (9 words, as above) as the kernel maps it: per lane l of the 64, has[l], src[l], asrc[l], dst[l], idx[l] (status index), and
// the unit's shape in shape[0..3] = ushift, vc, vr, rows of a full unit
void bu_emul_etc1s_rect_unit(int target, const uint64_t* entry, uint32_t lu, uint8_t* has, uint64_t* src, uint64_t* asrc, uint64_t* dst, uint64_t* idx, uint32_t* shape)
{
    const BuEtc1sRectDesc d = desc_of(entry);
    const uint32_t rb = bu_rect_row_bytes(target), rpb = bu_rect_rows_per_block(target);
    const BuEtc1sRectUnit u = bu_etc1s_rect_unit(d, lu, rb, rpb);
    for (uint32_t l = 0; l < BU_ETC1S_UNIT; l++) {
        has[l] = bu_etc1s_rect_has(u, l);
        src[l] = bu_etc1s_rect_src(u, l);
        asrc[l] = u.aidx ? bu_etc1s_rect_asrc(u, l) : 0;
        dst[l] = bu_etc1s_rect_dst(u, l, rb, rpb);
        idx[l] = u.base + bu_etc1s_rect_idx(u, l);
    }
    shape[0] = u.ushift, shape[1] = u.vc, shape[2] = u.vr, shape[3] = BU_ETC1S_UNIT >> u.ushift;
}

// the same for units lu0 .. lu0 + n of the entry, 64 lanes each, without the shapes
void bu_emul_etc1s_rect_units(int target, const uint64_t* entry, uint32_t lu0, uint32_t n, uint8_t* has, uint64_t* src, uint64_t* asrc, uint64_t* dst, uint64_t* idx)
{
    uint32_t shape[4];
    for (uint32_t i = 0; i < n; i++) bu_emul_etc1s_rect_unit(target, entry, lu0 + i, has + 64 * i, src + 64 * i, asrc + 64 * i, dst + 64 * i, idx + 64 * i, shape);
}

}  // extern "C"

#ifdef BU_EMUL_ETC1S_RECTS_MAIN
// bu_emul_etc1s_rects TARGET JOBS.bin OUT.bin: the plan of the job list (10 words per job), every unit of every launch walked the way a wave walks it; OUT.bin
// gets one record of 6 words per block that a lane holds: launch, job, index address, alpha index address (0: none), store address, status index
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int target = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint64_t> words;
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) words.push_back(w);
    fclose(f);
    const std::vector<BuEtc1sRectJobIn> jobs = jobs_of(words.data(), words.size() / 10);
    for (const BuEtc1sRectJobIn& j : jobs)
        if (!bu_etc1s_rect_job_ok(target, j)) return 3;
    std::vector<BuEtc1sRectsLaunch> plan;
    bu_plan_etc1s_rects(jobs.data(), jobs.size(), 256u, plan);
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    const uint32_t rb = bu_rect_row_bytes(target), rpb = bu_rect_rows_per_block(target);
    for (size_t li = 0; li < plan.size(); li++) {
        const BuEtc1sRectsLaunch& l = plan[li];
        for (uint32_t unit = 0; unit < l.n_units; unit++) {
            const uint32_t r = bu_etc1s_rect_unit_job(l.table.first_unit, unit);
            const BuEtc1sRectUnit u = bu_etc1s_rect_unit(l.table.job[r], unit - l.table.first_unit[r], rb, rpb);
            for (uint32_t lane = 0; lane < BU_ETC1S_UNIT; lane++) {
                if (!bu_etc1s_rect_has(u, lane)) continue;
                const uint64_t rec[6] = {li, l.job_of[r], bu_etc1s_rect_src(u, lane), u.aidx ? bu_etc1s_rect_asrc(u, lane) : 0, bu_etc1s_rect_dst(u, lane, rb, rpb),
                                         u.base + bu_etc1s_rect_idx(u, lane)};
                fwrite(rec, 8, 6, o);
            }
        }
    }
    fclose(o);
    printf("clean %zu launches\n", plan.size());
    return 0;
}
#endif
