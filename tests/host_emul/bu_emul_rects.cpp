// test-only host build of csrc/bu_rect_plan.hpp as it is: the launch plan of bu_uastc_transcode_rects_device and the address mapping its kernel runs
// (tests/test_rect_plan.py builds it twice: as a shared library for the plan, and -- with -DBU_EMUL_RECTS_MAIN -fsanitize=undefined -- as a stand-alone
// program that walks every tile of a job list and writes out every block's load address, store address and status index)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bu_uastc_dispatch.hpp"
#include "bu_rect_plan.hpp"

// jobs: n x 9 words (in, in_bpr, x0, y0, w, h, out, pitch, index_base)
static std::vector<BuRectJobIn> jobs_of(const uint64_t* w, size_t n)
{
    std::vector<BuRectJobIn> j(n);
    for (size_t i = 0; i < n; i++, w += 9) j[i] = BuRectJobIn{w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3], (uint32_t)w[4], (uint32_t)w[5], w[6], w[7], w[8]};
    return j;
}

extern "C" {

size_t bu_emul_rect_table_bytes() { return sizeof(BuRectTable); }  // the kernel argument the job table travels in
size_t bu_emul_rect_jobs_per_launch() { return BU_RECT_JOBS; }

int bu_emul_rect_job_ok(int target, const uint64_t* job) { return bu_rect_job_ok(target, jobs_of(job, 1)[0]) ? 1 : 0; }

// launches: per launch 4 words (entries, tiles, grid, block); entries: per table entry 10 words (in, out, pitch, base, in_bpr, w, h, tpr, first_tile, job).
// Returns the number of launches (or what it would take, when larger than launch_cap / the entries do not fit entry_cap: nothing is then complete).
size_t bu_emul_rects_plan(int target, size_t n_jobs, const uint64_t* job_words, int policy, unsigned cu_count, uint64_t* launches, size_t launch_cap, uint64_t* entries,
                          size_t entry_cap, uint64_t* tail_first_tiles)
{
    const std::vector<BuRectJobIn> jobs = jobs_of(job_words, n_jobs);
    std::vector<BuRectsLaunch> plan;
    bu_plan_rects(target, jobs.data(), n_jobs, plan);
    size_t e = 0;
    for (size_t i = 0; i < plan.size() && i < launch_cap; i++) {
        BuRectsLaunch& l = plan[i];
        bu_plan_rects_grid(target, policy, cu_count, l);
        launches[4 * i] = l.k, launches[4 * i + 1] = l.n_tiles, launches[4 * i + 2] = l.grid, launches[4 * i + 3] = l.block;
        for (size_t k = 0; k < l.k && e < entry_cap; k++, e++) {
            const BuRectDesc& d = l.table.job[k];
            const uint64_t row[10] = {d.in, d.out, d.pitch, d.base, d.in_bpr, d.w, d.h, d.tpr, l.table.first_tile[k], l.job_of[k]};
            for (int c = 0; c < 10; c++) entries[10 * e + c] = row[c];
        }
        // the unused first-tile numbers of the launch must all be ~0: their AND
        uint32_t tail = 0xFFFFFFFFu;
        for (size_t k = l.k; k < BU_RECT_JOBS; k++) tail &= l.table.first_tile[k];
        tail_first_tiles[i] = tail;
    }
    return plan.size();
}

// one tile of one table entry as the kernel maps it: per lane l of the BU_RECTS_TILE, has[l], src[l], dst[l], idx[l] (status index)
void bu_emul_rect_tile(int target, const uint64_t* entry, uint32_t lt, uint8_t* has, uint64_t* src, uint64_t* dst, uint64_t* idx)
{
    const BuRectDesc d = {entry[0], entry[1], entry[2], entry[3], (uint32_t)entry[4], (uint32_t)entry[5], (uint32_t)entry[6], (uint32_t)entry[7]};
    const BuRectTile t = bu_rect_tile(d, lt, bu_rect_row_bytes(target), bu_rect_rows_per_block(target));
    for (uint32_t l = 0; l < BU_RECTS_TILE; l++) {
        has[l] = bu_rect_has(t, l);
        src[l] = bu_rect_src(t, l);
        dst[l] = bu_rect_dst(t, l, bu_rect_row_bytes(target), bu_rect_rows_per_block(target));
        idx[l] = t.base + bu_rect_idx(t, l);
    }
}

}  // extern "C"

#ifdef BU_EMUL_RECTS_MAIN
// bu_emul_rects TARGET JOBS.bin OUT.bin: the plan of the job list (9 words per job), every tile of every launch walked the way a workgroup walks it; OUT.bin gets
// one record of 5 words per block that a lane holds: launch, job, load address, store address, status index
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
    const std::vector<BuRectJobIn> jobs = jobs_of(words.data(), words.size() / 9);
    for (const BuRectJobIn& j : jobs)
        if (!bu_rect_job_ok(target, j)) return 3;
    std::vector<BuRectsLaunch> plan;
    bu_plan_rects(target, jobs.data(), jobs.size(), plan);
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    const uint32_t rb = bu_rect_row_bytes(target), rpb = bu_rect_rows_per_block(target);
    for (size_t li = 0; li < plan.size(); li++) {
        const BuRectsLaunch& l = plan[li];
        for (uint32_t t = 0; t < l.n_tiles; t++) {
            // the kernel's search: the last entry whose first tile is <= t
            uint32_t cnt = 0;
            for (uint32_t lane = 0; lane < BU_RECT_JOBS; lane++) cnt += l.table.first_tile[lane] <= t;
            const uint32_t r = cnt - 1u;
            const BuRectTile q = bu_rect_tile(l.table.job[r], t - l.table.first_tile[r], rb, rpb);
            for (uint32_t lane = 0; lane < BU_RECTS_TILE; lane++) {
                if (!bu_rect_has(q, lane)) continue;
                const uint64_t rec[5] = {li, l.job_of[r], bu_rect_src(q, lane), bu_rect_dst(q, lane, rb, rpb), q.base + bu_rect_idx(q, lane)};
                fwrite(rec, 8, 5, o);
            }
        }
    }
    fclose(o);
    printf("clean %zu launches\n", plan.size());
    return 0;
}
#endif
