// TEST-ONLY host build of the kernels' per-block code (the same headers the HIP kernels include,
// compiled as plain C++).  It lets the CPU test-suite compare the exact device logic with the
// oracle on millions of blocks in a container that has no GPU.  It is never part of the product
// library and nothing under basisu_rs_amd/ loads it.
#include "bu_uastc_dispatch.hpp"
#include "bu_batch_plan.hpp"
#include "bu_launch_plan.hpp"

static BuTablesAll g_tables;
static bool g_init = false;
static const BuTables& tables()
{
    if (!g_init) {
        bu_build_tables(&g_tables);
        g_init = true;
    }
    return g_tables.t;
}

extern "C" {
// returns 0 ok / 1 bad mode / 2 bad pattern; out sized 16/16/8/16/64 bytes
int bu_emul_block(int target, const uint8_t* in, uint8_t* out)
{
    const BuTables& T = tables();
    BuBlk b;
    memcpy(b.w, in, 16);
    const uint32_t mode = T.mode_lut[b.w[0] & 127u];
    uint32_t o[16] = {0};
    int st;
    switch (target) {
    case BU_TGT_ASTC: st = bu_block_any<BU_TGT_ASTC>(T, mode, b, o); break;
    case BU_TGT_BC7: st = bu_block_any<BU_TGT_BC7>(T, mode, b, o); break;
    case BU_TGT_ETC1: st = bu_block_any<BU_TGT_ETC1>(T, mode, b, o); break;
    case BU_TGT_ETC2: st = bu_block_any<BU_TGT_ETC2>(T, mode, b, o); break;
    default: st = bu_block_any<BU_TGT_RGBA>(T, mode, b, o); break;
    }
    const int n = target == BU_TGT_ETC1 ? 8 : (target == BU_TGT_RGBA ? 64 : 16);
    memcpy(out, o, n);
    return st;
}
// block-linear batch (RGBA = 64 bytes per block); stops at nothing, statuses in st[]
void bu_emul_batch(int target, const uint8_t* in, size_t n_blocks, uint8_t* out, uint8_t* st)
{
    const size_t obs = target == BU_TGT_ETC1 ? 8 : (target == BU_TGT_RGBA ? 64 : 16);
    for (size_t i = 0; i < n_blocks; i++) st[i] = (uint8_t)bu_emul_block(target, in + 16 * i, out + obs * i);
}
size_t bu_emul_tables_size(void) { return sizeof(BuTablesAll); }
// what the mode-sorted kernel of `target` sorts by (tests/sort_cases.py): its row of BU_COST_ORDER (cost_order[k] = the mode of run k; 19 = the invalid
// mode codes) and of key_lut (key_lut[c] = the run of a block whose first seven bits are c).  Returns the row's number.
int bu_emul_sort_tables(int target, uint8_t* cost_order, uint8_t* key_lut)
{
    const int row = bu_cost_row(target);
    memcpy(cost_order, BU_COST_ORDER[row], 20);
    memcpy(key_lut, tables().key_lut[row], 128);
    return row;
}
// the launch plan of bu_uastc_transcode_batch_in_flight for a slice table given as ADDRESSES (nothing is dereferenced): rows of
// (launch, in, out, n_blocks, index base), one per run or piece, in launch order; returns the number of rows (or the number needed
// if `cap` is too small) and the number of launches in *out_launches
size_t bu_emul_plan_in_flight(size_t n_slices, const uint64_t* in_addr, const size_t* n_blocks, const uint64_t* out_addr, size_t block_bytes,
                              const uint64_t* index_base, int n_streams, size_t blocks_per_row, size_t max_runs, size_t group_blocks, uint64_t* rows,
                              size_t cap, size_t* out_launches)
{
    std::vector<const void*> in(n_slices);
    std::vector<void*> out(n_slices);
    for (size_t i = 0; i < n_slices; i++) {
        in[i] = reinterpret_cast<const void*>(in_addr[i]);
        out[i] = reinterpret_cast<void*>(out_addr[i]);
    }
    std::vector<BuRun> runs, pieces;
    bu_merge_runs(n_slices, in.data(), n_blocks, out.data(), block_bytes, index_base, runs);
    std::vector<BuLaunchGroup> groups;
    bu_plan_in_flight(runs, n_streams, blocks_per_row, block_bytes, max_runs, group_blocks, groups, pieces);
    size_t n = 0;
    for (size_t j = 0; j < groups.size(); j++)
        for (size_t k = 0; k < groups[j].count; k++, n++) {
            const size_t idx = groups[j].first + k;
            const BuRun& r = idx >= runs.size() ? pieces[idx - runs.size()] : runs[idx];
            if (n < cap) {
                rows[5 * n + 0] = j;
                rows[5 * n + 1] = reinterpret_cast<uint64_t>(r.in);
                rows[5 * n + 2] = reinterpret_cast<uint64_t>(r.out);
                rows[5 * n + 3] = r.n;
                rows[5 * n + 4] = r.base;
            }
        }
    if (out_launches) *out_launches = groups.size();
    return n;
}
// the launches of bu_launch_uastc for one slice (bu_plan_slice): BU_POLICY_AUTO stands for `auto_result` where the launcher would ask bu_auto_policy.
// Rows of 15: offset, n, kernel (-1: the one-lane-per-block kernel), its WGS, BPT, MINW, PREFETCH, RECT, grid, block, tile_rt, rect_magic, cus, bpr,
// wants_ticket; returns the number of launches (or the number needed if `cap` is too small), *needs_policy = bu_slice_needs_policy
size_t bu_emul_launch_plan(int target, size_t n_blocks, size_t bpr, unsigned grid_cap, int policy, int auto_result, unsigned cu_count, int64_t* rows, size_t cap,
                           int* needs_policy)
{
    *needs_policy = bu_slice_needs_policy(n_blocks, grid_cap, cu_count);
    if (policy == BU_POLICY_AUTO) policy = *needs_policy ? auto_result : (int)BU_POLICY_EXCLUSIVE;
    std::vector<BuSliceLaunch> plan;
    bu_plan_slice(target, n_blocks, bpr, grid_cap, policy, cu_count, plan);
    for (size_t i = 0; i < plan.size() && i < cap; i++) {
        const BuSliceLaunch& l = plan[i];
        const BuSortedKey k = l.kernel < 0 ? BuSortedKey{target, 0, 0, 0, false, false} : BU_SORTED_KERNELS[l.kernel];
        const int64_t r[15] = {(int64_t)l.offset, (int64_t)l.n, l.kernel, k.wgs, k.bpt, k.minw, k.prefetch, k.rect, l.grid, l.block, l.tile_rt, l.rect_magic, l.cus,
                               (int64_t)l.bpr, l.wants_ticket};
        memcpy(rows + 15 * i, r, sizeof(r));
    }
    return plan.size();
}
// the launches of bu_launch_runs (bu_plan_runs, then bu_plan_multi_kernel under `policy`, AUTO as above) for runs given as ADDRESSES.  Rows of 10 per launch:
// plain_run (-1: multi-run launch), k, n_tiles, tile, needs_policy, kernel (BU_MULTI_*), grid, block, wants_ticket, index of its first entry; entries
// rows of 5: run, offset, n, vshift, first_tile.  Returns the number of launches (0 if a table is too small).
size_t bu_emul_runs_plan(int target, size_t n_runs, const uint64_t* in_addr, const uint64_t* out_addr, const size_t* n_blocks, const uint64_t* base, size_t bpr,
                         int policy, int auto_result, unsigned cu_count, int64_t* rows, size_t cap, int64_t* entries, size_t entries_cap)
{
    std::vector<BuRun> runs;
    for (size_t i = 0; i < n_runs; i++)
        runs.push_back(BuRun{reinterpret_cast<const uint8_t*>(in_addr[i]), reinterpret_cast<uint8_t*>(out_addr[i]), n_blocks[i], base[i]});
    std::vector<BuRunsLaunch> plan;
    bu_plan_runs(target, runs.data(), n_runs, bpr, cu_count, plan);
    size_t e = 0;
    if (plan.size() > cap) return 0;
    for (size_t j = 0; j < plan.size(); j++) {
        BuRunsLaunch& l = plan[j];
        if (l.plain_run == SIZE_MAX) bu_plan_multi_kernel(target, policy != BU_POLICY_AUTO ? policy : l.needs_policy ? auto_result : (int)BU_POLICY_EXCLUSIVE, cu_count, l);
        const bool plain = l.plain_run != SIZE_MAX;
        const int64_t r[10] = {plain ? (int64_t)l.plain_run : -1, (int64_t)l.k, (int64_t)l.n_tiles, l.tile, l.needs_policy, plain ? -1 : l.kernel, l.grid, l.block, l.wants_ticket, (int64_t)e};
        memcpy(rows + 10 * j, r, sizeof(r));
        if (e + l.k > entries_cap) return 0;
        for (size_t i = 0; i < l.k; i++, e++) {
            const BuRunEntry& x = l.entries[i];
            const int64_t er[5] = {(int64_t)x.run, (int64_t)x.offset, (int64_t)x.n, x.vshift, x.first_tile};
            memcpy(entries + 5 * e, er, sizeof(er));
        }
    }
    return plan.size();
}
}
