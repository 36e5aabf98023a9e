// The launcher of one UASTC slice (bu_launch_uastc: the plan of bu_launch_plan.hpp, launched) with the kernel tables it indexes, the host-pointer
// driver shared by the slice-level UASTC entry points (bu_uastc_host, a staged call of bu_staged_call.hpp) and the per-block API's host side.
// Part of the single translation unit bu_hip.hip (included there behind bu_context.hpp and bu_staged_call.hpp; not a stand-alone header).
#pragma once

namespace {

// the kernels a plan names (bu_launch_plan.hpp): BU_TGT_* indexes the plain ones, BU_SORTED_KERNELS[i] is bu_sorted_kernels[i], the multi-run
// kernel BU_MULTI_* of target T is bu_multi_kernels[T][BU_MULTI_*]
static_assert(BU_TARGET_ASTC == BU_TGT_ASTC && BU_TARGET_BC7 == BU_TGT_BC7 && BU_TARGET_ETC1 == BU_TGT_ETC1 && BU_TARGET_ETC2 == BU_TGT_ETC2 &&
              BU_TARGET_RGBA32 == BU_TGT_RGBA && BU_TARGET_BC4_R == BU_TGT_BC4 && BU_TARGET_BC5_RG == BU_TGT_BC5 && BU_TARGET_EAC_R11 == BU_TGT_R11 &&
                  BU_TARGET_EAC_RG11 == BU_TGT_RG11 && BU_TARGET_BC1_RGB == BU_TGT_BC1 && BU_TARGET_BC3_RGBA == BU_TGT_BC3,
              "the launchers index kernels by bu_target");
constexpr unsigned BU_N_TARGETS = BU_TGT_BC3 + 1;  // (entries 5 and 10 of the tables are empty: they name no target, bu_target_block_bytes() == 0)
using BuPlainFn = decltype(&bu_uastc_kernel<BU_TGT_ASTC>);
const BuPlainFn bu_plain_kernels[BU_N_TARGETS] = {bu_uastc_kernel<BU_TGT_ASTC>, bu_uastc_kernel<BU_TGT_BC7>, bu_uastc_kernel<BU_TGT_ETC1>, bu_uastc_kernel<BU_TGT_ETC2>,
                                                  bu_uastc_kernel<BU_TGT_RGBA>, nullptr, bu_uastc_kernel<BU_TGT_BC4>, bu_uastc_kernel<BU_TGT_BC5>, bu_uastc_kernel<BU_TGT_R11>,
                                                  bu_uastc_kernel<BU_TGT_RG11>, nullptr, bu_uastc_kernel<BU_TGT_BC1>, bu_uastc_kernel<BU_TGT_BC3>};
using BuSortedFn = decltype(&bu_uastc_sorted_kernel<BU_TGT_BC7, 1024, 1, 1, false, BU_LAYOUT_STRIP>);
template <size_t... I>
constexpr std::array<BuSortedFn, sizeof...(I)> bu_sorted_fns(std::index_sequence<I...>)
{
    constexpr const BuSortedKey* K = BU_SORTED_KERNELS;
    return {bu_uastc_sorted_kernel<K[I].target, K[I].wgs, K[I].bpt, K[I].minw, K[I].prefetch, K[I].rect ? BU_LAYOUT_RECT : BU_LAYOUT_STRIP>...};
}
const std::array<BuSortedFn, std::size(BU_SORTED_KERNELS)> bu_sorted_kernels = bu_sorted_fns(std::make_index_sequence<std::size(BU_SORTED_KERNELS)>());
using BuMultiFn = decltype(&bu_uastc_multi_kernel<BU_TGT_BC7, 1024, 1>);
template <int T>
std::array<BuMultiFn, 4> bu_multi_fns()  // indexed by BU_MULTI_*; nullptr where T has no such kernel
{
    BuMultiFn etc_2048 = nullptr, whole = nullptr;
    if constexpr (bu_etc_family(T)) etc_2048 = bu_uastc_multi_kernel<T, 512, 4>;
    if constexpr (T == BU_TGT_BC7 || T == BU_TGT_ASTC) whole = bu_uastc_multi_kernel<T, 256, 4, true, true>;
    return {etc_2048, bu_uastc_multi_kernel<T, 1024, 1>, whole, bu_uastc_multi_kernel<T, 512, 2, true>};
}
const std::array<BuMultiFn, 4> bu_multi_kernels[BU_N_TARGETS] = {bu_multi_fns<BU_TGT_ASTC>(), bu_multi_fns<BU_TGT_BC7>(), bu_multi_fns<BU_TGT_ETC1>(),
                                                                 bu_multi_fns<BU_TGT_ETC2>(), bu_multi_fns<BU_TGT_RGBA>(), {}, bu_multi_fns<BU_TGT_BC4>(),
                                                                 bu_multi_fns<BU_TGT_BC5>(), bu_multi_fns<BU_TGT_R11>(), bu_multi_fns<BU_TGT_RG11>(), {},
                                                                 bu_multi_fns<BU_TGT_BC1>(), bu_multi_fns<BU_TGT_BC3>()};

// the rectangle kernels (bu_uastc_transcode_rects_device): one per target
using BuRectsFn = decltype(&bu_uastc_rects_kernel<BU_TGT_BC7>);
const BuRectsFn bu_rects_kernels[BU_N_TARGETS] = {bu_uastc_rects_kernel<BU_TGT_ASTC>, bu_uastc_rects_kernel<BU_TGT_BC7>, bu_uastc_rects_kernel<BU_TGT_ETC1>,
                                                  bu_uastc_rects_kernel<BU_TGT_ETC2>, bu_uastc_rects_kernel<BU_TGT_RGBA>, nullptr, bu_uastc_rects_kernel<BU_TGT_BC4>,
                                                  bu_uastc_rects_kernel<BU_TGT_BC5>, bu_uastc_rects_kernel<BU_TGT_R11>, bu_uastc_rects_kernel<BU_TGT_RG11>, nullptr,
                                                  bu_uastc_rects_kernel<BU_TGT_BC1>, bu_uastc_rects_kernel<BU_TGT_BC3>};

// One slice: resolve the policy, plan (bu_plan_slice), claim tile tickets where the plan asks for them, launch.
// policy = BU_POLICY_* of this launch, or -1 for the context's (bu_context_set_launch_policy; BU_POLICY_AUTO there is resolved per launch by
// bu_auto_policy): only the device-pointer slice entry points pass -1 -- the host-pointer and whole-file entry points issue their launches one
// after another on one stream, for which the exclusive shapes are the right ones whatever the context says.
bu_status bu_launch_uastc(bu_context* ctx, bu_target target, const void* d_in, size_t n_blocks, void* d_out, size_t bpr,
                          uint64_t base, uint64_t* d_status, hipStream_t stream, unsigned grid_cap = 0, int policy = BU_POLICY_EXCLUSIVE)
{
    if (n_blocks == 0) return BU_OK;
    if (bu_target_block_bytes(target) == 0) return BU_ERR_ARGUMENT;  // (also the empty entries 5 and 10 of the kernel tables)
    const unsigned cu_count = (unsigned)ctx->cu_count;
    if (policy < 0) policy = ctx->launch_policy.load(std::memory_order_relaxed);
    const bool big = bu_slice_needs_policy(n_blocks, grid_cap, cu_count);
    if (policy == BU_POLICY_AUTO) policy = big ? bu_auto_policy(ctx, stream) : (int)BU_POLICY_EXCLUSIVE;
    else if (big) bu_note_big_enqueue(ctx, stream);
    std::vector<BuSliceLaunch> plan;
    bu_plan_slice(target, n_blocks, bpr, grid_cap, policy, cu_count, plan);
    const uint4* in = static_cast<const uint4*>(d_in);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(d_status);
    const size_t obytes = bu_target_block_bytes(target);
    for (const BuSliceLaunch& l : plan) {
        void* out = static_cast<uint8_t*>(d_out) + l.offset * obytes;  // RGBA32: the plan cuts on whole rows
        if (l.kernel < 0) {
            hipLaunchKernelGGL(bu_plain_kernels[target], dim3(l.grid), dim3(l.block), 0, stream, in + l.offset, out, l.n, (unsigned)l.bpr, base + l.offset, st,
                               ctx->d_tables);
        } else {
            unsigned* const ticket = l.wants_ticket ? bu_ticket_for(ctx, stream) : nullptr;
            hipLaunchKernelGGL(bu_sorted_kernels[l.kernel], dim3(l.grid), dim3(l.block), 0, stream, in + l.offset, out, (unsigned)l.n, (unsigned)l.bpr,
                               (unsigned long long)(base + l.offset), st, ctx->d_tables, l.cus, BU_SORTED_KERNELS[l.kernel].rect ? l.rect_magic : l.tile_rt, ticket);
        }
        BU_HIP(ctx, hipGetLastError());
    }
    return BU_OK;
}

// host-pointer UASTC driver shared by transcode / decode_to_rgba / the per-block API
bu_status bu_uastc_host(bu_context* ctx, bu_target target, const uint8_t* in, size_t in_bytes, size_t bpr, uint8_t* out,
                        size_t out_bytes, uint64_t* first_bad)
{
    if (!ctx || (!in && in_bytes) || !out) return BU_ERR_ARGUMENT;
    const size_t bb = bu_target_block_bytes(target);
    if (bb == 0) return BU_ERR_ARGUMENT;
    if (in_bytes % 16 != 0) return BU_ERR_LENGTH;  // uastc.rs:54-59
    const size_t n = in_bytes / 16;
    if (out_bytes < n * bb) return BU_ERR_OUTPUT_SIZE;
    if (target == BU_TARGET_RGBA32 && bpr == 0) return BU_ERR_ARGUMENT;
    if (n == 0) return BU_OK;
    BuStagedCall call(ctx, 1);
    bu_status st;
    const void* din = nullptr;
    void* dout = nullptr;
    // RGBA32 with a ragged last block row stores whole image rows, past the 64*n bytes the caller sized: that one is never mapped, and staged in whole rows
    // (no public entry point hands one in today: bu_uastc_decode_to_rgba refuses it)
    const bool ragged = target == BU_TARGET_RGBA32 && n % bpr != 0;
    // (the output first: both reservations are made before the upload is queued)
    if ((st = call.begin()) || (st = call.output(out, ragged ? ((n + bpr - 1) / bpr) * bpr * 64 : n * bb, n * bb, !ragged, 16, &dout)) ||
        (st = call.input(in, in_bytes, true, 16, &din)))
        return st;
    // With a side mapped, a small persistent grid walks the tiles with prefetch, so tile k's posted writes travel upstream while tile k+1's
    // reads come down (PCIe is full duplex): 0.45 ms per 4096^2 atlas with both sides mapped, against 0.69 ms for upload + kernel + download.
    if ((st = call.status_reset()) ||
        (st = bu_launch_uastc(ctx, target, din, n, dout, bpr, 0, call.d_status, ctx->stream, (call.in_mapped || call.out_mapped) ? BU_ZEROCOPY_GRID : 0)) ||
        (st = call.finish()))
        return st;
    return call.status(first_bad);
}

// ---- the per-block API's host side (bu_capi_slice.hpp): the product's block code compiled for the host, over a host copy of the tables
const BuTablesAll& bu_host_tables()
{
    static const BuTablesAll* const tables = [] {
        BuTablesAll* t = new BuTablesAll();
        bu_build_tables(t);
        return t;
    }();
    return *tables;
}

template <int TARGET>
bu_status bu_block_on_host(const uint8_t in[16], void* out)
{
    const BuTables& T = bu_host_tables().t;
    BuBlk b;
    memcpy(b.w, in, 16);
    constexpr int NO = TARGET == BU_TGT_RGBA ? 16 : (TARGET == BU_TGT_ETC1 ? 2 : 4);
    uint32_t o[16] = {0};  // a failing block leaves its zeros (every path checks before it writes), as the kernels' result slots do
    const int st = bu_block_any<TARGET>(T, T.mode_lut[b.w[0] & 127u], b, o);
    memcpy(out, o, NO * sizeof(uint32_t));
    return st == BU_ST_OK ? BU_OK : (st == BU_ST_BAD_PATTERN ? BU_ERR_INVALID_PATTERN : BU_ERR_INVALID_MODE);
}

}  // namespace
