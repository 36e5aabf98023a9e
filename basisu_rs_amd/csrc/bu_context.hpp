// bu_context (device resources of one context), the error / drain helpers of the host side, the launcher of one slice (bu_launch_uastc:
// the plan of bu_launch_plan.hpp, launched) and the host-pointer driver shared by the slice-level entry points.
// Part of the single translation unit bu_hip.hip (included there; not a stand-alone header).
#pragma once

// ================================================================================================
constexpr int BU_FOREIGN_TICKET_SETS = 32;
struct bu_context {
    int device = -1;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    BuTablesAll* d_tables = nullptr;
    BuCrcTables* d_crc_tables = nullptr;  // bu_crc16_pieces_kernel
    void* d_in = nullptr;
    size_t in_cap = 0;
    void* d_out = nullptr;
    size_t out_cap = 0;
    void* d_aux = nullptr;  // codebooks / alpha indices of the host-pointer ETC1S calls
    size_t aux_cap = 0;
    void* lex_buf = nullptr;  // token buffer of the two-thread slice loop (bu_read_etc1s_streamed): malloc'ed, grows
    size_t lex_cap = 0;
    void* h_idx = nullptr;  // page-locked index buffer of the streamed ETC1S front door: the host decoder writes it, the kernels read it over PCIe
    size_t h_idx_cap = 0;
    unsigned long long* d_status = nullptr;
    unsigned* d_tickets = nullptr;  // tile-ticket sets of the persistent launches (kernel, `ticket`): own streams [0..7], `stream` [8], then the caller's streams in order of first use
    hipStream_t foreign_streams[32] = {};  // (bu_ticket_for, under ticket_lock)
    int n_foreign_streams = 0;
    std::mutex ticket_lock;
    std::atomic<unsigned long long> auto_picks[3] = {{0}, {0}, {0}};  // what BU_LAUNCH_AUTO chose so far: exclusive, one-tile shared, shared (bu_time_auto_policy_counts)
    std::atomic<bool> tickets_off{false};  // bu_time_set_tile_tickets (measurement: the fixed walk beside the ticketed one in one process)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_start[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // per-stream events of bu_time_uastc_launches_streams_window
    hipEvent_t ev_end[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // the context's own streams (bu_streams.hpp): created in groups of four under stream_lock, final once published (readers load without the lock)
    std::atomic<hipStream_t> extra_streams[8] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}, {nullptr}, {nullptr}, {nullptr}, {nullptr}};
    int streams_made = 0;                // 0, 4 or 8 (stream_lock)
    int stream_mode[2] = {0, 0};         // BU_STREAMS_* of each group of four (stream_lock)
    int stream_sharing[2] = {0, 0};      // the creation-time probe over streams 0..3 / 0..7: the largest number of them on one hardware queue (stream_lock)
    hipEvent_t probe_ev0 = nullptr, probe_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // bu_probe_streams_locked (stream_lock)
    std::atomic<long long> last_big_enqueue_ns[8] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}};  // host clock of the last large launch enqueued on each own stream (bu_auto_policy)
    std::atomic<int> launch_policy{2};  // BU_POLICY_*: how much of a CU one large launch of the mode-sorted kernel takes (bu_context_set_launch_policy); default BU_POLICY_AUTO
    // the blocking device-pointer entry points (bu_range_begin): their status word is page-locked host memory
    unsigned long long* h_status = nullptr;   // eight page-locked words, written by the host (reset) and by failing blocks (system-scope atomic min)
    unsigned long long* hd_status = nullptr;  // the same words as the device addresses them
    float win_start_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0}, win_end_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the last streams window: per-stream event times (bu_time_last_window_streams)
    int win_streams = 0;
    float win_enqueue_ms = 0;  // host time the last streams window spent enqueueing its win_enqueued launches (and their events)
    int win_enqueued = 0;
    std::atomic<bool> single_thread_enqueue{false};  // BU_ENQUEUE_THREADS=0 (diagnostic knob, bu_context_create): the pipelined batch call enqueues from the calling thread alone
    std::atomic<int> time_enqueue_threads{0};  // bu_time_set_enqueue_threads: the streams windows enqueue from one host thread per stream
    std::atomic<bool> block_api_on_device{false};  // per-block API: host build of the block code (default) or a 1-block launch
    size_t etc1s_lds_limit = 0;  // what the device reports a workgroup may use, less a margin (bu_context_create)
    // per slot of the ETC1S kernel table (bu_etc1s_slot, bu_capi_slice.hpp: ETC1, RGBA32, BC4, BC5, R11, RG11, BC1, BC3), for the slot's
    // LDS-staged kernel: 0 not asked, 1 refused, else dynamic LDS bytes granted
    std::atomic<size_t> etc1s_lds_state[8] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}};
    std::mutex stream_lock;  // creation of extra_streams (bu_ctx_streams)
    std::mutex lock;  // host-pointer entry points share the staging buffers
    std::mutex err_lock;  // `err` is written by whichever thread fails (device-pointer entry points run without `lock`)
    char err[256] = {0};
};

namespace {

bu_status bu_fail(bu_context* ctx, hipError_t e, const char* what)
{
    if (ctx) {
        std::lock_guard<std::mutex> g(ctx->err_lock);
        snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, hipGetErrorString(e));
    }
    return BU_ERR_HIP;
}
#define BU_HIP(ctx, call)                                       \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return bu_fail(ctx, e_, #call);   \
    } while (0)

// An early error return must not leave asynchronous copies in flight: they target the caller's stack frame (status
// words), vectors about to be freed, or the context's staging buffers the next caller will reuse.  Armed while work is
// queued; the success path disarms it after its own final synchronisation.
struct BuDrain {
    bu_context* ctx;
    bool armed = true;
    explicit BuDrain(bu_context* c) : ctx(c) {}
    ~BuDrain()
    {
        if (!armed || !ctx) return;
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (hipStream_t es : ctx->extra_streams)
            if (es) (void)hipStreamSynchronize(es);
    }
};

enum { BU_STREAMS_NONE = 0, BU_STREAMS_PLAIN = 1, BU_STREAMS_CU_MASK = 2 };
bu_status bu_ctx_streams(bu_context* ctx, int n);  // bu_streams.hpp

bu_status bu_reserve(bu_context* ctx, void** p, size_t* cap, size_t need)
{
    if (need <= *cap) return BU_OK;
    if (*p) BU_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    size_t sz = need < (1u << 20) ? (1u << 20) : need;
    BU_HIP(ctx, hipMalloc(p, sz));
    *cap = sz;
    return BU_OK;
}

int bu_auto_policy(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: BU_POLICY_AUTO resolved for one launch on `s`
void bu_note_big_enqueue(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: a large launch under an explicit policy goes to `s`
unsigned* bu_ticket_for(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: the tile-ticket pair of an own stream, nullptr for anybody else's

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

// device-side address of a page-locked host buffer; false for ordinary (pageable) memory
bool bu_device_view(const void* p, void** dev)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory reports an error on some runtimes: not sticky
        return false;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return false;
    if (reinterpret_cast<uintptr_t>(a.devicePointer) % 16 != 0) return false;  // the kernels move 16-byte vectors
    *dev = a.devicePointer;
    return true;
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
    std::lock_guard<std::mutex> g(ctx->lock);
    BU_HIP(ctx, hipSetDevice(ctx->device));
    bu_status st;
    // Page-locked caller buffers (bu_host_alloc, or anything the caller page-locked with the HIP runtime) are visible to
    // the GPU: the kernels read the slice and / or write the result straight over PCIe -- no staging copy on that side.
    // A small persistent grid walks the tiles with prefetch, so tile k's posted writes travel upstream while tile k+1's
    // reads come down (PCIe is full duplex): 0.45 ms per 4096^2 atlas with both sides mapped, against 0.69 ms for upload +
    // kernel + download.  Ordinary pageable memory cannot be mapped and is staged through the context's device buffers.
    void *zin = nullptr, *zout = nullptr;
    const bool map_in = bu_device_view(in, &zin);
    // RGBA32 with a ragged last block row stores whole image rows, past the 64*n bytes the caller sized: keep that staged
    const bool map_out = !(target == BU_TARGET_RGBA32 && n % bpr != 0) && bu_device_view(out, &zout);
    if (!map_in) {
        st = bu_reserve(ctx, &ctx->d_in, &ctx->in_cap, in_bytes);
        if (st) return st;
    }
    if (!map_out) {
        size_t out_need = n * bb;
        if (target == BU_TARGET_RGBA32) out_need = ((n + bpr - 1) / bpr) * bpr * 64;
        st = bu_reserve(ctx, &ctx->d_out, &ctx->out_cap, out_need);
        if (st) return st;
    }
    const void* din = map_in ? zin : ctx->d_in;
    void* dout = map_out ? zout : ctx->d_out;
    uint64_t word = 0;
    BuDrain drain(ctx);
    if (!map_in) BU_HIP(ctx, hipMemcpyAsync(ctx->d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    BU_HIP(ctx, hipMemsetAsync(ctx->d_status, 0xFF, sizeof(uint64_t), ctx->stream));
    st = bu_launch_uastc(ctx, target, din, n, dout, bpr, 0, reinterpret_cast<uint64_t*>(ctx->d_status), ctx->stream,
                         (map_in || map_out) ? BU_ZEROCOPY_GRID : 0);
    if (st) return st;
    BU_HIP(ctx, hipMemcpyAsync(&word, ctx->d_status, sizeof(word), hipMemcpyDeviceToHost, ctx->stream));
    if (!map_out) BU_HIP(ctx, hipMemcpyAsync(out, ctx->d_out, n * bb, hipMemcpyDeviceToHost, ctx->stream));
    BU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drain.armed = false;
    return bu_status_word_decode(word, first_bad);
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

