// bu_context (device resources of one context) and the error / drain / reservation helpers of the host side: everything that needs the HIP
// runtime API and no kernel (tests/host_emul/bu_staged_call_check.cpp compiles this text for the host against a recording runtime).
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

// the page-locked index buffer of the streamed ETC1S front door (h_idx), of at least `bytes`
bu_status bu_reserve_h_idx(bu_context* ctx, size_t idx_bytes)
{
    if (idx_bytes > ctx->h_idx_cap) {
        if (ctx->h_idx) BU_HIP(ctx, hipHostFree(ctx->h_idx));
        ctx->h_idx = nullptr;
        ctx->h_idx_cap = 0;
        const size_t cap = idx_bytes < ((size_t)4 << 20) ? ((size_t)4 << 20) : idx_bytes + idx_bytes / 4;
        BU_HIP(ctx, hipHostMalloc(&ctx->h_idx, cap, hipHostMallocDefault));
        ctx->h_idx_cap = cap;
    }
    return BU_OK;
}

// the token buffer of the two-thread slices lives in the context (no memory for it: lex_cap stays 0, the ordinary loop)
void bu_reserve_lex(bu_context* ctx, size_t tok_bytes)
{
    if (tok_bytes > ctx->lex_cap) {
        free(ctx->lex_buf);
        ctx->lex_cap = 0;
        ctx->lex_buf = malloc(tok_bytes + tok_bytes / 4);
        if (ctx->lex_buf) ctx->lex_cap = tok_bytes + tok_bytes / 4;
    }
}

int bu_auto_policy(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: BU_POLICY_AUTO resolved for one launch on `s`
void bu_note_big_enqueue(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: a large launch under an explicit policy goes to `s`
unsigned* bu_ticket_for(bu_context* ctx, hipStream_t s);  // bu_streams.hpp: the tile-ticket pair of an own stream, nullptr for anybody else's

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

}  // namespace

