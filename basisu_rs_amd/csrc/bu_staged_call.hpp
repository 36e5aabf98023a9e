// The protocol of the blocking host-pointer entry points, once.  Each of them takes host pointers, shares the context's staging buffers
// (d_in, d_out, d_aux) under ctx->lock, enqueues on the context stream and waits: bu_uastc_host (bu_uastc_launch.hpp), bu_etc1s_host
// (bu_capi_slice.hpp), bu_blocks_decode_rgba, bu_rgba_encode_blocks, and the three whole-file drivers of bu_capi_file.hpp.  A driver calls the
// steps below in the order it wants them on the stream -- uploads, status reset, its launches, finish -- and keeps only what is its own.
// What the steps guarantee: a HIP call that fails half-way returns through the drain, which synchronises before the landing area of the
// status words (and whatever the driver declared BEFORE the call object) dies, and before the lock is released.  The drain is armed from
// begin() on, so a reservation that fails synchronises the (idle) context stream too.  Every driver's aux reservation carries BU_AUX_SLACK,
// the slice-level ETC1S calls' included.
// Needs the HIP runtime API and no kernel: tests/host_emul/bu_staged_call_check.cpp runs this text on the CPU against a recording runtime.
// Part of the single translation unit bu_hip.hip (included there behind bu_context.hpp; not a stand-alone header).
#pragma once

extern "C" bu_status bu_status_word_decode(uint64_t word, uint64_t* first_bad_block)
{
    if (word == BU_STATUS_WORD_CLEAR) return BU_OK;
    // a report is (block << 8 | status) with status 1 or 2 (6 for ETC1S; 1 or 17 for the block decoders): anything else was never reset or was overwritten
    const unsigned st = (unsigned)(word & 0xFFu);
    if (st != BU_ERR_INVALID_MODE && st != BU_ERR_INVALID_PATTERN && st != BU_ERR_INDEX_RANGE && st != BU_ERR_UNSUPPORTED) return BU_ERR_ARGUMENT;
    if (first_bad_block) *first_bad_block = word >> 8;
    return static_cast<bu_status>(st);
}

namespace {

struct BuStagedCall {
    // (in this order: the drain runs first, then the landing area dies, then the lock is released)
    bu_context* const ctx;
    std::lock_guard<std::mutex> guard;
    std::vector<uint64_t> words;  // landing area of the status download, one word per image
    BuDrain drain;
    bool in_mapped = false, out_mapped = false;
    BuAuxLayout aux_layout;
    uint64_t* d_status;  // what the launches report to: the context's word, or the region aux() names
    void* out_host = nullptr;  // the staged output's way back (finish)
    const void* out_dev = nullptr;
    size_t out_download = 0;

    BuStagedCall(bu_context* c, size_t n_status) : ctx(c), guard(c->lock), words(n_status, 0), drain(c), d_status(reinterpret_cast<uint64_t*>(c->d_status))
    {
        drain.armed = false;  // nothing is queued before begin()
    }

    bu_status begin()
    {
        BU_HIP(ctx, hipSetDevice(ctx->device));
        drain.armed = true;
        return BU_OK;
    }

    // Page-locked caller buffers (bu_host_alloc, or anything the caller page-locked with the HIP runtime) are visible to the GPU: the kernels
    // read the input and / or write the result straight over PCIe -- no staging copy on that side.  Ordinary pageable memory cannot be mapped
    // and is staged through the context's device buffers.  *dev: the device view (may_map, and it is aligned to `align` bytes), else d_in with
    // `host`'s bytes on their way up.  host == nullptr (dev may be, too) only reserves d_in: the driver uploads in pieces of its own.
    bu_status input(const void* host, size_t bytes, bool may_map, size_t align, const void** dev)
    {
        void* view = nullptr;
        in_mapped = may_map && host && bu_device_view(host, &view) && reinterpret_cast<uintptr_t>(view) % align == 0;
        if (in_mapped) {
            *dev = view;
            return BU_OK;
        }
        const bu_status st = bu_reserve(ctx, &ctx->d_in, &ctx->in_cap, bytes ? bytes : 16);
        if (st) return st;
        if (host) BU_HIP(ctx, hipMemcpyAsync(ctx->d_in, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        if (dev) *dev = ctx->d_in;
        return BU_OK;
    }

    // the same for the result: the device view, else d_out of reserve_bytes, whose first download_bytes finish() brings down
    bu_status output(void* host, size_t reserve_bytes, size_t download_bytes, bool may_map, size_t align, void** dev)
    {
        void* view = nullptr;
        out_mapped = may_map && bu_device_view(host, &view) && reinterpret_cast<uintptr_t>(view) % align == 0;
        if (out_mapped) {
            *dev = view;
            return BU_OK;
        }
        const bu_status st = bu_reserve(ctx, &ctx->d_out, &ctx->out_cap, reserve_bytes ? reserve_bytes : 16);
        if (st) return st;
        *dev = ctx->d_out;
        out_host = host;
        out_dev = ctx->d_out;
        out_download = download_bytes;
        return BU_OK;
    }

    // d_aux for the regions of `l`; status_region >= 0: that region holds the status words
    bu_status aux(const BuAuxLayout& l, int status_region)
    {
        const bu_status st = bu_reserve(ctx, &ctx->d_aux, &ctx->aux_cap, l.total);
        if (st) return st;
        aux_layout = l;
        if (status_region >= 0) d_status = region<uint64_t>((size_t)status_region);
        return BU_OK;
    }
    template <class T>
    T* region(size_t i) const
    {
        return reinterpret_cast<T*>(static_cast<uint8_t*>(ctx->d_aux) + aux_layout.at(i));
    }

    bu_status status_reset()
    {
        BU_HIP(ctx, hipMemsetAsync(d_status, 0xFF, sizeof(uint64_t) * words.size(), ctx->stream));
        return BU_OK;
    }

    // Downloads -- the status words, `extra_bytes` from extra_dev into a landing range of the driver's (declared before this object), the output
    // where it was staged -- one synchronisation, and the drain is disarmed.
    bu_status finish(void* extra_host = nullptr, const void* extra_dev = nullptr, size_t extra_bytes = 0)
    {
        if (!words.empty()) BU_HIP(ctx, hipMemcpyAsync(words.data(), d_status, sizeof(uint64_t) * words.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (extra_bytes) BU_HIP(ctx, hipMemcpyAsync(extra_host, extra_dev, extra_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (out_download) BU_HIP(ctx, hipMemcpyAsync(out_host, out_dev, out_download, hipMemcpyDeviceToHost, ctx->stream));
        BU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        drain.armed = false;
        return BU_OK;
    }

    // after finish(): the first Err in image order ends the whole call, like the `?` in the reference drivers
    bu_status status(uint64_t* first_bad) const
    {
        for (const uint64_t w : words) {
            const bu_status st = bu_status_word_decode(w, first_bad);
            if (st) return st;
        }
        return BU_OK;
    }
};

}  // namespace
