// extern "C": blocks of the ten block formats -> RGBA8 (include/basisu_hip.h).
// Part of the single translation unit bu_hip.hip (included there; not a stand-alone header).
#pragma once

namespace {

using BuDecodeFn = decltype(&bu_decode_kernel<BU_TGT_BC7>);
const BuDecodeFn bu_decode_kernels[BU_N_TARGETS] = {bu_decode_kernel<BU_TGT_ASTC>, bu_decode_kernel<BU_TGT_BC7>, bu_decode_kernel<BU_TGT_ETC1>, bu_decode_kernel<BU_TGT_ETC2>,
                                                    nullptr, nullptr, bu_decode_kernel<BU_TGT_BC4>, bu_decode_kernel<BU_TGT_BC5>, bu_decode_kernel<BU_TGT_R11>,
                                                    bu_decode_kernel<BU_TGT_RG11>, nullptr, bu_decode_kernel<BU_TGT_BC1>, bu_decode_kernel<BU_TGT_BC3>};

// a format bu_blocks_decode_rgba takes: one of the ten (not RGBA32, not the non-targets 5 and 10, nothing outside the enumeration)
bool bu_decode_format_ok(bu_target format) { return (int)format >= 0 && (unsigned)format < BU_N_TARGETS && bu_decode_kernels[format] != nullptr; }

}  // namespace

extern "C" {

bu_status bu_blocks_decode_rgba_device(bu_context* ctx, bu_target format, const void* d_blocks, size_t n_blocks, void* d_rgba, size_t blocks_per_row,
                                       size_t out_pitch_bytes, uint64_t block_index_base, uint64_t* d_status, void* stream)
{
    if (!ctx || !bu_decode_format_ok(format) || (n_blocks && (!d_blocks || !d_rgba))) return BU_ERR_ARGUMENT;
    if (blocks_per_row == 0 || blocks_per_row > 0xFFFFFFFFull / 16 || n_blocks % blocks_per_row != 0) return BU_ERR_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_blocks) % bu_target_block_bytes(format) || reinterpret_cast<uintptr_t>(d_rgba) % 16) return BU_ERR_ARGUMENT;
    const size_t pitch = out_pitch_bytes ? out_pitch_bytes : 16 * blocks_per_row;
    if (pitch % 16 || pitch < 16 * blocks_per_row) return BU_ERR_ARGUMENT;
    if (n_blocks == 0) return BU_OK;
    hipLaunchKernelGGL(bu_decode_kernels[format], dim3(bu_grid_for(n_blocks, (unsigned)ctx->cu_count)), dim3(BU_WG), 0, static_cast<hipStream_t>(stream), d_blocks,
                       n_blocks, static_cast<uint8_t*>(d_rgba), (unsigned)blocks_per_row, pitch, (unsigned long long)block_index_base,
                       reinterpret_cast<unsigned long long*>(d_status), ctx->d_tables);
    BU_HIP(ctx, hipGetLastError());
    return BU_OK;
}

// A staged call (bu_staged_call.hpp) of one launch: a page-locked buffer is read or written by the kernel directly, pageable memory goes
// through the context's device buffers.
bu_status bu_blocks_decode_rgba(bu_context* ctx, bu_target format, const uint8_t* blocks, size_t blocks_bytes, size_t blocks_per_row, uint8_t* out,
                                size_t out_bytes, uint64_t* first_bad_block)
{
    if (!ctx || !bu_decode_format_ok(format) || (!blocks && blocks_bytes) || !out || blocks_per_row == 0) return BU_ERR_ARGUMENT;
    const size_t bb = bu_target_block_bytes(format);
    if (blocks_bytes % bb != 0) return BU_ERR_LENGTH;
    const size_t n = blocks_bytes / bb;
    if (n % blocks_per_row != 0) return BU_ERR_ARGUMENT;
    if (out_bytes / 64 < n) return BU_ERR_OUTPUT_SIZE;
    if (n == 0) return BU_OK;
    BuStagedCall call(ctx, 1);
    bu_status st;
    const void* d_blocks = nullptr;
    void* d_rgba = nullptr;
    if ((st = call.begin()) || (st = call.output(out, n * 64, n * 64, true, 16, &d_rgba)) || (st = call.input(blocks, blocks_bytes, true, 16, &d_blocks)) ||
        (st = call.status_reset()) ||
        (st = bu_blocks_decode_rgba_device(ctx, format, d_blocks, n, d_rgba, blocks_per_row, 0, 0, call.d_status, ctx->stream)) || (st = call.finish()))
        return st;
    return call.status(first_bad_block);
}

}  // extern "C"
