// extern "C": an RGBA8 image -> BC4, BC5, EAC R11, EAC RG11, BC1 or BC3 blocks (include/basisu_hip.h), or UASTC blocks (section 4.11).
// Part of the single translation unit bu_hip.hip (included there; not a stand-alone header).
#pragma once

namespace {

// the signature of every encode kernel: bu_encode_kernel<FORMAT>, and the two UASTC encode kernels, which are declared with the same parameter list on
// purpose so that one launcher (bu_encode_launch) serves both entry points
using BuEncodeFn = decltype(&bu_encode_kernel<BU_TGT_BC1>);
static_assert(std::is_same<BuEncodeFn, decltype(&bu_uastc_encode_kernel)>::value && std::is_same<BuEncodeFn, decltype(&bu_uastc_encode_hints_kernel)>::value,
              "the UASTC encode kernels take bu_encode_kernel's arguments");
const BuEncodeFn bu_encode_kernels[BU_N_TARGETS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bu_encode_kernel<BU_TGT_BC4>, bu_encode_kernel<BU_TGT_BC5>,
                                                    bu_encode_kernel<BU_TGT_R11>, bu_encode_kernel<BU_TGT_RG11>, nullptr, bu_encode_kernel<BU_TGT_BC1>, bu_encode_kernel<BU_TGT_BC3>};

// a format bu_rgba_encode_blocks takes: one of the six with an encoder from texels (nothing outside the enumeration)
bool bu_encode_format_ok(bu_target format) { return (int)format >= 0 && (unsigned)format < BU_N_TARGETS && bu_encode_kernels[format] != nullptr; }

// 0 = the tight pitch `tight`; else a multiple of `unit` of at least `tight`.  False for a bad pitch.
bool bu_encode_pitch(size_t given, size_t unit, size_t tight, size_t* pitch)
{
    *pitch = given ? given : tight;
    return *pitch % unit == 0 && *pitch >= tight;
}

// The device form of both encoders behind its format check: geometry, alignment and pitch rules, then one launch of `kernel` (bb = bytes per block)
// and, where given, one of `second` behind it on the same stream with the same arguments.
bu_status bu_encode_launch(bu_context* ctx, BuEncodeFn kernel, BuEncodeFn second, size_t bb, const void* d_rgba, size_t width, size_t height, size_t in_pitch_bytes, void* d_blocks,
                           size_t out_pitch_bytes, void* stream)
{
    const bool empty = width == 0 || height == 0;
    if (!empty && (!d_rgba || !d_blocks)) return BU_ERR_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_rgba) % 4 || reinterpret_cast<uintptr_t>(d_blocks) % bb) return BU_ERR_ARGUMENT;
    const size_t nbx = bu_enc_blocks(width), nby = bu_enc_blocks(height);
    if (nbx > BU_ENC_MAX_NBX) return BU_ERR_ARGUMENT;  // (in front of the pitches: 4 * width and nbx * bb cannot overflow below)
    size_t in_pitch, out_pitch;
    if (!bu_encode_pitch(in_pitch_bytes, 4, 4 * width, &in_pitch) || !bu_encode_pitch(out_pitch_bytes, bb, nbx * bb, &out_pitch)) return BU_ERR_ARGUMENT;
    if (empty) return BU_OK;
    if (nby > ((size_t)1 << 62) / nbx) return BU_ERR_ARGUMENT;  // (no such image exists: the block count stays a size_t)
    const size_t n_blocks = nbx * nby;
    hipLaunchKernelGGL(kernel, dim3(bu_grid_for(n_blocks, (unsigned)ctx->cu_count)), dim3(BU_WG), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_rgba), width, height, in_pitch, static_cast<uint8_t*>(d_blocks), (unsigned)nbx, n_blocks, out_pitch, ctx->d_tables);
    BU_HIP(ctx, hipGetLastError());
    if (second) {
        hipLaunchKernelGGL(second, dim3(bu_grid_for(n_blocks, (unsigned)ctx->cu_count)), dim3(BU_WG), 0, static_cast<hipStream_t>(stream),
                           static_cast<const uint8_t*>(d_rgba), width, height, in_pitch, static_cast<uint8_t*>(d_blocks), (unsigned)nbx, n_blocks, out_pitch, ctx->d_tables);
        BU_HIP(ctx, hipGetLastError());
    }
    return BU_OK;
}

// The host form of both: a staged call (bu_staged_call.hpp) of the device form's launches.  A page-locked buffer is read or written by the kernel directly (where it is
// aligned as the device form asks), pageable memory goes through the context's device buffers.  The image's last row ends at its last pixel.
bu_status bu_encode_staged(bu_context* ctx, BuEncodeFn kernel, BuEncodeFn second, size_t bb, const uint8_t* rgba, size_t width, size_t height, size_t in_pitch_bytes, uint8_t* out,
                           size_t out_bytes)
{
    const bool empty = width == 0 || height == 0;
    if (!empty && (!rgba || !out)) return BU_ERR_ARGUMENT;
    const size_t nbx = bu_enc_blocks(width), nby = bu_enc_blocks(height);
    if (nbx > BU_ENC_MAX_NBX) return BU_ERR_ARGUMENT;
    size_t in_pitch;
    if (!bu_encode_pitch(in_pitch_bytes, 4, 4 * width, &in_pitch)) return BU_ERR_ARGUMENT;
    if (empty) return BU_OK;
    if (nby > ((size_t)1 << 62) / nbx || height > ((size_t)1 << 62) / in_pitch) return BU_ERR_ARGUMENT;
    const size_t in_bytes = (height - 1) * in_pitch + 4 * width, need = nbx * nby * bb;
    if (out_bytes < need) return BU_ERR_OUTPUT_SIZE;
    BuStagedCall call(ctx, 0);  // (an encoder has nothing to refuse: no status word)
    bu_status st;
    const void* d_rgba = nullptr;
    void* d_blocks = nullptr;
    if ((st = call.begin()) || (st = call.output(out, need, need, true, bb, &d_blocks)) || (st = call.input(rgba, in_bytes, true, 4, &d_rgba)) ||
        (st = bu_encode_launch(ctx, kernel, second, bb, d_rgba, width, height, in_pitch, d_blocks, 0, ctx->stream)))
        return st;
    return call.finish();
}

}  // namespace

extern "C" {

bu_status bu_rgba_encode_blocks_device(bu_context* ctx, bu_target format, const void* d_rgba, size_t width, size_t height, size_t in_pitch_bytes, void* d_blocks,
                                       size_t out_pitch_bytes, void* stream)
{
    if (!bu_encode_format_ok(format) || !ctx) return BU_ERR_ARGUMENT;
    return bu_encode_launch(ctx, bu_encode_kernels[format], nullptr, bu_target_block_bytes(format), d_rgba, width, height, in_pitch_bytes, d_blocks, out_pitch_bytes, stream);
}

bu_status bu_rgba_encode_blocks(bu_context* ctx, bu_target format, const uint8_t* rgba, size_t width, size_t height, size_t in_pitch_bytes, uint8_t* out, size_t out_bytes)
{
    if (!bu_encode_format_ok(format) || !ctx) return BU_ERR_ARGUMENT;
    return bu_encode_staged(ctx, bu_encode_kernels[format], nullptr, bu_target_block_bytes(format), rgba, width, height, in_pitch_bytes, out, out_bytes);
}

// RGBA8 -> UASTC: the rules of the two calls above with 16-byte blocks; two launches on the stream
bu_status bu_rgba_encode_uastc_device(bu_context* ctx, const void* d_rgba, size_t width, size_t height, size_t in_pitch_bytes, void* d_blocks, size_t out_pitch_bytes,
                                      void* stream)
{
    if (!ctx) return BU_ERR_ARGUMENT;
    return bu_encode_launch(ctx, bu_uastc_encode_kernel, bu_uastc_encode_hints_kernel, 16, d_rgba, width, height, in_pitch_bytes, d_blocks, out_pitch_bytes, stream);
}

bu_status bu_rgba_encode_uastc(bu_context* ctx, const uint8_t* rgba, size_t width, size_t height, size_t in_pitch_bytes, uint8_t* out, size_t out_bytes)
{
    if (!ctx) return BU_ERR_ARGUMENT;
    return bu_encode_staged(ctx, bu_uastc_encode_kernel, bu_uastc_encode_hints_kernel, 16, rgba, width, height, in_pitch_bytes, out, out_bytes);
}

}  // extern "C"
