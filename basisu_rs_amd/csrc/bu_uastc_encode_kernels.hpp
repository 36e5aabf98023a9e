// The UASTC encode kernels: an RGBA8 image -> UASTC blocks (bu_rgba_encode_uastc_device).  The per-block code -- class, fit,
// hints, bytes -- is bu_uastc_encode.hpp's, which the CPU tests compile for the host; this header holds what only the device has: the loads, the
// quantiser tables' LDS image and the block stores.  Two launches on the same stream, the geometry of bu_encode_kernel in both (one lane per block
// and step, grid-stride on bu_grid_for):
//   bu_uastc_encode_kernel        class, fit of the candidate modes, etc2tm, mode 8's ETC1 fields -> the block, its other ETC1 fields 0
//   bu_uastc_encode_hints_kernel  re-reads the image and the block, unpacks the block, searches flip / diff / tables / bias and completes the
//                                 block's first word in place (mode 8 blocks are left alone: nothing is stored for them)
//   loads   base and pitch multiples of 16 (uniform over the launch) and the block wholly inside the image: four 16-byte bu_ld_stream loads;
//           edge blocks, and every block of an unaligned image: sixteen clamped 4-byte nontemporal loads (bu_enc_gather)
//   stores  one 16-byte bu_st_stream per lane: 1 KiB contiguous per wave
//   tables  every workgroup of the first kernel builds BuEncQuant (768 bytes) in LDS from BuTables::deq, three entries per lane, while its first
//           loads are in flight; all other tables are read from device memory (a few KiB, resident in the caches)
// The loader (BuEncImage) restates bu_encode_kernel's, kept apart so that the six kernels of section 4.10 stay byte-identical.
// (Included by bu_hip.hip after bu_kernels.hpp: bu_ld_stream, bu_st_stream.)
#pragma once

namespace {

// which block a linear index is, and its 16 texels
struct BuEncImage {
    const uint8_t* in;
    size_t width, height, in_pitch;
    unsigned nbx;
    bool fast, small;
    __device__ __forceinline__ BuEncImage(const uint8_t* in_, size_t w, size_t h, size_t pitch, unsigned nbx_, size_t n_blocks)
        : in(in_), width(w), height(h), in_pitch(pitch), nbx(nbx_), fast(((reinterpret_cast<uintptr_t>(in_) | pitch) & 15u) == 0),
          small(n_blocks <= 0xFFFFFFFFull)  // block row and column by a 32-bit division
    {
    }
    __device__ __forceinline__ void where(size_t i, size_t& bx, size_t& by) const
    {
        if (small) {
            const uint32_t y = (uint32_t)i / nbx;
            by = y, bx = (uint32_t)i - y * nbx;
        } else {
            by = i / nbx, bx = i - by * nbx;
        }
    }
    __device__ __forceinline__ void load(size_t i, uint32_t (&px)[16]) const
    {
        size_t bx, by;
        where(i, bx, by);
        if (fast && bu_enc_block_inside(width, height, bx, by)) {
            const uint8_t* src = in + 4 * by * in_pitch + 16 * bx;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint4 v = bu_ld_stream(reinterpret_cast<const uint4*>(src + (size_t)r * in_pitch));
                px[4 * r] = v.x, px[4 * r + 1] = v.y, px[4 * r + 2] = v.z, px[4 * r + 3] = v.w;
            }
        } else {
            const uint8_t* base = in;
            bu_enc_gather(width, height, in_pitch, bx, by, [base](size_t off) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(base + off)); }, px);
        }
    }
};

__global__ __launch_bounds__(BU_WG) void bu_uastc_encode_kernel(const uint8_t* __restrict__ in, size_t width, size_t height, size_t in_pitch, uint8_t* __restrict__ out,
                                                                unsigned nbx, size_t n_blocks, size_t out_pitch, const BuTablesAll* __restrict__ tables)
{
    __shared__ BuEncQuant s_quant;
    const size_t stride = (size_t)gridDim.x * BU_WG, first = (size_t)blockIdx.x * BU_WG + threadIdx.x;
    const BuEncImage img(in, width, height, in_pitch, nbx, n_blocks);
    uint32_t cur[16];
#pragma unroll
    for (int k = 0; k < 16; k++) cur[k] = 0;
    if (first < n_blocks) img.load(first, cur);  // in flight while the quantiser tables are built
    const BuTables& T = tables->t;
    for (unsigned i = threadIdx.x; i < BU_ENC_QUANT_ENTRIES; i += BU_WG) bu_enc_quant_entry(T, &s_quant, i);
    __syncthreads();
    for (size_t i = first; i < n_blocks; i += stride) {
        uint32_t o[4];
        bu_uastc_encode_block(T, s_quant, cur, o);
        size_t bx, by;
        img.where(i, bx, by);
        bu_st_stream(reinterpret_cast<uint4*>(out + by * out_pitch + bx * (size_t)16), make_uint4(o[0], o[1], o[2], o[3]));
        if (i + stride < n_blocks) img.load(i + stride, cur);
    }
}

// the same arguments; `out` holds the first kernel's blocks (same stream: they are complete)
__global__ __launch_bounds__(BU_WG) void bu_uastc_encode_hints_kernel(const uint8_t* __restrict__ in, size_t width, size_t height, size_t in_pitch, uint8_t* out,
                                                                      unsigned nbx, size_t n_blocks, size_t out_pitch, const BuTablesAll* __restrict__ tables)
{
    const size_t stride = (size_t)gridDim.x * BU_WG, first = (size_t)blockIdx.x * BU_WG + threadIdx.x;
    const BuEncImage img(in, width, height, in_pitch, nbx, n_blocks);
    const BuTables& T = tables->t;
    for (size_t i = first; i < n_blocks; i += stride) {
        uint32_t px[16];
        img.load(i, px);
        size_t bx, by;
        img.where(i, bx, by);
        uint4* dst = reinterpret_cast<uint4*>(out + by * out_pitch + bx * (size_t)16);
        const uint4 v = *dst;
        uint32_t o[4] = {v.x, v.y, v.z, v.w};
        bu_uastc_encode_hints(T, px, o);
        if (o[0] != v.x) bu_st_stream(dst, make_uint4(o[0], o[1], o[2], o[3]));  // (only the first word can change; all-zero hints: nothing to store)
    }
}

}  // namespace
