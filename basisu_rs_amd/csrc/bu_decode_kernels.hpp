// The block-decode kernels: blocks of one of the ten block formats -> an RGBA8 image (bu_blocks_decode_rgba_device).
// The per-block code is bu_decode_blocks.hpp's, which the CPU tests compile for the host; this header holds what only the device has: loads,
// the tables' LDS copies, the image stores and the status word.  The structure of bu_etc1s_target_kernel<T, false>: one lane per block and step,
// so a wave's lanes hold 64 consecutive blocks and its one load instruction reads 512 B or 1 KiB contiguous; grid-stride with the next step's
// blocks in flight; the four-row image store of the RGBA32 kernels (one 16-byte store per lane and pixel row: 1 KiB contiguous per wave and row
// while the wave sits inside one block row), 64-bit addresses from the pitch.
// (Included by bu_hip.hip after bu_kernels.hpp: bu_report, bu_ld_stream, bu_st_stream.)
#pragma once

namespace {

// the part of BuDecTables FORMAT's decoder reads, [lo, hi) in bytes (multiples of 16); the ETC / EAC decoders read BuTables instead
constexpr unsigned bu_dec_lds_lo(int format) { return format == 0 ? (unsigned)offsetof(BuDecTables, astc_trit) : 0u; }
constexpr unsigned bu_dec_lds_hi(int format) { return format == 0 ? (unsigned)sizeof(BuDecTables) : format == 1 ? (unsigned)offsetof(BuDecTables, astc_trit) : 0u; }
constexpr bool bu_dec_reads_etc(int format) { return format == 2 || format == 3 || format == 8 || format == 9; }
constexpr unsigned BU_DEC_ETC_BYTES = (unsigned)(offsetof(BuTables, eac_magic) - offsetof(BuTables, etc1_mod));  // etc1_mod, eac_mods
static_assert(BU_DEC_ETC_BYTES == 192 && offsetof(BuTables, eac_mods) - offsetof(BuTables, etc1_mod) == 64, "the ETC decoders' LDS image");

template <int FORMAT>
__global__ __launch_bounds__(BU_WG) void bu_decode_kernel(const void* __restrict__ in, size_t n_blocks, uint8_t* __restrict__ out, unsigned bpr, size_t pitch,
                                                          unsigned long long base, unsigned long long* status, const BuTablesAll* __restrict__ tables)
{
    constexpr int W = bu_dec_block_words(FORMAT);
    constexpr unsigned LO = bu_dec_lds_lo(FORMAT), HI = bu_dec_lds_hi(FORMAT);
    __shared__ uint4 s_dec[HI ? HI / 16 : 1];
    __shared__ uint4 s_etc[bu_dec_reads_etc(FORMAT) ? BU_DEC_ETC_BYTES / 16 : 1];
    const size_t stride = (size_t)gridDim.x * BU_WG, first = (size_t)blockIdx.x * BU_WG + threadIdx.x;
    auto load = [&](size_t i, uint32_t (&w)[4]) {
        if constexpr (W == 2) {
            const bu_v2u v = __builtin_nontemporal_load(static_cast<const bu_v2u*>(in) + i);
            w[0] = v.x, w[1] = v.y, w[2] = 0, w[3] = 0;
        } else {
            const uint4 v = bu_ld_stream(static_cast<const uint4*>(in) + i);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        }
    };
    uint32_t cur[4] = {0, 0, 0, 0};
    if (first < n_blocks) load(first, cur);  // in flight while the tables are staged
    if constexpr (HI != 0) {
        const uint4* s = reinterpret_cast<const uint4*>(&tables->dec);
        for (unsigned i = LO / 16 + threadIdx.x; i < HI / 16; i += BU_WG) s_dec[i] = s[i];
    }
    if constexpr (bu_dec_reads_etc(FORMAT)) {
        const uint4* s = reinterpret_cast<const uint4*>(tables->t.etc1_mod);
        if (threadIdx.x < BU_DEC_ETC_BYTES / 16) s_etc[threadIdx.x] = s[threadIdx.x];
    }
    if constexpr (HI != 0 || bu_dec_reads_etc(FORMAT)) __syncthreads();
    const BuDecView V = {reinterpret_cast<const BuDecTables*>(s_dec), reinterpret_cast<const int16_t*>(s_etc), reinterpret_cast<const int8_t*>(s_etc) + 64};
    const bool small = n_blocks <= 0xFFFFFFFFull;  // block row and column by a 32-bit division
    for (size_t i = first; i < n_blocks; i += stride) {
        const size_t in_next = i + stride;
        uint32_t nxt[4] = {0, 0, 0, 0};
        if (in_next < n_blocks) load(in_next, nxt);
        uint32_t px[16];
        const int st = bu_decode_block<FORMAT>(V, cur, px);  // zeros for a failing block
        if (st != BU_DEC_OK) bu_report(status, base + i, st);
        size_t by, bx;
        if (small) {
            const uint32_t y = (uint32_t)i / bpr;
            by = y, bx = (uint32_t)i - y * bpr;
        } else {
            by = i / bpr, bx = i - by * bpr;
        }
        uint8_t* dst = out + 4 * by * pitch + 16 * bx;
#pragma unroll
        for (int r = 0; r < 4; r++) bu_st_stream(reinterpret_cast<uint4*>(dst + (size_t)r * pitch), make_uint4(px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]));
#pragma unroll
        for (int k = 0; k < 4; k++) cur[k] = nxt[k];
    }
}

}  // namespace
