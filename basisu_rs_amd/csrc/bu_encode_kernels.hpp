// The block-encode kernels: an RGBA8 image -> blocks of BC4, BC5, EAC R11, EAC RG11, BC1 or BC3 (bu_rgba_encode_blocks_device).
// The mirror of bu_decode_kernel.  The per-block code -- which pixels are a block's texels, and the encoders -- is bu_encode_blocks.hpp's, which the
// CPU tests compile for the host; this header holds what only the device has: the loads, the EAC tables' LDS copy and the block stores.
// One lane per block and step, so a wave's lanes hold 64 consecutive blocks of a block row and each of a block's four row loads reads 1 KiB
// contiguous per wave while the wave sits inside one block row; grid-stride (bu_grid_for); 64-bit addresses from the pitches, block row and column by a
// 32-bit division below 2^32 blocks.
//   loads   base and pitch multiples of 16 (uniform over the launch) and the block wholly inside the image: four 16-byte bu_ld_stream loads;
//           edge blocks, and every block of an unaligned image: sixteen clamped 4-byte nontemporal loads (bu_enc_gather)
//   stores  one bu_st_stream per lane, 8 or 16 bytes: 512 B or 1 KiB contiguous per wave
//   steps   the next step's loads are issued behind the store.  Keeping them in flight across the encoder instead (the decode kernel's structure) was
//           built and measured for every format and lost (16 more VGPRs, 0.4 to 11 % slower: DESIGN.md section 4.10), so it is not here.
// (Included by bu_hip.hip after bu_kernels.hpp: bu_ld_stream, bu_st_stream.)
#pragma once

namespace {

// R11 / RG11 read eac_mods, eac_magic, (eac_mod_min,) eac_range of BuTables: staged at their offsets, so that the encoders take the LDS image as a BuTables
constexpr unsigned BU_ENC_LDS_LO = (unsigned)offsetof(BuTables, eac_mods), BU_ENC_LDS_HI = (unsigned)offsetof(BuTables, etc1_flags);
static_assert(BU_ENC_LDS_LO % 16 == 0 && BU_ENC_LDS_HI % 16 == 0 && BU_ENC_LDS_HI - BU_ENC_LDS_LO == 224, "the EAC encoders' LDS image, staged in 16-byte pieces");
constexpr bool bu_enc_reads_eac(int format) { return format == BU_TGT_R11 || format == BU_TGT_RG11; }

template <int FORMAT>
__global__ __launch_bounds__(BU_WG) void bu_encode_kernel(const uint8_t* __restrict__ in, size_t width, size_t height, size_t in_pitch, uint8_t* __restrict__ out,
                                                          unsigned nbx, size_t n_blocks, size_t out_pitch, const BuTablesAll* __restrict__ tables)
{
    constexpr int W = bu_enc_block_words(FORMAT);
    constexpr bool EAC = bu_enc_reads_eac(FORMAT);
    __shared__ uint4 s_eac[EAC ? BU_ENC_LDS_HI / 16 : 1];
    const size_t stride = (size_t)gridDim.x * BU_WG, first = (size_t)blockIdx.x * BU_WG + threadIdx.x;
    const bool fast = ((reinterpret_cast<uintptr_t>(in) | in_pitch) & 15u) == 0;
    const bool small = n_blocks <= 0xFFFFFFFFull;  // block row and column by a 32-bit division
    auto where = [&](size_t i, size_t& bx, size_t& by) {
        if (small) {
            const uint32_t y = (uint32_t)i / nbx;
            by = y, bx = (uint32_t)i - y * nbx;
        } else {
            by = i / nbx, bx = i - by * nbx;
        }
    };
    auto load = [&](size_t i, uint32_t (&px)[16]) {
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
            bu_enc_gather(width, height, in_pitch, bx, by, [&](size_t off) { return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(in + off)); }, px);
        }
    };
    uint32_t cur[16];
#pragma unroll
    for (int k = 0; k < 16; k++) cur[k] = 0;
    if (first < n_blocks) load(first, cur);  // in flight while the tables are staged
    if constexpr (EAC) {
        const uint4* s = reinterpret_cast<const uint4*>(&tables->t);
        for (unsigned i = BU_ENC_LDS_LO / 16 + threadIdx.x; i < BU_ENC_LDS_HI / 16; i += BU_WG) s_eac[i] = s[i];
        __syncthreads();
    }
    const BuTables& T = EAC ? *reinterpret_cast<const BuTables*>(s_eac) : tables->t;
    for (size_t i = first; i < n_blocks; i += stride) {
        const size_t in_next = i + stride;
        uint32_t o[4];
        bu_encode_block<FORMAT>(T, cur, o);
        size_t bx, by;
        where(i, bx, by);
        uint8_t* dst = out + by * out_pitch + bx * (size_t)(4 * W);
        if constexpr (W == 2) bu_st_stream(reinterpret_cast<uint2*>(dst), make_uint2(o[0], o[1]));
        else bu_st_stream(reinterpret_cast<uint4*>(dst), make_uint4(o[0], o[1], o[2], o[3]));
        if (in_next < n_blocks) load(in_next, cur);
    }
}

}  // namespace
