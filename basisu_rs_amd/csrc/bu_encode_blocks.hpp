// Block ENCODERS from pixels: an RGBA8 image -> BC4, BC5, EAC R11, EAC RG11, BC1 or BC3 blocks (which is the contract).
// For the gfx950 kernels (bu_encode_kernels.hpp) and, compiled for the host, for the CPU tests (tests/host_emul/bu_emul_encode.cpp,
// bu_emul_encode_main.cpp).  Not a new codec: the block is what bu_uastc_transcode writes for a UASTC block whose RGBA32 unpack is these 16
// texels, so the encoders are bu_bc4_block, bu_r11_block (bu_uastc_channel.hpp) and bu_bc1_block (bu_uastc_colour.hpp,
// section 4.5), called on the channels their UASTC front doors give them.  What is new here is the way in: which bytes of the image are a
// block's texels.
//   image   pixel (px, py) = the four bytes R, G, B, A at py * pitch + 4 * px, 0 <= px < width, 0 <= py < height
//   block   (bx, by) of ceil(width / 4) x ceil(height / 4); its texel (x, y) is pixel (min(4 bx + x, width - 1), min(4 by + y, height - 1)):
//           a partial edge block repeats the image's last column and row, and no byte outside [py * pitch, py * pitch + 4 * width) is read
//   px[16]  texel i = 4y + x as R | G << 8 | B << 16 | A << 24 (the words of the RGBA32 unpack)
#pragma once
#include "bu_uastc_dispatch.hpp"  // BU_TGT_*, bu_channel_target, bu_colour_target, bu_out_words; bu_bc4_block, bu_r11_block, bu_bc1_block through it

constexpr bool bu_enc_format_ok(int format) { return bu_channel_target(format) || bu_colour_target(format); }
constexpr int bu_enc_block_words(int format) { return bu_out_words(format); }
// the widest block grid a call takes: 4 * width stays below 2^32 and a block row's bytes below 2^32
constexpr size_t BU_ENC_MAX_NBX = (size_t)1 << 28;

BU_DEV size_t bu_enc_blocks(size_t pixels) { return pixels / 4 + (pixels % 4 != 0); }  // (no pixels + 3: any size_t is a legal question)
// every texel of block (bx, by) is a pixel of its own: no clamp applies
BU_DEV bool bu_enc_block_inside(size_t width, size_t height, size_t bx, size_t by) { return 4 * bx + 4 <= width && 4 * by + 4 <= height; }
// byte offset of texel column x of block column bx inside a pixel row, and of texel row y of block row by inside the image
BU_DEV size_t bu_enc_col_offset(size_t width, size_t bx, int x)
{
    const size_t px = 4 * bx + (size_t)x;
    return 4 * (px < width ? px : width - 1);
}
BU_DEV size_t bu_enc_row_offset(size_t height, size_t pitch, size_t by, int y)
{
    const size_t py = 4 * by + (size_t)y;
    return (py < height ? py : height - 1) * pitch;
}

// The 16 texels of block (bx, by), edge replication included: px[4y + x] = ld(byte offset of the pixel), one 4-byte read per texel.
template <typename LD>
BU_DEV void bu_enc_gather(size_t width, size_t height, size_t pitch, size_t bx, size_t by, LD ld, uint32_t px[16])
{
    size_t col[4];
    BU_UNROLL
    for (int x = 0; x < 4; x++) col[x] = bu_enc_col_offset(width, bx, x);
    BU_UNROLL
    for (int y = 0; y < 4; y++) {
        const size_t row = bu_enc_row_offset(height, pitch, by, y);
        BU_UNROLL
        for (int x = 0; x < 4; x++) px[4 * y + x] = ld(row + col[x]);
    }
}

// byte c (0 = R, 3 = A) of the four texels of every block row in the bytes of one word: what bu_bc4_block and bu_r11_block read
// (the packing of bu_block_channels: the 16 texel words are dead before a channel encoder runs)
template <int C>
BU_DEV void bu_enc_channel_rows(const uint32_t px[16], uint32_t c4[4])
{
    constexpr uint32_t PAIR = C == 0 ? 0x0C0C0400u : 0x0C0C0703u;
    static_assert(C == 0 || C == 3, "X = R and Y = A");
    BU_UNROLL
    for (int y = 0; y < 4; y++) c4[y] = bu_perm(bu_perm(px[4 * y + 3], px[4 * y + 2], PAIR), bu_perm(px[4 * y + 1], px[4 * y], PAIR), 0x05040100u);
}

// out: BC4 / R11 / BC1 -> out[0..1]; BC5 / RG11 -> out[0..1] of R, out[2..3] of A; BC3 -> out[0..1] BC4 of A, out[2..3] BC1.
// T is read by R11 / RG11 only (eac_mods, eac_magic, eac_range).
template <int FORMAT>
BU_DEV void bu_encode_block(const BuTables& T, const uint32_t px[16], uint32_t out[4])
{
    static_assert(bu_enc_format_ok(FORMAT), "BC4, BC5, EAC R11, EAC RG11, BC1 or BC3");
    if constexpr (bu_channel_target(FORMAT)) {
        constexpr bool BC = FORMAT == BU_TGT_BC4 || FORMAT == BU_TGT_BC5, TWO = FORMAT == BU_TGT_BC5 || FORMAT == BU_TGT_RG11;
        uint32_t r4[4], a4[4];
        bu_enc_channel_rows<0>(px, r4);
        if constexpr (TWO) bu_enc_channel_rows<3>(px, a4);
        if constexpr (BC) {
            bu_bc4_block(r4, out);
            if constexpr (TWO) bu_bc4_block(a4, out + 2);
        } else {
            bu_r11_block(T, r4, out);
            if constexpr (TWO) bu_r11_block(T, a4, out + 2);
        }
    } else if constexpr (FORMAT == BU_TGT_BC3) {
        uint32_t a4[4];
        bu_enc_channel_rows<3>(px, a4);
        bu_bc4_block(a4, out);
        bu_bc1_block(px, out + 2);
    } else {
        bu_bc1_block(px, out);
    }
}
