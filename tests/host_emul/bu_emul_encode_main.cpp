// TEST-ONLY stand-alone host build of the encoders from pixels (bu_encode_blocks.hpp) with its own main, so that tests/test_encode_blocks.py can build
// it with -fsanitize=address,undefined and run it as a child process.
//   usage: bu_emul_encode_main W H PAD [W H PAD ...]
// For every triple: an image of W x H pixels with pixel rows 4 W + PAD bytes apart, byte c of pixel (px, py) = (131 py + 31 px + 89 c + 7 (py ^ px)) & 255,
// on the heap in exactly (H - 1) * pitch + 4 W bytes -- a read of one byte past the last pixel is a heap overflow -- with 0xEE in the pitch padding.
// Every block is gathered and encoded to all six formats; one line per triple:
//   W H PAD g c6 c7 c8 c9 c11 c12      g = sum over the gathered texel words, in block raster order, of (k + 1) * word_k mod 2^64;
//                                      cF = the same sum over the bytes of format F's blocks
// Exit status 2 for a bad command line.  Never part of the product library.
#include <stdio.h>
#include <stdlib.h>

#include "bu_uastc_dispatch.hpp"
#include "bu_encode_blocks.hpp"

template <int FORMAT>
static void fold(const BuTables& T, const uint32_t px[16], uint64_t& sum, uint64_t& k)
{
    uint32_t o[4] = {0, 0, 0, 0};
    bu_encode_block<FORMAT>(T, px, o);
    uint8_t b[16];
    memcpy(b, o, 16);
    for (int i = 0; i < 4 * bu_enc_block_words(FORMAT); i++) sum += ++k * b[i];
}

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) return 2;
    static BuTablesAll tables;
    bu_build_tables(&tables);
    const BuTables& T = tables.t;
    for (int a = 1; a < argc; a += 3) {
        const size_t width = strtoull(argv[a], nullptr, 10), height = strtoull(argv[a + 1], nullptr, 10), pad = strtoull(argv[a + 2], nullptr, 10);
        if (width == 0 || height == 0 || pad % 4 != 0) return 2;
        const size_t pitch = 4 * width + pad, bytes = (height - 1) * pitch + 4 * width;
        uint8_t* img = static_cast<uint8_t*>(malloc(bytes));
        if (!img) return 2;
        memset(img, 0xEE, bytes);
        for (size_t py = 0; py < height; py++)
            for (size_t px = 0; px < width; px++)
                for (size_t c = 0; c < 4; c++) img[py * pitch + 4 * px + c] = (uint8_t)(131 * py + 31 * px + 89 * c + 7 * (py ^ px));
        const auto ld = [img](size_t off) {
            uint32_t w;
            memcpy(&w, img + off, 4);
            return w;
        };
        uint64_t g = 0, gk = 0, c[6] = {0, 0, 0, 0, 0, 0}, ck[6] = {0, 0, 0, 0, 0, 0};
        for (size_t by = 0; by < bu_enc_blocks(height); by++)
            for (size_t bx = 0; bx < bu_enc_blocks(width); bx++) {
                uint32_t px[16];
                bu_enc_gather(width, height, pitch, bx, by, ld, px);
                for (int i = 0; i < 16; i++) g += ++gk * px[i];
                fold<BU_TGT_BC4>(T, px, c[0], ck[0]);
                fold<BU_TGT_BC5>(T, px, c[1], ck[1]);
                fold<BU_TGT_R11>(T, px, c[2], ck[2]);
                fold<BU_TGT_RG11>(T, px, c[3], ck[3]);
                fold<BU_TGT_BC1>(T, px, c[4], ck[4]);
                fold<BU_TGT_BC3>(T, px, c[5], ck[5]);
            }
        free(img);
        printf("%zu %zu %zu %llu %llu %llu %llu %llu %llu %llu\n", width, height, pad, (unsigned long long)g, (unsigned long long)c[0], (unsigned long long)c[1],
               (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5]);
    }
    return 0;
}
