// TEST-ONLY stand-alone host build of the encoder from pixels to UASTC (bu_uastc_encode.hpp) with its own main, so that tests/test_uastc_encode.py can
// build it with -fsanitize=address,undefined and run it as a child process.
//   usage: bu_emul_uastc_encode_main W H PAD [W H PAD ...]
// For every triple: an image of W x H pixels with pixel rows 4 W + PAD bytes apart, on the heap in exactly (H - 1) * pitch + 4 W bytes -- a read of one
// byte past the last pixel is a heap overflow -- with 0xEE in the pitch padding.  Byte c of pixel (px, py) = (131 py + 31 px + 89 c + 7 (py ^ px)) & 255;
// with t = px / 8 + py / 8: alpha 255 where t is odd, and where t is a multiple of five the single colour (37 t, 11 t, 73 t, 5 t) & 255
// (tests/uastc_encode_cases.formula_image).  One line per triple:
//   W H PAD c      c = sum over the bytes of the blocks, in raster order, of (k + 1) * byte_k mod 2^64
// Exit status 2 for a bad command line.  Never part of the product library.
#include <stdio.h>
#include <stdlib.h>

#include "bu_uastc_dispatch.hpp"
#include "bu_uastc_encode.hpp"

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) return 2;
    static BuTablesAll tables;
    static BuEncQuant quant;
    bu_build_tables(&tables);
    for (unsigned i = 0; i < BU_ENC_QUANT_ENTRIES; i++) bu_enc_quant_entry(tables.t, &quant, i);
    for (int a = 1; a < argc; a += 3) {
        const size_t width = strtoull(argv[a], nullptr, 10), height = strtoull(argv[a + 1], nullptr, 10), pad = strtoull(argv[a + 2], nullptr, 10);
        if (width == 0 || height == 0 || pad % 4 != 0) return 2;
        const size_t pitch = 4 * width + pad, bytes = (height - 1) * pitch + 4 * width;
        uint8_t* img = static_cast<uint8_t*>(malloc(bytes));
        if (!img) return 2;
        memset(img, 0xEE, bytes);
        for (size_t py = 0; py < height; py++)
            for (size_t px = 0; px < width; px++) {
                const size_t t = px / 8 + py / 8;
                uint8_t* p = img + py * pitch + 4 * px;
                for (size_t c = 0; c < 4; c++) p[c] = (uint8_t)(131 * py + 31 * px + 89 * c + 7 * (py ^ px));
                if (t % 2 == 1) p[3] = 255;
                if (t % 5 == 0) p[0] = (uint8_t)(37 * t), p[1] = (uint8_t)(11 * t), p[2] = (uint8_t)(73 * t), p[3] = (uint8_t)(5 * t);
            }
        const auto ld = [img](size_t off) {
            uint32_t w;
            memcpy(&w, img + off, 4);
            return w;
        };
        uint64_t c = 0, k = 0;
        for (size_t by = 0; by < bu_enc_blocks(height); by++)
            for (size_t bx = 0; bx < bu_enc_blocks(width); bx++) {
                uint32_t px[16], o[4];
                bu_enc_gather(width, height, pitch, bx, by, ld, px);
                bu_uastc_encode_block(tables.t, quant, px, o);
                bu_uastc_encode_hints(tables.t, px, o);
                uint8_t b[16];
                memcpy(b, o, 16);
                for (int i = 0; i < 16; i++) c += ++k * b[i];
            }
        free(img);
        printf("%zu %zu %zu %llu\n", width, height, pad, (unsigned long long)c);
    }
    return 0;
}
