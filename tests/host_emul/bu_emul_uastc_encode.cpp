// TEST-ONLY host build of the encoder from pixels to UASTC (bu_uastc_encode.hpp): the header the HIP kernel includes, compiled as plain C++ by
// tests/test_uastc_encode.py (no sanitizer: it is loaded into the test process) and compared with the numpy model of tests/uastc_encode_model.py.
// Never part of the product library.
#include "bu_uastc_dispatch.hpp"
#include "bu_uastc_encode.hpp"

static BuTablesAll g_tables;
static BuEncQuant g_quant;
static bool g_init = false;

extern "C" {
// img: height rows of `pitch` bytes, the last up to its last pixel; out: ceil(width / 4) * ceil(height / 4) blocks of 16 bytes, tight
int bu_emul_uastc_encode_image(const uint8_t* img, size_t width, size_t height, size_t pitch, uint8_t* out)
{
    if (!g_init) {
        bu_build_tables(&g_tables);
        for (unsigned i = 0; i < BU_ENC_QUANT_ENTRIES; i++) bu_enc_quant_entry(g_tables.t, &g_quant, i);
        g_init = true;
    }
    const size_t nbx = bu_enc_blocks(width), nby = bu_enc_blocks(height);
    const auto ld = [img](size_t off) {
        uint32_t w;
        memcpy(&w, img + off, 4);
        return w;
    };
    for (size_t by = 0; by < nby; by++)
        for (size_t bx = 0; bx < nbx; bx++) {
            uint32_t px[16], o[4];
            bu_enc_gather(width, height, pitch, bx, by, ld, px);
            bu_uastc_encode_block(g_tables.t, g_quant, px, o);
            bu_uastc_encode_hints(g_tables.t, px, o);
            memcpy(out + 16 * (by * nbx + bx), o, 16);
        }
    return 0;
}
// the quantiser table of endpoint range 11, 13 or 19: value -> level index
int bu_emul_uastc_encode_quant(int range, uint8_t* out256)
{
    if (range != 11 && range != 13 && range != 19) return -1;
    uint8_t dummy[16] = {0};
    bu_emul_uastc_encode_image(dummy, 1, 1, 4, dummy);  // (builds the tables)
    memcpy(out256, g_quant.q[bu_encq_row(range)], 256);
    return 0;
}
}
