// TEST-ONLY host build of the encoders from pixels (bu_encode_blocks.hpp): the header the HIP kernels include, compiled as plain C++ by
// tests/test_encode_blocks.py (no sanitizer: it is loaded into the test process) and compared with the numpy models of tests/colour_model.py and
// tests/channel_model.py.  Never part of the product library.
#include "bu_uastc_dispatch.hpp"
#include "bu_encode_blocks.hpp"

static BuTablesAll g_tables;
static bool g_init = false;

template <int FORMAT>
static void run(const BuTables& T, const uint8_t* img, size_t width, size_t height, size_t pitch, uint8_t* out)
{
    constexpr size_t BB = 4 * (size_t)bu_enc_block_words(FORMAT);
    const size_t nbx = bu_enc_blocks(width), nby = bu_enc_blocks(height);
    const auto ld = [img](size_t off) {
        uint32_t w;
        memcpy(&w, img + off, 4);
        return w;
    };
    for (size_t by = 0; by < nby; by++)
        for (size_t bx = 0; bx < nbx; bx++) {
            uint32_t px[16], o[4] = {0, 0, 0, 0};
            bu_enc_gather(width, height, pitch, bx, by, ld, px);
            bu_encode_block<FORMAT>(T, px, o);
            memcpy(out + BB * (by * nbx + bx), o, BB);
        }
}

extern "C" {
// format: a bu_target of the six; img: height rows of `pitch` bytes, the last up to its last pixel; out: ceil(width / 4) * ceil(height / 4) blocks, tight.
// Returns -1 for any other format.
int bu_emul_encode_image(int format, const uint8_t* img, size_t width, size_t height, size_t pitch, uint8_t* out)
{
    if (!g_init) {
        bu_build_tables(&g_tables);
        g_init = true;
    }
    const BuTables& T = g_tables.t;
    switch (format) {
    case BU_TGT_BC4: run<BU_TGT_BC4>(T, img, width, height, pitch, out); break;
    case BU_TGT_BC5: run<BU_TGT_BC5>(T, img, width, height, pitch, out); break;
    case BU_TGT_R11: run<BU_TGT_R11>(T, img, width, height, pitch, out); break;
    case BU_TGT_RG11: run<BU_TGT_RG11>(T, img, width, height, pitch, out); break;
    case BU_TGT_BC1: run<BU_TGT_BC1>(T, img, width, height, pitch, out); break;
    case BU_TGT_BC3: run<BU_TGT_BC3>(T, img, width, height, pitch, out); break;
    default: return -1;
    }
    return 0;
}
}
