// TEST-ONLY host build of the per-block code of the colour targets (BC1, BC3): the same headers the HIP kernels include, compiled as
// plain C++ by tests/test_colour_targets.py (with and without UBSan) and compared with the numpy model of tests/colour_model.py.
// Never part of the product library.
#include "bu_uastc_dispatch.hpp"

static BuTablesAll g_tables;
static bool g_init = false;
static const BuTables& tables()
{
    if (!g_init) {
        bu_build_tables(&g_tables);
        g_init = true;
    }
    return g_tables.t;
}

template <int TARGET>
static int block(const BuTables& T, const uint8_t* in, uint8_t* out)
{
    BuBlk b;
    memcpy(b.w, in, 16);
    uint32_t o[4] = {0, 0, 0, 0};
    const int st = bu_block_any<TARGET>(T, T.mode_lut[b.w[0] & 127u], b, o);
    memcpy(out, o, 4 * bu_out_words(TARGET));
    return st;
}

extern "C" {
// target = BU_TARGET_BC1_RGB / BU_TARGET_BC3_RGBA; out: n_blocks x 8 / 16 bytes; statuses in st[] (0 ok / 1 bad mode / 2 bad pattern).
// Returns -1 for any other target.
int bu_emul_colour_batch(int target, const uint8_t* in, size_t n_blocks, uint8_t* out, uint8_t* st)
{
    const BuTables& T = tables();
    if (!bu_colour_target(target)) return -1;
    const size_t obs = 4 * (size_t)bu_out_words(target);
    for (size_t i = 0; i < n_blocks; i++) {
        const uint8_t* b = in + 16 * i;
        uint8_t* o = out + obs * i;
        st[i] = (uint8_t)(target == BU_TGT_BC1 ? block<BU_TGT_BC1>(T, b, o) : block<BU_TGT_BC3>(T, b, o));
    }
    return 0;
}
}
