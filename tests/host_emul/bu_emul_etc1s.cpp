// TEST-ONLY host build of the per-block code of the ETC1S back end (ETC1, RGBA32 and BC1, BC3, BC4, BC5, EAC R11, EAC RG11 in palette
// form, bu_etc1s_targets.hpp): the header the HIP kernels include, compiled as plain C++ by tests/test_etc1s_targets.py (with and without
// UBSan) and compared with the oracle's ETC1 and RGBA32 of the same blocks and with the numpy models applied to that RGBA32 decode.
// Never part of the product library.
#include "bu_uastc_dispatch.hpp"
#include "bu_etc1s_targets.hpp"

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

// ETC1: rows[i] is the word of the selector entry this target reads, its second (the ETC1 selector bytes)
static void run_etc1(const uint32_t* ep, const uint32_t* sel_y, size_t n, uint8_t* out)
{
    for (size_t i = 0; i < n; i++) {
        uint32_t o[2];
        bu_etc1s_etc1_block(ep[i], sel_y[i], o);
        memcpy(out + 8 * i, o, 8);
    }
}

// RGBA32: the block's 16 texels, row-major
static void run_rgba(const BuTables& T, const uint32_t* ep, const uint32_t* rows, const uint32_t* aep, const uint32_t* arows, size_t n, uint8_t* out)
{
    for (size_t i = 0; i < n; i++) {
        uint32_t pr, pg, pb, pa, px[16];
        bu_etc1s_palettes(T.etc1s_pal, ep[i], aep ? aep[i] : 0u, pr, pg, pb, pa);
        bu_etc1s_block_rgba(pr, pg, pb, pa, rows[i], aep != nullptr, aep ? arows[i] : 0u, px);
        memcpy(out + 64 * i, px, 64);
    }
}

template <int TARGET>
static void run(const BuTables& T, const uint32_t* ep, const uint32_t* rows, const uint32_t* aep, const uint32_t* arows, size_t n, uint8_t* out)
{
    const size_t obs = 4 * (size_t)bu_out_words(TARGET);
    for (size_t i = 0; i < n; i++) {
        uint32_t pr, pg, pb, pa;
        bu_etc1s_palettes(T.etc1s_pal, ep[i], aep ? aep[i] : 0u, pr, pg, pb, pa);
        uint32_t o[4] = {0, 0, 0, 0};
        bu_etc1s_target_block<TARGET>(T, pr, pg, pb, rows[i], aep != nullptr, pa, aep ? arows[i] : 0u, o);
        memcpy(out + obs * i, o, obs);
    }
}

extern "C" {
// One block per entry: ep[i] / rows[i] the colour endpoint word and selector rows, aep[i] / arows[i] the alpha ones (both NULL: no
// alpha slice).  target = BU_TARGET_ETC1 (rows[i] = the selector entry's SECOND word, no alpha), BU_TARGET_RGBA32 or one of the six of
// bu_etc1s_transcode; out: n x bu_target_block_bytes(target) bytes.  Returns -1 for any other target.
int bu_emul_etc1s_batch(int target, const uint32_t* ep, const uint32_t* rows, const uint32_t* aep, const uint32_t* arows, size_t n, uint8_t* out)
{
    const BuTables& T = tables();
    switch (target) {
    case BU_TGT_ETC1: run_etc1(ep, rows, n, out); return 0;
    case BU_TGT_RGBA: run_rgba(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_BC1: run<BU_TGT_BC1>(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_BC3: run<BU_TGT_BC3>(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_BC4: run<BU_TGT_BC4>(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_BC5: run<BU_TGT_BC5>(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_R11: run<BU_TGT_R11>(T, ep, rows, aep, arows, n, out); return 0;
    case BU_TGT_RG11: run<BU_TGT_RG11>(T, ep, rows, aep, arows, n, out); return 0;
    default: return -1;
    }
}

// bu_etc1s_index of one block: out = e, s, ae, as, bad
void bu_emul_etc1s_index(uint32_t ix, int has_a, uint32_t ax, uint32_t n_ep, uint32_t n_sel, uint32_t out[5])
{
    const BuEtc1sIndex k = bu_etc1s_index(ix, has_a != 0, ax, n_ep, n_sel);
    out[0] = k.e, out[1] = k.s, out[2] = k.ae, out[3] = k.as, out[4] = k.bad ? 1u : 0u;
}
}
