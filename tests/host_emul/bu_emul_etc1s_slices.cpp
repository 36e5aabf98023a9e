// TEST-ONLY host build of the slice lookup of the whole-file ETC1S kernels (bu_etc1s_unit_slice, bu_etc1s_targets.hpp): the part of
// those kernels that block-level tests never see, compiled as plain C++ with UBSan by tests/test_read_file_targets.py.
// Never part of the product library.
#include "bu_uastc_dispatch.hpp"
#include "bu_etc1s_targets.hpp"

extern "C" {
// sizeof(BuEtc1sSlice): the caller builds the table as records of this size (unit0, n_blocks, nbx, idx_ofs, aidx_ofs, image: u32; out_ofs: u64)
size_t bu_emul_etc1s_slice_bytes(void) { return sizeof(BuEtc1sSlice); }

// out[u] = bu_etc1s_unit_slice(table, n_slices, u) for every unit u < n_units; table holds n_slices entries and the sentinel
void bu_emul_etc1s_unit_slices(const void* table, uint32_t n_slices, uint32_t n_units, uint32_t* out)
{
    const BuEtc1sSlice* slices = static_cast<const BuEtc1sSlice*>(table);
    for (uint32_t u = 0; u < n_units; u++) out[u] = bu_etc1s_unit_slice(slices, n_slices, u);
}
}
