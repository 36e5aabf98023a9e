// TEST-ONLY stand-alone host build of the block decoders (bu_decode_blocks.hpp): the header the HIP kernels include, compiled as plain C++
// with its own main, so that tests/test_decode_blocks.py can build it with -fsanitize=address,undefined and run it as a child process.
//   usage: bu_emul_decode IN OUT
//   IN   4 bytes little-endian: the format (a bu_target value), then n blocks of the format's size
//   OUT  n x 64 bytes of texels (R, G, B, A; texel 4y + x), then n status bytes (0, 1 = BU_ERR_INVALID_MODE, 17 = BU_ERR_UNSUPPORTED)
// Exit status 2 for a bad command line, file or format.  Never part of the product library.
#include <stdio.h>

#include <vector>

#include "bu_uastc_dispatch.hpp"
#include "bu_decode_blocks.hpp"

template <int FORMAT>
static void run(const BuDecView& V, const uint8_t* in, size_t n, uint8_t* px, uint8_t* st)
{
    constexpr size_t BB = 4 * (size_t)bu_dec_block_words(FORMAT);
    for (size_t i = 0; i < n; i++) {
        uint32_t w[4] = {0, 0, 0, 0}, o[16];
        memcpy(w, in + BB * i, BB);
        st[i] = (uint8_t)bu_decode_block<FORMAT>(V, w, o);
        memcpy(px + 64 * i, o, 64);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) in.insert(in.end(), buf, buf + k);
    fclose(f);
    if (in.size() < 4) return 2;
    int32_t format;
    memcpy(&format, in.data(), 4);
    if (format < 0 || format > 12 || !bu_dec_format_ok(format)) return 2;
    const size_t bb = format == 2 || format == 6 || format == 8 || format == 11 ? 8 : 16;
    if ((in.size() - 4) % bb) return 2;
    const size_t n = (in.size() - 4) / bb;
    static BuTablesAll tables;
    bu_build_tables(&tables);
    const BuDecView V = {&tables.dec, tables.t.etc1_mod, tables.t.eac_mods};
    std::vector<uint8_t> out(65 * n);
    const uint8_t* blocks = in.data() + 4;
    uint8_t *px = out.data(), *st = out.data() + 64 * n;
    switch (format) {
    case 0: run<0>(V, blocks, n, px, st); break;
    case 1: run<1>(V, blocks, n, px, st); break;
    case 2: run<2>(V, blocks, n, px, st); break;
    case 3: run<3>(V, blocks, n, px, st); break;
    case 6: run<6>(V, blocks, n, px, st); break;
    case 7: run<7>(V, blocks, n, px, st); break;
    case 8: run<8>(V, blocks, n, px, st); break;
    case 9: run<9>(V, blocks, n, px, st); break;
    case 11: run<11>(V, blocks, n, px, st); break;
    default: run<12>(V, blocks, n, px, st); break;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    return fclose(f) == 0 && ok ? 0 : 2;
}
