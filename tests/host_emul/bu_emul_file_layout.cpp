// TEST-ONLY stand-alone build of the whole-file layout (csrc/bu_file_layout.hpp) as it is, plain C++ with and without UBSan
// (tests/test_file_layout.py).  Prints what the layout of a file is as one JSON object.  Never part of the product library.
//   etc1s <read target> <six: 0 | 1> <file>    index buffer and slice table, and bu_etc1s_unit_slice of every unit over that table
//   etc1s-huge                                  the same for a hand-made plan of two slices of 65 535 x 65 535 blocks (no file bytes)
//   runs <read target> <file>                   the UASTC runs
//   piece <run bytes> <read target> <mapped: 0 | 1> [<BU_RUN_PIECE_MIB>]
//   aux <alignment> <region bytes> ...          the carve-up of the aux buffer (BuAuxLayout): offset of every region, total with the slack
//   fold <file> <offset:length> ...             the payload CRC folded from piece registers of those ranges (crc16_raw from a zero register,
//                                               what bu_crc16_pieces_kernel leaves) against the header's data_crc16
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "bu_file_layout.hpp"

static std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> v;
    FILE* fp = fopen(path, "rb");
    if (!fp) exit(2);
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(fp);
    return v;
}

template <class V, class F>
static void list(const char* name, const V& v, F item, const char* end = ", ")
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%s", i ? ", " : "", item(v[i]).c_str());
    printf("]%s", end);
}
static std::string num(unsigned long long v) { return std::to_string(v); }

static int etc1s(const bu_host::BuFilePlan& p)
{
    BuEtc1sFileLayout l;
    const bu_status st = bu_etc1s_file_layout(p, l);
    printf("{\"status\": %d, ", (int)st);
    if (!st) {
        printf("\"words\": %zu, \"n_units\": %u, ", l.words, l.n_units);
        list("idx_ofs", l.idx_ofs, num);
        list("aidx_ofs", l.aidx_ofs, num);
        list("unit0", l.unit0, num);
        list("units_of", l.units_of, num);
        list("descs", l.descs, [](const BuEtc1sSlice& d) {
            return "[" + num(d.unit0) + ", " + num(d.n_blocks) + ", " + num(d.nbx) + ", " + num(d.idx_ofs) + ", " + num(d.aidx_ofs) + ", " + num(d.image) + ", " +
                   num(d.out_ofs) + "]";
        });
        std::vector<uint32_t> units(l.n_units);
        for (uint32_t u = 0; u < l.n_units; u++) units[u] = bu_etc1s_unit_slice(l.descs.data(), (uint32_t)(l.descs.size() - 1), u);
        list("unit_slice", units, num, "");
    } else
        printf("\"words\": 0");
    printf("}\n");
    return 0;
}

int main(int argc, char** argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "etc1s" && argc == 5) {
        const std::vector<uint8_t> f = read_file(argv[4]);
        bu_host::BuFilePlan p;
        if (bu_host::bu_plan_file((bu_read_target)atoi(argv[2]), f.data(), f.size(), p, true, atoi(argv[3]) != 0)) return 3;
        return etc1s(p);
    }
    if (cmd == "etc1s-huge") {
        bu_host::BuFilePlan p;
        p.etc1s = true;
        for (uint64_t k = 0; k < 2; k++) {
            bu_slice_desc s = {};
            s.num_blocks_x = s.num_blocks_y = 65535;
            p.slices.push_back(s);
            p.first_slice.push_back(k);
            p.images.push_back(bu_image{65535, 65535, 0, 0, k * 65535ull * 65535ull * 8, 65535ull * 65535ull * 8});
        }
        return etc1s(p);
    }
    if (cmd == "runs" && argc == 4) {
        const std::vector<uint8_t> f = read_file(argv[3]);
        bu_host::BuFilePlan p;
        if (bu_host::bu_plan_file((bu_read_target)atoi(argv[2]), f.data(), f.size(), p)) return 3;
        BuUastcFileLayout l;
        bu_uastc_file_layout(p, l);
        printf("{\"total_in\": %zu, ", l.total_in);
        list("in_off", l.in_off, num);
        list("runs", l.runs, [](const BuFileRun& r) { return "[" + num(r.first) + ", " + num(r.last) + ", " + num(r.in_off) + ", " + num(r.file_ofs) + ", " + num(r.bytes) + "]"; }, "");
        printf("}\n");
        return 0;
    }
    if (cmd == "piece" && (argc == 5 || argc == 6)) {
        const size_t run_bytes = strtoull(argv[2], nullptr, 10), piece = bu_run_piece_bytes(run_bytes, argc == 6 ? argv[5] : nullptr);
        printf("{\"piece\": %zu, \"pieced\": %d}\n", piece, (int)bu_run_is_pieced((bu_read_target)atoi(argv[3]), atoi(argv[4]) != 0, piece, run_bytes));
        return 0;
    }
    if (cmd == "aux" && argc >= 3 && (size_t)argc - 3 <= BU_AUX_MAX_REGIONS) {
        std::vector<size_t> sizes;
        for (int a = 3; a < argc; a++) sizes.push_back(strtoull(argv[a], nullptr, 10));
        const BuAuxLayout l(sizes.data(), sizes.size(), strtoull(argv[2], nullptr, 10));
        printf("{\"slack\": %zu, \"total\": %zu, ", BU_AUX_SLACK, l.total);
        list("off", std::vector<size_t>(l.off, l.off + l.n), num, "");
        printf("}\n");
        return 0;
    }
    if (cmd == "fold" && argc >= 3) {
        const std::vector<uint8_t> f = read_file(argv[2]);
        if (f.size() < 77) return 3;
        std::vector<BuCrcSeg> segs;
        std::vector<uint16_t> parts;
        for (int a = 3; a < argc; a++) {
            unsigned long long ofs = 0, len = 0;
            if (sscanf(argv[a], "%llu:%llu", &ofs, &len) != 2) return 2;
            const size_t np = len / BU_CRC_PIECE;
            segs.push_back({(size_t)ofs, (size_t)len, parts.size(), np});
            for (size_t i = 0; i < np; i++)  // (a range that leaves the file has no registers worth having: zeros)
                parts.push_back(bu_host::in_file(f.size(), ofs, len) ? bu_host::crc16_raw(f.data() + ofs + i * BU_CRC_PIECE, BU_CRC_PIECE, 0) : 0);
        }
        const uint16_t want = (uint16_t)(f[12] | f[13] << 8);
        bool folded = false;
        const bool ok = bu_crc_fold(f.data(), f.size(), segs, parts.data(), want, &folded);
        printf("{\"ok\": %d, \"folded\": %d, \"host\": %d}\n", (int)ok, (int)folded, (int)(bu_host::crc16(f.data() + 77, f.size() - 77, 0) == want));
        return 0;
    }
    return 2;
}
