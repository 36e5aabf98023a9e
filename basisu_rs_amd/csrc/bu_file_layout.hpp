// Host-side layout of the whole-file calls (bu_capi_file.hpp): where the slices of a planned file (BuFilePlan, bu_container.hpp) go in the staged input, what the
// whole-file ETC1S kernels are told about them, how a UASTC run is cut into pieces, how the aux buffer of a blocking host-pointer call is carved
// into regions (BuAuxLayout), and the fold of the device's CRC piece registers.  Pure arithmetic
// over file fields -- the code that faces a hostile slice table.  No HIP in here: tests/host_emul/bu_emul_file_layout.cpp compiles it as it is and
// tests/test_file_layout.py checks it without a GPU.
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "bu_basis.hpp"
#include "bu_etc1s_targets.hpp"  // BuEtc1sSlice

// v into a 32-bit field of a descriptor; false: it does not fit (the file claims more than the field can say)
inline bool bu_narrow_u32(size_t v, uint32_t& out)
{
    out = (uint32_t)v;
    return v <= 0xFFFFFFFFull;
}

// ---- ETC1S: the index buffer and the kernels' slice table ---------------------------------------------------------------------------
// The index arrays of the images follow each other in file order, colour then (alpha pairs) alpha, each padded to whole 64-word units: a
// wave owns a unit.  Everything is in WORDS from the start of the buffer; an upload multiplies by 4.  Images without blocks get no
// entry in the table (bu_etc1s_targets.hpp: consecutive entries never share a unit0); the table ends with the sentinel.
namespace {  // (BuEtc1sSlice's)

struct BuEtc1sFileLayout {
    std::vector<uint32_t> idx_ofs, aidx_ofs;  // per image: its colour / alpha indices (aidx_ofs: alpha pairs only)
    std::vector<uint32_t> unit0, units_of;    // per image: its first unit and how many it has (none: an image without blocks)
    std::vector<BuEtc1sSlice> descs;          // one entry per image with blocks, then the sentinel
    size_t words = 0;                         // of the whole index buffer
    uint32_t n_units = 0;
};

// BU_ERR_BOUNDS: an offset, the unit count or a slice's block count does not fit the table's 32-bit fields
inline bu_status bu_etc1s_file_layout(const bu_host::BuFilePlan& p, BuEtc1sFileLayout& l)
{
    const size_t n_img = p.images.size();
    l = BuEtc1sFileLayout();
    l.idx_ofs.assign(n_img, 0);
    l.aidx_ofs.assign(n_img, 0);
    l.unit0.assign(n_img, 0);
    l.units_of.assign(n_img, 0);
    l.descs.reserve(n_img + 1);
    size_t units = 0;
    bool fits = true;
    for (size_t k = 0; k < n_img; k++) {
        const bu_slice_desc& s = p.slices[p.first_slice[k]];
        const size_t nblk = (size_t)s.num_blocks_x * s.num_blocks_y, padded = (nblk + 63) & ~(size_t)63;
        BuEtc1sSlice d = {};
        fits &= bu_narrow_u32(l.words, l.idx_ofs[k]);
        l.words += padded;
        if (p.alpha_pairs) {
            fits &= bu_narrow_u32(l.words, l.aidx_ofs[k]);
            l.words += padded;
        }
        fits &= bu_narrow_u32(units, l.unit0[k]) && bu_narrow_u32(nblk, d.n_blocks);
        if (!fits) return BU_ERR_BOUNDS;  // (before the sums can wrap: every term is below 2^33)
        if (p.images[k].size == 0 || nblk == 0) continue;
        d.unit0 = l.unit0[k];
        d.nbx = s.num_blocks_x;
        d.idx_ofs = l.idx_ofs[k];
        d.aidx_ofs = p.alpha_pairs ? l.aidx_ofs[k] : 0xFFFFFFFFu;
        d.image = (uint32_t)k;  // (an image is a slice of the table: below 2^24)
        d.out_ofs = p.images[k].offset;
        l.descs.push_back(d);
        l.units_of[k] = (uint32_t)(padded / 64);
        units += padded / 64;
    }
    BuEtc1sSlice end = {};
    if (!bu_narrow_u32(units, end.unit0) || l.words > 0xFFFFFFFFull) return BU_ERR_BOUNDS;
    l.n_units = end.unit0;
    l.descs.push_back(end);
    return BU_OK;
}

}  // namespace

// ---- UASTC: runs ----------------------------------------------------------------------------------------------------------------
// Consecutive slices that sit back to back in the file (the usual layout of a mip chain or a texture array) are staged back to back
// with ONE upload, and -- for the block-linear targets, whose outputs are then contiguous too -- transcoded with ONE launch over the
// whole run: 512 slices of 65 536 blocks are one 33 M-block launch (0.3 ms) instead of 512 latency-bound ones (3.9 ms).  The lowest
// failing block of a run lies in its first failing slice, so the reported error is the sequential loop's.
struct BuFileRun {
    size_t first, last;  // images
    size_t in_off;       // of its first byte in the staged input: a multiple of 256
    size_t file_ofs, bytes;
};
struct BuUastcFileLayout {
    std::vector<size_t> in_off;  // per image
    std::vector<BuFileRun> runs;
    size_t total_in = 0;
};

inline size_t bu_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the carve-up of the context's aux buffer -------------------------------------------------------------------------------------------
// The blocking host-pointer calls (bu_staged_call.hpp) keep what is neither input nor output in ONE device buffer: codebooks, status words,
// slice table, CRC registers.  From the byte sizes of the regions a call wants, in order: where each starts -- a multiple of `align`, a power
// of two -- and what to reserve, the rounded sizes and BU_AUX_SLACK.
constexpr size_t BU_AUX_SLACK = 512;
constexpr size_t BU_AUX_MAX_REGIONS = 4;
struct BuAuxLayout {
    size_t n = 0, off[BU_AUX_MAX_REGIONS] = {}, total = BU_AUX_SLACK;
    BuAuxLayout() = default;
    BuAuxLayout(const size_t* sizes, size_t n_sizes, size_t align = 256) : n(n_sizes)
    {
        assert(n_sizes <= BU_AUX_MAX_REGIONS && align && (align & (align - 1)) == 0);
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            off[i] = at;
            at += (sizes[i] + align - 1) & ~(align - 1);
        }
        total = at + BU_AUX_SLACK;
    }
    // BuAuxLayout({a, b, c}) / BuAuxLayout({a, b, c}, 16): one region more than the layout holds does not compile
    template <size_t N>
    BuAuxLayout(const size_t (&sizes)[N], size_t align = 256) : BuAuxLayout(sizes, N, align)
    {
        static_assert(N <= BU_AUX_MAX_REGIONS, "BuAuxLayout holds BU_AUX_MAX_REGIONS regions");
    }
    size_t at(size_t i) const
    {
        assert(i < n);
        return off[i];
    }
};

// a slice joins its predecessor's run when it starts where that one ends and both are whole blocks, at least one
inline void bu_uastc_file_layout(const bu_host::BuFilePlan& p, BuUastcFileLayout& l)
{
    const size_t n_img = p.images.size();
    l = BuUastcFileLayout();
    l.in_off.assign(n_img, 0);
    for (size_t k = 0; k < n_img; k++) {
        const bu_slice_desc& s = p.slices[p.first_slice[k]];
        bool joins = false;
        if (k > 0) {
            const bu_slice_desc& q = p.slices[p.first_slice[k - 1]];
            joins = s.file_size % 16 == 0 && s.file_size != 0 && q.file_size % 16 == 0 && q.file_size != 0 && (size_t)q.file_ofs + q.file_size == s.file_ofs;
        }
        if (joins) {
            BuFileRun& r = l.runs.back();
            l.in_off[k] = r.in_off + r.bytes;
            r.last = k;
            r.bytes += s.file_size;
        } else {
            l.total_in = bu_align256(l.total_in);
            l.in_off[k] = l.total_in;
            l.runs.push_back(BuFileRun{k, k, l.total_in, s.file_ofs, s.file_size});
        }
        l.total_in = l.in_off[k] + s.file_size;
    }
    l.total_in = bu_align256(l.total_in);
}

// ---- UASTC: pieces of a run -----------------------------------------------------------------------------------------------------
// A large block-linear run with a mapped (page-locked) output is uploaded and transcoded in pieces on two streams, so that piece i's
// results cross PCIe upstream while piece i+1 comes down.  Piece size: a quarter of the run in whole MiB, between 4 and 16 MiB (a 16 MiB
// file: 0.672 ms in one piece, 0.585 in four, 0.645 in eight -- tools/exp/file_time.py); fixed_mib (BU_RUN_PIECE_MIB) sets it, 0 = no pieces.
// (The same pieces for a PAGEABLE output -- four streams, upload and launch of a piece on one stream -- lose from runs of 64 MiB on: 2.64
// against 2.52 ms for a 64 MiB file, 5.17 against 4.97 for 128 MiB.  The call is two PCIe copies long and the kernels are 1 % of it; with a
// pageable output the run stays one upload, one launch -- which draws its tiles by ticket from 2^24 blocks on -- and one download.)
inline size_t bu_run_piece_bytes(size_t run_bytes, const char* fixed_mib)
{
    constexpr size_t MIB = (size_t)1 << 20;
    if (fixed_mib) return (size_t)atoll(fixed_mib) << 20;
    const size_t quarter = (run_bytes / 4) & ~(MIB - 1);
    return std::min(std::max(quarter, 4 * MIB), 16 * MIB);
}
inline bool bu_run_is_pieced(bu_read_target target, bool mapped_out, size_t piece_bytes, size_t run_bytes)
{
    return target != BU_READ_RGBA && mapped_out && piece_bytes && run_bytes >= 2 * piece_bytes;
}

// ---- the payload CRC from the device's piece registers ------------------------------------------------------------------------------
// bu_crc16_pieces_kernel (bu_kernels.hpp) leaves one register per whole BU_CRC_PIECE bytes of an uploaded range, each from a zero register.
// The CRC is linear (bu_container.hpp: crc16), so the payload's register is folded in file order from those and from the bytes only the host
// has seen: slice table, gaps, the tail of a range behind its last whole piece.
constexpr unsigned BU_CRC_PIECE = 65536;
struct BuCrcSeg {
    size_t file_ofs, len, first_piece, n_pieces;  // an uploaded range of the file; its registers are parts[first_piece ...]
};

// true: the payload (byte 77 to the end) has the CRC `want`.  Ranges that overlap or leave the file (a hostile slice table) cannot be
// folded: the plain host CRC decides then.  Sorts segs by file offset.
inline bool bu_crc_fold(const uint8_t* file, size_t len, std::vector<BuCrcSeg>& segs, const uint16_t* parts, uint16_t want, bool* folded = nullptr)
{
    std::sort(segs.begin(), segs.end(), [](const BuCrcSeg& a, const BuCrcSeg& b) { return a.file_ofs < b.file_ofs; });
    bool foldable = true;
    size_t pos = 77;
    for (const BuCrcSeg& g : segs) {
        if (g.file_ofs < pos || !bu_host::in_file(len, g.file_ofs, g.len)) foldable = false;
        pos = g.file_ofs + g.len;
    }
    if (folded) *folded = foldable;
    if (!foldable) return bu_host::crc16(file + 77, len - 77, 0) == want;
    const uint16_t shift_piece = bu_host::crc16_shift(1, BU_CRC_PIECE);  // x^(8 * 65536)
    uint16_t reg = 0xFFFF;  // register of CRC-16/GENIBUS before the first payload byte
    pos = 77;
    for (const BuCrcSeg& g : segs) {
        reg = bu_host::crc16_raw(file + pos, g.file_ofs - pos, reg);
        for (size_t i = 0; i < g.n_pieces; i++) reg = (uint16_t)(bu_host::crc16_gf_mul(reg, shift_piece) ^ parts[g.first_piece + i]);
        const size_t covered = g.n_pieces * BU_CRC_PIECE;
        reg = bu_host::crc16_raw(file + g.file_ofs + covered, g.len - covered, reg);
        pos = g.file_ofs + g.len;
    }
    reg = bu_host::crc16_raw(file + pos, len - pos, reg);
    return (uint16_t)~reg == want;
}
