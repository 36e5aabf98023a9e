// The `.basis` container on the host: CRC-16, the 77-byte header, the 23-byte slice descriptors, the selector codebook's entry
// layout, and the whole-file plan (every check of read_to_* that needs no block work).
//
// Replaces, for this repo's C++ host facade:
//   src/basis.rs:8-260              the checks and the image geometry of read_to_*
//   src/basis.rs:300-372, 417-572   header (77 B), slice descs (23 B), CRC-16/GENIBUS
// Written for speed where it is free: table-driven CRC (8 bits per step), large payloads cut into pieces on the worker pool.
// Everything the reference would `panic!`/`assert!` on is a BU_ERR_BOUNDS status.
#pragma once
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <vector>

#include "../../include/basisu_hip.h"
#include "bu_host_pool.hpp"

namespace bu_host {

// ---- CRC-16/GENIBUS (basis.rs:364-372): poly 0x1021, init 0xFFFF, xorout 0xFFFF, not reflected ----
// Slicing-by-8: t[k][b] = register after byte b followed by k zero bytes, so 8 message bytes cost 8 independent lookups.
struct Crc16Table {
    uint16_t t[8][256];
    Crc16Table()
    {
        for (int b = 0; b < 256; b++) {
            uint16_t crc = (uint16_t)(b << 8);
            for (int k = 0; k < 8; k++) crc = (uint16_t)((crc & 0x8000) ? ((crc << 1) ^ 0x1021) : (crc << 1));
            t[0][b] = crc;
        }
        for (int k = 1; k < 8; k++)
            for (int b = 0; b < 256; b++) t[k][b] = (uint16_t)((t[k - 1][b] << 8) ^ t[0][t[k - 1][b] >> 8]);
    }
};
// raw register update (no init / final complement)
inline uint16_t crc16_raw(const uint8_t* p, size_t n, uint16_t s)
{
    static const Crc16Table tab;
    while (n >= 8) {
        s = (uint16_t)(tab.t[7][p[0] ^ (s >> 8)] ^ tab.t[6][p[1] ^ (s & 0xFF)] ^ tab.t[5][p[2]] ^ tab.t[4][p[3]] ^ tab.t[3][p[4]] ^ tab.t[2][p[5]] ^
                       tab.t[1][p[6]] ^ tab.t[0][p[7]]);
        p += 8;
        n -= 8;
    }
    for (size_t i = 0; i < n; i++) s = (uint16_t)((s << 8) ^ tab.t[0][((s >> 8) ^ p[i]) & 0xFF]);
    return s;
}
// a * b in GF(2)[x] / (x^16 + x^12 + x^5 + 1)
inline uint16_t crc16_gf_mul(uint16_t a, uint16_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x11021u;
        if ((b >> i) & 1u) r ^= a;
    }
    return (uint16_t)r;
}
// register s after n zero bytes = s * x^(8n)
inline uint16_t crc16_shift(uint16_t s, size_t n)
{
    uint16_t result = 1, base = 0x0100;
    for (; n; n >>= 1) {
        if (n & 1) result = crc16_gf_mul(result, base);
        base = crc16_gf_mul(base, base);
    }
    return crc16_gf_mul(s, result);
}
// The CRC is linear: register(s, A || B) = register(s, A) * x^(8|B|) + register(0, B).  Large payloads (a 4096^2 UASTC
// file is 16 MiB; config 5 is 512 MiB) are cut into pieces whose registers are computed concurrently and then folded.
inline uint16_t crc16(const uint8_t* p, size_t n, uint16_t crc)
{
    uint16_t s = (uint16_t)~crc;
    constexpr size_t PIECE = (size_t)1 << 18;
    const size_t pieces = (n + PIECE - 1) / PIECE;
    if (pieces < 4) return (uint16_t)~crc16_raw(p, n, s);
    std::vector<uint16_t> part(pieces, 0);
    std::atomic<size_t> next{0};
    const std::function<void()> work = [&] {
        for (size_t k; (k = next.fetch_add(1)) < pieces;) {
            const size_t lo = k * PIECE, len = (n - lo < PIECE) ? n - lo : PIECE;
            part[k] = crc16_raw(p + lo, len, 0);
        }
    };
    pool().run((unsigned)(pieces - 1 < Pool::capacity() ? pieces - 1 : Pool::capacity()), work);
    for (size_t k = 0; k < pieces; k++) {
        const size_t lo = k * PIECE, len = (n - lo < PIECE) ? n - lo : PIECE;
        s = (uint16_t)(crc16_shift(s, len) ^ part[k]);
    }
    return (uint16_t)~s;
}

inline uint32_t le(const uint8_t* p, int n)
{
    uint32_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint32_t)p[i] << (8 * i);
    return v;
}

// basis.rs:475-516
inline void parse_header(const uint8_t* b, bu_basis_header* h)
{
    h->sig = (uint16_t)le(b + 0, 2);
    h->ver = (uint16_t)le(b + 2, 2);
    h->header_size = (uint16_t)le(b + 4, 2);
    h->header_crc16 = (uint16_t)le(b + 6, 2);
    h->data_size = le(b + 8, 4);
    h->data_crc16 = (uint16_t)le(b + 12, 2);
    h->total_slices = le(b + 14, 3);
    h->total_images = le(b + 17, 3);
    h->tex_format = b[20];
    h->flags = (uint16_t)le(b + 21, 2);
    h->tex_type = b[23];
    h->us_per_frame = le(b + 24, 3);
    h->reserved = le(b + 27, 4);
    h->userdata0 = le(b + 31, 4);
    h->userdata1 = le(b + 35, 4);
    h->total_endpoints = (uint16_t)le(b + 39, 2);
    h->endpoint_cb_file_ofs = le(b + 41, 4);
    h->endpoint_cb_file_size = le(b + 45, 3);
    h->total_selectors = (uint16_t)le(b + 48, 2);
    h->selector_cb_file_ofs = le(b + 50, 4);
    h->selector_cb_file_size = le(b + 54, 3);
    h->tables_file_ofs = le(b + 57, 4);
    h->tables_file_size = le(b + 61, 4);
    h->slice_desc_file_ofs = le(b + 65, 4);
    h->extended_file_ofs = le(b + 69, 4);
    h->extended_file_size = le(b + 73, 4);
}

// basis.rs:307-336
inline bu_status read_header(const uint8_t* file, size_t len, bu_basis_header* h)
{
    if (len < 2 || le(file, 2) != 0x4273u) return BU_ERR_SIG;
    if (len < 77) return BU_ERR_HEADER_TRUNCATED;
    parse_header(file, h);
    if (h->header_size != 77) return BU_ERR_HEADER_SIZE;
    if (crc16(file + 8, 77 - 8, 0) != h->header_crc16) return BU_ERR_HEADER_CRC;
    return BU_OK;
}

// basis.rs:343-362, 554-571
inline bu_status read_slice_descs(const uint8_t* file, size_t len, const bu_basis_header* h, std::vector<bu_slice_desc>& out)
{
    out.clear();
    const size_t start = h->slice_desc_file_ofs;
    for (size_t i = 0; i < h->total_slices; i++) {
        const size_t s = start + 23 * i;
        if (s > len) return BU_ERR_BOUNDS;
        if (len - s < 23) return BU_ERR_SLICE_DESC;
        const uint8_t* p = file + s;
        bu_slice_desc d;
        d.image_index = le(p, 3);
        d.level_index = p[3];
        d.flags = p[4];
        d.orig_width = (uint16_t)le(p + 5, 2);
        d.orig_height = (uint16_t)le(p + 7, 2);
        d.num_blocks_x = (uint16_t)le(p + 9, 2);
        d.num_blocks_y = (uint16_t)le(p + 11, 2);
        d.file_ofs = le(p + 13, 4);
        d.file_size = le(p + 17, 4);
        d.slice_data_crc16 = (uint16_t)le(p + 21, 2);
        out.push_back(d);
    }
    return BU_OK;
}

inline bool in_file(size_t len, size_t ofs, size_t size) { return ofs <= len && size <= len - ofs; }

// etc::Selector::set_selector (etc.rs:363-393) for all 16 texels of one codebook entry: ETC1 code = [3,2,0,1][value],
// pixel id = x*4 + y, MSB plane in bytes 4-5 (pixels 8-15, then 0-7), LSB plane in bytes 6-7; bytes 0-3 keep the raw rows
inline void selector_from_rows(const uint8_t rows[4], uint8_t out_entry[8])
{
    static const uint8_t to_etc1[4] = {3, 2, 0, 1};  // etc.rs:433
    uint32_t msb = 0, lsb = 0;
    for (unsigned y = 0; y < 4; y++)
        for (unsigned x = 0; x < 4; x++) {
            const unsigned code = to_etc1[(rows[y] >> (2 * x)) & 3u];
            msb |= (code >> 1) << (x * 4 + y);
            lsb |= (code & 1u) << (x * 4 + y);
        }
    memcpy(out_entry, rows, 4);
    out_entry[4] = (uint8_t)(msb >> 8);
    out_entry[5] = (uint8_t)(msb & 0xFF);
    out_entry[6] = (uint8_t)(lsb >> 8);
    out_entry[7] = (uint8_t)(lsb & 0xFF);
}

// ---- whole-file planning (basis.rs:8-260): every check of read_to_* that needs no block work ----
struct BuFilePlan {
    bu_basis_header h;
    std::vector<bu_slice_desc> slices;
    std::vector<bu_image> images;       // one per output image
    std::vector<size_t> first_slice;    // slice feeding image i (its colour slice for RGBA+alpha)
    size_t out_bytes = 0;
    bool etc1s = false, alpha_pairs = false;  // alpha_pairs: an image is a colour / alpha slice pair (ETC1S with alpha: RGBA32 and the six targets)
    bool etc1s_six = false;                   // an ETC1S file read to BC4 .. BC3 (bu_read_file_to): block-linear images, the image list of RGBA32
};

// everything of read_to_* that needs no block work: checks in the reference's order, image geometry
// check_data_crc = false: the caller verifies the payload CRC itself (bu_read_to overlaps it with the upload) and gives
// a CRC failure precedence over any later error, as the reference's order of checks would
// etc1s_six = true (bu_read_file_query / bu_read_file_to): an ETC1S file takes BU_READ_BC4 .. BU_READ_BC3 too -- the image list and the
// alpha-slice checks of BU_READ_RGBA, block-linear images of the target's block size; nothing else changes
inline bu_status bu_plan_file(bu_read_target target, const uint8_t* file, size_t len, BuFilePlan& p, bool check_data_crc = true, bool etc1s_six = false)
{
    if (!file) return BU_ERR_ARGUMENT;
    if ((int)target < 0 || (int)target > (int)BU_READ_BC3 || (int)target == 10) return BU_ERR_ARGUMENT;  // (10 names no read target)
    bu_status st = read_header(file, len, &p.h);
    if (st) return st;
    if (check_data_crc && crc16(file + 77, len - 77, 0) != p.h.data_crc16) return BU_ERR_DATA_CRC;  // to EOF, basis.rs:338-341
    st = read_slice_descs(file, len, &p.h, p.slices);
    if (st) return st;
    if (p.h.tex_format > 1) return BU_ERR_TEX_FORMAT;
    p.etc1s = p.h.tex_format == 0;
    const bool has_alpha = (p.h.flags & 4) != 0;
    p.etc1s_six = p.etc1s && etc1s_six && (int)target >= (int)BU_READ_BC4;
    if (p.etc1s && (int)target >= (int)BU_READ_BC4 && !p.etc1s_six) return BU_ERR_ARGUMENT;  // (ETC1S to the channel and colour targets: bu_read_file_to)
    if (p.etc1s && !(target == BU_READ_RGBA || target == BU_READ_ETC1 || p.etc1s_six)) return BU_ERR_UNSUPPORTED;
    if (p.etc1s && has_alpha && (p.slices.size() % 2) != 0) return BU_ERR_ALPHA_SLICES;
    p.alpha_pairs = p.etc1s && has_alpha && (target == BU_READ_RGBA || p.etc1s_six);
    for (size_t i = 0; i < p.slices.size(); i++) {
        const bu_slice_desc& s = p.slices[i];
        if (!in_file(len, s.file_ofs, s.file_size)) return BU_ERR_BOUNDS;
        if (p.alpha_pairs) {
            if (i & 1) continue;
            const bu_slice_desc& a = p.slices[i + 1];
            if (!(a.flags & 1)) return BU_ERR_ALPHA_SLICES;
            if (a.num_blocks_x != s.num_blocks_x || a.num_blocks_y != s.num_blocks_y) return BU_ERR_ALPHA_SLICES;
        }
        const size_t nblk = (size_t)s.num_blocks_x * s.num_blocks_y, nb16 = s.file_size / 16;
        const bool eight = target == BU_READ_ETC1 || target == BU_READ_BC4 || target == BU_READ_EAC_R11 || target == BU_READ_BC1;  // 8-byte blocks
        bu_image im = {s.orig_width, s.orig_height, 0, 0, p.out_bytes, 0};
        if (p.etc1s) {
            if (target == BU_READ_RGBA) {
                im.size = nblk * 64;
                im.stride = 16u * s.orig_width;  // basis.rs:46,64 x4 (lib.rs:75): reference quirk, rows are 16*nbx apart
            } else {  // ETC1 and the six targets: block-linear
                im.size = nblk * (eight ? 8 : 16);
                im.stride = (eight ? 8u : 16u) * s.num_blocks_x;
            }
        } else {
            if (target != BU_READ_UASTC && s.file_size % 16) return BU_ERR_LENGTH;  // uastc.rs:54-59
            switch (target) {
            case BU_READ_RGBA:
                if (s.num_blocks_x == 0 && nb16) return BU_ERR_BOUNDS;
                if (s.num_blocks_x && nb16 % s.num_blocks_x) return BU_ERR_BOUNDS;  // the reference indexes past its image
                im.size = nb16 * 64;
                im.stride = 16u * s.num_blocks_x;
                break;
            case BU_READ_UASTC: im.size = s.file_size; im.stride = 16u * s.num_blocks_x; break;
            case BU_READ_ETC1:
            case BU_READ_BC4:
            case BU_READ_EAC_R11:
            case BU_READ_BC1: im.size = nb16 * 8; im.stride = 8u * s.num_blocks_x; break;
            default: im.size = nb16 * 16; im.stride = 16u * s.num_blocks_x; break;
            }
        }
        p.images.push_back(im);
        p.first_slice.push_back(i);
        p.out_bytes += im.size;
    }
    return BU_OK;
}

}  // namespace bu_host
