// UASTC -> BC4 / BC5 / EAC R11 / EAC RG11 (the one- and two-channel targets) for the gfx950 kernels.
// The reference has no such targets, so there is nothing to mirror: the two encoders are the exact integer rules of DESIGN.md
// section 4.4 (repeated beside the code below), pinned by the independent model of tests/channel_model.py, which spec decoders pin in turn.
//   input     byte c of texel i (i = 4y + x) of what BU_TARGET_RGBA32 writes for the block: the block goes through the RGBA32 unpack
//             (bu_block_rgba, the same front end and sink) and the encoders read channel R (byte 0) and A (byte 3) of its texels
//   BC4       8 bytes: one channel                         BC5   BC4(R) then BC4(A)
//   EAC R11   8 bytes: one channel, unsigned              RG11  R11(R) then R11(A)
// Two-channel output takes R and A, the convention of normal maps (X in RGB, Y in alpha); a block without alpha decodes to A = 255.
#pragma once
#include "bu_uastc_etc.hpp"

#if defined(__HIPCC__)
#define BU_ROLLED _Pragma("unroll 1")
#else
#define BU_ROLLED _Pragma("GCC unroll 1")
#endif

// BC4 UNORM of one channel, c4[y] = the channel's bytes of block row y (byte x); out[0..1] = bytes 0..7.
//   mn = min v, mx = max v, d = mx - mn; byte 0 = mx, byte 1 = mn (byte 0 > byte 1: the 8-value mode; mn == mx writes mn twice)
//   q = floor((14 (v - mn) + d) / (2d)) in 0..7, the nearest step of the ideal ramp (halves round up), counted without a division:
//       q = #{j in 1..7 : 14 (v - mn) >= (2j - 1) d}      (d = 0: every test passes, q = 7, so a solid block has all selectors 0)
//   code: q = 7 -> 0, q = 0 -> 1, else 8 - q   (the nibbles of 0x02345671)
//   bytes 2..7: a 48-bit little-endian string, texel i's code at bits 3i .. 3i + 2
BU_DEV void bu_bc4_block(const uint32_t c4[4], uint32_t out[2])
{
    uint32_t v[16];
    BU_UNROLL
    for (int i = 0; i < 16; i++) v[i] = (c4[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    uint32_t mn = v[0], mx = v[0];
    BU_UNROLL
    for (int i = 1; i < 16; i++) {
        mn = bu_umin(mn, v[i]);
        mx = bu_umax(mx, v[i]);
    }
    const uint32_t d = mx - mn;
    uint32_t thr[7];  // (2j - 1) d
    BU_UNROLL
    for (int j = 1; j <= 7; j++) thr[j - 1] = (uint32_t)(2 * j - 1) * d;
    uint32_t lo = 0, hi = 0;  // bits 0..23 / 24..47 of the selector string
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t e = 14u * (v[i] - mn);
        uint32_t q = 0;
        BU_UNROLL
        for (int j = 0; j < 7; j++) q += e >= thr[j] ? 1u : 0u;
        const uint32_t code = (0x02345671u >> (4 * q)) & 7u;
        if (i < 8) lo |= code << (3 * i);
        else hi |= code << (3 * (i - 8));
    }
    out[0] = mx | (mn << 8) | (lo << 16);
    out[1] = (lo >> 16) | (hi << 8);
}

// The eight values of EAC modifier table `table` around base `base`, in rank (ascending) order, and the thresholds between them.
// scale = 8 * multiplier, or 1 for multiplier 0.  val[r] = clamp(8 base + 4 + scale * mod, 0, 2047).
// thr[r] (r = 1..7): the first 11-bit value that takes rank r over rank r - 1.  A tie goes to the LOWER spec index j; ranks 0..3 are
// j = 3, 2, 1, 0 and ranks 4..7 j = 4..7, so ranks 1..3 win their tie (ceil of the midpoint) and ranks 4..7 lose it (floor + 1) --
// as bu_eac_block does for 8-bit alpha.  Clamped duplicates fall out right (equal values at 0 give threshold 0, always passed: the
// higher rank = the lower j; at 2047 threshold 2048, never passed: the lower rank = the lower j).
BU_DEV void bu_r11_ramp(const BuTables& T, uint32_t table, int scale, int base, int val[8], int thr[8])
{
    BU_UNROLL
    for (int r = 0; r < 8; r++) val[r] = bu_clampi(8 * base + 4 + scale * (int)T.eac_mods[8 * table + r], 0, 2047);
    BU_UNROLL
    for (int r = 1; r < 8; r++) thr[r] = (val[r - 1] + val[r] + (r < 4 ? 1 : 2)) >> 1;
}

// EAC R11 unsigned of one channel (c4 as bu_bc4_block); out[0..1] = bytes 0..7.
//   t = (2047 v + 127) / 255 (= round(v 2047 / 255), no ties), mn = min t, mx = max t
//   solid (mn == mx): multiplier 0, table 13, base = min(mn >> 3, 255), values 8 base + 4 + mod[13][j]
//   else, for every table k: R = mod_max - mod_min; mult = min(15, ceil((mx - mn) / (8R))); base = min(255, floor((mn + mx + 8 mult) / 16));
//        values clamp(8 base + 4 + 8 mult mod[k][j], 0, 2047); E_k = sum over texels of (nearest value - t)^2; the smallest E_k wins, a tie
//        the lower k
//   nearest value: among equal distances the lower spec index j (both branches; bu_r11_ramp)
//   byte 0 = base, byte 1 = mult << 4 | table, bytes 2..7 the 48-bit selector string big-endian, pixel id = 4x + y at bits 45 - 3 id
//   (the layout of the ETC2 alpha half, bu_eac_block)
// Cost: the search is 16 tables x 16 texels x (7 threshold tests + select + squared error) -- about 16 VALU per texel and table, ~4.3k per
// channel and block.
BU_DEV void bu_r11_block(const BuTables& T, const uint32_t c4[4], uint32_t out[2])
{
    int t[16];
    BU_UNROLL
    for (int i = 0; i < 16; i++) t[i] = (int)((2047u * ((c4[i >> 2] >> (8 * (i & 3))) & 0xFFu) + 127u) / 255u);
    int mn = t[0], mx = t[0];
    BU_UNROLL
    for (int i = 1; i < 16; i++) {
        mn = mn < t[i] ? mn : t[i];
        mx = mx > t[i] ? mx : t[i];
    }
    uint32_t table = 13;
    int mult = 0, base = (mn >> 3) < 255 ? (mn >> 3) : 255;
    if (mn != mx) {
        const uint32_t span = (uint32_t)(mx - mn);
        uint32_t best = 0xFFFFFFFFu;
        BU_ROLLED
        for (uint32_t k = 0; k < 16; k++) {
            // ceil(span / 8R) = floor(floor((span + 8R - 1) / 4) / 2R); eac_magic = ceil(2^20 / 2R) divides exactly below 14791 (here <= 569)
            const uint32_t r8 = 8u * T.eac_range[k];
            const uint32_t m = (((span + r8 - 1u) >> 2) * T.eac_magic[k]) >> 20;
            const int mk = m < 15u ? (int)m : 15;
            const int bs = (mn + mx + 8 * mk) >> 4, bk = bs < 255 ? bs : 255;
            int val[8], thr[8];
            bu_r11_ramp(T, k, 8 * mk, bk, val, thr);
            uint32_t err = 0;
            BU_UNROLL
            for (int i = 0; i < 16; i++) {
                int s = val[0];
                BU_UNROLL
                for (int r = 1; r < 8; r++) s = t[i] >= thr[r] ? val[r] : s;
                const int e = s - t[i];
                err += (uint32_t)(e * e);
            }
            if (err < best) {
                best = err;
                table = k;
                mult = mk;
                base = bk;
            }
        }
    }
    int val[8], thr[8];
    bu_r11_ramp(T, table, mult ? 8 * mult : 1, base, val, thr);
    uint64_t sel = 0;  // the 48-bit selector string
    BU_UNROLL
    for (int id = 0; id < 16; id++) {
        const int i = 4 * (id & 3) + (id >> 2);  // id = 4x + y -> texel 4y + x
        int c = 0;
        BU_UNROLL
        for (int r = 1; r < 8; r++) c += t[i] >= thr[r] ? 1 : 0;
        const uint32_t j = c < 4 ? (uint32_t)(3 - c) : (uint32_t)c;
        sel |= (uint64_t)j << (45 - 3 * id);
    }
    const uint64_t be = ((uint64_t)base << 56) | ((uint64_t)((uint32_t)mult << 4 | table) << 48) | sel;  // the block as a big-endian number
    out[0] = __builtin_bswap32((uint32_t)(be >> 32));
    out[1] = __builtin_bswap32((uint32_t)be);
}

// out: BC4 / R11 -> out[0..1] (channel R); BC5 / RG11 -> out[0..1] R, out[2..3] A
template <int M, bool BC, bool TWO>
BU_DEV int bu_block_channels(const BuTables& T, const BuBlk& b, uint32_t out[4])
{
    uint32_t px[16];
    const int st = bu_block_rgba<M>(T, b, px);
    if (st) return st;
    // R and A of each block row in the bytes of one word: the 16 texel words are dead before the encoders run (RG11's
    // 1024 x 4 and 512 x 4 kernels spilled to scratch with them live across the R search)
    uint32_t r4[4], a4[4];
    BU_UNROLL
    for (int y = 0; y < 4; y++) {
        r4[y] = bu_perm(bu_perm(px[4 * y + 3], px[4 * y + 2], 0x0C0C0400u), bu_perm(px[4 * y + 1], px[4 * y], 0x0C0C0400u), 0x05040100u);
        a4[y] = bu_perm(bu_perm(px[4 * y + 3], px[4 * y + 2], 0x0C0C0703u), bu_perm(px[4 * y + 1], px[4 * y], 0x0C0C0703u), 0x05040100u);
    }
    if constexpr (BC) {
        bu_bc4_block(r4, out);
        if constexpr (TWO) bu_bc4_block(a4, out + 2);
    } else {
        bu_r11_block(T, r4, out);
        if constexpr (TWO) bu_r11_block(T, a4, out + 2);
    }
    return BU_ST_OK;
}
