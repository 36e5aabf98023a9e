// Block DECODERS: ASTC 4x4 LDR, BC7, ETC1, ETC2 RGBA, BC1, BC3, BC4, BC5, EAC R11, EAC RG11 -> 16 RGBA8 texels (which is
// the contract: the rules there and this code change together).  For the gfx950 kernels (bu_decode_kernels.hpp) and, compiled for the host, for
// the CPU tests (tests/host_emul/bu_emul_decode_main.cpp).  Written from the format specifications (Khronos Data Format Specification: S3TC, RGTC,
// BPTC, ETC2 / EAC, ASTC LDR profile).
//   in   w[2] or w[4]: the block's bytes as little-endian words
//   out  px[16]: texel i = 4y + x as R | G << 8 | B << 16 | A << 24; a failing block leaves 16 zero words
//   returns BU_DEC_OK, BU_DEC_INVALID (a reserved or illegal encoding) or BU_DEC_UNSUPPORTED (a legal block outside the stated scope)
// BC7 and ASTC run ONE path for every mode: field widths and counts come out of small mode tables, every loop runs to a fixed bound and a
// field that a mode does not have is read with width 0, so a wave whose lanes hold blocks of different modes stays convergent.  The bit
// string is consumed from the low end by a shifting reader (four funnel shifts per field); endpoints, indices and weights stay packed in
// words and are picked by constant shifts -- nothing here indexes a register array with a per-lane value.
#pragma once
#include "bu_uastc_colour.hpp"

enum { BU_DEC_OK = 0, BU_DEC_INVALID = 1, BU_DEC_UNSUPPORTED = 17 };  // (= BU_OK, BU_ERR_INVALID_MODE, BU_ERR_UNSUPPORTED)

// what the decoders read of the table blob: on the device the LDS copies the kernel staged, on the host the blob itself
struct BuDecView {
    const BuDecTables* d;
    const int16_t* etc1_mod;  // BuTables::etc1_mod: [8][4], rising
    const int8_t* eac_mods;   // BuTables::eac_mods: [16][8], each table rising (specification entries 3, 2, 1, 0, 4, 5, 6, 7)
};

constexpr int bu_dec_block_words(int format) { return bu_out_words(format); }
constexpr bool bu_dec_format_ok(int format)
{
    return format == 0 || format == 1 || format == 2 || format == 3 || (format >= 6 && format <= 9) || format == 11 || format == 12;
}

BU_DEV void bu_dec_zero(uint32_t px[16])
{
    BU_UNROLL
    for (int i = 0; i < 16; i++) px[i] = 0;
}
BU_DEV uint32_t bu_dec_funnel(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (n & 31u)); }  // (v_alignbit_b32)
BU_DEV uint32_t bu_dec_brev(uint32_t v)  // (v_bfrev_b32)
{
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(v);
#endif
}
BU_DEV uint32_t bu_dec_clamp255(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
BU_DEV uint32_t bu_dec_rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | g << 8 | b << 16 | a << 24; }

// A bit string of up to 128 bits, consumed from bit 0 upwards: take(n), 0 <= n <= 31, returns the next n bits and drops them.
struct BuDecBits {
    uint32_t a, b, c, d;
    BU_DEVM uint32_t take(uint32_t n)
    {
        const uint32_t v = a & ((1u << n) - 1u);
        a = bu_dec_funnel(b, a, n);
        b = bu_dec_funnel(c, b, n);
        c = bu_dec_funnel(d, c, n);
        d >>= n;
        return v;
    }
};

// ---- BC1 / BC4 and what is built from them --------------------------------------------------------------------------------------
// RGB565 -> R | G << 8 | B << 16 by bit replication
BU_DEV uint32_t bu_dec_565(uint32_t w)
{
    const uint32_t r = w >> 11, g = (w >> 5) & 63u, b = w & 31u;
    return (r << 3 | r >> 2) | (g << 2 | g >> 4) << 8 | (b << 3 | b >> 2) << 16;
}
// (wa * a + wb * b) / den per byte of the three colour channels, round half up: (2 num + den) / (2 den)
BU_DEV uint32_t bu_dec_mix3(uint32_t a, uint32_t b, uint32_t wa, uint32_t wb, uint32_t den)
{
    uint32_t o = 0;
    BU_UNROLL
    for (int ch = 0; ch < 3; ch++) o |= ((2u * (wa * bu_byte(a, ch) + wb * bu_byte(b, ch)) + den) / (2u * den)) << (8 * ch);
    return o;
}
// the colour half of BC1 / BC3: FOUR = always the four-colour form (BC3); alpha goes into byte 3 of every texel (BC1: 255, code 3 of the
// three-colour form 0 with black)
template <bool FOUR>
BU_DEV void bu_dec_bc1_colour(uint32_t w0, uint32_t w1, uint32_t px[16])
{
    const uint32_t q0 = w0 & 0xFFFFu, q1 = w0 >> 16;
    const uint32_t c0 = bu_dec_565(q0), c1 = bu_dec_565(q1);
    const bool four = FOUR || q0 > q1;
    const uint32_t opaque = FOUR ? 0u : 0xFF000000u;
    const uint32_t p2 = (four ? bu_dec_mix3(c0, c1, 2, 1, 3) : bu_dec_mix3(c0, c1, 1, 1, 2)) | opaque;
    const uint32_t p3 = four ? bu_dec_mix3(c0, c1, 1, 2, 3) | opaque : 0u;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t code = (w1 >> (2 * i)) & 3u;
        px[i] = code == 0 ? (c0 | opaque) : code == 1 ? (c1 | opaque) : code == 2 ? p2 : p3;
    }
}
// BC4: the eight values of the ramp as bytes of a 64-bit word, then texel i's code at bits 3i of the 48-bit string; v[i] = the value
BU_DEV void bu_dec_bc4(uint32_t w0, uint32_t w1, uint32_t v[16])
{
    const uint32_t r0 = w0 & 255u, r1 = (w0 >> 8) & 255u;
    const bool eight = r0 > r1;
    uint64_t ramp = (uint64_t)r0 | (uint64_t)r1 << 8;
    BU_UNROLL
    for (uint32_t k = 2; k < 8; k++) {
        const uint32_t v8 = (2u * ((8u - k) * r0 + (k - 1u) * r1) + 7u) / 14u;
        const uint32_t v6 = k == 6 ? 0u : k == 7 ? 255u : (2u * ((6u - k) * r0 + (k - 1u) * r1) + 5u) / 10u;
        ramp |= (uint64_t)(eight ? v8 : v6) << (8 * k);
    }
    const uint64_t codes = (uint64_t)(w0 >> 16) | (uint64_t)w1 << 16;
    BU_UNROLL
    for (int i = 0; i < 16; i++) v[i] = (uint32_t)(ramp >> (8u * ((uint32_t)(codes >> (3 * i)) & 7u))) & 255u;
}

// ---- EAC ---------------------------------------------------------------------------------------------------------------------------
// One 8-byte EAC block: R11 = false the 8-bit alpha of ETC2 (clamp(base + mult * mod)), R11 = true the unsigned 11-bit value scaled to a
// byte, (255 t + 1023) / 2047.  Selectors: texel (x, y) is pixel 4x + y at bits 45 - 3 (4x + y) of the big-endian 48-bit string.
template <bool R11>
BU_DEV void bu_dec_eac(const BuDecView& V, uint32_t w0, uint32_t w1, uint32_t v[16])
{
    const uint32_t base = w0 & 255u, mult = (w0 >> 12) & 15u, table = (w0 >> 8) & 15u;
    uint32_t m2[2];
    __builtin_memcpy(m2, V.eac_mods + 8 * table, 8);
    const uint64_t mods = (uint64_t)m2[0] | (uint64_t)m2[1] << 32;  // rising: byte k = specification entry k < 4 ? 3 - k : k
    const uint64_t sel = (uint64_t)(__builtin_bswap32(w0) & 0xFFFFu) << 32 | __builtin_bswap32(w1);
    const int scale = R11 ? (mult ? 8 * (int)mult : 1) : (int)mult;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const int p = 4 * (i & 3) + (i >> 2);
        const uint32_t j = (uint32_t)(sel >> (45 - 3 * p)) & 7u, k = j < 4u ? 3u - j : j;
        const int mod = (int)(int8_t)(uint8_t)(mods >> (8u * k));
        if (R11) {
            const int t = 8 * (int)base + 4 + scale * mod;
            v[i] = (255u * (uint32_t)(t < 0 ? 0 : t > 2047 ? 2047 : t) + 1023u) / 2047u;
        } else {
            v[i] = bu_dec_clamp255((int)base + scale * mod);
        }
    }
}

// ---- ETC1 (and the colour half of ETC2 RGBA) ------------------------------------------------------------------------------------------------
// Individual and differential blocks; a differential block whose second base colour leaves 0..31 is an ETC2 T / H / planar block:
// BU_DEC_UNSUPPORTED, px untouched.  Alpha 255; the ETC2 caller replaces it.
BU_DEV int bu_dec_etc1_colour(const BuDecView& V, uint32_t w0, uint32_t w1, uint32_t px[16])
{
    const bool diff = (w0 >> 25) & 1u, flip = (w0 >> 24) & 1u;
    const uint32_t t0 = (w0 >> 29) & 7u, t1 = (w0 >> 26) & 7u;
    int c0[3], c1[3];
    bool over = false;
    BU_UNROLL
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t byte = bu_byte(w0, ch);
        const int a5 = (int)(byte >> 3), b5 = a5 + ((int)((byte & 7u) ^ 4u) - 4);  // 3-bit two's complement
        over = over || b5 < 0 || b5 > 31;
        const uint32_t ub = (uint32_t)b5 & 31u;
        c0[ch] = diff ? (int)((uint32_t)a5 << 3 | (uint32_t)a5 >> 2) : (int)((byte >> 4) * 17u);
        c1[ch] = diff ? (int)(ub << 3 | ub >> 2) : (int)((byte & 15u) * 17u);
    }
    if (diff && over) return BU_DEC_UNSUPPORTED;
    // the two intensity rows: magnitudes a < b at entries 2 and 3
    const int a0 = V.etc1_mod[4 * t0 + 2], b0 = V.etc1_mod[4 * t0 + 3], a1 = V.etc1_mod[4 * t1 + 2], b1 = V.etc1_mod[4 * t1 + 3];
    const uint32_t msb = __builtin_bswap32(w1) >> 16, lsb = __builtin_bswap32(w1) & 0xFFFFu;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const int x = i & 3, y = i >> 2, p = 4 * x + y;
        const bool second = flip ? y >= 2 : x >= 2;
        const bool large = (lsb >> p) & 1u, neg = (msb >> p) & 1u;
        const int mag = second ? (large ? b1 : a1) : (large ? b0 : a0), mod = neg ? -mag : mag;
        px[i] = bu_dec_rgba(bu_dec_clamp255((second ? c1[0] : c0[0]) + mod), bu_dec_clamp255((second ? c1[1] : c0[1]) + mod),
                            bu_dec_clamp255((second ? c1[2] : c0[2]) + mod), 255u);
    }
    return BU_DEC_OK;
}

// ---- BC7 -----------------------------------------------------------------------------------------------------------------------------------
// The mode table: one nibble per mode, mode 0 lowest.
//   subsets, partition bits, rotation bits, colour bits, alpha bits, endpoint p-bits, shared p-bits, index bits, second index bits
constexpr uint32_t BU_BC7_NS = 0x21112323u, BU_BC7_PB = 0x60006664u, BU_BC7_RB = 0x00220000u, BU_BC7_CB = 0x57757564u, BU_BC7_AB = 0x57860000u,
                   BU_BC7_EPB = 0x11001001u, BU_BC7_SPB = 0x00000010u, BU_BC7_IB = 0x24222233u, BU_BC7_IB2 = 0x00230000u;

BU_DEV int bu_dec_bc7(const BuDecView& V, const uint32_t w[4], uint32_t px[16])
{
    if ((w[0] & 255u) == 0) return BU_DEC_INVALID;
    const uint32_t mode = (uint32_t)__builtin_ctz(w[0] & 255u), sh = 4u * mode;
    const uint32_t ns = (BU_BC7_NS >> sh) & 15u, cb = (BU_BC7_CB >> sh) & 15u, ab = (BU_BC7_AB >> sh) & 15u, epb = (BU_BC7_EPB >> sh) & 1u,
                   spb = (BU_BC7_SPB >> sh) & 1u, ib = (BU_BC7_IB >> sh) & 15u, ib2 = (BU_BC7_IB2 >> sh) & 15u;
    BuDecBits r = {w[0], w[1], w[2], w[3]};
    (void)r.take(mode + 1u);
    const uint32_t part = r.take((BU_BC7_PB >> sh) & 15u), rot = r.take((BU_BC7_RB >> sh) & 15u), isel = r.take(mode == 4u ? 1u : 0u);
    // endpoints: all R, all G, all B, all A; endpoint e of subset s = ep[2s + e], one byte per channel
    uint32_t ep[6] = {0, 0, 0, 0, 0, 0};
    BU_UNROLL
    for (int ch = 0; ch < 4; ch++) {
        BU_UNROLL
        for (uint32_t e = 0; e < 6; e++) ep[e] |= r.take(e < 2u * ns ? (ch < 3 ? cb : ab) : 0u) << (8 * ch);
    }
    // p-bits: one per endpoint, or one per subset (mode 1)
    uint32_t pbit[6];
    BU_UNROLL
    for (uint32_t e = 0; e < 6; e++) {
        const uint32_t own = r.take(e < 2u * ns && (epb || (spb && !(e & 1u))) ? 1u : 0u);
        pbit[e] = (e & 1u) && spb ? pbit[e & ~1u] : own;  // (the subset's first endpoint)
    }
    const uint32_t hasp = epb | spb, cprec = cb + hasp, aprec = ab ? ab + hasp : 8u;
    BU_UNROLL
    for (uint32_t e = 0; e < 6; e++) {
        uint32_t o = 0;
        BU_UNROLL
        for (int ch = 0; ch < 4; ch++) {
            const uint32_t prec = ch < 3 ? cprec : aprec;
            uint32_t v = bu_byte(ep[e], ch);
            if (ch == 3 && ab == 0) v = 255u;
            else if (hasp) v = v << 1 | pbit[e];
            o |= (((v << (8u - prec)) | (v >> (2u * prec - 8u))) & 255u) << (8 * ch);
        }
        ep[e] = o;
    }
    // the partition's subsets and anchors
    const BuU2 pr = V.d->bc7_part[(ns == 3u ? 64u : 0u) + part];
    const uint32_t pat = ns == 1u ? 0u : pr.x, anchor1 = ns >= 2u ? pr.y & 15u : 16u, anchor2 = ns == 3u ? pr.y >> 4 : 16u;
    // index bits: the anchors of the subsets lose their top bit; 4 bits per texel in i1 / i2
    uint64_t i1 = 0, i2 = 0;
    BU_UNROLL
    for (uint32_t i = 0; i < 16; i++) i1 |= (uint64_t)r.take(ib - (i == 0 || i == anchor1 || i == anchor2 ? 1u : 0u)) << (4 * i);
    BU_UNROLL
    for (uint32_t i = 0; i < 16; i++) i2 |= (uint64_t)r.take(ib2 ? ib2 - (i == 0 ? 1u : 0u) : 0u) << (4 * i);
    // which index and how many bits the colour and the alpha channel read
    const bool two = ib2 != 0, swap = two && isel;
    const uint64_t ci = swap ? i2 : i1, ai = two && !swap ? i2 : i1;
    const uint32_t cofs = (1u << (swap ? ib2 : ib)) - 4u, aofs = (1u << (two && !swap ? ib2 : ib)) - 4u;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t s = (pat >> (2 * i)) & 3u;
        const uint32_t e0 = s == 0 ? ep[0] : s == 1 ? ep[2] : ep[4], e1 = s == 0 ? ep[1] : s == 1 ? ep[3] : ep[5];
        const uint32_t wc = V.d->bc7_w[cofs + ((uint32_t)(ci >> (4 * i)) & 15u)], wa = V.d->bc7_w[aofs + ((uint32_t)(ai >> (4 * i)) & 15u)];
        uint32_t c[4];
        BU_UNROLL
        for (int ch = 0; ch < 4; ch++) {
            const uint32_t wt = ch < 3 ? wc : wa;
            c[ch] = (bu_byte(e0, ch) * (64u - wt) + bu_byte(e1, ch) * wt + 32u) >> 6;
        }
        const uint32_t a = c[3];  // rotation: alpha swapped with R, G or B
        px[i] = bu_dec_rgba(rot == 1u ? a : c[0], rot == 2u ? a : c[1], rot == 3u ? a : c[2], rot == 0u ? a : rot == 1u ? c[0] : rot == 2u ? c[1] : c[2]);
    }
    return BU_DEC_OK;
}

// ---- ASTC 4x4 LDR -------------------------------------------------------------------------------------------------------------------------
// bits the integer sequence of n values of range (bits, trits, quints) takes
BU_DEV uint32_t bu_astc_ise_bits(uint32_t n, uint32_t bits, uint32_t trits, uint32_t quints)
{
    return n * bits + (trits ? (8u * n + 4u) / 5u : 0u) + (quints ? (7u * n + 2u) / 3u : 0u);
}

// Reads the integer sequence of n <= N values of range rng (astc_rng's byte) off `r` and unquantises each through tab[ofs + (digit << bits |
// bit value)]: out = the N bytes, value i in byte i & 3 of word i >> 2 (bytes past n: some entry of the table).  A trit block's T bits follow its five
// values in pieces of 2, 2, 1, 2, 1 bits, a quint block's Q bits in pieces of 3, 2, 2; a last block that is cut short reads the missing bits
// as zero.  Both block shapes are gathered whatever the range is (pieces of width 0 for the other one).
template <int N>
BU_DEV void bu_astc_ise(const BuDecView& V, BuDecBits& r, uint32_t n, uint32_t rng, const uint8_t* tab, uint32_t ofs, uint32_t (&out)[(N + 3) / 4])
{
    constexpr int NT = (N + 4) / 5, NQ = (N + 2) / 3;
    constexpr uint32_t TB[5] = {2, 2, 1, 2, 1}, TP[5] = {0, 2, 4, 5, 7}, QB[3] = {3, 2, 2}, QP[3] = {0, 3, 5};
    const uint32_t bits = rng & 15u;
    const bool tr = (rng >> 4) & 1u, qu = (rng >> 5) & 1u;
    uint32_t m[(N + 3) / 4], T[NT], Q[NQ];
    BU_UNROLL
    for (int i = 0; i < (N + 3) / 4; i++) m[i] = 0;
    BU_UNROLL
    for (int i = 0; i < NT; i++) T[i] = 0;
    BU_UNROLL
    for (int i = 0; i < NQ; i++) Q[i] = 0;
    BU_UNROLL
    for (int i = 0; i < N; i++) {
        const bool on = (uint32_t)i < n;
        m[i / 4] |= r.take(on ? bits : 0u) << (8 * (i % 4));
        const uint32_t e = r.take(on ? (tr ? TB[i % 5] : qu ? QB[i % 3] : 0u) : 0u);
        T[i / 5] |= (tr ? e : 0u) << TP[i % 5];
        Q[i / 3] |= (qu ? e : 0u) << QP[i % 3];
    }
    BU_UNROLL
    for (int i = 0; i < NT; i++) T[i] = tr ? V.d->astc_trit[T[i] & 255u] : 0u;
    BU_UNROLL
    for (int i = 0; i < NQ; i++) Q[i] = qu ? V.d->astc_quint[Q[i] & 127u] : 0u;
    BU_UNROLL
    for (int i = 0; i < (N + 3) / 4; i++) out[i] = 0;
    BU_UNROLL
    for (int i = 0; i < N; i++) {
        const uint32_t digit = ((T[i / 5] >> (2 * (i % 5))) & 3u) | ((Q[i / 3] >> (3 * (i % 3))) & 7u);  // (at most one of them is not zero)
        out[i / 4] |= (uint32_t)tab[ofs + ((digit << bits) | bu_byte(m[i / 4], i % 4))] << (8 * (i % 4));
    }
}

// the specification's partition hash
BU_DEV uint32_t bu_astc_hash52(uint32_t p)
{
    p ^= p >> 15;
    p -= p << 17;
    p += p << 7;
    p += p << 4;
    p ^= p >> 5;
    p += p << 16;
    p ^= p >> 7;
    p ^= p >> 3;
    p ^= p << 6;
    p ^= p >> 17;
    return p;
}

BU_DEV int bu_dec_astc(const BuDecView& V, const uint32_t w[4], uint32_t px[16])
{
    const uint32_t mode = w[0] & 0x7FFu;
    if ((mode & 0x1FFu) == 0x1FCu) {  // void extent: a constant colour, UNORM16 -> the top byte
        if (mode & 0x200u) return BU_DEC_UNSUPPORTED;  // HDR
        if (((w[0] >> 10) & 3u) != 3u) return BU_DEC_INVALID;
        // the extent, four 13-bit coordinates from bit 12: all ones = none; otherwise low < high on s and on t
        const uint32_t s_lo = (w[0] >> 12) & 0x1FFFu, s_hi = (w[0] >> 25 | w[1] << 7) & 0x1FFFu, t_lo = (w[1] >> 6) & 0x1FFFu, t_hi = w[1] >> 19;
        if ((s_lo & s_hi & t_lo & t_hi) != 0x1FFFu && (s_lo >= s_hi || t_lo >= t_hi)) return BU_DEC_INVALID;
        const uint32_t c = bu_dec_rgba((w[2] >> 8) & 255u, w[2] >> 24, (w[3] >> 8) & 255u, w[3] >> 24);
        BU_UNROLL
        for (int i = 0; i < 16; i++) px[i] = c;
        return BU_DEC_OK;
    }
    // block mode: only the layout with a 4-wide, 4-high weight grid is in scope (bits 2..3 = 0, A = 2, B = 0)
    if ((mode & 15u) == 0) return BU_DEC_INVALID;
    if ((mode & 3u) == 0) return ((mode >> 6) & 7u) == 7u ? BU_DEC_INVALID : BU_DEC_UNSUPPORTED;  // bits 6..8 all set: reserved (void extent left above)
    if (((mode >> 2) & 3u) != 0 || ((mode >> 5) & 3u) != 2u || ((mode >> 7) & 3u) != 0) return BU_DEC_UNSUPPORTED;
    const uint32_t R = ((mode >> 4) & 1u) | (mode & 3u) << 1, hp = (mode >> 9) & 1u, dual = (mode >> 10) & 1u;
    if (R < 2u) return BU_DEC_INVALID;
    const uint32_t wrng_i = (hp ? 6u : 0u) + R - 2u, wrng = V.d->astc_rng[wrng_i];
    const uint32_t n_weights = dual ? 32u : 16u, wbits = bu_astc_ise_bits(n_weights, wrng & 15u, (wrng >> 4) & 1u, (wrng >> 5) & 1u);
    if (wbits < 24u || wbits > 96u) return BU_DEC_INVALID;
    BuDecBits r = {w[0], w[1], w[2], w[3]};
    (void)r.take(11);
    const uint32_t parts = r.take(2) + 1u;
    if (dual && parts == 4u) return BU_DEC_INVALID;
    const bool multi = parts > 1u;
    const uint32_t seed = r.take(multi ? 10u : 0u), cem_sel = r.take(multi ? 2u : 0u), cem = r.take(4);
    if (cem_sel != 0) return BU_DEC_UNSUPPORTED;  // one endpoint mode per partition
    if (cem & 3u) return BU_DEC_UNSUPPORTED;      // modes 0 (L), 4 (LA), 8 (RGB), 12 (RGBA) only
    const uint32_t vpp = (cem >> 1) + 2u, n_vals = vpp * parts;  // values per partition: 2, 4, 6, 8
    if (n_vals > 18u) return BU_DEC_INVALID;
    // the colour range: the largest whose sequence fits the bits between the header and the weights (and the plane selector)
    const uint32_t avail = 128u - wbits - (multi ? 29u : 17u) - (dual ? 2u : 0u);
    int crng_i = -1;
    BU_UNROLL
    for (int i = 0; i < 21; i++)
        if (bu_astc_ise_bits(n_vals, BU_BISE[i].bits, BU_BISE[i].trits, BU_BISE[i].quints) <= avail) crng_i = i;
    if (crng_i < 4) return BU_DEC_INVALID;  // fewer than 6 levels
    uint32_t cv[5];
    bu_astc_ise<18>(V, r, n_vals, V.d->astc_rng[crng_i], V.d->astc_cdeq, V.d->astc_cofs[crng_i], cv);
    // the weights run down from bit 127: the block reversed bit for bit, read upwards; the plane selector follows them
    BuDecBits rw = {bu_dec_brev(w[3]), bu_dec_brev(w[2]), bu_dec_brev(w[1]), bu_dec_brev(w[0])};
    uint32_t wv[8];
    bu_astc_ise<32>(V, rw, n_weights, wrng, V.d->astc_wdeq, V.d->astc_wofs[wrng_i], wv);
    const uint32_t ccs_rev = rw.take(dual ? 2u : 0u), ccs = dual ? ((ccs_rev & 1u) << 1 | ccs_rev >> 1) : 4u;
    // endpoints of partition p: its vpp values are the low bytes of the value string, which then moves down by vpp bytes
    uint32_t e0[4], e1[4];
    BU_UNROLL
    for (int p = 0; p < 4; p++) {
        uint32_t v[8];
        BU_UNROLL
        for (int i = 0; i < 8; i++) v[i] = bu_byte(cv[i / 4], i % 4);
        const bool lum = cem < 8u;
        uint32_t r0 = v[0], r1 = v[1], g0 = lum ? v[0] : v[2], g1 = lum ? v[1] : v[3], b0 = lum ? v[0] : v[4], b1 = lum ? v[1] : v[5];
        uint32_t a0 = cem == 4u ? v[2] : cem == 12u ? v[6] : 255u, a1 = cem == 4u ? v[3] : cem == 12u ? v[7] : 255u;
        if (!lum && v[1] + v[3] + v[5] < v[0] + v[2] + v[4]) {  // blue contraction, endpoints swapped
            const uint32_t tr0 = r0, tg0 = g0, tb0 = b0, ta0 = a0;
            r0 = (r1 + b1) >> 1, g0 = (g1 + b1) >> 1, b0 = b1, a0 = a1;
            r1 = (tr0 + tb0) >> 1, g1 = (tg0 + tb0) >> 1, b1 = tb0, a1 = ta0;
        }
        e0[p] = bu_dec_rgba(r0, g0, b0, a0);
        e1[p] = bu_dec_rgba(r1, g1, b1, a1);
        // shift the value string down by vpp = 2, 4, 6 or 8 bytes
        if (vpp & 2u) cv[0] = cv[0] >> 16 | cv[1] << 16, cv[1] = cv[1] >> 16 | cv[2] << 16, cv[2] = cv[2] >> 16 | cv[3] << 16, cv[3] = cv[3] >> 16 | cv[4] << 16, cv[4] >>= 16;
        if (vpp & 4u) cv[0] = cv[1], cv[1] = cv[2], cv[2] = cv[3], cv[3] = cv[4], cv[4] = 0;
        if (vpp & 8u) cv[0] = cv[2], cv[1] = cv[3], cv[2] = cv[4], cv[3] = 0, cv[4] = 0;
    }
    // the partition function of a block of fewer than 31 texels (coordinates doubled)
    const uint32_t pseed = seed + (parts - 1u) * 1024u, rnum = bu_astc_hash52(pseed);
    uint32_t sd[8];
    {
        const uint32_t sh1 = (pseed & 1u) ? ((pseed & 2u) ? 4u : 5u) : (parts == 3u ? 6u : 5u);
        const uint32_t sh2 = (pseed & 1u) ? (parts == 3u ? 6u : 5u) : ((pseed & 2u) ? 4u : 5u);
        BU_UNROLL
        for (int k = 0; k < 8; k++) {
            const uint32_t s = (rnum >> (4 * k)) & 15u;
            sd[k] = (s * s) >> ((k & 1) ? sh2 : sh1);
        }
    }
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t x = 2u * (uint32_t)(i & 3), y = 2u * (uint32_t)(i >> 2);
        const uint32_t a = (sd[0] * x + sd[1] * y + (rnum >> 14)) & 63u;
        uint32_t b = (sd[2] * x + sd[3] * y + (rnum >> 10)) & 63u, c = (sd[4] * x + sd[5] * y + (rnum >> 6)) & 63u, d = (sd[6] * x + sd[7] * y + (rnum >> 2)) & 63u;
        if (parts < 4u) d = 0;
        if (parts < 3u) c = 0;
        if (parts < 2u) b = 0;
        const uint32_t p = !multi ? 0u : (a >= b && a >= c && a >= d) ? 0u : (b >= c && b >= d) ? 1u : c >= d ? 2u : 3u;
        const uint32_t c0 = p == 0 ? e0[0] : p == 1 ? e0[1] : p == 2 ? e0[2] : e0[3], c1 = p == 0 ? e1[0] : p == 1 ? e1[1] : p == 2 ? e1[2] : e1[3];
        // weights: one plane = byte i of the weight string, two planes = bytes 2i (first) and 2i + 1 (second)
        const uint32_t w0 = dual ? bu_byte(wv[(2 * i) / 4], (2 * i) % 4) : bu_byte(wv[i / 4], i % 4);
        const uint32_t w1 = dual ? bu_byte(wv[(2 * i + 1) / 4], (2 * i + 1) % 4) : w0;
        uint32_t o = 0;
        BU_UNROLL
        for (uint32_t ch = 0; ch < 4; ch++) {
            const uint32_t wt = ch == ccs ? w1 : w0;
            const uint32_t v0 = bu_byte(c0, (int)ch) * 257u, v1 = bu_byte(c1, (int)ch) * 257u;
            o |= (((v0 * (64u - wt) + v1 * wt + 32u) >> 6) >> 8) << (8 * ch);
        }
        px[i] = o;
    }
    return BU_DEC_OK;
}

// ---- one block of FORMAT (a bu_target value) ---------------------------------------------------------------------------------------------
// w: bu_dec_block_words(FORMAT) words.  Returns the status; px = the 16 texels, all zero unless the status is BU_DEC_OK.
template <int FORMAT>
BU_DEV int bu_decode_block(const BuDecView& V, const uint32_t* w, uint32_t px[16])
{
    static_assert(bu_dec_format_ok(FORMAT), "one of the ten block formats");
    int st = BU_DEC_OK;
    if constexpr (FORMAT == 0) {
        st = bu_dec_astc(V, w, px);
    } else if constexpr (FORMAT == 1) {
        st = bu_dec_bc7(V, w, px);
    } else if constexpr (FORMAT == 2) {
        st = bu_dec_etc1_colour(V, w[0], w[1], px);
    } else if constexpr (FORMAT == 3) {
        st = bu_dec_etc1_colour(V, w[2], w[3], px);
        if (st == BU_DEC_OK) {
            uint32_t a[16];
            bu_dec_eac<false>(V, w[0], w[1], a);
            BU_UNROLL
            for (int i = 0; i < 16; i++) px[i] = (px[i] & 0x00FFFFFFu) | a[i] << 24;
        }
    } else if constexpr (FORMAT == 11) {
        bu_dec_bc1_colour<false>(w[0], w[1], px);
    } else if constexpr (FORMAT == 12) {
        uint32_t a[16];
        bu_dec_bc4(w[0], w[1], a);
        bu_dec_bc1_colour<true>(w[2], w[3], px);
        BU_UNROLL
        for (int i = 0; i < 16; i++) px[i] |= a[i] << 24;
    } else {
        constexpr bool BC = FORMAT == 6 || FORMAT == 7, TWO = FORMAT == 7 || FORMAT == 9;
        uint32_t x[16], y[16];
        if constexpr (BC) bu_dec_bc4(w[0], w[1], x);
        else bu_dec_eac<true>(V, w[0], w[1], x);
        if constexpr (TWO) {
            if constexpr (BC) bu_dec_bc4(w[2], w[3], y);
            else bu_dec_eac<true>(V, w[2], w[3], y);
        }
        BU_UNROLL
        for (int i = 0; i < 16; i++) px[i] = bu_dec_rgba(x[i], TWO ? y[i] : 0u, 0u, 255u);
    }
    if (st != BU_DEC_OK) bu_dec_zero(px);
    return st;
}
