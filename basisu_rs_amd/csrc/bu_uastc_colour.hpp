// UASTC -> BC1 / BC3 (the colour targets) for the gfx950 kernels.
// The reference has no such targets, so there is nothing to mirror: the encoder is the exact integer rule of DESIGN.md section 4.5
// (repeated beside the code below), pinned by the independent model of tests/colour_model.py, which a spec decoder pins in turn.
//   input  x_i = (R, G, B) of texel i (i = 4y + x) of what BU_TARGET_RGBA32 writes for the block: the block goes through the RGBA32
//          unpack (bu_block_rgba, the same front end and sink); A is read by BC3 only
//   BC1    8 bytes: w(c0), w(c1) little-endian, then 2-bit indices, texel i at bits 2i (four-colour mode, or w0 == w1 with every index 0)
//   BC3    BC4 of A (bu_bc4_block) then the BC1 block
// Every intermediate fits in 32 bits (the bounds are asserted by the model).
#pragma once
#include "bu_uastc_bc7.hpp"  // bu_byte
#include "bu_uastc_channel.hpp"

// 5/6/5 endpoints <-> 8 bits: e5(c) = c << 3 | c >> 2, e6(c) = c << 2 | c >> 4; q(v) = (m v + 127) / 255 with m = 31 / 63 / 31
BU_DEV int bu_bc1_e(int c, int ch) { return ch == 1 ? (c << 2) | (c >> 4) : (c << 3) | (c >> 2); }
BU_DEV int bu_bc1_q(int v, int ch) { return ((ch == 1 ? 63 : 31) * v + 127) / 255; }
BU_DEV uint32_t bu_bc1_word(const int c[3]) { return (uint32_t)(c[0] << 11 | c[1] << 5 | c[2]); }
BU_DEV uint32_t bu_uabs(int v) { return (uint32_t)(v < 0 ? -v : v); }
// number of significant bits of m >= 0 (m | 1: bitlen(0) reads as 1, which every caller clamps the same way)
BU_DEV int bu_bitlen(uint32_t m) { return 32 - __builtin_clz(m | 1u); }
// u >> max(0, bitlen(max_c |u_c|) - 13), an arithmetic shift: |u_c| <= 2^13 after it
BU_DEV void bu_bc1_norm(int u[3])
{
    const uint32_t m = bu_umax(bu_umax(bu_uabs(u[0]), bu_uabs(u[1])), bu_uabs(u[2]));
    const int sh = bu_bitlen(m) - 13;
    if (sh > 0) {
        BU_UNROLL
        for (int c = 0; c < 3; c++) u[c] >>= sh;
    }
}

// The texels stay packed (px[i]: byte c = channel c) through the whole encoder and every sum over them is a byte dot product
// (v_dot4_u32_u8): 16 words live instead of 48 bytes (the unpacked form took 164 VGPRs on its own and spilled in every kernel shape).
// The texel loops of the fit and of the least-squares sums stay rolled (px indexed by the uniform loop counter, no scratch): unrolled,
// their 16 independent texels were scheduled side by side and the encoder alone took 102 VGPRs -- 58 rolled.
// d = dp - dn with bytes dp, dn >= 0: x.d = dot4(x, dp) - dot4(x, dn) (byte 3 of both is 0, so A never counts)
BU_DEV uint32_t bu_bc1_pack(int a, int b, int c) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16; }

// Selectors and error of the endpoints c0, c1 (5/6/5 values).  The palette is kept in thirds: 3E0, 2E0 + E1, E0 + 2E1, 3E1.
//   d = E1 - E0, D = d.d, s_i = (x_i - E0).d, q_i = #{j in 1..3 : 6 s_i > (2j - 1) D} (a tie goes toward E0; D = 0: q_i = 0)
//   E = sum |3 x_i - (3 E0 + q_i d)|^2 = 9 X2 - 18 S.E0 + 144 E0.E0 - 6 sum q_i s_i + D sum q_i^2   (X2 = sum |x_i|^2, S = sum x_i; E < 48 * 765^2)
// q_i goes to bits 2i of `sel`; returns E.
BU_DEV uint32_t bu_bc1_fit(const uint32_t px[16], int X2, const int S[3], const int c0[3], const int c1[3], uint32_t& sel)
{
    int e0[3], d[3];
    BU_UNROLL
    for (int c = 0; c < 3; c++) {
        e0[c] = bu_bc1_e(c0[c], c);
        d[c] = bu_bc1_e(c1[c], c) - e0[c];
    }
    const int D = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const int D3 = 3 * D, D5 = 5 * D, e0d = e0[0] * d[0] + e0[1] * d[1] + e0[2] * d[2];
    const uint32_t dp = bu_bc1_pack(d[0] > 0 ? d[0] : 0, d[1] > 0 ? d[1] : 0, d[2] > 0 ? d[2] : 0);
    const uint32_t dn = bu_bc1_pack(d[0] < 0 ? -d[0] : 0, d[1] < 0 ? -d[1] : 0, d[2] < 0 ? -d[2] : 0);
    int qs = 0, qq = 0;
    sel = 0;
    BU_ROLLED
    for (int i = 0; i < 16; i++) {
        const int si = (int)bu_udot4(px[i], dp, 0u) - (int)bu_udot4(px[i], dn, 0u) - e0d;
        const int s6 = 6 * si;
        const int q = (s6 > D ? 1 : 0) + (s6 > D3 ? 1 : 0) + (s6 > D5 ? 1 : 0);
        qs += q * si;
        qq += q * q;
        sel |= (uint32_t)q << (2 * i);
    }
    const int se0 = S[0] * e0[0] + S[1] * e0[1] + S[2] * e0[2], e0e0 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
    return (uint32_t)(9 * X2 - 18 * se0 + 144 * e0e0 - 6 * qs + D * qq);
}

// BC1 of the RGB bytes of px[16] (texel words, byte c = channel c) -> out[0..1] = bytes 0..7.  The rule:
//   solid (all 16 RGB equal): per channel the pair (a, b) = BU_BC1_OM5 / OM6[v] (|2 e(a) + e(b) - 3v| least, tools/gen_tables.py);
//       c0 = a, c1 = b, every q = 1
//   else: covariance C of 16 x_i - S (S = sum x_i; |C| < 2^28), Cs = C >> max(0, bitlen(max |C|) - 16); v0 = norm(column k of Cs) for the
//       largest Cs_kk (first of R, G, B on a tie); v = norm(Cs v) four times (v = v0 if it ends at 0); H / L = the texels of largest /
//       smallest v.x_i (lowest i on a tie); c0 = q(H), c1 = q(L); then one least-squares pass on the weights a_i = 3 - q_i, b_i = q_i,
//       kept if its error is smaller
//   order: w(c0) < w(c1) swaps the endpoints (q -> 3 - q); w(c0) == w(c1) sets every q to 0; index = 0, 2, 3, 1 for q = 0, 1, 2, 3
// Cost: ~0.8k VALU on top of the unpack.
BU_DEV void bu_bc1_block(const uint32_t px[16], uint32_t out[2])
{
    const uint32_t rgb0 = px[0] & 0xFFFFFFu;
    bool solid = true;
    BU_UNROLL
    for (int i = 1; i < 16; i++) solid = solid && (px[i] & 0xFFFFFFu) == rgb0;
    int c0[3], c1[3];
    uint32_t sel;
    if (solid) {
        BU_UNROLL
        for (int c = 0; c < 3; c++) {
            const uint32_t ab = (c == 1 ? BU_BC1_OM6 : BU_BC1_OM5)[bu_byte(rgb0, c)];
            c0[c] = (int)(ab & 0xFFu);
            c1[c] = (int)(ab >> 8);
        }
        sel = 0x55555555u;
    } else {
        // S and P_ab = sum x_a x_b in one pass; then C = sum (16 x - S)(16 x - S)^T = 256 P - 16 S S^T (256 P < 2^28)
        int S[3] = {0, 0, 0}, P00 = 0, P01 = 0, P02 = 0, P11 = 0, P12 = 0, P22 = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) {
            const int r = (int)bu_byte(px[i], 0), g = (int)bu_byte(px[i], 1), b = (int)bu_byte(px[i], 2);
            S[0] += r;
            S[1] += g;
            S[2] += b;
            P00 += r * r;
            P01 += r * g;
            P02 += r * b;
            P11 += g * g;
            P12 += g * b;
            P22 += b * b;
        }
        const int X2 = P00 + P11 + P22;
        int C00 = 256 * P00 - 16 * S[0] * S[0], C01 = 256 * P01 - 16 * S[0] * S[1], C02 = 256 * P02 - 16 * S[0] * S[2];
        int C11 = 256 * P11 - 16 * S[1] * S[1], C12 = 256 * P12 - 16 * S[1] * S[2], C22 = 256 * P22 - 16 * S[2] * S[2];
        // max |C_ab| is the largest diagonal entry (|C_ab| <= sqrt(C_aa C_bb)), > 0 for a block that is not solid
        const int sh = bu_bitlen(bu_umax(bu_umax((uint32_t)C00, (uint32_t)C11), (uint32_t)C22)) - 16;
        if (sh > 0) {
            C00 >>= sh;
            C01 >>= sh;
            C02 >>= sh;
            C11 >>= sh;
            C12 >>= sh;
            C22 >>= sh;
        }
        int v0[3];
        if (C11 > C00 && C11 >= C22) v0[0] = C01, v0[1] = C11, v0[2] = C12;
        else if (C22 > C00 && C22 > C11) v0[0] = C02, v0[1] = C12, v0[2] = C22;
        else v0[0] = C00, v0[1] = C01, v0[2] = C02;
        bu_bc1_norm(v0);
        int v[3] = {v0[0], v0[1], v0[2]};
        BU_ROLLED
        for (int it = 0; it < 4; it++) {  // |Cs v| < 3 * 2^29
            int u[3] = {C00 * v[0] + C01 * v[1] + C02 * v[2], C01 * v[0] + C11 * v[1] + C12 * v[2], C02 * v[0] + C12 * v[1] + C22 * v[2]};
            bu_bc1_norm(u);
            v[0] = u[0], v[1] = u[1], v[2] = u[2];
        }
        if ((v[0] | v[1] | v[2]) == 0) v[0] = v0[0], v[1] = v0[1], v[2] = v0[2];
        // p_i = v.x_i with v_c in [-2^13, 2^13): v_c = 64 vh_c + vl_c, vh_c + 128 and vl_c bytes -> p_i = 64 (dot4(x, vh + 128) - 128 dot4(x, 1)) + dot4(x, vl)
        const uint32_t vh = bu_bc1_pack((v[0] >> 6) + 128, (v[1] >> 6) + 128, (v[2] >> 6) + 128), vl = bu_bc1_pack(v[0] & 63, v[1] & 63, v[2] & 63);
        // H / L by value as the texels go by (strict comparisons: the lowest i on a tie; no indexed register access)
        uint32_t wh = px[0], wl = px[0];
        int phi = 0, plo = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) {
            const int p = 64 * ((int)bu_udot4(px[i], vh, 0u) - 128 * (int)bu_udot4(px[i], 0x010101u, 0u)) + (int)bu_udot4(px[i], vl, 0u);
            if (i == 0 || p > phi) phi = p, wh = px[i];
            if (i == 0 || p < plo) plo = p, wl = px[i];
        }
        BU_UNROLL
        for (int c = 0; c < 3; c++) {
            c0[c] = bu_bc1_q((int)bu_byte(wh, c), c);
            c1[c] = bu_bc1_q((int)bu_byte(wl, c), c);
        }
        const uint32_t err = bu_bc1_fit(px, X2, S, c0, c1, sel);
        // least squares in thirds: minimise sum |3 x_i - a_i E0 - b_i E1|^2 -> E0 = NA / det, E1 = NB / det (det <= 20736).
        // Sbx = sum q_i x_i in 16-bit lanes (R | B << 16, and G << 8: every lane sum <= 48 * 255 < 2^16)
        int Sb = 0, Sbb = 0;
        uint32_t srb = 0, sg = 0;
        BU_ROLLED
        for (int i = 0; i < 16; i++) {
            const uint32_t q = (sel >> (2 * i)) & 3u;
            Sb += (int)q;
            Sbb += (int)(q * q);
            srb += q * (px[i] & 0x00FF00FFu);
            sg += q * (px[i] & 0x0000FF00u);
        }
        const int Sbx[3] = {(int)(srb & 0xFFFFu), (int)(sg >> 8), (int)(srb >> 16)};
        const int Saa = 144 - 6 * Sb + Sbb, Sab = 3 * Sb - Sbb;
        const int det = Saa * Sbb - Sab * Sab;
        if (det > 0) {
            int r0[3], r1[3];
            const int den = 510 * det;
            BU_UNROLL
            for (int c = 0; c < 3; c++) {
                const int m = c == 1 ? 63 : 31, Sax = 3 * S[c] - Sbx[c];
                const int na = 3 * (Sbb * Sax - Sab * Sbx[c]), nb = 3 * (Saa * Sbx[c] - Sab * Sax);
                // clamp(floor((2 m N + 255 det) / (510 det)), 0, m): a negative numerator clamps to 0 under floor and truncation alike
                const int ta = 2 * m * na + 255 * det, tb = 2 * m * nb + 255 * det;
                r0[c] = ta < 0 ? 0 : (int)bu_umin((uint32_t)ta / (uint32_t)den, (uint32_t)m);
                r1[c] = tb < 0 ? 0 : (int)bu_umin((uint32_t)tb / (uint32_t)den, (uint32_t)m);
            }
            uint32_t sel2;
            const uint32_t err2 = bu_bc1_fit(px, X2, S, r0, r1, sel2);
            if (err2 < err) {
                BU_UNROLL
                for (int c = 0; c < 3; c++) c0[c] = r0[c], c1[c] = r1[c];
                sel = sel2;
            }
        }
    }
    uint32_t w0 = bu_bc1_word(c0), w1 = bu_bc1_word(c1);
    if (w0 < w1) {
        const uint32_t t = w0;
        w0 = w1;
        w1 = t;
        sel = ~sel;  // q -> 3 - q in every 2-bit field
    }
    if (w0 == w1) sel = 0;
    // q = (h, l) -> index (h ^ l, h): 0 -> 0, 1 -> 2, 2 -> 3, 3 -> 1
    const uint32_t h = (sel >> 1) & 0x55555555u, l = sel & 0x55555555u;
    out[0] = w0 | (w1 << 16);
    out[1] = h | ((h ^ l) << 1);
}

// out: BC1 -> out[0..1]; BC3 -> out[0..1] BC4 of A, out[2..3] BC1
template <int M, bool BC3>
BU_DEV int bu_block_colour(const BuTables& T, const BuBlk& b, uint32_t out[4])
{
    uint32_t px[16];
    const int st = bu_block_rgba<M>(T, b, px);
    if (st) return st;
    if constexpr (BC3) {
        uint32_t a4[4];  // A of each block row in the bytes of one word (bu_block_channels)
        BU_UNROLL
        for (int y = 0; y < 4; y++) a4[y] = bu_perm(bu_perm(px[4 * y + 3], px[4 * y + 2], 0x0C0C0703u), bu_perm(px[4 * y + 1], px[4 * y], 0x0C0C0703u), 0x05040100u);
        bu_bc4_block(a4, out);
        bu_bc1_block(px, out + 2);
    } else {
        bu_bc1_block(px, out);
    }
    return BU_ST_OK;
}
