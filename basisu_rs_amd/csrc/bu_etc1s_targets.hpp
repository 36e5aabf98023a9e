// The per-block code of the ETC1S back end for the gfx950 kernels (bu_etc1s_kernels.hpp) and, compiled for the host, for the CPU tests
// (tests/host_emul/bu_emul_etc1s.cpp): ETC1S -> BC1 / BC3 / BC4 / BC5 / EAC R11 / EAC RG11 in palette form and,
// at the end, the pieces every ETC1S kernel shares -- palettes, index split and check, the ETC1 block, the RGBA32 block.
// The output of every target is the rule of DESIGN.md section 4.4 / 4.5 applied to the block that BU_TARGET_RGBA32 decodes
// (bu_etc1s_block_rgba): the 16-texel encoders of bu_uastc_channel.hpp / bu_uastc_colour.hpp, bit for bit.  An ETC1S block holds
// at most four colours -- one etc1s_pal word per channel, byte s = the value of selector s -- and a 2-bit selector per texel, texel
// i = 4y + x at bits 2i of the selector entry's `rows` word (bits 8y + 2x: BC1's index layout).  Every sum of the rules is over
// texels, so it becomes a sum over the four selectors weighted by n_s, the number of texels with selector s; every extreme and every
// tie that is decided by "the lowest texel" is decided by f_s, the lowest texel with selector s.  Unused selectors (n_s = 0) count
// nowhere.  The integers are those of the 16-texel rules, so the bytes are too (tests/test_etc1s_targets.py).
//   input  pr, pg, pb   etc1s_pal words of the colour endpoint's R, G, B;  rows  its selector entry's texel rows
//          pa, arows    the alpha endpoint's G palette word and the alpha selector rows (A); no alpha slice: A = 255 everywhere
//   BC4 / R11 of R, BC5 / RG11 = R then A, BC1 of RGB, BC3 = BC4 of A then BC1 (the layouts of sections 4.4 and 4.5)
#pragma once
#include "bu_uastc_colour.hpp"

// m[s]: bit 2i set <=> texel i has selector s (a field equal to s xors to 0 against s * 0x55555555)
BU_DEV void bu_etc1s_masks(uint32_t rows, uint32_t m[4])
{
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        const uint32_t x = rows ^ (0x55555555u * (uint32_t)s);
        m[s] = ~(x | (x >> 1)) & 0x55555555u;
    }
}

// BC4 of one palette channel (bu_bc4_block's rule): mn / mx over the used values, each selector's code once, then texel i's code at
// bits 3i of the 48-bit string.  An unused entry gets a code too (its unsigned 14 (v - mn) may wrap); no texel reads it.
BU_DEV void bu_etc1s_bc4(uint32_t p, uint32_t rows, const uint32_t m[4], uint32_t out[2])
{
    uint32_t mn = 255, mx = 0;
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        if (m[s]) {
            mn = bu_umin(mn, bu_byte(p, s));
            mx = bu_umax(mx, bu_byte(p, s));
        }
    }
    const uint32_t d = mx - mn;
    uint32_t codes = 0;  // selector s's code at bits 3s
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        const uint32_t e = 14u * (bu_byte(p, s) - mn);
        uint32_t q = 0;
        BU_UNROLL
        for (uint32_t j = 1; j <= 7; j++) q += e >= (2u * j - 1u) * d ? 1u : 0u;
        codes |= ((0x02345671u >> (4 * q)) & 7u) << (3 * s);
    }
    uint32_t lo = 0, hi = 0;  // bits 0..23 / 24..47 of the selector string
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t code = (codes >> (3 * ((rows >> (2 * i)) & 3u))) & 7u;
        if (i < 8) lo |= code << (3 * i);
        else hi |= code << (3 * (i - 8));
    }
    out[0] = mx | (mn << 8) | (lo << 16);
    out[1] = (lo >> 16) | (hi << 8);
}

// EAC R11 of one palette channel (bu_r11_block's rule): t_s per selector, mn / mx over the used ones, the 16-table search over at
// most four values with E_k = sum n_s (nearest - t_s)^2 (the same sum as over texels), then selector s's index once and texel
// i's index at the column-major big-endian position of section 4.4.
BU_DEV void bu_etc1s_r11(const BuTables& T, uint32_t p, uint32_t rows, const uint32_t m[4], uint32_t out[2])
{
    int t[4], n[4];
    int mn = 2047, mx = 0;
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        t[s] = (int)((2047u * bu_byte(p, s) + 127u) / 255u);
        n[s] = (int)bu_popc(m[s]);
        if (m[s]) {
            mn = mn < t[s] ? mn : t[s];
            mx = mx > t[s] ? mx : t[s];
        }
    }
    uint32_t table = 13;
    int mult = 0, base = (mn >> 3) < 255 ? (mn >> 3) : 255;
    if (mn != mx) {
        const uint32_t span = (uint32_t)(mx - mn);
        uint32_t best = 0xFFFFFFFFu;
        BU_ROLLED
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t r8 = 8u * T.eac_range[k];
            const uint32_t mm = (((span + r8 - 1u) >> 2) * T.eac_magic[k]) >> 20;
            const int mk = mm < 15u ? (int)mm : 15;
            const int bs = (mn + mx + 8 * mk) >> 4, bk = bs < 255 ? bs : 255;
            int val[8], thr[8];
            bu_r11_ramp(T, k, 8 * mk, bk, val, thr);
            uint32_t err = 0;
            BU_UNROLL
            for (int s = 0; s < 4; s++) {
                int v = val[0];
                BU_UNROLL
                for (int r = 1; r < 8; r++) v = t[s] >= thr[r] ? val[r] : v;
                const int e = v - t[s];
                err += (uint32_t)(n[s] * e * e);
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
    uint32_t js = 0;  // selector s's spec index j at bits 3s
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        int c = 0;
        BU_UNROLL
        for (int r = 1; r < 8; r++) c += t[s] >= thr[r] ? 1 : 0;
        js |= (c < 4 ? (uint32_t)(3 - c) : (uint32_t)c) << (3 * s);
    }
    uint64_t sel = 0;
    BU_UNROLL
    for (int id = 0; id < 16; id++) {
        const int i = 4 * (id & 3) + (id >> 2);  // id = 4x + y -> texel 4y + x
        sel |= (uint64_t)((js >> (3 * ((rows >> (2 * i)) & 3u))) & 7u) << (45 - 3 * id);
    }
    const uint64_t be = ((uint64_t)base << 56) | ((uint64_t)((uint32_t)mult << 4 | table) << 48) | sel;
    out[0] = __builtin_bswap32((uint32_t)(be >> 32));
    out[1] = __builtin_bswap32((uint32_t)be);
}

// The A channel of a block without an alpha slice is a solid 255: BC4 = {255, 255, codes 0}; R11 = base 255, multiplier 0,
// table 13, every index 7 (t = 2047: the value 8 * 255 + 4 + 9 clamps to 2047, an exact hit).
constexpr uint32_t BU_BC4_SOLID255[2] = {0x0000FFFFu, 0x00000000u};
constexpr uint32_t BU_R11_SOLID255[2] = {0xFFFF0DFFu, 0xFFFFFFFFu};

// Selectors and error of the endpoints c0, c1 over the palette (bu_bc1_fit's rule): s_s = (c_s - E0).d and q_s once per selector,
// sums weighted by n_s, and the texels' q gathered through the masks (q_s * m[s] fills texel i's field with q_s).  q_s of
// selector s goes to bits 2s of q4 for the least-squares sums.
BU_DEV uint32_t bu_etc1s_bc1_fit(const uint32_t cs[4], const int n[4], const uint32_t m[4], int X2, const int S[3], const int c0[3],
                                 const int c1[3], uint32_t& sel, uint32_t& q4)
{
    int e0[3], d[3];
    BU_UNROLL
    for (int c = 0; c < 3; c++) {
        e0[c] = bu_bc1_e(c0[c], c);
        d[c] = bu_bc1_e(c1[c], c) - e0[c];
    }
    const int D = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const int D3 = 3 * D, D5 = 5 * D, e0d = e0[0] * d[0] + e0[1] * d[1] + e0[2] * d[2];
    int qs = 0, qq = 0;
    sel = 0;
    q4 = 0;
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        const int si = (int)bu_byte(cs[s], 0) * d[0] + (int)bu_byte(cs[s], 1) * d[1] + (int)bu_byte(cs[s], 2) * d[2] - e0d;
        const int s6 = 6 * si;
        const int q = (s6 > D ? 1 : 0) + (s6 > D3 ? 1 : 0) + (s6 > D5 ? 1 : 0);
        qs += n[s] * q * si;
        qq += n[s] * q * q;
        sel += (uint32_t)q * m[s];
        q4 |= (uint32_t)q << (2 * s);
    }
    const int se0 = S[0] * e0[0] + S[1] * e0[1] + S[2] * e0[2], e0e0 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
    return (uint32_t)(9 * X2 - 18 * se0 + 144 * e0e0 - 6 * qs + D * qq);
}

// BC1 of the palette colours (bu_bc1_block's rule): cs[s] = (R, G, B) of selector s in bytes 0..2.
//   solid: every used selector has the same RGB -- texel 0's selector is always used, so it is compared with the others
//   else S, P, X2 and the covariance from count-weighted sums; the same shift, start column and four power steps; H / L = the used
//   selector of largest / smallest v.c_s, the smaller f_s on a tie; the fit and the least-squares pass over the four selectors
//   order: the unchanged swap, w0 == w1 and the 0, 2, 3, 1 index mapping
BU_DEV void bu_etc1s_bc1(uint32_t pr, uint32_t pg, uint32_t pb, uint32_t rows, const uint32_t m[4], uint32_t out[2])
{
    uint32_t cs[4];
    int n[4];
    BU_UNROLL
    for (int s = 0; s < 4; s++) {
        cs[s] = bu_byte(pr, s) | bu_byte(pg, s) << 8 | bu_byte(pb, s) << 16;
        n[s] = (int)bu_popc(m[s]);
    }
    const uint32_t rgb0 = cs[rows & 3u];
    bool solid = true;
    BU_UNROLL
    for (int s = 0; s < 4; s++) solid = solid && (m[s] == 0 || cs[s] == rgb0);
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
        int S[3] = {0, 0, 0}, P00 = 0, P01 = 0, P02 = 0, P11 = 0, P12 = 0, P22 = 0;
        BU_UNROLL
        for (int s = 0; s < 4; s++) {
            const int r = (int)bu_byte(cs[s], 0), g = (int)bu_byte(cs[s], 1), b = (int)bu_byte(cs[s], 2), k = n[s];
            S[0] += k * r;
            S[1] += k * g;
            S[2] += k * b;
            P00 += k * r * r;
            P01 += k * r * g;
            P02 += k * r * b;
            P11 += k * g * g;
            P12 += k * g * b;
            P22 += k * b * b;
        }
        const int X2 = P00 + P11 + P22;
        int C00 = 256 * P00 - 16 * S[0] * S[0], C01 = 256 * P01 - 16 * S[0] * S[1], C02 = 256 * P02 - 16 * S[0] * S[2];
        int C11 = 256 * P11 - 16 * S[1] * S[1], C12 = 256 * P12 - 16 * S[1] * S[2], C22 = 256 * P22 - 16 * S[2] * S[2];
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
        for (int it = 0; it < 4; it++) {
            int u[3] = {C00 * v[0] + C01 * v[1] + C02 * v[2], C01 * v[0] + C11 * v[1] + C12 * v[2], C02 * v[0] + C12 * v[1] + C22 * v[2]};
            bu_bc1_norm(u);
            v[0] = u[0], v[1] = u[1], v[2] = u[2];
        }
        if ((v[0] | v[1] | v[2]) == 0) v[0] = v0[0], v[1] = v0[1], v[2] = v0[2];
        // H / L over the used selectors: |v.c_s| < 3 * 2^13 * 255; a tie goes to the selector whose first texel comes first
        uint32_t wh = rgb0, wl = rgb0;
        int phi = 0, plo = 0, fhi = 16, flo = 16;
        BU_UNROLL
        for (int s = 0; s < 4; s++) {
            if (m[s] == 0) continue;
            const int p = (int)bu_byte(cs[s], 0) * v[0] + (int)bu_byte(cs[s], 1) * v[1] + (int)bu_byte(cs[s], 2) * v[2];
            const int f = __builtin_ctz(m[s]) >> 1;
            if (fhi == 16 || p > phi || (p == phi && f < fhi)) phi = p, fhi = f, wh = cs[s];
            if (flo == 16 || p < plo || (p == plo && f < flo)) plo = p, flo = f, wl = cs[s];
        }
        BU_UNROLL
        for (int c = 0; c < 3; c++) {
            c0[c] = bu_bc1_q((int)bu_byte(wh, c), c);
            c1[c] = bu_bc1_q((int)bu_byte(wl, c), c);
        }
        uint32_t q4;
        const uint32_t err = bu_etc1s_bc1_fit(cs, n, m, X2, S, c0, c1, sel, q4);
        // least squares in thirds (bu_bc1_block): Sb, Sbb, Sbx weighted by n_s
        int Sb = 0, Sbb = 0, Sbx[3] = {0, 0, 0};
        BU_UNROLL
        for (int s = 0; s < 4; s++) {
            const int q = (int)((q4 >> (2 * s)) & 3u), kq = n[s] * q;
            Sb += kq;
            Sbb += kq * q;
            BU_UNROLL
            for (int c = 0; c < 3; c++) Sbx[c] += kq * (int)bu_byte(cs[s], c);
        }
        const int Saa = 144 - 6 * Sb + Sbb, Sab = 3 * Sb - Sbb;
        const int det = Saa * Sbb - Sab * Sab;
        if (det > 0) {
            int r0[3], r1[3];
            const int den = 510 * det;
            BU_UNROLL
            for (int c = 0; c < 3; c++) {
                const int mq = c == 1 ? 63 : 31, Sax = 3 * S[c] - Sbx[c];
                const int na = 3 * (Sbb * Sax - Sab * Sbx[c]), nb = 3 * (Saa * Sbx[c] - Sab * Sax);
                const int ta = 2 * mq * na + 255 * det, tb = 2 * mq * nb + 255 * det;
                r0[c] = ta < 0 ? 0 : (int)bu_umin((uint32_t)ta / (uint32_t)den, (uint32_t)mq);
                r1[c] = tb < 0 ? 0 : (int)bu_umin((uint32_t)tb / (uint32_t)den, (uint32_t)mq);
            }
            uint32_t sel2, q42;
            const uint32_t err2 = bu_etc1s_bc1_fit(cs, n, m, X2, S, r0, r1, sel2, q42);
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
        sel = ~sel;
    }
    if (w0 == w1) sel = 0;
    const uint32_t h = (sel >> 1) & 0x55555555u, l = sel & 0x55555555u;
    out[0] = w0 | (w1 << 16);
    out[1] = h | ((h ^ l) << 1);
}

// One block of TARGET (bu_uastc_dispatch.hpp's ids: 6 BC4, 7 BC5, 8 R11, 9 RG11, 11 BC1, 12 BC3) from its palette words and rows;
// has_a = false: A is the solid 255 block.  out: bu_out_words(TARGET) words.
template <int TARGET>
BU_DEV void bu_etc1s_target_block(const BuTables& T, uint32_t pr, uint32_t pg, uint32_t pb, uint32_t rows, bool has_a, uint32_t pa,
                                  uint32_t arows, uint32_t out[4])
{
    uint32_t m[4];
    bu_etc1s_masks(rows, m);
    if constexpr (TARGET == 11) {
        bu_etc1s_bc1(pr, pg, pb, rows, m, out);
    } else if constexpr (TARGET == 12) {
        if (has_a) {
            uint32_t am[4];
            bu_etc1s_masks(arows, am);
            bu_etc1s_bc4(pa, arows, am, out);
        } else {
            out[0] = BU_BC4_SOLID255[0];
            out[1] = BU_BC4_SOLID255[1];
        }
        bu_etc1s_bc1(pr, pg, pb, rows, m, out + 2);
    } else {
        constexpr bool BC = TARGET == 6 || TARGET == 7, TWO = TARGET == 7 || TARGET == 9;
        static_assert(TARGET >= 6 && TARGET <= 9, "an ETC1S target of bu_etc1s_targets.hpp");
        if constexpr (BC) bu_etc1s_bc4(pr, rows, m, out);
        else bu_etc1s_r11(T, pr, rows, m, out);
        if constexpr (TWO) {
            if (has_a) {
                uint32_t am[4];
                bu_etc1s_masks(arows, am);
                if constexpr (BC) bu_etc1s_bc4(pa, arows, am, out + 2);
                else bu_etc1s_r11(T, pa, arows, am, out + 2);
            } else {
                out[2] = BC ? BU_BC4_SOLID255[0] : BU_R11_SOLID255[0];
                out[3] = BC ? BU_BC4_SOLID255[1] : BU_R11_SOLID255[1];
            }
        }
    }
}

// The palette words of one block: ep / aep = endpoint words (r5 | g5 << 8 | b5 << 16 | inten << 24), pal = the etc1s_pal table
// (LDS or host); A = the alpha endpoint's G (basis_lz/mod.rs:139-143).
BU_DEV void bu_etc1s_palettes(const uint32_t* pal, uint32_t ep, uint32_t aep, uint32_t& pr, uint32_t& pg, uint32_t& pb, uint32_t& pa)
{
    const uint32_t it = (ep >> 19) & 0xE0u;
    pr = pal[it | (ep & 31u)];
    pg = pal[it | ((ep >> 8) & 31u)];
    pb = pal[it | ((ep >> 16) & 31u)];
    pa = pal[((aep >> 19) & 0xE0u) | ((aep >> 8) & 31u)];
}

// ---- the pieces every ETC1S kernel shares ---------------------------------------------------------------------------------------
// The index words of one block: ix = endpoint index | selector index << 16 of the colour slice, ax the same of the alpha slice
// (read only with has_a); bad = some index lies outside its codebook.
struct BuEtc1sIndex {
    uint32_t e, s, ae, as;
    bool bad;
};
BU_DEV BuEtc1sIndex bu_etc1s_index(uint32_t ix, bool has_a, uint32_t ax, uint32_t n_ep, uint32_t n_sel)
{
    BuEtc1sIndex k;
    k.e = ix & 0xFFFFu;
    k.s = ix >> 16;
    k.ae = has_a ? ax & 0xFFFFu : 0u;
    k.as = has_a ? ax >> 16 : 0u;
    k.bad = k.e >= n_ep || k.s >= n_sel || (has_a && (k.ae >= n_ep || k.as >= n_sel));
    return k;
}

// ETC1 of one block (basis_lz/mod.rs:163-181): the endpoint word's 5-bit colours as bytes r5 << 3, g5 << 3, b5 << 3 and the
// intensity twice, inten << 5 | inten << 2 | 0b11 (u8 arithmetic); sel_y = the selector entry's second word, the ETC1 selector bytes.
BU_DEV void bu_etc1s_etc1_block(uint32_t ep, uint32_t sel_y, uint32_t out[2])
{
    const uint32_t inten = ep >> 24;
    out[0] = ((ep << 3) & 0x00F8F8F8u) | ((((inten << 5) | (inten << 2) | 3u) & 0xFFu) << 24);
    out[1] = sel_y;
}

// RGBA32 of one block (basis_lz/mod.rs:122-146): 16 texels = colours[selector] of the colour endpoint, alpha = colours[selector].g of
// the alpha slice's endpoint (:139-143), from the palette words of bu_etc1s_palettes.  The selectors of a block COLUMN are
// byte-aligned -- texel (x, y) sits at bits 8y + 2x of `rows` (etc.rs:354-361), so (rows >> 2x) & 0x03030303 is the column's four
// selectors, one per byte: exactly a v_perm_b32 selector.  One v_perm per channel and column looks the four texels up, two levels
// of byte permutes turn the channel columns into texel words (round 2: sixteen four-way select chains per plane).
BU_DEV void bu_etc1s_block_rgba(uint32_t pr, uint32_t pg, uint32_t pb, uint32_t pa, uint32_t rows, bool has_a, uint32_t arows, uint32_t px[16])
{
    BU_UNROLL
    for (int x = 0; x < 4; x++) {
        const uint32_t sel = (rows >> (2 * x)) & 0x03030303u;
        const uint32_t r = bu_perm(0u, pr, sel), g = bu_perm(0u, pg, sel), b = bu_perm(0u, pb, sel);
        const uint32_t t01 = bu_perm(g, r, 0x05010400u), t23 = bu_perm(g, r, 0x07030602u);  // R0 G0 R1 G1 / R2 G2 R3 G3
        if (has_a) {
            const uint32_t a = bu_perm(0u, pa, (arows >> (2 * x)) & 0x03030303u);
            const uint32_t u01 = bu_perm(a, b, 0x05010400u), u23 = bu_perm(a, b, 0x07030602u);
            px[x] = bu_perm(u01, t01, 0x05040100u);
            px[4 + x] = bu_perm(u01, t01, 0x07060302u);
            px[8 + x] = bu_perm(u23, t23, 0x05040100u);
            px[12 + x] = bu_perm(u23, t23, 0x07060302u);
        } else {
            px[x] = bu_perm(b, t01, 0x0D040100u);  // R G B 255
            px[4 + x] = bu_perm(b, t01, 0x0D050302u);
            px[8 + x] = bu_perm(b, t23, 0x0D060100u);
            px[12 + x] = bu_perm(b, t23, 0x0D070302u);
        }
    }
}

// ---- the slice table of the whole-file kernels (bu_etc1s_kernels.hpp) -------------------------------------------------------------
// The host concatenates the per-slice index arrays (each padded to a multiple of 64 words) and describes the slices in this table; a
// wave owns one 64-block unit and finds its slice by a binary search over the units' prefix.  Slices without blocks get no entry, so
// consecutive entries never share a unit0.  (In the unnamed namespace of the kernels that take it.)
namespace {

struct BuEtc1sSlice {
    uint32_t unit0;     // first 64-block unit of this slice (the table ends with a sentinel holding the total)
    uint32_t n_blocks;  // nbx * nby
    uint32_t nbx;       // blocks per row (RGBA addressing)
    uint32_t idx_ofs;   // colour indices, in words from the start of the staged index buffer
    uint32_t aidx_ofs;  // alpha indices (alpha pairs: RGBA32 and the six targets), 0xFFFFFFFF = none
    uint32_t image;     // status word / image number
    uint64_t out_ofs;   // byte offset of the image in the output buffer
};
static_assert(sizeof(BuEtc1sSlice) == 32, "descriptor layout is shared with the host code");

// The slice that holds `unit`: the largest s < n_slices with slices[s].unit0 <= unit (n_slices >= 1, slices[0].unit0 == 0).  Lane
// (unit - unit0) * 64 + lane of that slice is a block of it when it lies below n_blocks: the last unit of a slice may be part empty.
// On the device `unit` is wave-uniform and the table is read through the scalar cache.
BU_DEV uint32_t bu_etc1s_unit_slice(const BuEtc1sSlice* slices, uint32_t n_slices, uint32_t unit)
{
    uint32_t lo = 0, hi = n_slices;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (slices[mid].unit0 <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace
