// The block ENCODER from pixels to UASTC: 16 RGBA8 texels -> one valid UASTC block (which is the contract; the numpy model
// tests/uastc_encode_model.py is written from that section and agrees byte for byte).  For the gfx950 kernel (bu_uastc_encode_kernels.hpp) and,
// compiled for the host, for the CPU tests (tests/host_emul/bu_emul_uastc_encode.cpp, bu_emul_uastc_encode_main.cpp).
// An exact integer rule, no floating point.  Single-subset, single-plane modes and the solid mode only:
//   all 16 texels equal -> 8; every A == 255 -> the best of 5, 0, 18; R == G == B everywhere -> 15; else the best of 14, 12, 10
// Per candidate mode (bu_enc_fit): principal axis by an integer power iteration, the extreme texels along it as endpoints, every texel to its
// nearest entry of the exact decoded palette, one least-squares pass over the endpoints that is kept only if it lowers the error.  Then the anchor
// rule, the transcoding hints (etc2tm, mode 8's ETC1 fields) and the bytes, by the field positions of BuLayout<M>.  The ETC1 fields of the other
// modes are a second step over the finished block (bu_uastc_encode_hints), which the device runs as a kernel of its own.
// No dynamically indexed private array anywhere: texel loops are unrolled with compile-time indices, loops over palette entries and hint
// candidates stay rolled and compute what they need from the loop counter (a private array indexed by a register spills to scratch).
#pragma once
#include "bu_encode_blocks.hpp"  // the gather of a block's texels (section 4.10); the UASTC front end, the ETC helpers and BU_ROLLED through it

// value 0..255 -> index (trit << bits | bits) of the nearest dequantised level of BISE ranges 11, 13 and 19, the lower level on a tie.  Built from
// the decode table BuTables::deq (bu_enc_nearest), by every workgroup into LDS and by the host build once; range 20 is the identity.
struct BuEncQuant {
    uint8_t q[3][256];
};
constexpr int bu_encq_row(int range) { return range == 11 ? 0 : range == 13 ? 1 : 2; }
constexpr int bu_enc_levels(int range) { return (bu_bise_trits(range) ? 3 : 1) << bu_bise_bits(range); }

template <int RANGE>
BU_DEV uint32_t bu_enc_deq(const BuTables& T, uint32_t idx)
{
    constexpr int bits = bu_bise_bits(RANGE);
    return bu_deq<RANGE>(T, idx >> bits, idx & ((1u << bits) - 1u));
}
template <int RANGE>
BU_DEV uint32_t bu_enc_nearest(const BuTables& T, uint32_t v)
{
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < (uint32_t)bu_enc_levels(RANGE); i++) {
        const uint32_t lv = bu_enc_deq<RANGE>(T, i), d = lv > v ? lv - v : v - lv;
        best = bu_umin(best, (d << 16) | (lv << 8) | i);  // distance, then the lower level; i <= 191
    }
    return best & 0xFFu;
}
BU_DEV uint32_t bu_enc_nearest_row(const BuTables& T, int row, uint32_t v)
{
    return row == 0 ? bu_enc_nearest<11>(T, v) : row == 1 ? bu_enc_nearest<13>(T, v) : bu_enc_nearest<19>(T, v);
}
template <int RANGE>
BU_DEV uint32_t bu_enc_level(const BuEncQuant& Q, uint32_t v)
{
    if constexpr (RANGE == 20) return v;
    else return Q.q[bu_encq_row(RANGE)][v];
}

// the prefix codes of the modes the encoder writes (uastc.rs:560-577)
constexpr uint32_t bu_enc_mode_code(int m) { return m == 0 ? 0x1u : m == 5 ? 0xBu : m == 8 ? 0x17u : m == 10 ? 0x2u : m == 12 ? 0x6u : m == 14 ? 0xDu : m == 15 ? 0x5u : 0x9u; }
// unquantised weight of index k (uastc.rs:697-719; every weight range here is plain bits: replicate to six bits, + 1 above 32)
template <int WB>
BU_DEV uint32_t bu_enc_weight(uint32_t k)
{
    const uint32_t w = WB == 2 ? k * 21u : WB == 3 ? k * 9u : WB == 4 ? (k << 2) | (k >> 2) : (k << 1) | (k >> 4);
    return w + (w > 32u ? 1u : 0u);
}
// channel j of the mode's channels out of a texel word: RGB / RGBA byte j; LA: R, A
template <int FMT>
BU_DEV int32_t bu_enc_x(uint32_t px, int j)
{
    return (int32_t)((px >> (FMT == BU_FMT_LA && j == 1 ? 24 : 8 * j)) & 0xFFu);
}
// the decoder's interpolation (bu_block_unpack) of dequantised endpoints
BU_DEV int32_t bu_enc_lerp(uint32_t lo, uint32_t hi, uint32_t w) { return (int32_t)(((257u * lo * (64u - w) + 257u * hi * w + 32u) >> 6) >> 8); }
BU_DEV uint32_t bu_bitlen32(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }
BU_DEV uint32_t bu_bitlen64(uint64_t v) { return v ? 64u - (uint32_t)__builtin_clzll(v) : 0u; }
BU_DEV uint32_t bu_absi(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

template <int C>
BU_DEV void bu_enc_norm12(int32_t u[C])
{
    uint32_t m = 0;
    BU_UNROLL
    for (int j = 0; j < C; j++) m = bu_umax(m, bu_absi(u[j]));
    const uint32_t bl = bu_bitlen32(m), sh = bl > 12u ? bl - 12u : 0u;
    BU_UNROLL
    for (int j = 0; j < C; j++) u[j] >>= sh;  // (arithmetic)
}

// One candidate mode M on the texels px: the block (hints zero) into out[4], the decoded alpha of texel i into byte i % 4 of adec[i / 4] (modes with
// alpha), returns E = the squared error of the block's decode over the mode's channels.
template <int M>
BU_DEV uint32_t bu_enc_fit(const BuTables& T, const BuEncQuant& Q, const uint32_t px[16], uint32_t out[4], uint32_t adec[4])
{
    using L = BuLayout<M>;
    constexpr int C = L::channels, RANGE = L::d.range, WB = L::d.wb, K = 1 << WB, FMT = L::d.fmt;
    static_assert(L::d.subsets == 1 && L::d.planes == 1 && M != 8, "single subset, single plane");
    // 1: the principal axis
    int32_t S[C], cov[C][C], w[C], v0[C];
    BU_UNROLL
    for (int j = 0; j < C; j++) {
        S[j] = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) S[j] += bu_enc_x<FMT>(px[i], j);
        BU_UNROLL
        for (int b = 0; b < C; b++) cov[j][b] = 0;
    }
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        int32_t dev[C];
        BU_UNROLL
        for (int j = 0; j < C; j++) dev[j] = 16 * bu_enc_x<FMT>(px[i], j) - S[j];
        BU_UNROLL
        for (int a = 0; a < C; a++)
            BU_UNROLL
            for (int b = a; b < C; b++) cov[a][b] += dev[a] * dev[b];  // < 2^29
    }
    uint32_t cmax = 0;
    BU_UNROLL
    for (int a = 0; a < C; a++)
        BU_UNROLL
        for (int b = a; b < C; b++) cmax = bu_umax(cmax, bu_absi(cov[a][b]));
    const uint32_t cbl = bu_bitlen32(cmax), csh = cbl > 16u ? cbl - 16u : 0u;
    BU_UNROLL
    for (int a = 0; a < C; a++)
        BU_UNROLL
        for (int b = a; b < C; b++) {
            cov[a][b] >>= csh;
            cov[b][a] = cov[a][b];
        }
    int kd = 0;
    int32_t dmax = cov[0][0];
    BU_UNROLL
    for (int a = 1; a < C; a++)
        if (cov[a][a] > dmax) dmax = cov[a][a], kd = a;
    BU_UNROLL
    for (int j = 0; j < C; j++) {
        v0[j] = cov[j][0];
        BU_UNROLL
        for (int a = 1; a < C; a++) v0[j] = kd == a ? cov[j][a] : v0[j];
    }
    bu_enc_norm12<C>(v0);
    BU_UNROLL
    for (int j = 0; j < C; j++) w[j] = v0[j];
    BU_ROLLED
    for (int it = 0; it < 4; it++) {
        int32_t cv[C];
        BU_UNROLL
        for (int a = 0; a < C; a++) {
            cv[a] = 0;
            BU_UNROLL
            for (int b = 0; b < C; b++) cv[a] += cov[a][b] * w[b];  // |cov| <= 2^16, |w| < 2^12
        }
        bu_enc_norm12<C>(cv);
        BU_UNROLL
        for (int j = 0; j < C; j++) w[j] = cv[j];
    }
    bool zero = true;
    BU_UNROLL
    for (int j = 0; j < C; j++) zero = zero && w[j] == 0;
    BU_UNROLL
    for (int j = 0; j < C; j++) w[j] = zero ? v0[j] : w[j];
    // 2: the extreme texels along it, quantised
    int32_t pmax = 0, pmin = 0;
    uint32_t H = px[0], Lo = px[0];
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        int32_t p = 0;
        BU_UNROLL
        for (int j = 0; j < C; j++) p += bu_enc_x<FMT>(px[i], j) * w[j];
        if (i == 0 || p > pmax) pmax = p, H = px[i];
        if (i == 0 || p < pmin) pmin = p, Lo = px[i];
    }
    uint32_t cl[C], ch[C];  // candidate endpoints: level indices
    BU_UNROLL
    for (int j = 0; j < C; j++) {
        cl[j] = bu_enc_level<RANGE>(Q, (uint32_t)bu_enc_x<FMT>(Lo, j));
        ch[j] = bu_enc_level<RANGE>(Q, (uint32_t)bu_enc_x<FMT>(H, j));
    }
    uint32_t el[C], eh[C], k[16], E = 0;  // the accepted endpoints, weight indices and error
    BU_UNROLL
    for (int j = 0; j < C; j++) el[j] = eh[j] = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) k[i] = 0;
    BU_ROLLED
    for (int pass = 0; pass < 2; pass++) {
        // 3: every texel to its nearest palette entry
        uint32_t dl[C], dh[C], best[16], kk[16];
        BU_UNROLL
        for (int j = 0; j < C; j++) {
            dl[j] = bu_enc_deq<RANGE>(T, cl[j]);
            dh[j] = bu_enc_deq<RANGE>(T, ch[j]);
        }
        BU_UNROLL
        for (int i = 0; i < 16; i++) best[i] = 0xFFFFFFFFu, kk[i] = 0;
        BU_ROLLED
        for (uint32_t e = 0; e < (uint32_t)K; e++) {
            const uint32_t wt = bu_enc_weight<WB>(e);
            int32_t pal[C];
            BU_UNROLL
            for (int j = 0; j < C; j++) pal[j] = bu_enc_lerp(dl[j], dh[j], wt);
            BU_UNROLL
            for (int i = 0; i < 16; i++) {
                uint32_t d = 0;
                BU_UNROLL
                for (int j = 0; j < C; j++) {
                    const int32_t t = pal[j] - bu_enc_x<FMT>(px[i], j);
                    d += (uint32_t)(t * t);
                }
                if (d < best[i]) best[i] = d, kk[i] = e;
            }
        }
        uint32_t E2 = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) E2 += best[i];
        if (pass == 0 || E2 < E) {
            E = E2;
            BU_UNROLL
            for (int i = 0; i < 16; i++) k[i] = kk[i];
            BU_UNROLL
            for (int j = 0; j < C; j++) el[j] = cl[j], eh[j] = ch[j];
        }
        if (pass == 1) break;
        // 4: least squares over the endpoints with the weights just chosen
        uint32_t Saa = 0, Sbb = 0, Sab = 0, Sax[C], Sbx[C];
        BU_UNROLL
        for (int j = 0; j < C; j++) Sax[j] = Sbx[j] = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) {
            const uint32_t b = bu_enc_weight<WB>(k[i]), a = 64u - b;
            Saa += a * a, Sbb += b * b, Sab += a * b;
            BU_UNROLL
            for (int j = 0; j < C; j++) {
                Sax[j] += a * (uint32_t)bu_enc_x<FMT>(px[i], j);
                Sbx[j] += b * (uint32_t)bu_enc_x<FMT>(px[i], j);
            }
        }
        const uint32_t det = Saa * Sbb - Sab * Sab;  // <= 2^30
        uint64_t NA[C], NB[C], nmax = 0;
        BU_UNROLL
        for (int j = 0; j < C; j++) {
            const int64_t na = (int64_t)((uint64_t)Sbb * Sax[j]) - (int64_t)((uint64_t)Sab * Sbx[j]);
            const int64_t nb = (int64_t)((uint64_t)Saa * Sbx[j]) - (int64_t)((uint64_t)Sab * Sax[j]);
            NA[j] = na < 0 ? 0u : (uint64_t)na;
            NB[j] = nb < 0 ? 0u : (uint64_t)nb;
            nmax = nmax > NA[j] ? nmax : NA[j];
            nmax = nmax > NB[j] ? nmax : NB[j];
        }
        const uint32_t nbl = bu_bitlen64(nmax), t = nbl > 23u ? nbl - 23u : 0u;
        const uint32_t d2 = det >> t;
        if (d2 == 0) break;
        BU_UNROLL
        for (int j = 0; j < C; j++) {
            const uint32_t ra = bu_umin(255u, (128u * (uint32_t)(NA[j] >> t) + d2) / (2u * d2));
            const uint32_t rb = bu_umin(255u, (128u * (uint32_t)(NB[j] >> t) + d2) / (2u * d2));
            cl[j] = bu_enc_level<RANGE>(Q, ra);
            ch[j] = bu_enc_level<RANGE>(Q, rb);
        }
    }
    // the decoded alpha, before the anchor rule (which leaves the decode as it is)
    if constexpr (L::has_alpha) {
        const uint32_t al = bu_enc_deq<RANGE>(T, el[C - 1]), ah = bu_enc_deq<RANGE>(T, eh[C - 1]);
        BU_UNROLL
        for (int r = 0; r < 4; r++) {
            adec[r] = 0;
            BU_UNROLL
            for (int x = 0; x < 4; x++) adec[r] |= (uint32_t)bu_enc_lerp(al, ah, bu_enc_weight<WB>(k[4 * r + x])) << (8 * x);
        }
    }
    // anchor: the top bit of texel 0's weight is not stored
    const bool inv = (k[0] & (uint32_t)(K >> 1)) != 0;
    BU_UNROLL
    for (int j = 0; j < C; j++) {
        const uint32_t a = el[j], b = eh[j];
        el[j] = inv ? b : a;
        eh[j] = inv ? a : b;
    }
    BU_UNROLL
    for (int i = 0; i < 16; i++) k[i] = inv ? (uint32_t)(K - 1) - k[i] : k[i];
    // bytes
    BU_UNROLL
    for (int q = 0; q < 4; q++) out[q] = 0;
    bu_put(out, 0, L::d.code_size, bu_enc_mode_code(M));
    constexpr int ebits = L::ebits;
    if constexpr (L::trits) {
        BU_UNROLL
        for (int g = 0; g * 5 < L::ep_count; g++) {
            uint32_t v = 0, p3 = 1;
            BU_UNROLL
            for (int q = 0; q < 5; q++) {
                const int i = 5 * g + q;
                if (i < L::ep_count) {
                    v += p3 * (((i & 1) ? eh[i >> 1] : el[i >> 1]) >> ebits);
                    p3 *= 3u;
                }
            }
            bu_put(out, L::pos_ep + 8 * g, g < L::tq_full ? 8 : L::tq_rem_bits, v);
        }
    }
    BU_UNROLL
    for (int i = 0; i < L::ep_count; i++) bu_put(out, L::pos_epbits + ebits * i, ebits, ((i & 1) ? eh[i >> 1] : el[i >> 1]) & ((1u << ebits) - 1u));
    bu_put(out, L::pos_w, WB - 1, k[0]);
    BU_UNROLL
    for (int i = 1; i < 16; i++) bu_put(out, L::pos_w + WB * i - 1, WB, k[i]);
    return E;
}

// etc2tm of a block whose decoded alphas are adec and whose source alphas are byte 3 of px: the byte mult << 4 | table, mult 1..15, of the smallest
// sum of (value the transcoder's EAC rule picks for the decoded alpha - source alpha)^2, the lowest byte on a tie (bu_eac_block's centre, values and
// thresholds; the value of rank r is val[0] + the steps passed, so that no array is indexed by the rank).
BU_DEV uint32_t bu_enc_etc2tm(const BuTables& T, const uint32_t px[16], const uint32_t adec[4])
{
    uint32_t mn = 255, mx = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const uint32_t a = (adec[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        mn = bu_umin(mn, a), mx = bu_umax(mx, a);
    }
    if (mn == mx) return 0x10u;  // a solid EAC block whatever the byte says: every candidate ties
    uint32_t best = 0xFFFFFFFFu, best_tm = 0x10u;
    BU_ROLLED
    for (uint32_t tm = 0x10u; tm < 0x100u; tm++) {
        const uint32_t table = tm & 15u;
        const int mult = (int)(tm >> 4);
        const int mm = T.eac_mod_min[table], range = T.eac_range[table];
        const uint32_t num = (uint32_t)(2 * ((int)mn * (range + mm) - (int)mx * mm) + range);
        const int center = (int)((num * T.eac_magic[table]) >> 20);
        int val[8];
        BU_UNROLL
        for (int r = 0; r < 8; r++) val[r] = bu_clampi(center + T.eac_mods[8 * table + r] * mult, 0, 255);
        int thr[8], step[8];
        BU_UNROLL
        for (int r = 1; r < 8; r++) {
            thr[r] = (val[r - 1] + val[r] + (r < 4 ? 1 : 2)) >> 1;
            step[r] = val[r] - val[r - 1];
        }
        uint32_t err = 0;
        BU_UNROLL
        for (int i = 0; i < 16; i++) {
            const int a = (int)((adec[i >> 2] >> (8 * (i & 3))) & 0xFFu), src = (int)(px[i] >> 24);
            int v = val[0];
            BU_UNROLL
            for (int r = 1; r < 8; r++) v += a >= thr[r] ? step[r] : 0;
            err += (uint32_t)((v - src) * (v - src));
        }
        if (err < best) best = err, best_tm = tm;
    }
    return best_tm;
}

// The ETC1 modifiers of the specification, {small, large} per table
// (table i in byte i of a 64-bit constant: a constant array indexed by a register would have to live in memory)
constexpr uint64_t bu_enc_pack8(int a, int b, int c, int d, int e, int f, int g, int h)
{
    return (uint64_t)a | (uint64_t)b << 8 | (uint64_t)c << 16 | (uint64_t)d << 24 | (uint64_t)e << 32 | (uint64_t)f << 40 | (uint64_t)g << 48 | (uint64_t)h << 56;
}
constexpr uint64_t BU_ENC_ETC1_SMALL = bu_enc_pack8(2, 5, 9, 13, 18, 24, 33, 47), BU_ENC_ETC1_LARGE = bu_enc_pack8(8, 17, 29, 42, 60, 80, 106, 183);
// Mode 8's ETC1 fields d | i << 1 | s << 4 | r << 6 | g << 11 | b << 16 (their order in the block from bit 37): the lowest tuple (d, i, s, r, g, b) of
// the smallest squared RGB error of the ETC1 block bu_block_etc<8> writes for them, decoded.  For a fixed (d, i, s) the channels are independent.
BU_DEV uint32_t bu_enc_mode8_etc1(uint32_t rgba)
{
    uint32_t best = 0xFFFFFFFFu, fields = 0;
    BU_ROLLED
    for (uint32_t dis = 0; dis < 64u; dis++) {
        const uint32_t d = dis >> 5, in = (dis >> 2) & 7u, s = dis & 3u;
        const int mag = (int)((((s == 0 || s == 3) ? BU_ENC_ETC1_LARGE : BU_ENC_ETC1_SMALL) >> (8 * in)) & 0xFFu), mod = s < 2 ? -mag : mag;
        uint32_t cbest[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};  // error << 8 | value: the lowest value on a tie
        BU_ROLLED
        for (uint32_t c = 0; c < 32u; c++) {
            const uint32_t byte = (d ? c << 3 : (c << 4) | c) & 0xFFu;
            const int b0 = d ? (int)((c << 3) | (c >> 2)) : (int)((byte >> 4) * 17u), b1 = d ? b0 : (int)((byte & 15u) * 17u);
            const int v0 = bu_clampi(b0 + mod, 0, 255), v1 = bu_clampi(b1 + mod, 0, 255);
            BU_UNROLL
            for (int ch = 0; ch < 3; ch++) {
                const int x = (int)((rgba >> (8 * ch)) & 0xFFu);
                const uint32_t e = (uint32_t)(8 * ((v0 - x) * (v0 - x) + (v1 - x) * (v1 - x)));  // <= 16 * 255^2 < 2^21
                cbest[ch] = bu_umin(cbest[ch], (e << 8) | c);
            }
        }
        const uint32_t tot = (cbest[0] >> 8) + (cbest[1] >> 8) + (cbest[2] >> 8);
        if (tot < best) {
            best = tot;
            fields = d | (in << 1) | (s << 4) | ((cbest[0] & 31u) << 6) | ((cbest[1] & 31u) << 11) | ((cbest[2] & 31u) << 16);
        }
    }
    return fields;
}

// px[i] = texel i = 4y + x as R | G << 8 | B << 16 | A << 24 -> the 16 bytes of the block in out[0..3]
BU_DEV void bu_uastc_encode_block(const BuTables& T, const BuEncQuant& Q, const uint32_t px[16], uint32_t out[4])
{
    uint32_t all_or = 0, all_and = 0xFFFFFFFFu, grey = 0;
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        all_or |= px[i] ^ px[0];
        all_and &= px[i];
        grey |= (px[i] ^ (px[i] >> 8)) & 0xFFFFu;  // R ^ G in byte 0, G ^ B in byte 1
    }
    BU_UNROLL
    for (int q = 0; q < 4; q++) out[q] = 0;
    if (all_or == 0) {
        const uint32_t f = bu_enc_mode8_etc1(px[0]);
        bu_put(out, 0, 5, bu_enc_mode_code(8));
        bu_put(out, 5, 32, px[0]);
        bu_put(out, 37, 21, f);
        return;
    }
    uint32_t adec[4] = {0, 0, 0, 0};
    if ((all_and >> 24) == 0xFFu) {
        uint32_t o2[4], dummy[4];
        uint32_t E = bu_enc_fit<5>(T, Q, px, out, dummy);
        uint32_t E2 = bu_enc_fit<0>(T, Q, px, o2, dummy);
        if (E2 < E) {
            E = E2;
            BU_UNROLL
            for (int q = 0; q < 4; q++) out[q] = o2[q];
        }
        E2 = bu_enc_fit<18>(T, Q, px, o2, dummy);
        if (E2 < E) {
            BU_UNROLL
            for (int q = 0; q < 4; q++) out[q] = o2[q];
        }
        return;
    }
    int tm_pos;
    if (grey == 0) {
        bu_enc_fit<15>(T, Q, px, out, adec);
        tm_pos = BuLayout<15>::pos_etc2tm;
    } else {
        uint32_t o2[4], a2[4];
        uint32_t E = bu_enc_fit<14>(T, Q, px, out, adec);
        tm_pos = BuLayout<14>::pos_etc2tm;
        uint32_t E2 = bu_enc_fit<12>(T, Q, px, o2, a2);
        if (E2 < E) {
            E = E2, tm_pos = BuLayout<12>::pos_etc2tm;
            BU_UNROLL
            for (int q = 0; q < 4; q++) out[q] = o2[q], adec[q] = a2[q];
        }
        E2 = bu_enc_fit<10>(T, Q, px, o2, a2);
        if (E2 < E) {
            tm_pos = BuLayout<10>::pos_etc2tm;
            BU_UNROLL
            for (int q = 0; q < 4; q++) out[q] = o2[q], adec[q] = a2[q];
        }
    }
    static_assert(BuLayout<15>::pos_etc2tm + 8 <= 32 && BuLayout<14>::pos_etc2tm + 8 <= 32 && BuLayout<12>::pos_etc2tm + 8 <= 32 && BuLayout<10>::pos_etc2tm + 8 <= 32,
                  "etc2tm lies in the block's first word");
    out[0] |= bu_enc_etc2tm(T, px, adec) << tm_pos;
}

// ---- the ETC1 hints of the non-solid modes: the second step (a kernel of its own on the device) -------------------------------------------------
// (flip, diff, inten0, inten1, bias) of the smallest squared RGB error, against the source texels px, of the ETC1 block bu_block_etc writes for
// them, decoded; the lowest tuple in that order on a tie; (0, 0, 0, 0, 0) is one of the candidates.  dec = the block's own RGBA32 unpack, which is
// what the transcoder averages and takes lumas of.  Factored: the base colours depend on (flip, diff, bias) only -- quadrant sums, bu_block_etc's
// quantiser, its bias tables etc1_bias2 / etc1_biasv0 / etc1_biasv1, the differential clamp -- and then each half picks its table alone.  A texel's
// decoded value is candidate 0 plus the steps whose luma threshold it passes, so nothing is indexed by the selector; the four 2 x 2 quadrants keep
// compile-time texel indices, and the flip only says which half's candidates the two off-diagonal quadrants take.
// has_bias = false (modes 10 - 12): no bias field, the quantised averages are the base colours.  Returns flip | diff << 1 | inten0 << 2 | inten1 << 5
// | bias << 8, the fields in their order in the block.
BU_DEV uint32_t bu_enc_etc1_search(const BuTables& T, const uint32_t px[16], const uint32_t dec[16], bool has_bias)
{
    int lum[16], qs[4][3];
    BU_UNROLL
    for (int i = 0; i < 16; i++) {
        const int q = ((i >> 3) << 1) | ((i >> 1) & 1);  // row >= 2, column >= 2
        lum[i] = 0;
        BU_UNROLL
        for (int ch = 0; ch < 3; ch++) {
            const int v = (int)((dec[i] >> (8 * ch)) & 0xFFu);
            lum[i] += v * (ch == 0 ? 108 : ch == 1 ? 366 : 38);
            qs[q][ch] = (i & 5) == 0 ? v : qs[q][ch] + v;
        }
    }
    const uint32_t nb = has_bias ? 32u : 1u;
    uint32_t best = 0xFFFFFFFFu, bestkey = 0;
    BU_ROLLED
    for (uint32_t combo = 0; combo < 4u * nb; combo++) {
        const uint32_t fd = combo / nb, bias = combo - fd * nb;
        const bool f = (fd >> 1) != 0, d = (fd & 1u) != 0;
        const int limit = d ? 31 : 15;
        const BuU2 bw = T.etc1_bias2[bias];
        int c[2][3], ext[2][3];
        BU_UNROLL
        for (int ch = 0; ch < 3; ch++) {
            const int s0 = qs[0][ch] + (f ? qs[1][ch] : qs[2][ch]), s1 = qs[3][ch] + (f ? qs[2][ch] : qs[1][ch]);
            const uint32_t a0 = (uint32_t)(s0 * limit + 1020) / 2040u, a1 = (uint32_t)(s1 * limit + 1020) / 2040u;
            const uint32_t hi = d ? 0x80u : 0u;
            c[0][ch] = has_bias ? (int)(T.etc1_biasv0[hi | ((bw.x >> (8 * ch)) & 0x60u) | a0] >> 3) : (int)a0;
            c[1][ch] = has_bias ? (int)(T.etc1_biasv1[hi | ((bw.y >> (8 * ch)) & 0x60u) | a1] >> 1) : (int)a1;
            if (d) c[1][ch] = c[0][ch] + bu_clampi(c[1][ch] - c[0][ch], -4, 3);
            BU_UNROLL
            for (int h = 0; h < 2; h++) ext[h][ch] = d ? ((c[h][ch] << 3) | (c[h][ch] >> 2)) : c[h][ch] * 17;
        }
        uint32_t mn0 = 0xFFFFFFFFu, mn1 = 0xFFFFFFFFu, i0 = 0, i1 = 0;
        BU_ROLLED
        for (uint32_t t = 0; t < 8u; t++) {
            const int ms = (int)((BU_ENC_ETC1_SMALL >> (8 * t)) & 0xFFu), ml = (int)((BU_ENC_ETC1_LARGE >> (8 * t)) & 0xFFu);
            int c0[2][3], st[2][3][3], thr[2][3];  // per half: candidate 0, the three steps per channel, the three luma thresholds
            BU_UNROLL
            for (int h = 0; h < 2; h++) {
                int lc[4] = {0, 0, 0, 0};
                BU_UNROLL
                for (int ch = 0; ch < 3; ch++) {
                    const int wgt = ch == 0 ? 108 : ch == 1 ? 366 : 38;
                    const int v0 = bu_clampi(ext[h][ch] - ml, 0, 255), v1 = bu_clampi(ext[h][ch] - ms, 0, 255);
                    const int v2 = bu_clampi(ext[h][ch] + ms, 0, 255), v3 = bu_clampi(ext[h][ch] + ml, 0, 255);
                    c0[h][ch] = v0, st[h][0][ch] = v1 - v0, st[h][1][ch] = v2 - v1, st[h][2][ch] = v3 - v2;
                    lc[0] += wgt * v0, lc[1] += wgt * v1, lc[2] += wgt * v2, lc[3] += wgt * v3;
                }
                BU_UNROLL
                for (int j = 0; j < 3; j++) thr[h][j] = (lc[j] + lc[j + 1]) >> 1;
            }
            uint32_t qe[4];
            BU_UNROLL
            for (int q = 0; q < 4; q++) {
                const bool h1 = q == 3 || (q == 1 && !f) || (q == 2 && f);  // the quadrant lies in half 1
                int b0[3], sq[3][3], tq[3];
                BU_UNROLL
                for (int j = 0; j < 3; j++) {
                    tq[j] = h1 ? thr[1][j] : thr[0][j];
                    b0[j] = h1 ? c0[1][j] : c0[0][j];
                    BU_UNROLL
                    for (int ch = 0; ch < 3; ch++) sq[j][ch] = h1 ? st[1][j][ch] : st[0][j][ch];
                }
                qe[q] = 0;
                BU_UNROLL
                for (int k = 0; k < 4; k++) {
                    const int i = ((q >> 1) << 3) + ((q & 1) << 1) + ((k >> 1) << 2) + (k & 1);
                    BU_UNROLL
                    for (int ch = 0; ch < 3; ch++) {
                        int v = b0[ch];
                        BU_UNROLL
                        for (int j = 0; j < 3; j++) v += lum[i] >= tq[j] ? sq[j][ch] : 0;
                        const int e = v - (int)((px[i] >> (8 * ch)) & 0xFFu);
                        qe[q] += (uint32_t)(e * e);
                    }
                }
            }
            const uint32_t e0 = qe[0] + (f ? qe[1] : qe[2]), e1 = qe[3] + (f ? qe[2] : qe[1]);
            if (e0 < mn0) mn0 = e0, i0 = t;
            if (e1 < mn1) mn1 = e1, i1 = t;
        }
        const uint32_t tot = mn0 + mn1, key = (fd << 11) | (i0 << 8) | (i1 << 5) | bias;
        if (tot < best || (tot == best && key < bestkey)) best = tot, bestkey = key;
    }
    return (bestkey >> 12) | (((bestkey >> 11) & 1u) << 1) | (((bestkey >> 8) & 7u) << 2) | (((bestkey >> 5) & 7u) << 5) | ((bestkey & 31u) << 8);
}

// The second step on a block bu_uastc_encode_block wrote: its ETC1 flip / diff / table / bias fields, searched.  Mode 8 blocks are complete already.
BU_DEV void bu_uastc_encode_hints(const BuTables& T, const uint32_t px[16], uint32_t blk[4])
{
    const uint32_t mode = T.mode_lut[blk[0] & 127u];
    if (mode == 8u) return;
    BuBlk b;
    BU_UNROLL
    for (int q = 0; q < 4; q++) b.w[q] = blk[q];
    uint32_t dec[16];
    int pos;
    switch (mode) {
    case 5: bu_block_rgba<5>(T, b, dec), pos = BuLayout<5>::pos_etc1f; break;
    case 0: bu_block_rgba<0>(T, b, dec), pos = BuLayout<0>::pos_etc1f; break;
    case 18: bu_block_rgba<18>(T, b, dec), pos = BuLayout<18>::pos_etc1f; break;
    case 15: bu_block_rgba<15>(T, b, dec), pos = BuLayout<15>::pos_etc1f; break;
    case 14: bu_block_rgba<14>(T, b, dec), pos = BuLayout<14>::pos_etc1f; break;
    case 12: bu_block_rgba<12>(T, b, dec), pos = BuLayout<12>::pos_etc1f; break;
    default: bu_block_rgba<10>(T, b, dec), pos = BuLayout<10>::pos_etc1f; break;  // (the encoder writes no other mode)
    }
    static_assert(BuLayout<15>::pos_etc1f + 13 <= 32, "the ETC1 fields lie in the block's first word in every mode");
    blk[0] |= bu_enc_etc1_search(T, px, dec, !(mode == 10u || mode == 12u)) << pos;
}

// the table of BuEncQuant, entry by entry: what a workgroup's lanes (and the host build's loop) fill
BU_DEV void bu_enc_quant_entry(const BuTables& T, BuEncQuant* q, unsigned i) { q->q[i >> 8][i & 255u] = (uint8_t)bu_enc_nearest_row(T, (int)(i >> 8), i & 255u); }
constexpr unsigned BU_ENC_QUANT_ENTRIES = 3 * 256;
