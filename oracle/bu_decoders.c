/* TEST INFRASTRUCTURE ONLY -- never linked into or called by the product.
 *
 * Independent decoders of the TARGET formats, written from the public format specifications (Khronos Data
 * Format Specification: ASTC LDR profile, BPTC/BC7, ETC2 EAC), NOT from the reference crate -- which has no such
 * decoders.  They close the loop on paths the reference's 3 040 known-answer vectors do not reach (SURVEY.md 8c
 * "extra self-consistency checks", 8f rank 4):
 *
 *   ASTC  UASTC is a strict subset of ASTC 4x4 LDR, so decoding the transcoder's ASTC output with a generic ASTC
 *         decoder must reproduce decode_block_to_rgba (uastc.rs:237-327) EXACTLY, texel for texel.
 *   BC7   the repack requantises endpoints (7+p / 5 / 6+p bits) and sometimes weights: decoding must stay CLOSE to
 *         the UASTC colours (bounded per-channel error) -- catches wrong partitions, swapped endpoints, un-inverted
 *         weights, misplaced p-bits.
 *   EAC   the ETC2 alpha half: decoded alpha must stay close to the UASTC alpha.
 *   ETC1  the colour block of ETC1 and of ETC2 RGB(A) (bytes 8..16): individual / differential modes, both flip
 *         orientations, the ETC2 T / H / planar modes detected (differential blocks whose base colour leaves 0..31);
 *         the decoded fields are returned with the texels so that a test can rebuild every selector (tests/etc_model.py).
 *
 * Everything a conformant decoder derives from the bitstream is derived here (block mode, weight range, the colour
 * endpoint range from the bits left over, the partition from the hash function / the BPTC tables); nothing is taken
 * from the transcoder's own tables.
 */
#include <stdint.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------------ bits */
static unsigned get_bits(const uint8_t b[16], int pos, int n) /* little-endian bit order, n <= 24 */
{
    unsigned v = 0;
    for (int i = 0; i < n; i++) {
        int p = pos + i;
        if (p >= 0 && p < 128) v |= ((unsigned)(b[p >> 3] >> (p & 7)) & 1u) << i;
    }
    return v;
}

/* ================================================================================================ ASTC */
/* Integer sequence encoding: value ranges as (trits, quints, bits) */
typedef struct {
    int trits, quints, bits;
} ise_t;
/* the 21 ranges of the specification in increasing order of size */
static const ise_t ISE_RANGES[21] = {{0, 0, 1}, {1, 0, 0}, {0, 0, 2}, {0, 1, 0}, {1, 0, 1}, {0, 0, 3}, {0, 1, 1}, {1, 0, 2}, {0, 0, 4}, {0, 1, 2}, {1, 0, 3},
                                     {0, 0, 5}, {0, 1, 3}, {1, 0, 4}, {0, 0, 6}, {0, 1, 4}, {1, 0, 5}, {0, 0, 7}, {0, 1, 5}, {1, 0, 6}, {0, 0, 8}};

static int ise_size(ise_t r, int n) /* bits needed for n values */
{
    return n * r.bits + (r.trits ? (8 * n + 4) / 5 : 0) + (r.quints ? (7 * n + 2) / 3 : 0);
}

/* decode n values of range r starting at bit `pos`; reads upward when dir = +1, downward (bit-reversed
 * stream read from the top of the block) when dir = -1.  out[i] = (digit, bits) */
typedef struct {
    uint8_t digit, bits;
} isev_t;

static unsigned stream_bit(const uint8_t b[16], int pos, int dir, int k) { return get_bits(b, dir > 0 ? pos + k : pos - k, 1); }
static unsigned stream_bits(const uint8_t b[16], int pos, int dir, int k, int n)
{
    unsigned v = 0;
    for (int i = 0; i < n; i++) v |= stream_bit(b, pos, dir, k + i) << i;
    return v;
}

static void ise_decode(const uint8_t b[16], int pos, int dir, ise_t r, int n, isev_t* out)
{
    int k = 0; /* stream offset */
    if (r.trits) {
        for (int base = 0; base < n; base += 5) {
            unsigned m[5] = {0, 0, 0, 0, 0}, T = 0;
            static const int tbits[5] = {2, 2, 1, 2, 1};
            int tpos = 0;
            for (int i = 0; i < 5; i++) {
                if (base + i >= n) break; /* a truncated final block: missing bits read as zero */
                m[i] = stream_bits(b, pos, dir, k, r.bits);
                k += r.bits;
                T |= stream_bits(b, pos, dir, k, tbits[i]) << tpos;
                k += tbits[i];
                tpos += tbits[i];
            }
            unsigned t[5], C;
            if (((T >> 2) & 7) == 7) {
                C = (((T >> 5) & 7) << 2) | (T & 3);
                t[4] = t[3] = 2;
            } else {
                C = T & 0x1F;
                if (((T >> 5) & 3) == 3) {
                    t[4] = 2;
                    t[3] = (T >> 7) & 1;
                } else {
                    t[4] = (T >> 7) & 1;
                    t[3] = (T >> 5) & 3;
                }
            }
            if ((C & 3) == 3) {
                t[2] = 2;
                t[1] = (C >> 4) & 1;
                t[0] = (((C >> 3) & 1) << 1) | (((C >> 2) & 1) & ~((C >> 3) & 1));
            } else if (((C >> 2) & 3) == 3) {
                t[2] = 2;
                t[1] = 2;
                t[0] = C & 3;
            } else {
                t[2] = (C >> 4) & 1;
                t[1] = (C >> 2) & 3;
                t[0] = (((C >> 1) & 1) << 1) | ((C & 1) & ~((C >> 1) & 1));
            }
            for (int i = 0; i < 5 && base + i < n; i++) {
                out[base + i].digit = (uint8_t)t[i];
                out[base + i].bits = (uint8_t)m[i];
            }
        }
    } else if (r.quints) {
        for (int base = 0; base < n; base += 3) {
            unsigned m[3] = {0, 0, 0}, Q = 0;
            static const int qbits[3] = {3, 2, 2};
            int qpos = 0;
            for (int i = 0; i < 3; i++) {
                if (base + i >= n) break;
                m[i] = stream_bits(b, pos, dir, k, r.bits);
                k += r.bits;
                Q |= stream_bits(b, pos, dir, k, qbits[i]) << qpos;
                k += qbits[i];
                qpos += qbits[i];
            }
            unsigned q[3];
            if (((Q >> 1) & 3) == 3 && ((Q >> 5) & 3) == 0) {
                q[2] = ((Q & 1) << 2) | ((((Q >> 4) & 1) & ~(Q & 1)) << 1) | (((Q >> 3) & 1) & ~(Q & 1));
                q[1] = q[0] = 4;
            } else {
                unsigned C;
                if (((Q >> 1) & 3) == 3) {
                    q[2] = 4;
                    C = (((Q >> 3) & 3) << 3) | ((~(Q >> 5) & 3) << 1) | (Q & 1);
                } else {
                    q[2] = (Q >> 5) & 3;
                    C = Q & 0x1F;
                }
                if ((C & 7) == 5) {
                    q[1] = 4;
                    q[0] = (C >> 3) & 3;
                } else {
                    q[1] = (C >> 3) & 3;
                    q[0] = C & 7;
                }
            }
            for (int i = 0; i < 3 && base + i < n; i++) {
                out[base + i].digit = (uint8_t)q[i];
                out[base + i].bits = (uint8_t)m[i];
            }
        }
    } else {
        for (int i = 0; i < n; i++) {
            out[i].digit = 0;
            out[i].bits = (uint8_t)stream_bits(b, pos, dir, k, r.bits);
            k += r.bits;
        }
    }
}

/* colour endpoint unquantisation to 0..255 (specification table "colour unquantisation parameters") */
static unsigned unquant_color(ise_t r, isev_t v)
{
    const unsigned m = v.bits, n = (unsigned)r.bits;
    if (!r.trits && !r.quints) { /* bit replication */
        unsigned x = m << (8 - n), out = x;
        for (unsigned s = n; s < 8; s += n) out |= x >> s;
        return out & 0xFF;
    }
    if (n == 0) return r.trits ? (v.digit * 255u) / 2u : (v.digit * 255u) / 4u;
    const unsigned a = m & 1, b1 = (m >> 1) & 1, c = (m >> 2) & 1, d = (m >> 3) & 1, e = (m >> 4) & 1, f = (m >> 5) & 1;
    const unsigned A = a ? 0x1FF : 0;
    unsigned B = 0, C = 0;
    if (r.trits) {
        switch (n) {
        case 1: B = 0; C = 204; break;
        case 2: B = (b1 << 8) | (b1 << 4) | (b1 << 2) | (b1 << 1); C = 93; break;
        case 3: B = (c << 8) | (b1 << 7) | (c << 3) | (b1 << 2) | (c << 1) | b1; C = 44; break;
        case 4: B = (d << 8) | (c << 7) | (b1 << 6) | (d << 2) | (c << 1) | b1; C = 22; break;
        case 5: B = (e << 8) | (d << 7) | (c << 6) | (b1 << 5) | (e << 1) | d; C = 11; break;
        default: B = (f << 8) | (e << 7) | (d << 6) | (c << 5) | (b1 << 4) | f; C = 5; break;
        }
    } else {
        switch (n) {
        case 1: B = 0; C = 113; break;
        case 2: B = (b1 << 8) | (b1 << 3) | (b1 << 2); C = 54; break;
        case 3: B = (c << 8) | (b1 << 7) | (c << 2) | (b1 << 1) | c; C = 26; break;
        case 4: B = (d << 8) | (c << 7) | (b1 << 6) | (d << 1) | c; C = 13; break;
        default: B = (e << 8) | (d << 7) | (c << 6) | (b1 << 5) | e; C = 6; break;
        }
    }
    unsigned T = v.digit * C + B;
    T ^= A;
    return (A & 0x80) | (T >> 2);
}

/* weight unquantisation to 0..64 */
static int unquant_weight(ise_t r, isev_t v)
{
    const unsigned m = v.bits, n = (unsigned)r.bits;
    unsigned w;
    if (!r.trits && !r.quints) {
        unsigned x = m << (6 - n);
        w = x;
        for (unsigned s = n; s < 6; s += n) w |= x >> s;
        w &= 63;
    } else if (n == 0) {
        w = r.trits ? (v.digit == 0 ? 0 : v.digit == 1 ? 32 : 63) : (v.digit == 0 ? 0 : v.digit == 1 ? 16 : v.digit == 2 ? 32 : v.digit == 3 ? 47 : 63);
    } else {
        const unsigned a = m & 1, b1 = (m >> 1) & 1, c = (m >> 2) & 1;
        const unsigned A = a ? 0x7F : 0;
        unsigned B = 0, C = 0;
        if (r.trits) {
            if (n == 1) { B = 0; C = 50; }
            else if (n == 2) { B = (b1 << 6) | (b1 << 2) | b1; C = 23; }
            else { B = (c << 6) | (b1 << 5) | (c << 1) | b1; C = 11; }
        } else {
            if (n == 1) { B = 0; C = 28; }
            else { B = (b1 << 6) | (b1 << 1); C = 13; }
        }
        unsigned T = v.digit * C + B;
        T ^= A;
        w = (A & 0x20) | (T >> 2);
    }
    if (w > 32) w += 1;
    return (int)w;
}

static uint32_t hash52(uint32_t p)
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

static int select_partition(int seed, int x, int y, int z, int partitioncount, int small_block)
{
    if (small_block) {
        x <<= 1;
        y <<= 1;
        z <<= 1;
    }
    seed += (partitioncount - 1) * 1024;
    uint32_t rnum = hash52((uint32_t)seed);
    uint8_t seed1 = rnum & 0xF, seed2 = (rnum >> 4) & 0xF, seed3 = (rnum >> 8) & 0xF, seed4 = (rnum >> 12) & 0xF;
    uint8_t seed5 = (rnum >> 16) & 0xF, seed6 = (rnum >> 20) & 0xF, seed7 = (rnum >> 24) & 0xF, seed8 = (rnum >> 28) & 0xF;
    uint8_t seed9 = (rnum >> 18) & 0xF, seed10 = (rnum >> 22) & 0xF, seed11 = (rnum >> 26) & 0xF, seed12 = ((rnum >> 30) | (rnum << 2)) & 0xF;
    seed1 *= seed1; seed2 *= seed2; seed3 *= seed3; seed4 *= seed4; seed5 *= seed5; seed6 *= seed6;
    seed7 *= seed7; seed8 *= seed8; seed9 *= seed9; seed10 *= seed10; seed11 *= seed11; seed12 *= seed12;
    int sh1, sh2, sh3;
    if (seed & 1) {
        sh1 = (seed & 2) ? 4 : 5;
        sh2 = (partitioncount == 3) ? 6 : 5;
    } else {
        sh1 = (partitioncount == 3) ? 6 : 5;
        sh2 = (seed & 2) ? 4 : 5;
    }
    sh3 = (seed & 0x10) ? sh1 : sh2;
    seed1 >>= sh1; seed2 >>= sh2; seed3 >>= sh1; seed4 >>= sh2; seed5 >>= sh1; seed6 >>= sh2; seed7 >>= sh1; seed8 >>= sh2;
    seed9 >>= sh3; seed10 >>= sh3; seed11 >>= sh3; seed12 >>= sh3;
    int a = seed1 * x + seed2 * y + seed11 * z + (int)(rnum >> 14);
    int bb = seed3 * x + seed4 * y + seed12 * z + (int)(rnum >> 10);
    int c = seed5 * x + seed6 * y + seed9 * z + (int)(rnum >> 6);
    int d = seed7 * x + seed8 * y + seed10 * z + (int)(rnum >> 2);
    a &= 0x3F; bb &= 0x3F; c &= 0x3F; d &= 0x3F;
    if (partitioncount < 4) d = 0;
    if (partitioncount < 3) c = 0;
    if (a >= bb && a >= c && a >= d) return 0;
    if (bb >= c && bb >= d) return 1;
    if (c >= d) return 2;
    return 3;
}

/* exported for tests: ASTC partition of texel (x, y) of a 4x4 block */
int bu_dec_astc_partition_4x4(int seed, int x, int y, int partitioncount) { return select_partition(seed, x, y, 0, partitioncount, 1); }

enum { DEC_OK = 0, DEC_RESERVED = 1, DEC_UNSUPPORTED = 2, DEC_ILLEGAL = 3 };

/* ASTC 4x4 LDR block -> 16 RGBA8 texels (row-major), decode mode = UNORM8 (the top 8 bits of the 16-bit result).
 * Supports every weight-grid <= 4x4... in fact only W = H = 4 (no infill), any weight range, 1-4 partitions with a
 * single shared CEM, CEMs 0 / 4 / 8 / 12 (L, LA, RGB, RGBA direct), dual plane, and void-extent blocks.
 * Anything else returns DEC_UNSUPPORTED so that a test can tell "not UASTC-shaped" from "wrong". */
int bu_dec_astc_4x4(const uint8_t b[16], uint8_t out[64])
{
    const unsigned mode = get_bits(b, 0, 11);
    if ((mode & 0x1FF) == 0x1FC) { /* void extent */
        if (mode & 0x200) return DEC_UNSUPPORTED; /* HDR */
        if (get_bits(b, 10, 2) != 3) return DEC_RESERVED;
        /* extent coordinates: all ones = no extent; otherwise low < high on s and on t -- then the colour is constant either way */
        const unsigned s_lo = get_bits(b, 12, 13), s_hi = get_bits(b, 25, 13), t_lo = get_bits(b, 38, 13), t_hi = get_bits(b, 51, 13);
        const int no_extent = s_lo == 0x1FFF && s_hi == 0x1FFF && t_lo == 0x1FFF && t_hi == 0x1FFF;
        if (!no_extent && (s_lo >= s_hi || t_lo >= t_hi)) return DEC_ILLEGAL;
        for (int t = 0; t < 16; t++)
            for (int c = 0; c < 4; c++) out[4 * t + c] = (uint8_t)(get_bits(b, 64 + 16 * c, 16) >> 8);
        return DEC_OK;
    }
    if ((mode & 0xF) == 0) return DEC_RESERVED;
    int W, H;
    unsigned R;
    const unsigned Hp = (mode >> 9) & 1, D = (mode >> 10) & 1;
    if ((mode & 3) != 0) {
        R = ((mode >> 4) & 1) | ((mode & 3) << 1);
        const unsigned A = (mode >> 5) & 3, B = (mode >> 7) & 3;
        switch ((mode >> 2) & 3) {
        case 0: W = (int)B + 4; H = (int)A + 2; break;
        case 1: W = (int)B + 8; H = (int)A + 2; break;
        case 2: W = (int)A + 2; H = (int)B + 8; break;
        default:
            if (B & 2) { W = (int)(B & 1) + 2; H = (int)A + 2; }
            else { W = (int)A + 2; H = (int)(B & 1) + 6; }
            break;
        }
    } else {
        if (((mode >> 6) & 7) == 7) return DEC_RESERVED; /* bits 6..8 all set and not void-extent: reserved by the block-mode table */
        return DEC_UNSUPPORTED; /* the large-grid layouts cannot describe 4x4 */
    }
    if (W != 4 || H != 4) return DEC_UNSUPPORTED;
    if (R < 2) return DEC_RESERVED;
    /* weight range: R = 2..7 -> (H=0) 0..1, 0..2, 0..3, 0..4, 0..5, 0..7; (H=1) 0..9, 0..11, 0..15, 0..19, 0..23, 0..31 */
    static const int WR_LO[6] = {0, 1, 2, 3, 4, 5}, WR_HI[6] = {6, 7, 8, 9, 10, 11};
    const ise_t wr = ISE_RANGES[Hp ? WR_HI[R - 2] : WR_LO[R - 2]];
    const int n_weights = 16 * (D ? 2 : 1);
    const int weight_bits = ise_size(wr, n_weights);
    if (n_weights > 64 || weight_bits < 24 || weight_bits > 96) return DEC_ILLEGAL;
    const int parts = (int)get_bits(b, 11, 2) + 1;
    if (D && parts == 4) return DEC_ILLEGAL;
    int cem, ep_pos, seed = 0;
    if (parts == 1) {
        cem = (int)get_bits(b, 13, 4);
        ep_pos = 17;
    } else {
        seed = (int)get_bits(b, 13, 10);
        if (get_bits(b, 23, 2) != 0) return DEC_UNSUPPORTED; /* per-partition CEMs */
        cem = (int)get_bits(b, 25, 4);
        ep_pos = 29;
    }
    if (cem != 0 && cem != 4 && cem != 8 && cem != 12) return DEC_UNSUPPORTED;
    const int vals_per_part = 2 * (cem / 4 + 1), n_vals = vals_per_part * parts;
    if (n_vals > 18) return DEC_ILLEGAL;
    int avail = 128 - weight_bits - ep_pos - (D ? 2 : 0);
    /* the colour endpoint range is the largest one whose encoding fits the bits left over */
    int cr = -1;
    for (int i = 20; i >= 0; i--)
        if (ise_size(ISE_RANGES[i], n_vals) <= avail) {
            cr = i;
            break;
        }
    if (cr < 4) return DEC_ILLEGAL; /* fewer than 6 levels */
    const ise_t er = ISE_RANGES[cr];
    isev_t ev[18], wv[32];
    ise_decode(b, ep_pos, +1, er, n_vals, ev);
    ise_decode(b, 127, -1, wr, n_weights, wv);
    const unsigned ccs = D ? get_bits(b, 128 - weight_bits - 2, 2) : 0;
    int e0[4][4], e1[4][4];
    for (int p = 0; p < parts; p++) {
        unsigned v[8];
        for (int i = 0; i < vals_per_part; i++) v[i] = unquant_color(er, ev[p * vals_per_part + i]);
        if (cem == 0) {
            for (int c = 0; c < 3; c++) { e0[p][c] = (int)v[0]; e1[p][c] = (int)v[1]; }
            e0[p][3] = e1[p][3] = 255;
        } else if (cem == 4) {
            for (int c = 0; c < 3; c++) { e0[p][c] = (int)v[0]; e1[p][c] = (int)v[1]; }
            e0[p][3] = (int)v[2];
            e1[p][3] = (int)v[3];
        } else {
            const int s0 = (int)(v[0] + v[2] + v[4]), s1 = (int)(v[1] + v[3] + v[5]);
            const int a0 = cem == 12 ? (int)v[6] : 255, a1 = cem == 12 ? (int)v[7] : 255;
            if (s1 >= s0) {
                e0[p][0] = (int)v[0]; e0[p][1] = (int)v[2]; e0[p][2] = (int)v[4]; e0[p][3] = a0;
                e1[p][0] = (int)v[1]; e1[p][1] = (int)v[3]; e1[p][2] = (int)v[5]; e1[p][3] = a1;
            } else { /* blue contraction, endpoints swapped */
                e0[p][0] = ((int)v[1] + (int)v[5]) >> 1; e0[p][1] = ((int)v[3] + (int)v[5]) >> 1; e0[p][2] = (int)v[5]; e0[p][3] = a1;
                e1[p][0] = ((int)v[0] + (int)v[4]) >> 1; e1[p][1] = ((int)v[2] + (int)v[4]) >> 1; e1[p][2] = (int)v[4]; e1[p][3] = a0;
            }
        }
    }
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            const int t = y * 4 + x;
            const int p = parts == 1 ? 0 : select_partition(seed, x, y, 0, parts, 1);
            const int w0 = unquant_weight(wr, wv[D ? 2 * t : t]);
            const int w1 = D ? unquant_weight(wr, wv[2 * t + 1]) : w0;
            for (int c = 0; c < 4; c++) {
                const int w = (D && (unsigned)c == ccs) ? w1 : w0;
                const int c0 = (e0[p][c] << 8) | e0[p][c], c1 = (e1[p][c] << 8) | e1[p][c];
                const int r = (c0 * (64 - w) + c1 * w + 32) >> 6;
                out[4 * t + c] = (uint8_t)(r >> 8);
            }
        }
    return DEC_OK;
}

/* ================================================================================================= BC7 */
/* BPTC partition tables, 2 subsets: bit t = subset of texel t; 3 subsets: 2 bits per texel */
static const uint16_t BC7_PART2[64] = {
    0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
    0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c,
    0xaaaa, 0xf0f0, 0x5a5a, 0x33cc, 0x3c3c, 0x55aa, 0x9696, 0xa55a, 0x73ce, 0x13c8, 0x324c, 0x3bdc, 0x6996, 0xc33c, 0x9966, 0x0660,
    0x0272, 0x04e4, 0x4e40, 0x2720, 0xc936, 0x936c, 0x39c6, 0x639c, 0x9336, 0x9cc6, 0x817e, 0xe718, 0xccf0, 0x0fcc, 0x7744, 0xee22};
static const uint32_t BC7_PART3[64] = {
    0xaa685050, 0x6a5a5040, 0x5a5a4200, 0x5450a0a8, 0xa5a50000, 0xa0a05050, 0x5555a0a0, 0x5a5a5050, 0xaa550000, 0xaa555500, 0xaaaa5500,
    0x90909090, 0x94949494, 0xa4a4a4a4, 0xa9a59450, 0x2a0a4250, 0xa5945040, 0x0a425054, 0xa5a5a500, 0x55a0a0a0, 0xa8a85454, 0x6a6a4040,
    0xa4a45000, 0x1a1a0500, 0x0050a4a4, 0xaaa59090, 0x14696914, 0x69691400, 0xa08585a0, 0xaa821414, 0x50a4a450, 0x6a5a0200, 0xa9a58000,
    0x5090a0a8, 0xa8a09050, 0x24242424, 0x00aa5500, 0x24924924, 0x24499224, 0x50a50a50, 0x500aa550, 0xaaaa4444, 0x66660000, 0xa5a0a5a0,
    0x50a050a0, 0x69286928, 0x44aaaa44, 0x66666600, 0xaa444444, 0x54a854a8, 0x95809580, 0x96969600, 0xa85454a8, 0x80959580, 0xaa141414,
    0x96960000, 0xaaaa1414, 0xa05050a0, 0xa0a5a5a0, 0x96000000, 0x40804080, 0xa9a8a9a8, 0xaaaaaa44, 0x2a4a5254};

int bu_dec_bc7_subset(int n_subsets, int partition, int texel)
{
    if (n_subsets == 2) return (BC7_PART2[partition & 63] >> texel) & 1;
    if (n_subsets == 3) return (int)((BC7_PART3[partition & 63] >> (2 * texel)) & 3);
    return 0;
}

/* anchor (fix-up) index of a subset = ... the specification lists them; they are also derivable: subset 0's anchor is
 * texel 0; for 2 subsets the second anchor is given by a table.  We derive nothing here: the tables below are the
 * specification's. */
static const uint8_t BC7_ANCHOR2_1[64] = {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
                                          15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15};
static const uint8_t BC7_ANCHOR3_1[64] = {3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
                                          8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3};
static const uint8_t BC7_ANCHOR3_2[64] = {15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
                                          15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8};

int bu_dec_bc7_anchor(int n_subsets, int partition, int subset)
{
    if (subset == 0) return 0;
    if (n_subsets == 2) return BC7_ANCHOR2_1[partition & 63];
    return subset == 1 ? BC7_ANCHOR3_1[partition & 63] : BC7_ANCHOR3_2[partition & 63];
}

static const uint8_t BC7_W2[4] = {0, 21, 43, 64}, BC7_W3[8] = {0, 9, 18, 27, 37, 46, 55, 64},
                     BC7_W4[16] = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};

typedef struct {
    int ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2;
} bc7_mode_t;
/*                                       NS PB RB ISB CB AB EPB SPB IB IB2 */
static const bc7_mode_t BC7_MODES[8] = {{3, 4, 0, 0, 4, 0, 1, 0, 3, 0}, {2, 6, 0, 0, 6, 0, 0, 1, 3, 0}, {3, 6, 0, 0, 5, 0, 0, 0, 2, 0}, {2, 6, 0, 0, 7, 0, 1, 0, 2, 0},
                                        {1, 0, 2, 1, 5, 6, 0, 0, 2, 3}, {1, 0, 2, 0, 7, 8, 0, 0, 2, 2}, {1, 0, 0, 0, 7, 7, 1, 0, 4, 0}, {2, 6, 0, 0, 5, 5, 1, 0, 2, 0}};

static int bc7_interp(int e0, int e1, int idx, int bits)
{
    const int w = bits == 2 ? BC7_W2[idx] : bits == 3 ? BC7_W3[idx] : BC7_W4[idx];
    return (e0 * (64 - w) + e1 * w + 32) >> 6;
}

int bu_dec_bc7(const uint8_t b[16], uint8_t out[64])
{
    int mode = 0;
    while (mode < 8 && !((b[0] >> mode) & 1)) mode++;
    if (mode == 8) { /* reserved: decodes to zero */
        memset(out, 0, 64);
        return DEC_RESERVED;
    }
    const bc7_mode_t m = BC7_MODES[mode];
    int pos = mode + 1;
    const int part = (int)get_bits(b, pos, m.pb);
    pos += m.pb;
    const int rot = (int)get_bits(b, pos, m.rb);
    pos += m.rb;
    const int isel = (int)get_bits(b, pos, m.isb);
    pos += m.isb;
    int ep[6][4]; /* endpoint e of subset s = ep[2s + e] */
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 2 * m.ns; i++) {
            ep[i][c] = (int)get_bits(b, pos, m.cb);
            pos += m.cb;
        }
    for (int i = 0; i < 2 * m.ns; i++) {
        ep[i][3] = m.ab ? (int)get_bits(b, pos, m.ab) : 255;
        pos += m.ab;
    }
    int cbits = m.cb, abits = m.ab;
    if (m.epb) {
        for (int i = 0; i < 2 * m.ns; i++) {
            const int p = (int)get_bits(b, pos++, 1);
            for (int c = 0; c < 3; c++) ep[i][c] = (ep[i][c] << 1) | p;
            if (m.ab) ep[i][3] = (ep[i][3] << 1) | p;
        }
        cbits++;
        if (m.ab) abits++;
    } else if (m.spb) {
        for (int s = 0; s < m.ns; s++) {
            const int p = (int)get_bits(b, pos++, 1);
            for (int e = 0; e < 2; e++)
                for (int c = 0; c < 3; c++) ep[2 * s + e][c] = (ep[2 * s + e][c] << 1) | p;
        }
        cbits++;
    }
    for (int i = 0; i < 2 * m.ns; i++) {
        for (int c = 0; c < 3; c++) {
            ep[i][c] <<= (8 - cbits);
            ep[i][c] |= ep[i][c] >> cbits;
        }
        if (m.ab) {
            ep[i][3] <<= (8 - abits);
            ep[i][3] |= ep[i][3] >> abits;
        }
    }
    int idx[16], idx2[16];
    for (int t = 0; t < 16; t++) {
        const int s = bu_dec_bc7_subset(m.ns, part, t);
        const int anchor = (t == bu_dec_bc7_anchor(m.ns, part, s));
        const int n = m.ib - anchor;
        idx[t] = (int)get_bits(b, pos, n);
        pos += n;
    }
    if (m.ib2)
        for (int t = 0; t < 16; t++) {
            const int n = m.ib2 - (t == 0);
            idx2[t] = (int)get_bits(b, pos, n);
            pos += n;
        }
    if (pos != 128) return DEC_ILLEGAL; /* every BC7 mode fills the block exactly */
    for (int t = 0; t < 16; t++) {
        const int s = bu_dec_bc7_subset(m.ns, part, t);
        int px[4];
        if (!m.ib2) {
            for (int c = 0; c < 4; c++) px[c] = bc7_interp(ep[2 * s][c], ep[2 * s + 1][c], idx[t], m.ib);
        } else {
            /* two index sets: isel = 0 -> colour uses the first (ib bits), alpha the second (ib2 bits) */
            const int ci = isel ? idx2[t] : idx[t], cb = isel ? m.ib2 : m.ib;
            const int ai = isel ? idx[t] : idx2[t], ab = isel ? m.ib : m.ib2;
            for (int c = 0; c < 3; c++) px[c] = bc7_interp(ep[0][c], ep[1][c], ci, cb);
            px[3] = bc7_interp(ep[0][3], ep[1][3], ai, ab);
        }
        if (rot) {
            const int tmp = px[3];
            px[3] = px[rot - 1];
            px[rot - 1] = tmp;
        }
        for (int c = 0; c < 4; c++) out[4 * t + c] = (uint8_t)px[c];
    }
    return DEC_OK;
}

/* ================================================================================================= EAC */
/* ETC2 EAC alpha half (8 bytes) -> 16 alpha values in ROW-major texel order (the codes are stored column-major) */
static const int8_t EAC_MOD[16][8] = {{-3, -6, -9, -15, 2, 5, 8, 14}, {-3, -7, -10, -13, 2, 6, 9, 12}, {-2, -5, -8, -13, 1, 4, 7, 12}, {-2, -4, -6, -13, 1, 3, 5, 12},
                                      {-3, -6, -8, -12, 2, 5, 7, 11}, {-3, -7, -9, -11, 2, 6, 8, 10}, {-4, -7, -8, -11, 3, 6, 7, 10}, {-3, -5, -8, -11, 2, 4, 7, 10},
                                      {-2, -6, -8, -10, 1, 5, 7, 9},  {-2, -5, -8, -10, 1, 4, 7, 9},  {-2, -4, -8, -10, 1, 3, 7, 9},  {-2, -5, -7, -10, 1, 4, 6, 9},
                                      {-3, -4, -7, -10, 2, 3, 6, 9},  {-1, -2, -3, -10, 0, 1, 2, 9},  {-4, -6, -8, -9, 3, 5, 7, 8},   {-3, -5, -7, -9, 2, 4, 6, 8}};

void bu_dec_eac_alpha(const uint8_t b[8], uint8_t out[16])
{
    const int base = b[0], mult = b[1] >> 4, table = b[1] & 15;
    uint64_t sel = 0;
    for (int i = 2; i < 8; i++) sel = (sel << 8) | b[i];
    for (int x = 0; x < 4; x++)
        for (int y = 0; y < 4; y++) {
            const int i = x * 4 + y; /* texel i of the column-major order: MSB first, 3 bits each */
            const int s = (int)((sel >> (45 - 3 * i)) & 7);
            int v = base + EAC_MOD[table][s] * mult;
            v = v < 0 ? 0 : v > 255 ? 255 : v;
            out[y * 4 + x] = (uint8_t)v;
        }
}

/* ================================================================================================ ETC1 */
/* ETC1 / ETC2 RGB colour block (8 bytes).  The 64-bit block is read big-endian: bytes 0..2 base colours, byte 3 = table
 * codeword 1 (bits 7..5), table codeword 2 (bits 4..2), diff bit (1), flip bit (0); bytes 4..7 = the 32-bit pixel index word,
 * most significant bits of the 16 texels in its upper half, least significant in its lower half, texel j = 4 * x + y (the
 * texels run down the columns) at bit j of either half.
 *   individual   (diff 0): two 4-bit base colours, R1 | R2 << 4 per byte, each extended by replication (x * 17).
 *   differential (diff 1): a 5-bit base colour and a 3-bit two's-complement delta per byte; the second colour is their sum,
 *                which must stay in 0..31 for ETC1.  ETC2 uses the overflow: R out of range = T mode, else G = H mode, else
 *                B = planar mode.  5-bit values are extended as (x << 3) | (x >> 2).
 *   flip 0: sub-block 1 = columns 0-1, sub-block 2 = columns 2-3;  flip 1: sub-block 1 = rows 0-1, sub-block 2 = rows 2-3.
 *   pixel index (msb, lsb): 0 0 -> +a, 0 1 -> +b, 1 0 -> -a, 1 1 -> -b, {a, b} the row of the intensity table below.
 * ETC2 T / H / planar blocks are detected, not decoded (their texels are returned as zeros). */
static const int ETC1_INTEN[8][2] = {{2, 8}, {5, 17}, {9, 29}, {13, 42}, {18, 60}, {24, 80}, {33, 106}, {47, 183}};

enum { ETC_INDIVIDUAL = 0, ETC_DIFFERENTIAL = 1, ETC_T = 2, ETC_H = 3, ETC_PLANAR = 4 };

/* fields[32]: base colour 1 RGB (4 or 5 bits), base colour 2 RGB, codeword 1, codeword 2, diff, flip, ETC2 mode, 0, then the
 * selector of each texel in ROW-major order as an index 0..3 into the table row in increasing order {-b, -a, +a, +b}, 4 zeros */
int bu_dec_etc1(const uint8_t b[8], uint8_t out[64], uint8_t fields[32])
{
    memset(out, 0, 64);
    memset(fields, 0, 32);
    const int diff = (b[3] >> 1) & 1, flip = b[3] & 1;
    const int cw[2] = {b[3] >> 5, (b[3] >> 2) & 7};
    int base[2][3], mode = diff ? ETC_DIFFERENTIAL : ETC_INDIVIDUAL;
    for (int c = 0; c < 3; c++) {
        if (!diff) {
            base[0][c] = b[c] >> 4;
            base[1][c] = b[c] & 15;
        } else {
            const int d = (b[c] & 7) >= 4 ? (b[c] & 7) - 8 : (b[c] & 7);
            base[0][c] = b[c] >> 3;
            base[1][c] = base[0][c] + d;
            if ((base[1][c] < 0 || base[1][c] > 31) && mode == ETC_DIFFERENTIAL) mode = c == 0 ? ETC_T : c == 1 ? ETC_H : ETC_PLANAR;
        }
    }
    fields[6] = (uint8_t)cw[0];
    fields[7] = (uint8_t)cw[1];
    fields[8] = (uint8_t)diff;
    fields[9] = (uint8_t)flip;
    fields[10] = (uint8_t)mode;
    if (mode > ETC_DIFFERENTIAL) return mode;
    for (int s = 0; s < 2; s++)
        for (int c = 0; c < 3; c++) fields[3 * s + c] = (uint8_t)base[s][c];
    const uint32_t idx = (uint32_t)b[4] << 24 | (uint32_t)b[5] << 16 | (uint32_t)b[6] << 8 | b[7];
    static const int TABLE_INDEX[4] = {2, 3, 1, 0}; /* pixel index value -> position in {-b, -a, +a, +b} */
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 4; x++) {
            const int j = 4 * x + y, s = flip ? y >= 2 : x >= 2;
            const int msb = (idx >> (16 + j)) & 1, lsb = (idx >> j) & 1;
            const int a = ETC1_INTEN[cw[s]][0], bb = ETC1_INTEN[cw[s]][1];
            const int mod = lsb ? (msb ? -bb : bb) : (msb ? -a : a);
            fields[12 + 4 * y + x] = (uint8_t)TABLE_INDEX[2 * msb + lsb];
            for (int c = 0; c < 3; c++) {
                const int e = diff ? (base[s][c] << 3) | (base[s][c] >> 2) : base[s][c] * 17;
                const int v = e + mod;
                out[4 * (4 * y + x) + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
            }
            out[4 * (4 * y + x) + 3] = 255;
        }
    return mode;
}

/* ---- batch wrappers for the ctypes tests ---- */
void bu_dec_astc_batch(const uint8_t* in, size_t n, uint8_t* out, uint8_t* st)
{
    for (size_t i = 0; i < n; i++) st[i] = (uint8_t)bu_dec_astc_4x4(in + 16 * i, out + 64 * i);
}
void bu_dec_bc7_batch(const uint8_t* in, size_t n, uint8_t* out, uint8_t* st)
{
    for (size_t i = 0; i < n; i++) st[i] = (uint8_t)bu_dec_bc7(in + 16 * i, out + 64 * i);
}
void bu_dec_eac_batch(const uint8_t* in, size_t stride, size_t n, uint8_t* out)
{
    for (size_t i = 0; i < n; i++) bu_dec_eac_alpha(in + stride * i, out + 16 * i);
}

/* stride 8: ETC1 blocks; stride 16 with in + 8: the colour half of ETC2 RGBA blocks */
void bu_dec_etc1_batch(const uint8_t* in, size_t stride, size_t n, uint8_t* out, uint8_t* fields)
{
    for (size_t i = 0; i < n; i++) bu_dec_etc1(in + stride * i, out + 64 * i, fields + 32 * i);
}

/* the specification's ETC1 intensity table {a, b} per codeword, exported for the tests' candidate colours */
const int16_t ETC1_INTEN_EXPORT[16] = {2, 8, 5, 17, 9, 29, 13, 42, 18, 60, 24, 80, 33, 106, 47, 183};

/* the specification's EAC modifier table, exported so that a test can rebuild a block's candidate values */
const int8_t EAC_MOD_EXPORT[128] = {-3, -6, -9, -15, 2, 5, 8, 14, -3, -7, -10, -13, 2, 6, 9, 12, -2, -5, -8, -13, 1, 4, 7, 12, -2, -4, -6, -13, 1, 3, 5, 12,
                                    -3, -6, -8, -12, 2, 5, 7, 11, -3, -7, -9, -11, 2, 6, 8, 10, -4, -7, -8, -11, 3, 6, 7, 10, -3, -5, -8, -11, 2, 4, 7, 10,
                                    -2, -6, -8, -10, 1, 5, 7, 9,  -2, -5, -8, -10, 1, 4, 7, 9,  -2, -4, -8, -10, 1, 3, 7, 9,  -2, -5, -7, -10, 1, 4, 6, 9,
                                    -3, -4, -7, -10, 2, 3, 6, 9,  -1, -2, -3, -10, 0, 1, 2, 9,  -4, -6, -8, -9, 3, 5, 7, 8,   -3, -5, -7, -9, 2, 4, 6, 8};
