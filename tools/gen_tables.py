#!/usr/bin/env python3
"""Generate the format-constant tables used by the oracle and the HIP kernels.

The numbers are Basis Universal / ASTC / BC7 / ETC format constants.  They are
read from the reference checkout (default /root/reference, read-only) at
generation time and re-emitted in THIS repo's own packed layout (one record per
UASTC partition pattern, 2 bits per texel, nibble-packed anchors ...), so the
generated header is data, not reference source.  The two BC7 "optimal
endpoint" tables are not read at all: they are recomputed by the brute-force
search the reference documents (bc7.rs:1158-1250) and then compared with the
reference literals as a self-check.

Usage:  python tools/gen_tables.py [--ref /root/reference] [--out basisu_rs_amd/csrc/bu_tables.h]
                                   [--oracle-out oracle/bu_oracle_tables.h]
The output is committed; the GPU box never runs this script.
"""
import argparse
import os
import re
import sys


def strip_comments(text):
    text = re.sub(r"//[^\n]*", "", text)
    return text


def table_body(text, name):
    """Return the text between '= [' / '= &[' and the matching '];' of item `name`."""
    m = re.search(r"(?:static|const)\s+" + re.escape(name) + r"\s*:[^=]*=\s*&?\[", text)
    if not m:
        raise KeyError(name)
    i = m.end()
    depth = 1
    j = i
    while depth:
        c = text[j]
        if c == "[":
            depth += 1
        elif c == "]":
            depth -= 1
        j += 1
    return text[i : j - 1]


TOKEN = re.compile(r"-?0x[0-9A-Fa-f_]+|-?0b[01_]+|-?\d+|true|false")


def ints(body):
    out = []
    for t in TOKEN.findall(body):
        if t == "true":
            out.append(1)
        elif t == "false":
            out.append(0)
        else:
            out.append(int(t.replace("_", ""), 0))
    return out


def chunks(v, n):
    assert len(v) % n == 0
    return [v[i : i + n] for i in range(0, len(v), n)]


def pack2(pattern16):
    """16 subset ids (0..2) -> u32, 2 bits per texel, texel 0 in the low bits."""
    v = 0
    for i, s in enumerate(pattern16):
        v |= (s & 3) << (2 * i)
    return v


def pack_nibbles(vals):
    v = 0
    for i, s in enumerate(vals):
        v |= (s & 15) << (4 * i)
    return v


def brute_mode6():
    """bc7.rs:1158-1212 restated: best (l,h) 7-bit pair with p-bit 0 at 4-bit weight index 5."""
    w = 21  # WEIGHTS4[5]
    tab = []
    for c in range(256):
        best = (0, 0)
        best_err = 1 << 30
        for l in range(128):
            low = l << 1
            for h in range(l, 128):
                high = h << 1
                k = (low * (64 - w) + high * w + 32) >> 6
                err = (k - c) * (k - c)
                if err < best_err:
                    best_err = err
                    best = (l, h)
        tab.append(best)
    return tab


def brute_mode5():
    """bc7.rs:1214-1250 restated: best (l,h) 7-bit pair at 2-bit weight index 1."""
    w = 21  # WEIGHTS2[1]
    tab = []
    for c in range(256):
        best = (0, 0)
        best_err = 1 << 30
        for l in range(128):
            low = (l << 1) | (l >> 6)
            for h in range(l, 128):
                high = (h << 1) | (h >> 6)
                k = (low * (64 - w) + high * w + 32) >> 6
                err = (k - c) * (k - c)
                if err < best_err:
                    best_err = err
                    best = (l, h)
        assert best_err == 0
        tab.append(best)
    return tab


def bc1_solid_pairs(bits):
    """for every 8-bit v, the (a, b) of `bits`-bit values whose thirds point 2 e(a) + e(b) lies nearest 3v
    (e = bit replication to 8 bits); ties -> smaller |a - b|, then smaller a, then smaller b.  Exhaustive."""
    n = 1 << bits
    e = [(c << (8 - bits)) | (c >> (2 * bits - 8)) for c in range(n)]
    return [min(((a, b) for a in range(n) for b in range(n)), key=lambda p: (abs(2 * e[p[0]] + e[p[1]] - 3 * v), abs(p[0] - p[1]), p[0], p[1]))
            for v in range(256)]


# The partition shapes of the BPTC (BC7) specification, 4x4 texels in raster order.
BC7_PART2 = [
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22,
]
BC7_PART3 = [
    0xAA685050, 0x6A5A5040, 0x5A5A4200, 0x5450A0A8, 0xA5A50000, 0xA0A05050, 0x5555A0A0, 0x5A5A5050,
    0xAA550000, 0xAA555500, 0xAAAA5500, 0x90909090, 0x94949494, 0xA4A4A4A4, 0xA9A59450, 0x2A0A4250,
    0xA5945040, 0x0A425054, 0xA5A5A500, 0x55A0A0A0, 0xA8A85454, 0x6A6A4040, 0xA4A45000, 0x1A1A0500,
    0x0050A4A4, 0xAAA59090, 0x14696914, 0x69691400, 0xA08585A0, 0xAA821414, 0x50A4A450, 0x6A5A0200,
    0xA9A58000, 0x5090A0A8, 0xA8A09050, 0x24242424, 0x00AA5500, 0x24924924, 0x24499224, 0x50A50A50,
    0x500AA550, 0xAAAA4444, 0x66660000, 0xA5A0A5A0, 0x50A050A0, 0x69286928, 0x44AAAA44, 0x66666600,
    0xAA444444, 0x54A854A8, 0x95809580, 0x96969600, 0xA85454A8, 0x80959580, 0xAA141414, 0x96960000,
    0xAAAA1414, 0xA05050A0, 0xA0A5A5A0, 0x96000000, 0x40804080, 0xA9A8A9A8, 0xAAAAAA44, 0x2A4A5254,
]


def fmt_array(ctype, name, vals, per_line=12, hexw=None):
    lines = []
    for i in range(0, len(vals), per_line):
        row = vals[i : i + per_line]
        if hexw:
            lines.append("    " + ", ".join("0x%0*X" % (hexw, v) for v in row) + ",")
        else:
            lines.append("    " + ", ".join(str(v) for v in row) + ",")
    return "BU_TABLE %s %s[%d] = {\n%s\n};\n" % (ctype, name, len(vals), "\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "basisu_rs_amd", "csrc", "bu_tables.h"))
    ap.add_argument("--oracle-out", default=os.path.join(os.path.dirname(__file__), "..", "oracle", "bu_oracle_tables.h"))
    args = ap.parse_args()

    rd = lambda p: strip_comments(open(os.path.join(args.ref, p)).read())
    uastc = rd("src/uastc.rs")
    astc = rd("src/target_formats/astc.rs")
    bc7 = rd("src/target_formats/bc7.rs")
    etc = rd("src/target_formats/etc.rs")

    out = []
    out.append("// GENERATED by tools/gen_tables.py -- do not edit.\n"
               "// Basis Universal / ASTC / BC7 / ETC format constants in this repo's packed layout.\n"
               "// Provenance of each table is cited next to it (reference file:line).\n"
               "#pragma once\n#include <stdint.h>\n"
               "#ifndef BU_TABLE\n#define BU_TABLE static const\n#endif\n")

    # ---- mode code LUT (uastc.rs:560-577) --------------------------------
    mode_lut = ints(table_body(uastc, "MODE_LUT"))
    assert len(mode_lut) == 128
    out.append("// 7-bit code -> UASTC mode id, 19 = invalid (uastc.rs:560-577)\n")
    out.append(fmt_array("uint8_t", "BU_MODE_LUT", mode_lut, 16))

    # ---- partition records -------------------------------------------------
    p2 = chunks(ints(table_body(uastc, "PATTERNS_2")), 16)
    p3 = chunks(ints(table_body(uastc, "PATTERNS_3")), 16)
    p23 = chunks(ints(table_body(uastc, "PATTERNS_2_3")), 16)
    a2 = chunks(ints(table_body(uastc, "PATTERNS_2_ANCHORS")), 2)
    a3 = chunks(ints(table_body(uastc, "PATTERNS_3_ANCHORS")), 3)
    a23 = chunks(ints(table_body(uastc, "PATTERNS_2_3_ANCHORS")), 2)
    assert (len(p2), len(p3), len(p23)) == (30, 11, 19)
    s2 = ints(table_body(astc, "PATTERNS_2_ASTC_INDEX_10"))
    s3 = ints(table_body(astc, "PATTERNS_3_ASTC_INDEX_10"))
    s23 = ints(table_body(astc, "PATTERNS_2_3_ASTC_INDEX_10"))
    b2 = chunks(ints(table_body(bc7, "PATTERNS_2_BC7")), 16)
    b3 = chunks(ints(table_body(bc7, "PATTERNS_3_BC7")), 16)
    b23 = chunks(ints(table_body(bc7, "PATTERNS_2_3_BC7")), 16)
    i2 = chunks(ints(table_body(bc7, "PATTERNS_2_BC7_INDEX_INV")), 2)
    i3 = chunks(ints(table_body(bc7, "PATTERNS_3_BC7_INDEX_PERM")), 2)
    i23 = chunks(ints(table_body(bc7, "PATTERNS_2_3_BC7_INDEX_PERM")), 2)
    perm3 = chunks(ints(table_body(bc7, "PATTERNS_3_BC7_TO_ASTC_PERMUTATIONS")), 3)
    perm23 = chunks(ints(table_body(bc7, "PATTERNS_2_3_BC7_TO_ASTC_PERMUTATIONS")), 3)
    ba2 = chunks(ints(table_body(bc7, "PATTERNS_2_BC7_ANCHORS")), 2)
    ba3 = chunks(ints(table_body(bc7, "PATTERNS_3_BC7_ANCHORS")), 3)
    assert len(ba2) == 64 and len(ba3) == 64

    recs = []  # (upat, uanch, astc_seed, bpat, bpart, banch, perm)
    for k in range(30):  # 2-subset family, records 0..29
        idx, inv = i2[k]
        perm = [1, 0] if inv else [0, 1]
        recs.append((pack2(p2[k]), pack_nibbles(a2[k]), s2[k], pack2(b2[k]), idx, pack_nibbles(ba2[idx]), pack2(perm)))
    for k in range(11):  # 3-subset family, records 30..40
        idx, p = i3[k]
        recs.append((pack2(p3[k]), pack_nibbles(a3[k]), s3[k], pack2(b3[k]), idx, pack_nibbles(ba3[idx]), pack2(perm3[p])))
    for k in range(19):  # mode-7 family (2 UASTC subsets -> 3 BC7 subsets), records 41..59
        idx, p = i23[k]
        recs.append((pack2(p23[k]), pack_nibbles(a23[k]), s23[k], pack2(b23[k]), idx, pack_nibbles(ba3[idx]), pack2(perm23[p])))
    # record 60: UASTC mode 1 (1 subset) emitted as BC7 mode 3 partition 0 with both
    # subsets = the single endpoint pair (bc7.rs:119-127)
    idx0 = i2[0][0]
    recs.append((0, 0, 0, pack2(b2[0]), idx0, pack_nibbles(ba2[idx0]), pack2([0, 0])))

    out.append(
        "// One record per UASTC partition pattern.  Families: [0,30) 2-subset, [30,41) 3-subset,\n"
        "// [41,60) mode 7 (2 UASTC subsets / 3 BC7 subsets), 60 = UASTC mode 1 -> BC7 mode 3.\n"
        "//   upat   : UASTC/ASTC subset of each texel, 2 bits/texel, texel 0 low (uastc.rs:748-789)\n"
        "//   uanch  : UASTC anchor texel of subset s in nibble s (uastc.rs:792-811)\n"
        "//   seed   : 10-bit ASTC partition seed (astc.rs:183-193)\n"
        "//   bpat   : BC7 subset of each texel, 2 bits/texel (bc7.rs:656-696)\n"
        "//   bpart  : BC7 partition id (bc7.rs:592-622)\n"
        "//   banch  : BC7 anchor texel of BC7 subset s in nibble s (bc7.rs:701-722)\n"
        "//   perm   : UASTC subset feeding BC7 subset s in bits [2s,2s+2) (bc7.rs:592-627, 144)\n"
        "typedef struct { uint32_t upat, bpat; uint16_t seed, uanch, banch; uint8_t bpart, perm; } bu_part_rec;\n"
        "#define BU_PART_BASE2 0\n#define BU_PART_BASE3 30\n#define BU_PART_BASE23 41\n#define BU_PART_MODE1 60\n")
    lines = []
    for r in recs:
        lines.append("    {0x%08Xu, 0x%08Xu, %4d, 0x%03X, 0x%03X, %2d, 0x%02X}," % (r[0], r[3], r[2], r[1], r[5], r[4], r[6]))
    out.append("BU_TABLE bu_part_rec BU_PART[%d] = {\n%s\n};\n" % (len(recs), "\n".join(lines)))

    # ---- BISE endpoint dequantisation LUTs (uastc.rs:585-614 + astc.rs:309-331) ----
    # ranges actually used by UASTC: 7,8,11,12,13,18,19,20 (uastc.rs:530-556)
    bise_body = table_body(astc, "BISE_RANGES")
    rows = re.findall(r'bits:\s*(\d+),\s*trits:\s*(\d+),\s*quints:\s*(\d+),\s*deq_b:\s*b"([^"]*)",\s*deq_c:\s*(\d+)', bise_body)
    assert len(rows) == 21
    bise = [(int(b), int(t), int(q), s, int(c)) for b, t, q, s, c in rows]

    def unquant(range_idx, tq, bits_v):
        b, t, q, deq_b, deq_c = bise[range_idx]
        if t == 0 and q == 0 and b > 0:
            bits_la = (bits_v << (8 - b)) & 0xFFFF
            val = 0
            while bits_la > 0:
                val |= bits_la
                bits_la >>= b
            return val & 0xFF
        a = 511 if (bits_v & 1) else 0
        bb = 0
        for j in range(9):
            bb <<= 1
            ch = deq_b[j]
            if ch != "0":
                bb |= (bits_v >> (ord(ch) - ord("a"))) & 1
        val = (tq * deq_c + bb) & 0xFFFF
        val ^= a
        return ((a & 0x80) | (val >> 2)) & 0xFF

    out.append("// BISE range facts for the ranges UASTC uses: {bits, trits, quints} (astc.rs:309-331)\n")
    out.append("typedef struct { uint8_t bits, trits, quints, lut_ofs_div8; } bu_bise_rec;\n")
    used = [7, 8, 11, 12, 13, 18, 19, 20]
    lut = []
    ofs = {}
    for r in used:
        b, t, q, _, _ = bise[r]
        n_tq = 3 if t else (5 if q else 1)
        ofs[r] = len(lut)
        # index = tq << bits | bits_value
        for tq in range(n_tq):
            for v in range(1 << b):
                lut.append(unquant(r, tq, v))
        while len(lut) % 8:
            lut.append(0)
    lines = []
    for r in range(21):
        b, t, q, _, _ = bise[r]
        lines.append("    {%d, %d, %d, %d}," % (b, t, q, (ofs.get(r, 0) // 8)))
    out.append("BU_TABLE bu_bise_rec BU_BISE[21] = {\n%s\n};\n" % "\n".join(lines))
    out.append("// dequantised endpoint = BU_ENDPOINT_DEQ[8*lut_ofs_div8 + (trit_or_quint << bits | bits_value)]\n"
               "// (uastc.rs:585-614 evaluated for every input)\n")
    out.append(fmt_array("uint8_t", "BU_ENDPOINT_DEQ", lut, 16))

    # ---- ASTC tables -------------------------------------------------------
    out.append("// ASTC integer-sequence packing of 3 quints / 5 trits (astc.rs:208-264)\n")
    out.append(fmt_array("uint8_t", "BU_ASTC_QUINT_ENC", ints(table_body(astc, "ASTC_QUINT_ENCODE_LUT")), 16, 2))
    out.append(fmt_array("uint8_t", "BU_ASTC_TRIT_ENC", ints(table_body(astc, "ASTC_TRIT_ENCODE_LUT")), 16, 2))
    out.append("// 13-bit ASTC block mode + config per UASTC mode (astc.rs:333-354)\n")
    out.append(fmt_array("uint16_t", "BU_ASTC_BLOCK_MODE13", ints(table_body(astc, "UASTC_TO_ASTC_BLOCK_MODE_13")), 10, 4))

    # ---- weight tables -----------------------------------------------------
    for nm, cname in (("LUT1", "BU_WEIGHT_DEQ1"), ("LUT2", "BU_WEIGHT_DEQ2"), ("LUT3", "BU_WEIGHT_DEQ3"), ("LUT4", "BU_WEIGHT_DEQ4"), ("LUT5", "BU_WEIGHT_DEQ5")):
        out.append(fmt_array("uint8_t", cname, ints(table_body(uastc, nm)), 16))
    out.append("// UASTC weight -> BC7 weight remaps (bc7.rs:378-384)\n")
    for nm, cname in (("UASTC_1_TO_BC7_2", "BU_W1_TO_BC7_2"), ("UASTC_2_TO_BC7_4", "BU_W2_TO_BC7_4"), ("UASTC_3_TO_BC7_4", "BU_W3_TO_BC7_4"), ("UASTC_5_TO_BC7_4", "BU_W5_TO_BC7_4")):
        out.append(fmt_array("uint8_t", cname, ints(table_body(bc7, nm)), 16))
    out.append("// UASTC mode -> BC7 mode (bc7.rs:582-589)\n")
    out.append(fmt_array("uint8_t", "BU_UASTC_TO_BC7_MODE", ints(table_body(bc7, "UASTC_TO_BC7_MODES")), 20))

    # ---- BC7 solid-colour optimal endpoints, recomputed ---------------------
    m6 = brute_mode6()
    m5 = brute_mode5()
    ref5 = chunks(ints(table_body(bc7, "BC7_MODE_5_OPTIMAL_ENDPOINTS")), 2)
    ref6 = chunks(ints(table_body(bc7, "BC7_MODE_6_OPTIMAL_ENDPOINTS")), 2)
    assert [list(x) for x in m5] == ref5, "mode-5 table mismatch vs reference"
    assert [list(x) for x in m6] == ref6[1:], "mode-6 table mismatch vs reference"
    assert ref6[0] == [0, 0]
    out.append("// BC7 mode 5 solid colour: lo | hi<<8 (recomputed by brute force, bc7.rs:1214-1250; checked == bc7.rs:734-863)\n")
    out.append(fmt_array("uint16_t", "BU_BC7_M5_OPT", [l | (h << 8) for l, h in m5], 12, 4))
    out.append("// BC7 mode 6 solid colour, 257 entries: index c + (p ? 0 : 1) (bc7.rs:1126-1131, 1158-1212; checked == bc7.rs:866-1124)\n")
    out.append(fmt_array("uint16_t", "BU_BC7_M6_OPT", [0] + [l | (h << 8) for l, h in m6], 12, 4))

    # ---- ETC tables ----------------------------------------------------------
    em = ints(table_body(etc, "ETC1_MODIFIERS"))
    assert len(em) == 32
    out.append("// ETC1 intensity modifier tables [8][4] (etc.rs:435-445)\n")
    out.append(fmt_array("int16_t", "BU_ETC1_MOD", em, 4))
    am = ints(table_body(etc, "ETC2_ALPHA_MODIFIERS"))
    assert len(am) == 128
    out.append("// ETC2 EAC alpha modifier tables [16][8] (etc.rs:450-468)\n")
    out.append(fmt_array("int8_t", "BU_ETC2_ALPHA_MOD", am, 8))
    out.append("// selector id -> ETC1 2-bit code (etc.rs:433)\n")
    out.append(fmt_array("uint8_t", "BU_SEL_TO_ETC1", ints(table_body(etc, "SELECTOR_ID_TO_ETC1")), 4))

    # ---- BC1 solid-colour endpoints (no counterpart in the reference) ----
    out.append("// BC1 solid colour, 5-bit channel: v -> a | b<<8, the pair minimising |2 e5(a) + e5(b) - 3v|, then |a - b|, then a, then b\n"
               "// (exhaustive search, bc1_solid_pairs)\n")
    out.append(fmt_array("uint16_t", "BU_BC1_OM5", [a | (b << 8) for a, b in bc1_solid_pairs(5)], 12, 4))
    out.append("// the same for the 6-bit channel (e6)\n")
    out.append(fmt_array("uint16_t", "BU_BC1_OM6", [a | (b << 8) for a, b in bc1_solid_pairs(6)], 12, 4))

    # ---- BPTC partition tables for the block decoder (bu_decode_blocks.hpp) ----
    # All 64 + 64 partitions of the BPTC specification (the records above hold only the ones UASTC maps to).  The shapes are the
    # specification's own tables, written here in their usual compact form: bit t of a 2-subset entry = subset of texel t, and 2 bits
    # per texel, texel 0 low, for 3 subsets.  Self-check: every record above must agree with them.
    assert len(BC7_PART2) == 64 and len(BC7_PART3) == 64
    for r in recs[:30] + recs[60:]:
        assert sum(((BC7_PART2[r[4]] >> t) & 1) << (2 * t) for t in range(16)) == r[3], r
    for r in recs[30:60]:
        assert BC7_PART3[r[4]] == r[3], r
    out.append("// BPTC partitions, 2 subsets: bit t = subset of texel t (specification table \"partition table for 2 subset\")\n")
    out.append(fmt_array("uint16_t", "BU_BC7_PART2", BC7_PART2, 12, 4))
    out.append("// BPTC partitions, 3 subsets: 2 bits per texel, texel 0 low\n")
    out.append(fmt_array("uint32_t", "BU_BC7_PART3", BC7_PART3, 8, 8))
    out.append("// BPTC anchor texels: [p] = second subset's of 2-subset partition p; [64 + p] = a1 | a2 << 4 of 3-subset partition p (bc7.rs:701-722)\n")
    assert all(a[0] == 0 for a in ba2) and all(a[0] == 0 for a in ba3)
    out.append(fmt_array("uint8_t", "BU_BC7_ANCHORS", [a[1] for a in ba2] + [a[1] | (a[2] << 4) for a in ba3], 16, 2))


    # ======================= oracle tables (unpacked, formula-level) =======================
    oo = []
    oo.append("// GENERATED by tools/gen_tables.py -- do not edit.\n"
              "// Format constants for the CPU oracle, kept in their natural (unpacked) shape so the oracle\n"
              "// does not share the product's packed layout or its precomputed LUTs.\n"
              "#pragma once\n#include <stdint.h>\n")

    def arr2(ctype, name, rows, cite):
        w = len(rows[0])
        body = "\n".join("    {" + ", ".join(str(v) for v in r) + "}," for r in rows)
        return "// %s\nstatic const %s %s[%d][%d] = {\n%s\n};\n" % (cite, ctype, name, len(rows), w, body)

    def arr1(ctype, name, vals, cite, per_line=16):
        body = "\n".join("    " + ", ".join(str(v) for v in vals[i:i + per_line]) + "," for i in range(0, len(vals), per_line))
        return "// %s\nstatic const %s %s[%d] = {\n%s\n};\n" % (cite, ctype, name, len(vals), body)

    oo.append(arr1("uint8_t", "ORC_MODE_LUT", mode_lut, "uastc.rs:560-577"))
    oo.append(arr2("uint8_t", "ORC_PAT2", p2, "uastc.rs:748-764"))
    oo.append(arr2("uint8_t", "ORC_PAT3", p3, "uastc.rs:768-775"))
    oo.append(arr2("uint8_t", "ORC_PAT23", p23, "uastc.rs:778-789"))
    oo.append(arr2("uint8_t", "ORC_PAT2_ANCH", a2, "uastc.rs:792-798"))
    oo.append(arr2("uint8_t", "ORC_PAT3_ANCH", a3, "uastc.rs:801-804"))
    oo.append(arr2("uint8_t", "ORC_PAT23_ANCH", a23, "uastc.rs:807-811"))
    oo.append(arr1("uint16_t", "ORC_PAT2_ASTC", s2, "astc.rs:183-186"))
    oo.append(arr1("uint16_t", "ORC_PAT3_ASTC", s3, "astc.rs:188-189"))
    oo.append(arr1("uint16_t", "ORC_PAT23_ASTC", s23, "astc.rs:191-193"))
    oo.append(arr1("uint8_t", "ORC_ASTC_QUINT_ENC", ints(table_body(astc, "ASTC_QUINT_ENCODE_LUT")), "astc.rs:208-217"))
    oo.append(arr1("uint8_t", "ORC_ASTC_TRIT_ENC", ints(table_body(astc, "ASTC_TRIT_ENCODE_LUT")), "astc.rs:247-264"))
    oo.append(arr1("uint16_t", "ORC_ASTC_BLOCK_MODE13", ints(table_body(astc, "UASTC_TO_ASTC_BLOCK_MODE_13")), "astc.rs:333-354"))
    body = "\n".join('    {%d, %d, %d, "%s", %d},' % (b, t, q, s_.replace(" ", "0"), c) for b, t, q, s_, c in bise)
    oo.append("// astc.rs:299-331 (deq_b: one char per output bit, MSB first, '0' = constant 0, 'a'.. = input bit)\n"
              "typedef struct { uint8_t bits, trits, quints; char deq_b[10]; uint8_t deq_c; } orc_bise;\n"
              "static const orc_bise ORC_BISE[21] = {\n%s\n};\n" % body)
    for nm, cname in (("LUT1", "ORC_WLUT1"), ("LUT2", "ORC_WLUT2"), ("LUT3", "ORC_WLUT3"), ("LUT4", "ORC_WLUT4"), ("LUT5", "ORC_WLUT5")):
        oo.append(arr1("uint8_t", cname, ints(table_body(uastc, nm)), "uastc.rs:698-705"))
    for nm, cname in (("UASTC_1_TO_BC7_2", "ORC_W1_BC7_2"), ("UASTC_2_TO_BC7_4", "ORC_W2_BC7_4"), ("UASTC_3_TO_BC7_4", "ORC_W3_BC7_4"), ("UASTC_5_TO_BC7_4", "ORC_W5_BC7_4")):
        oo.append(arr1("uint8_t", cname, ints(table_body(bc7, nm)), "bc7.rs:378-384"))
    oo.append(arr1("uint8_t", "ORC_UASTC_TO_BC7_MODE", ints(table_body(bc7, "UASTC_TO_BC7_MODES")), "bc7.rs:582-589", 20))
    oo.append(arr2("uint8_t", "ORC_PAT2_BC7_INDEX_INV", i2, "bc7.rs:592-601 {index, inv}"))
    oo.append(arr2("uint8_t", "ORC_PAT3_BC7_INDEX_PERM", i3, "bc7.rs:604-608 {index, perm id}"))
    oo.append(arr2("uint8_t", "ORC_PAT3_BC7_PERMS", perm3, "bc7.rs:611-613"))
    oo.append(arr2("uint8_t", "ORC_PAT23_BC7_INDEX_PERM", i23, "bc7.rs:616-622 {index, perm id}"))
    oo.append(arr2("uint8_t", "ORC_PAT23_BC7_PERMS", perm23, "bc7.rs:625-627"))
    oo.append(arr2("uint8_t", "ORC_PAT2_BC7", b2, "bc7.rs:656-672"))
    oo.append(arr2("uint8_t", "ORC_PAT3_BC7", b3, "bc7.rs:675-682"))
    oo.append(arr2("uint8_t", "ORC_PAT23_BC7", b23, "bc7.rs:685-696"))
    oo.append(arr2("uint8_t", "ORC_BC7_ANCH2", ba2, "bc7.rs:701-710"))
    oo.append(arr2("uint8_t", "ORC_BC7_ANCH3", ba3, "bc7.rs:713-722"))
    oo.append(arr2("uint8_t", "ORC_BC7_M5_OPT", [list(x) for x in m5], "bc7.rs:734-863 {lo, hi}; recomputed by brute force (bc7.rs:1214-1250)"))
    oo.append(arr2("uint8_t", "ORC_BC7_M6_OPT", [[0, 0]] + [list(x) for x in m6], "bc7.rs:866-1124 {lo, hi}; recomputed by brute force (bc7.rs:1158-1212)"))
    oo.append(arr2("int16_t", "ORC_ETC1_MOD", chunks(em, 4), "etc.rs:435-445"))
    oo.append(arr2("int8_t", "ORC_ETC2_ALPHA_MOD", chunks(am, 8), "etc.rs:450-468"))
    oo.append(arr1("uint8_t", "ORC_SEL_TO_ETC1", ints(table_body(etc, "SELECTOR_ID_TO_ETC1")), "etc.rs:433"))
    opath = os.path.abspath(args.oracle_out)
    with open(opath, "w") as f:
        f.write("\n".join(oo))
    print("wrote", opath)

    path = os.path.abspath(args.out)
    with open(path, "w") as f:
        f.write("\n".join(out))
    print("wrote", path, sum(len(s) for s in out), "bytes")


if __name__ == "__main__":
    sys.exit(main())
