// Host side of the drop-in: the BasisLZ (ETC1S) entropy decoder.  It stays on the CPU by design -- it is symbol-serial (north star:
// "the host/container parser ... stays [on the host] and calls through a thin C-ABI into HIP") -- and feeds the GPU kernels.
// The rest of the host side lives in the three headers included below and is reached through this one: the worker pool
// (bu_host_pool.hpp), the `.basis` container with its CRC-16 and the whole-file plan (bu_container.hpp), the bit reader and the
// Huffman tables (bu_huffman.hpp).
//
// Replaces, for this repo's C++ host facade:
//   src/basis_lz/mod.rs:64-95, 188-656  codebooks, tables section, the per-slice symbol loop
// Written for speed where it is free: the slice loop's fast forms below.  Reads past the end of a section return zeros like the
// reference's reader (bitreader.rs:45,55); everything the reference would `panic!`/`assert!` on is a BU_ERR_BOUNDS status.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/basisu_hip.h"
#include "bu_container.hpp"
#include "bu_host_pool.hpp"
#include "bu_huffman.hpp"

namespace bu_host {

// ---- the steps of the fast slice loops, each written once -------------------------------------------------------------------------
// BasisLz::decode_slice_fast, slice_lex and slice_resolve (below) are three performance forms of one state machine; these are its
// steps.  Every step is forced inline: the state has to live in registers in each of the three loops.  That includes the destructors
// of the structs that own a buffer -- with one left out of line (the compiler did so for EndpointRows, on the unwind path) the struct's
// address escapes and its fields stay in stack memory (profiles/basislz_one_copy.txt).  The structs point into their own buffers, so
// they are not copyable.  decode_slice_exact, the arbiter the fast forms are compared against, shares none of this on purpose.

// The bit window of the lexing steps: `have` valid bits in `acc`.  The slice loops refill it to >= 56 once per block (a block consumes at
// most 16 + 16 + 16 bits outside the rare escape paths, which refill for themselves); bytes past the end read as zeros (bitreader.rs:45,55)
struct BitWindow {
    uint64_t acc = 0;
    unsigned have = 0;
    size_t pos = 0;
    const uint8_t* data;
    size_t len;
    BitWindow(const uint8_t* d, size_t n) : data(d), len(n) {}
    __attribute__((always_inline)) void refill()
    {
        if (pos + 8 <= len) {
            uint64_t w;
            memcpy(&w, data + pos, 8);
            acc |= w << have;
            pos += (63u - have) >> 3;
            have |= 56u;
        } else {
            while (have <= 56) {
                const uint64_t byte = pos < len ? data[pos] : 0;
                pos++;
                acc |= byte << have;
                have += 8;
            }
        }
    }
    // the next 32 bits, for a table probe under the table's mask; drop(n) consumes the code found there
    __attribute__((always_inline)) uint32_t head() const { return (uint32_t)acc; }
    __attribute__((always_inline)) void drop(unsigned n)
    {
        acc >>= n;
        have -= n;
    }
    __attribute__((always_inline)) uint32_t take(unsigned n)
    {
        const uint32_t v = (uint32_t)(acc & ((1ull << n) - 1ull));
        drop(n);
        return v;
    }
    // mod.rs:585-608; false = more than 32 bits (panic!() in the reference)
    __attribute__((always_inline)) bool vlc(unsigned chunk_bits, uint32_t* out)
    {
        uint32_t v = 0;
        for (unsigned ofs = 0;; ofs += chunk_bits) {
            if (ofs >= 32) return false;
            if (have < 16) refill();
            const uint32_t sy = take(chunk_bits + 1);
            v |= (sy & ((1u << chunk_bits) - 1u)) << ofs;
            if (!(sy >> chunk_bits)) break;
        }
        *out = v;
        return true;
    }
};

// The bit-serial half: the window, the four tables (entry = symbol << 5 | code_size, see Huffman::table) and exactly the state that
// decides WHICH table reads next -- predictor bits, predictor-repeat and selector-run counters.  A missing code where the stream goes on
// regardless sets the sticky `bad`; a step that cannot go on returns false.  Either way the fast form gives up.
struct SliceLexer {
    BitWindow w;
    const uint32_t *tp, *td, *ts, *tr;
    const uint32_t mp, md, msel, mr;
    const uint32_t n_sel, hs, rle_sym;
    uint32_t sel_rle = 0, pred_repeat = 0, prev_pred_sym = 0, bad = 0;
    std::vector<uint8_t> saved_bits;  // per 2-block group: the predictors of the odd row below

    SliceLexer(const Huffman& pred, const Huffman& delta, const Huffman& sel, const Huffman& rle, uint32_t n_selectors, uint32_t history_size, size_t nbx,
               const uint8_t* data, size_t len)
        : w(data, len), tp(pred.table()), td(delta.table()), ts(sel.table()), tr(rle.table()), mp((1u << pred.bits()) - 1u),
          md((1u << delta.bits()) - 1u), msel((1u << sel.bits()) - 1u), mr((1u << rle.bits()) - 1u), n_sel(n_selectors), hs(history_size),
          rle_sym((n_selectors + history_size) & 0xFFFFu), saved_bits((nbx + 1) / 2, 0)
    {
    }
    SliceLexer(const SliceLexer&) = delete;
    SliceLexer& operator=(const SliceLexer&) = delete;
    __attribute__((always_inline)) ~SliceLexer() {}
    // the predictor bits of the block pair at the even column bx (block bx: bits 0-1, block bx + 1: bits 2-3).  On an even row they
    // are the low half of the 2 x 2 group's 8 bits -- a symbol, or the previous symbol again inside a repeat run -- and the high
    // half is kept for the odd row below.
    __attribute__((always_inline)) bool pair_bits(size_t bx, bool even, uint32_t* bits)
    {
        if (!even) {
            *bits = saved_bits[bx >> 1];
            return true;
        }
        if (pred_repeat) {
            pred_repeat--;
            *bits = prev_pred_sym;
        } else {
            const uint32_t e0 = tp[w.head() & mp];
            bad |= (e0 & 31u) == 0u;
            w.drop(e0 & 31u);
            const uint32_t sy = e0 >> 5;
            if (sy == 256) {
                uint32_t v;
                if (!w.vlc(4, &v)) return false;
                pred_repeat = v + 2;
                *bits = prev_pred_sym;
                w.refill();
            } else {
                *bits = sy & 0xFF;
                prev_pred_sym = sy & 0xFF;
            }
        }
        saved_bits[bx >> 1] = (uint8_t)(*bits >> 4);
        return true;
    }
    // the delta-endpoint symbol of a block with predictor `pred`.  The code at the window's head is looked up whether or not this
    // block uses it, and consumed by a conditional move: the predictor is a coin toss to the branch predictor (the 4-way switch
    // mispredicts three times in four on real streams)
    __attribute__((always_inline)) uint32_t delta(uint32_t pred)
    {
        const uint32_t ed = td[w.head() & md];
        const bool is3 = pred == 3;
        w.drop(is3 ? (ed & 31u) : 0u);
        bad |= is3 & ((ed & 31u) == 0u);
        return ed >> 5;
    }
    // true = this block lies inside a run of history entry 0 (mod.rs:380-396) and reads no selector code
    __attribute__((always_inline)) bool in_run()
    {
        if (!sel_rle) return false;
        sel_rle--;
        return true;
    }
    // the selector token of a block outside a run: the selector code and, where it starts a run, the run's length.  *tok = the
    // symbol, or n_sel (history entry 0) for the first block of a run
    __attribute__((always_inline)) bool selector_token(uint32_t* tok)
    {
        const uint32_t es = ts[w.head() & msel];
        bad |= (es & 31u) == 0u;
        w.drop(es & 31u);
        uint32_t sym = es >> 5;
        if (sym == rle_sym) {
            if (hs == 0) return false;
            if (w.have < 16) w.refill();
            const uint32_t er = tr[w.head() & mr];
            if ((er & 31u) == 0u) return false;
            w.drop(er & 31u);
            uint32_t run = er >> 5;
            if (run == 63) {
                uint32_t v;
                if (!w.vlc(7, &v)) return false;
                run = v;
            }
            sel_rle = 3 + run - 1;
            sym = n_sel;
        }
        *tok = sym;
        return true;
    }
};

// Endpoint prediction over two rows of per-column endpoint indices.  [0] of either row is the column left of the slice: never a valid
// source, it only keeps the above-left read of column 0 inside the buffer.
struct EndpointRows {
    std::vector<uint16_t> above_v, cur_v;
    uint16_t *above, *cur_row;
    const uint32_t n_ep;
    const bool video;
    uint32_t prev_ep = 0;
    EndpointRows(size_t nbx, uint32_t n_endpoints, bool is_video)
        : above_v(nbx + 1, 0), cur_v(nbx + 1, 0), above(above_v.data() + 1), cur_row(cur_v.data() + 1), n_ep(n_endpoints), video(is_video)
    {
    }
    EndpointRows(const EndpointRows&) = delete;
    EndpointRows& operator=(const EndpointRows&) = delete;
    __attribute__((always_inline)) ~EndpointRows() {}
    // predictor p is invalid where bit p of the edge mask is set: 0 (left) in column 0, 1 (above) in row 0, 2 (above-left) in
    // both -- except in texture video, where 2 means "previous frame" (mod.rs:301-355)
    __attribute__((always_inline)) uint32_t edge_mask(bool first_col, bool first_row) const
    {
        return (first_row ? (video ? 2u : 6u) : 0u) | (first_col ? (video ? 1u : 5u) : 0u);
    }
    // the endpoint index of block bx from its predictor and delta symbol; an invalid predictor (`edge`: edge_mask() on the slice's first
    // row and column, a literal 0 compiles the test away for the interior) or an index past the codebook sets the caller's sticky `bad`
    // (the fused loop passes the lexer's: one flag, one register)
    __attribute__((always_inline)) uint32_t predict(uint32_t pred, uint32_t delta, size_t bx, uint32_t edge, uint32_t& bad)
    {
        bad |= (edge >> pred) & 1u;
        const bool is3 = pred == 3;
        uint32_t e3 = (delta + prev_ep) & 0xFFFFu;
        e3 = e3 >= n_ep ? (e3 - n_ep) & 0xFFFFu : e3;
        bad |= is3 & (e3 >= n_ep);
        const uint32_t e01 = (pred & 1) ? above[bx] : prev_ep;
        const uint32_t e2 = video ? 0u : above[(ptrdiff_t)bx - 1];  // (texture video: the previous frame's index, zero: mod.rs:236-237)
        const uint32_t e = is3 ? e3 : ((pred & 2) ? e2 : e01);      // (copies of earlier, checked indices: < n_ep)
        cur_row[bx] = (uint16_t)e;
        prev_ep = e;
        return e;
    }
    __attribute__((always_inline)) void next_row() { std::swap(above, cur_row); }
};

// The approximate move-to-front history of selector symbols (mod.rs:610-656)
struct SelectorHistory {
    std::vector<uint16_t> hist;
    uint16_t* const h;
    const uint32_t hs;
    uint32_t rover;
    explicit SelectorHistory(uint32_t history_size) : hist(history_size ? history_size : 1, 0), h(hist.data()), hs(history_size), rover(history_size / 2) {}
    SelectorHistory(const SelectorHistory&) = delete;
    SelectorHistory& operator=(const SelectorHistory&) = delete;
    __attribute__((always_inline)) ~SelectorHistory() {}
    __attribute__((always_inline)) uint32_t front() const { return h[0]; }
    __attribute__((always_inline)) uint32_t use(uint32_t hi)
    {
        const uint32_t sel = h[hi];
        const uint16_t t = h[hi / 2];  // (hi == 0: swaps entry 0 with itself)
        h[hi / 2] = (uint16_t)sel;
        h[hi] = t;
        return sel;
    }
    __attribute__((always_inline)) void add(uint32_t sym)
    {
        if (hs) {
            h[rover] = (uint16_t)sym;
            rover = rover + 1 == hs ? hs / 2 : rover + 1;
        }
    }
    // the selector index of a token: a symbol below n_sel enters the history, any other names a history entry (false: past its end).
    // (*sel: a symbol below n_sel or a history entry, i.e. an earlier such symbol or the initial 0)
    __attribute__((always_inline)) bool resolve(uint32_t tok, uint32_t n_sel, uint32_t* sel)
    {
        if (tok >= n_sel) {
            const uint32_t hi = tok - n_sel;
            if (hi >= hs) return false;
            *sel = use(hi);
        } else {
            add(tok);
            *sel = tok;
        }
        return true;
    }
};

// ---- BasisLZ decoder state (basis_lz/mod.rs:50-95) ----
struct BasisLz {
    Huffman endpoint_pred, delta_endpoint, selector, history_rle;
    uint32_t history_size = 0;
    bool is_video = false;
    std::vector<uint32_t> endpoints;  // r5 | g5<<8 | b5<<16 | inten<<24
    std::vector<uint8_t> selectors;   // 8 B per entry: rows[4], etc1_bytes[4]
    // Codebook sizes as the slice loop checks them (mod.rs:443-445).  Kept beside the vectors because bu_read_to decodes the
    // codebooks on another thread WHILE the slices' symbol streams are decoded: the slice loop needs the sizes and the four
    // Huffman tables (init_tables), never the codebook entries.
    uint32_t n_endpoints = 0, n_selectors = 0;

    // mod.rs:461-516
    bu_status decode_endpoints(size_t num, const uint8_t* p, size_t n)
    {
        BitReader r(p, n);
        Huffman model[3], inten;
        for (int m = 0; m < 3; m++) {
            bu_status st = read_huffman_table(r, model[m]);
            if (st) return st;
        }
        bu_status st = read_huffman_table(r, inten);
        if (st) return st;
        const bool grayscale = r.read(1) != 0;
        endpoints.assign(num, 0);
        uint32_t prev[3] = {16, 16, 16}, prev_inten = 0;
        for (size_t i = 0; i < num; i++) {
            uint32_t s;
            if (!inten.decode(r, &s)) return BU_ERR_BASISLZ;
            prev_inten = (s + prev_inten) & 7u;
            uint32_t c[3];
            for (int ch = 0; ch < (grayscale ? 1 : 3); ch++) {
                const Huffman& m = model[prev[ch] <= 9 ? 0 : (prev[ch] <= 21 ? 1 : 2)];  // mod.rs:28-37
                if (!m.decode(r, &s)) return BU_ERR_BASISLZ;
                prev[ch] = (prev[ch] + s) & 31u;  // u8 wrapping_add then & 31
                c[ch] = prev[ch];
            }
            if (grayscale) c[1] = c[2] = c[0];
            endpoints[i] = c[0] | (c[1] << 8) | (c[2] << 16) | (prev_inten << 24);
        }
        return BU_OK;
    }

    // mod.rs:524-583
    bu_status decode_selectors(size_t num, const uint8_t* p, size_t n)
    {
        BitReader r(p, n);
        const bool global = r.read(1), hybrid = r.read(1), raw = r.read(1);
        if (global || hybrid) return BU_ERR_BASISLZ;
        selectors.assign(num * 8, 0);
        Huffman delta;
        if (!raw) {
            bu_status st = read_huffman_table(r, delta);
            if (st) return st;
        }
        uint8_t prev[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < num; i++) {
            uint8_t rows[4];
            for (int y = 0; y < 4; y++) {
                if (raw || i == 0) {
                    rows[y] = (uint8_t)r.read(8);
                } else {
                    uint32_t s;
                    if (!delta.decode(r, &s)) return BU_ERR_BASISLZ;
                    rows[y] = (uint8_t)(s ^ prev[y]);
                }
                prev[y] = rows[y];
            }
            selector_from_rows(rows, &selectors[8 * i]);
        }
        return BU_OK;
    }

    void set_sizes(size_t n_ep, size_t n_sel, bool video)
    {
        is_video = video;
        n_endpoints = (uint32_t)n_ep;
        n_selectors = (uint32_t)n_sel;
    }
    // mod.rs:77-83: the four tables of the slice loop and the history size (sets the sizes itself: the streamed path calls it alone)
    bu_status init_tables(size_t n_ep, size_t n_sel, const uint8_t* tables, size_t tables_len, bool video)
    {
        set_sizes(n_ep, n_sel, video);
        BitReader r(tables, tables_len);
        bu_status st;
        if ((st = read_huffman_table(r, endpoint_pred))) return st;
        if ((st = read_huffman_table(r, delta_endpoint))) return st;
        if ((st = read_huffman_table(r, selector))) return st;
        if ((st = read_huffman_table(r, history_rle))) return st;
        history_size = r.read(13);
        return BU_OK;
    }
    // mod.rs:69-76: both codebooks (errors of the endpoint codebook come first, as in the reference)
    bu_status init_codebooks(const uint8_t* ep, size_t ep_len, const uint8_t* sel, size_t sel_len)
    {
        bu_status st = decode_endpoints(n_endpoints, ep, ep_len);
        if (st) return st;
        return decode_selectors(n_selectors, sel, sel_len);
    }
    // mod.rs:64-95 in the reference's order: codebooks (of the sizes given), then tables
    bu_status init(size_t n_ep, size_t n_sel, const uint8_t* ep, size_t ep_len, const uint8_t* sel, size_t sel_len,
                   const uint8_t* tables, size_t tables_len, bool video)
    {
        set_sizes(n_ep, n_sel, video);
        bu_status st = init_codebooks(ep, ep_len, sel, sel_len);
        if (st) return st;
        return init_tables(n_ep, n_sel, tables, tables_len, video);
    }

    // mod.rs:585-608
    static bool vlc(BitReader& r, unsigned chunk_bits, uint32_t* out)
    {
        uint32_t v = 0;
        for (unsigned ofs = 0;; ofs += chunk_bits) {
            if (ofs >= 32) return false;  // panic!() in the reference
            const uint32_t s = r.read(chunk_bits + 1);
            v |= (s & ((1u << chunk_bits) - 1u)) << ofs;
            if (!(s >> chunk_bits)) break;
        }
        *out = v;
        return true;
    }

    // mod.rs:188-458: the serial symbol loop.  idx[i] = endpoint_index | selector_index << 16, raster order.
    // A slice's stream is serial, so this loop IS the end-to-end time of a single-slice ETC1S file (BASELINE config 4: 1.86 of
    // 2.6 ms).  decode_slice_fast is the same state machine written for the host core's pipeline -- one 8-byte window refill per
    // block, the delta-endpoint code looked up speculatively and consumed by a conditional move, edge violations and missing codes
    // folded into sticky flags -- and decides nothing about errors: whenever a flag is set the exact loop below (decode_slice_exact,
    // the round-1 code, status for status the oracle's) decodes the slice again from its first bit.
    // rows_done (optional): the number of complete block rows in idx[], published row by row (release) for a consumer that
    // works on finished rows while the rest is decoded; only rows free of any irregularity are ever published, and those are
    // final.  abort (optional): checked between rows; a set flag ends the call with BU_ERR_ARGUMENT (the caller discards it).
    bu_status decode_slice(size_t nbx, size_t nby, const uint8_t* data, size_t len, uint32_t* idx, std::atomic<uint32_t>* rows_done = nullptr,
                           const std::atomic<bool>* abort = nullptr) const
    {
        if (nbx && nby && decode_slice_fast(nbx, nby, data, len, idx, rows_done, abort)) return BU_OK;
        if (abort && abort->load(std::memory_order_relaxed)) return BU_ERR_ARGUMENT;
        return decode_slice_exact(nbx, nby, data, len, idx);
    }

    // true = the slice decoded without any irregularity and idx[] is complete; false = anything else (idx[] partly written)
    bool decode_slice_fast(size_t nbx, size_t nby, const uint8_t* data, size_t len, uint32_t* idx, std::atomic<uint32_t>* rows_done = nullptr,
                           const std::atomic<bool>* abort = nullptr) const
    {
        if (n_endpoints == 0 || n_selectors == 0 || n_endpoints > 65536u || n_selectors > 65536u) return false;
        if (!endpoint_pred.bits() || !delta_endpoint.bits() || !selector.bits() || !history_rle.bits()) return false;
        SliceLexer lx = lexer(nbx, data, len);
        EndpointRows ep(nbx, n_endpoints, is_video);
        SelectorHistory hist(lx.hs);  // (sizes and flags the steps already hold are read from them: one register each in the fused loop)
        const bool video = ep.video;
        uint32_t* out_row = idx;
        // one block: the lexer's and the resolver's steps back to back, with two ways out before the selector code.  Returns false
        // where the fast path gives up.
        auto block = [&](size_t bx, uint32_t pred, uint32_t edge) __attribute__((always_inline)) -> bool {
            const uint32_t e = ep.predict(pred, lx.delta(pred), bx, edge, lx.bad);
            if (video && pred == 2) {  // previous frame's selector: zero (mod.rs:236-237, 428-431)
                out_row[bx] = e;
                return true;
            }
            if (lx.in_run()) {  // use_index(0) swaps the entry with itself
                out_row[bx] = e | (hist.front() << 16);
                return true;
            }
            uint32_t tok, sel;
            if (!lx.selector_token(&tok) || !hist.resolve(tok, lx.n_sel, &sel)) return false;
            out_row[bx] = e | (sel << 16);
            return true;
        };
        for (size_t by = 0; by < nby; by++) {
            const bool even = !(by & 1);
            out_row = idx + by * nbx;
            for (size_t bx = 0; bx < nbx; bx += 2) {
                lx.w.refill();
                uint32_t bits;
                if (!lx.pair_bits(bx, even, &bits)) return false;
                if (bx == 0 || by == 0) {
                    if (!block(bx, bits & 3, ep.edge_mask(bx == 0, by == 0))) return false;
                    if (bx + 1 < nbx) {
                        lx.w.refill();
                        if (!block(bx + 1, (bits >> 2) & 3, ep.edge_mask(false, by == 0))) return false;
                    }
                } else {
                    if (!block(bx, bits & 3, 0u)) return false;
                    if (bx + 1 < nbx) {
                        lx.w.refill();
                        if (!block(bx + 1, (bits >> 2) & 3, 0u)) return false;
                    }
                }
            }
            if (lx.bad) return false;
            ep.next_row();
            if (rows_done) {
                rows_done->store((uint32_t)(by + 1), std::memory_order_release);
                if (abort && abort->load(std::memory_order_relaxed)) return false;
            }
        }
        return true;
    }

    // ---- the slice loop on TWO threads (round 4) -----------------------------------------------------------------------------------
    // The loop above is bound by instruction throughput on one host core (~21 clocks per block), and half of its instructions do
    // not touch the bit stream: endpoint prediction, the selector history, the index store.  slice_lex is the bit-serial half -- the
    // SliceLexer steps alone -- and leaves one token pair per block: tok_ep = predictor | delta symbol << 2, tok_sel = selector symbol
    // (a run block: n_selectors, i.e. history entry 0; a texture-video block that keeps the previous frame's selector: SPLIT_SKIP).
    // slice_resolve, on another thread, turns tokens into indices one row behind.  Rows are handed over through `rows_lexed` (release /
    // acquire); the token arrays cover the whole slice, so the lexer never waits for the resolver.  Like decode_slice_fast both halves only
    // handle regular streams: any irregularity makes them give up (`failed`), and the caller decodes the slice again with the exact loop.
    static constexpr uint16_t SPLIT_SKIP = 0xFFFF;
    bool split_ok() const
    {
        return n_endpoints != 0 && n_selectors != 0 && n_endpoints <= 65536u && (uint64_t)n_selectors + history_size < 0xFFFFu && endpoint_pred.bits() &&
               delta_endpoint.bits() && selector.bits() && history_rle.bits();
    }
    bool slice_lex(size_t nbx, size_t nby, const uint8_t* data, size_t len, uint32_t* tok_ep, uint16_t* tok_sel, std::atomic<uint32_t>& rows_lexed,
                   std::atomic<bool>& failed) const
    {
        SliceLexer lx = lexer(nbx, data, len);
        const bool video = is_video;
        auto block = [&](size_t i, uint32_t pred) __attribute__((always_inline)) -> bool {
            tok_ep[i] = pred | (lx.delta(pred) << 2);
            uint32_t tok;
            if (video && pred == 2)
                tok = SPLIT_SKIP;
            else if (lx.in_run())
                tok = lx.n_sel;
            else if (!lx.selector_token(&tok))
                return false;
            tok_sel[i] = (uint16_t)tok;
            return true;
        };
        for (size_t by = 0; by < nby; by++) {
            const bool even = !(by & 1);
            const size_t row = by * nbx;
            for (size_t bx = 0; bx < nbx; bx += 2) {
                lx.w.refill();
                uint32_t bits;
                bool ok = lx.pair_bits(bx, even, &bits) && block(row + bx, bits & 3);
                if (ok && bx + 1 < nbx) {
                    lx.w.refill();
                    ok = block(row + bx + 1, (bits >> 2) & 3);
                }
                if (!ok) {
                    failed.store(true, std::memory_order_release);
                    return false;
                }
            }
            if (lx.bad || failed.load(std::memory_order_relaxed)) {
                failed.store(true, std::memory_order_release);
                return false;
            }
            rows_lexed.store((uint32_t)(by + 1), std::memory_order_release);
        }
        return true;
    }
    bool slice_resolve(size_t nbx, size_t nby, const uint32_t* tok_ep, const uint16_t* tok_sel, uint32_t* idx, const std::atomic<uint32_t>& rows_lexed,
                       std::atomic<bool>& failed, std::atomic<uint32_t>* rows_done, const std::atomic<bool>* abort) const
    {
        const uint32_t n_sel = n_selectors;
        EndpointRows ep(nbx, n_endpoints, is_video);
        SelectorHistory hist(history_size);
        uint32_t bad = 0;
        for (size_t by = 0; by < nby; by++) {
            for (unsigned spin = 0; rows_lexed.load(std::memory_order_acquire) <= by; spin++) {
                if (failed.load(std::memory_order_acquire) || (abort && abort->load(std::memory_order_relaxed))) return false;
                if (spin > 256) std::this_thread::yield();
            }
            const uint32_t* te = tok_ep + by * nbx;
            const uint16_t* tsl = tok_sel + by * nbx;
            uint32_t* out_row = idx + by * nbx;
            for (size_t bx = 0; bx < nbx; bx++) {
                const uint32_t t = te[bx];
                const uint32_t e = ep.predict(t & 3u, t >> 2, bx, ep.edge_mask(bx == 0, by == 0), bad);
                const uint32_t tok = tsl[bx];
                uint32_t sel = 0;
                if (tok != SPLIT_SKIP && !hist.resolve(tok, n_sel, &sel)) {
                    failed.store(true, std::memory_order_release);
                    return false;
                }
                out_row[bx] = e | (sel << 16);
            }
            if (bad) {
                failed.store(true, std::memory_order_release);
                return false;
            }
            ep.next_row();
            if (rows_done) rows_done->store((uint32_t)(by + 1), std::memory_order_release);
        }
        return true;
    }

    bu_status decode_slice_exact(size_t nbx, size_t nby, const uint8_t* data, size_t len, uint32_t* idx) const
    {
        BitReader r(data, len);
        const uint32_t n_ep = n_endpoints, n_sel = n_selectors;
        // two rows of per-column state: endpoint index of the row above / pending 4 predictor bits for the row below
        std::vector<uint16_t> above(nbx, 0), cur_row(nbx, 0);
        std::vector<uint8_t> saved_bits(nbx, 0);
        std::vector<uint16_t> hist(history_size ? history_size : 1, 0);  // ApproxMoveToFront, mod.rs:610-656
        size_t rover = history_size / 2;
        const uint32_t rle_sym = n_sel + history_size;
        uint32_t sel_rle = 0, pred_repeat = 0, cur_bits = 0, prev_pred_sym = 0, prev_ep = 0;
        // texture video: the reference re-zeroes its "previous frame" per slice (mod.rs:236-237), so predictor 2
        // always reads the indices written earlier in this same slice -- i.e. zeros
        for (size_t by = 0; by < nby; by++) {
            for (size_t bx = 0; bx < nbx; bx++) {
                if (!(bx & 1)) {
                    if (!(by & 1)) {
                        if (pred_repeat) {
                            pred_repeat--;
                            cur_bits = prev_pred_sym;
                        } else {
                            uint32_t s;
                            if (!endpoint_pred.decode(r, &s)) return BU_ERR_BASISLZ;
                            if (s == 256) {
                                uint32_t v;
                                if (!vlc(r, 4, &v)) return BU_ERR_BOUNDS;
                                pred_repeat = v + 2;
                                cur_bits = prev_pred_sym;
                            } else {
                                cur_bits = s & 0xFF;
                                prev_pred_sym = cur_bits;
                            }
                        }
                        saved_bits[bx] = (uint8_t)(cur_bits >> 4);
                    } else {
                        cur_bits = saved_bits[bx];
                    }
                }
                const uint32_t pred = cur_bits & 3;
                cur_bits >>= 2;
                uint32_t e;
                switch (pred) {
                case 0:
                    if (bx == 0) return BU_ERR_BOUNDS;
                    e = prev_ep;
                    break;
                case 1:
                    if (by == 0) return BU_ERR_BOUNDS;
                    e = above[bx];
                    break;
                case 2:
                    if (is_video) {
                        e = 0;
                    } else {
                        if (bx == 0 || by == 0) return BU_ERR_BOUNDS;
                        e = above[bx - 1];
                    }
                    break;
                default: {
                    uint32_t s;
                    if (!delta_endpoint.decode(r, &s)) return BU_ERR_BASISLZ;
                    e = (s + prev_ep) & 0xFFFFu;
                    if (e >= n_ep) e = (e - n_ep) & 0xFFFFu;
                }
                }
                cur_row[bx] = (uint16_t)e;
                prev_ep = e;

                uint32_t sel;
                if (!is_video || pred != 2) {
                    uint32_t sym;
                    if (sel_rle) {
                        sel_rle--;
                        sym = n_sel;
                    } else {
                        if (!selector.decode(r, &sym)) return BU_ERR_BASISLZ;
                        if (sym == (rle_sym & 0xFFFFu)) {
                            uint32_t run;
                            if (!history_rle.decode(r, &run)) return BU_ERR_BASISLZ;
                            if (run == 63) {
                                uint32_t v;
                                if (!vlc(r, 7, &v)) return BU_ERR_BOUNDS;
                                sel_rle = 3 + v;
                            } else {
                                sel_rle = 3 + run;
                            }
                            sel_rle--;
                            sym = n_sel;
                        }
                    }
                    if (sym >= n_sel) {
                        const size_t hi = sym - n_sel;
                        if (history_size == 0 || hi >= history_size) return BU_ERR_BOUNDS;
                        sel = hist[hi];
                        if (hi) std::swap(hist[hi / 2], hist[hi]);
                    } else {
                        if (history_size) {
                            hist[rover] = (uint16_t)sym;
                            if (++rover == history_size) rover = history_size / 2;
                        }
                        sel = sym;
                    }
                } else {
                    sel = 0;  // previous frame's selector: zero, see above
                }
                if (e >= n_ep || sel >= n_sel) return BU_ERR_BOUNDS;  // asserts mod.rs:443-445
                idx[by * nbx + bx] = e | (sel << 16);
            }
            // the row just finished becomes "above"; the saved predictor bits written on even rows are read on the next (odd) row
            above.swap(cur_row);
        }
        return BU_OK;
    }

private:
    SliceLexer lexer(size_t nbx, const uint8_t* data, size_t len) const
    {
        return SliceLexer(endpoint_pred, delta_endpoint, selector, history_rle, n_selectors, history_size, nbx, data, len);
    }
};

// ---- all slices of a file ----
// The reference decodes slice after slice (basis.rs:42-58, 103-123).  The symbol stream is serial WITHIN a slice, but
// slices share nothing except the read-only codebooks and Huffman tables (the "previous frame" of texture video is
// re-zeroed per slice, mod.rs:236-237), so they decode concurrently on the host cores.  The visible result is that of
// the sequential loop: the status of the first failing slice in file order.
struct SliceJob {
    size_t nbx, nby;
    const uint8_t* data;
    size_t len;
    uint32_t* idx;
    bu_status st;
};

inline bu_status decode_slices(const BasisLz& lz, std::vector<SliceJob>& jobs, unsigned max_threads = 0, size_t min_parallel_blocks = 16384)
{
    size_t total = 0;
    for (const SliceJob& j : jobs) total += j.nbx * j.nby;
    unsigned nt = max_threads ? max_threads : Pool::capacity() + 1;
    if (nt > jobs.size()) nt = (unsigned)jobs.size();
    if (nt <= 1 || total < min_parallel_blocks) {
        for (SliceJob& j : jobs) {
            j.st = lz.decode_slice(j.nbx, j.nby, j.data, j.len, j.idx);
            if (j.st) return j.st;
        }
        return BU_OK;
    }
    std::atomic<size_t> next{0};
    const std::function<void()> work = [&] {
        for (size_t k; (k = next.fetch_add(1)) < jobs.size();) {
            try {  // (a copy of this runs on pool threads: an exception must become a status there)
                jobs[k].st = lz.decode_slice(jobs[k].nbx, jobs[k].nby, jobs[k].data, jobs[k].len, jobs[k].idx);
            } catch (...) {
                jobs[k].st = BU_ERR_BOUNDS;
            }
        }
    };
    pool().run(nt - 1, work);
    for (const SliceJob& j : jobs)
        if (j.st) return j.st;
    return BU_OK;
}

inline bu_status bu_make_lz(const uint8_t* file, size_t len, const bu_basis_header& h, BasisLz& lz)
{
    if (!in_file(len, h.endpoint_cb_file_ofs, h.endpoint_cb_file_size) || !in_file(len, h.selector_cb_file_ofs, h.selector_cb_file_size) ||
        !in_file(len, h.tables_file_ofs, h.tables_file_size) || !in_file(len, h.extended_file_ofs, h.extended_file_size))
        return BU_ERR_BOUNDS;
    // total_selectors for both codebooks: basis.rs:289-291
    return lz.init(h.total_selectors, h.total_selectors, file + h.endpoint_cb_file_ofs, h.endpoint_cb_file_size, file + h.selector_cb_file_ofs,
                   h.selector_cb_file_size, file + h.tables_file_ofs, h.tables_file_size, h.tex_type == 3);
}

}  // namespace bu_host
