// The bit reader and the canonical Huffman tables of the BasisLZ (ETC1S) streams: codebooks, tables section, slice data.
//
// Replaces, for this repo's C++ host facade:
//   src/basis_lz/huffman.rs:43-199  Huffman table records, canonical decode tables
// Written for speed where it is free: a 64-bit refilling bit reader, single-probe Huffman decode.  Reads past the end of a
// section return zeros like the reference's reader (bitreader.rs:45,55).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/basisu_hip.h"

namespace bu_host {

// ---- LSB-first bit reader with a 64-bit window ----
class BitReader {
public:
    BitReader(const uint8_t* p, size_t n) : p_(p), n_(n) {}
    uint32_t peek(unsigned count)
    {
        if (have_ < count) refill();
        return (uint32_t)(acc_ & ((count >= 32) ? 0xFFFFFFFFull : ((1ull << count) - 1ull)));
    }
    void skip(unsigned count)
    {
        if (have_ < count) refill();
        acc_ >>= count;
        have_ -= count;
    }
    uint32_t read(unsigned count)
    {
        const uint32_t v = peek(count);
        skip(count);
        return v;
    }

private:
    void refill()
    {
        while (have_ <= 56) {
            const uint64_t byte = pos_ < n_ ? p_[pos_] : 0;  // zeros past the end (bitreader.rs:45,55)
            pos_++;
            acc_ |= byte << have_;
            have_ += 8;
        }
    }
    const uint8_t* p_;
    size_t n_, pos_ = 0;
    uint64_t acc_ = 0;
    unsigned have_ = 0;
};

// ---- canonical Huffman, single-probe table (huffman.rs:120-199) ----
class Huffman {
public:
    // code_sizes[sym] in 0..16.  Over-subscribed length sets are accepted exactly like the reference does
    // (huffman.rs:163-170: the code is truncated to its length and later symbols overwrite earlier entries);
    // only a length whose running code count passes 2^16 is an error (huffman.rs:176-178).
    bu_status build(const std::vector<uint8_t>& sizes)
    {
        uint32_t count[17] = {0};
        max_ = 0;
        for (uint8_t s : sizes) {
            if (s > 16) return BU_ERR_BOUNDS;
            count[s]++;
            if (s > max_) max_ = s;
        }
        count[0] = 0;
        uint32_t next[17] = {0}, total = 0;
        for (int bits = 1; bits <= 16; bits++) {
            total = (total + count[bits - 1]) << 1;
            next[bits] = total;
        }
        table_.assign((size_t)1 << max_, 0u);
        // Kraft sum in units of 2^-max_: above 2^max_ the length set is over-subscribed and entries collide
        uint64_t kraft = 0;
        for (int bits = 1; bits <= 16; bits++) kraft += (uint64_t)count[bits] << (max_ >= (unsigned)bits ? max_ - bits : 0);
        auto rev_code = [](uint32_t code, unsigned size) {  // the low `size` bits of code, reversed
            uint32_t v = code;
            v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
            v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
            v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
            v = ((v >> 8) & 0x00FFu) | ((v & 0x00FFu) << 8);
            return (v & 0xFFFFu) >> (16 - size);
        };
        if (kraft > ((uint64_t)1 << max_)) {
            // over-subscribed (a damaged file): the reference's symbol-order fill, later symbols overwriting earlier ones
            for (size_t sym = 0; sym < sizes.size(); sym++) {
                const unsigned size = sizes[sym];
                if (!size) continue;
                const uint32_t code = next[size]++;
                uint32_t rev = 0;
                for (unsigned k = 0; k < size; k++) rev |= ((code >> k) & 1u) << (size - 1 - k);
                const uint32_t entry = ((uint32_t)sym << 5) | size;
                for (uint32_t id = rev; id < ((uint32_t)1 << max_); id += (1u << size)) table_[id] = entry;
            }
        } else {
            // a prefix code: no two symbols share an entry, so the fill order is free.  Symbol by symbol the copies of a code lie
            // 2^size entries apart -- 32 768 cache-missing stores for a 15-bit selector table (0.1 ms: on the critical path of a
            // single-slice file).  Grouped by length and walked copy by copy instead, every pass stays inside one window of
            // 2^size entries.
            std::vector<uint32_t> ent(sizes.size()), revs(sizes.size());
            uint32_t first[18] = {0};
            for (int bits = 1; bits <= 16; bits++) first[bits + 1] = first[bits] + count[bits];
            uint32_t fill[18];
            memcpy(fill, first, sizeof(fill));
            for (size_t sym = 0; sym < sizes.size(); sym++) {
                const unsigned size = sizes[sym];
                if (!size) continue;
                const uint32_t code = next[size]++;
                const uint32_t at = fill[size]++;
                revs[at] = rev_code(code, size);
                ent[at] = ((uint32_t)sym << 5) | size;
            }
            for (unsigned size = 1; size <= max_; size++) {
                const uint32_t a = first[size], b = first[size + 1];
                if (a == b) continue;
                for (uint32_t hi = 0; hi < ((uint32_t)1 << (max_ - size)); hi++) {
                    uint32_t* const win = table_.data() + ((size_t)hi << size);
                    for (uint32_t k = a; k < b; k++) win[revs[k]] = ent[k];
                }
            }
        }
        for (int bits = 0; bits <= 16; bits++)
            if (next[bits] > 65536u) return BU_ERR_BASISLZ;
        return BU_OK;
    }
    // returns false on "No matching code found" (huffman.rs:189-197)
    bool decode(BitReader& r, uint32_t* sym) const
    {
        const uint32_t e = table_[r.peek(max_)];
        if ((e & 0x1F) == 0) return false;
        r.skip(e & 0x1F);
        *sym = e >> 5;
        return true;
    }

    // the fast slice loop reads the table directly: entry = symbol << 5 | code_size (0 = no code), index = the next bits() bits
    const uint32_t* table() const { return table_.data(); }
    unsigned bits() const { return max_; }

private:
    std::vector<uint32_t> table_;  // symbol << 5 | code_size, indexed by the next max_ bits (LSB first)
    unsigned max_ = 0;
};

// huffman.rs:43-118
inline bu_status read_huffman_table(BitReader& r, Huffman& out)
{
    const size_t total_used = r.read(14);
    Huffman cl;
    {
        const size_t n = r.read(5);
        static const uint8_t order[21] = {17, 18, 19, 20, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 16};
        if (n > 21) return BU_ERR_BOUNDS;
        std::vector<uint8_t> sizes(21, 0);
        for (size_t i = 0; i < n; i++) sizes[order[i]] = (uint8_t)r.read(3);
        bu_status st = cl.build(sizes);
        if (st) return st;
    }
    std::vector<uint8_t> sizes;
    sizes.reserve(total_used + 140);
    while (sizes.size() < total_used) {
        uint32_t s;
        if (!cl.decode(r, &s)) return BU_ERR_BASISLZ;
        if (s <= 16) {
            sizes.push_back((uint8_t)s);
        } else if (s <= 18) {
            const size_t count = s == 17 ? 3 + r.read(3) : 11 + r.read(7);
            sizes.insert(sizes.end(), count, 0);
        } else {
            if (sizes.empty() || sizes.back() == 0) return BU_ERR_BASISLZ;  // huffman.rs:82-107
            const size_t count = s == 19 ? 3 + r.read(2) : 7 + r.read(7);
            sizes.insert(sizes.end(), count, sizes.back());
        }
    }
    return out.build(sizes);
}

}  // namespace bu_host
