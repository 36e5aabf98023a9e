// test-only host build of csrc/bu_multi_addr.hpp as it is: the run cursor, the tile corner and the lane offsets of the multi-run kernels
// (tests/test_multi_addr.py builds it as a shared library, and -- with -DBU_EMUL_MULTI_ADDR_MAIN -fsanitize=undefined -- as a stand-alone program that walks a
// table the way a workgroup does)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bu_multi_addr.hpp"

extern "C" {

uint32_t bu_emul_multi_max_width() { return (uint32_t)BU_MULTI_MAX_WIDTH; }
uint32_t bu_emul_multi_rgba_max_bpr() { return (uint32_t)BU_MULTI_RGBA_MAX_BPR; }
uint32_t bu_emul_multi_runs() { return BU_MULTI_RUNS; }
uint32_t bu_emul_multi_strips() { return BU_RUN_STRIPS; }

// the lane offsets of a thread's blocks: off[l] for l in [0, tile)
void bu_emul_multi_lane_offs(int whole, uint32_t width, uint32_t tile, uint64_t* off)
{
    for (uint32_t l = 0; l < tile; l++) off[l] = bu_lane_off(whole != 0, width, l);
}

// A workgroup's walk over `tiles[0 .. n_t)` of a table of `k` runs (5 words each: in, out, base, n, vshift; first_tile[k + 32] with the unused entries ~0): the
// cursor is kept from tile to tile as the kernel keeps it -- a tile inside it takes the scalar path, any other the look-up.  Per tile 9 words come back:
// fast (1: no look-up), in, out, base, first, n, width, bx0, run; and in `fresh` the same 9 with the cursor thrown away in front of every tile (always the look-up).
void bu_emul_multi_walk(uint32_t tile, uint32_t out_bytes, uint32_t rgba_bpr, uint32_t k, const uint64_t* runs, const uint32_t* first_tile, uint32_t n_t,
                        const uint32_t* tiles, uint64_t* walked, uint64_t* fresh)
{
    auto rec = [&](uint32_t r) { return BuRunRec{runs[5 * r], runs[5 * r + 1], runs[5 * r + 2], (uint32_t)runs[5 * r + 3], (uint32_t)runs[5 * r + 4]}; };
    auto put = [&](uint64_t* o, bool fast, const BuMultiTile& d, uint32_t r) {
        const uint64_t w[9] = {fast, d.in, d.out, d.base, d.first, d.n, d.width, d.bx0, r};
        for (int i = 0; i < 9; i++) o[i] = w[i];
    };
    BuRunCursor cur = bu_no_run();
    uint32_t cur_run = 0;
    for (uint32_t i = 0; i < n_t; i++) {
        const uint32_t t = tiles[i];
        const bool fast = bu_cursor_holds(cur, t);
        if (!fast) {
            cur_run = bu_run_of_tile(first_tile, k + 32, t);
            cur = bu_run_cursor(rec(cur_run), first_tile[cur_run], tile);
        }
        put(walked + 9 * i, fast, bu_tile_of(cur, t, tile, out_bytes, rgba_bpr), cur_run);
        const uint32_t r = bu_run_of_tile(first_tile, k + 32, t);
        put(fresh + 9 * i, false, bu_tile_of(bu_run_cursor(rec(r), first_tile[r], tile), t, tile, out_bytes, rgba_bpr), r);
    }
}

// RGBA32: the byte offset from the tile's `out` of pixel row 0 of every block of the tile described by (first, width, bx0)
void bu_emul_multi_rgba_offs(uint32_t width, uint32_t bx0, uint32_t bpr, uint32_t tile, uint64_t* off)
{
    BuMultiTile d = {};
    d.width = width;
    d.bx0 = bx0;
    for (uint32_t l = 0; l < tile; l++) off[l] = bu_lane_off_rgba(d, bu_lane_off(false, width, l), bpr);
}

}  // extern "C"

#ifdef BU_EMUL_MULTI_ADDR_MAIN
// bu_emul_multi_addr: a table of 96 runs of mixed widths and strips up to 2^32 - 1 blocks, every run's first, middle and last tile and the tile behind it, all
// lanes -- the arithmetic under UBSan (shift counts, overflow of the signed kind); prints a checksum
int main()
{
    std::vector<uint64_t> runs;
    std::vector<uint32_t> first(BU_MULTI_RUNS + 32, 0xFFFFFFFFu);
    uint64_t tiles = 0;
    uint32_t k = 0;
    for (; k < BU_MULTI_RUNS; k++) {
        const uint32_t vshift = k % 3 == 2 ? BU_RUN_STRIPS : k % 15;
        uint64_t n = k % 3 == 2 ? 1000u + 77777u * k : (uint64_t)16 * (64u << vshift) * (1 + k % 5);
        if (k == 41) n = 3000000000u;  // (a long strip run, indices past 2^31; the launch's tiles x 1024 stays below 2^32)
        if (tiles + (n + 1023) / 1024 >= ((uint64_t)1 << 22) - 1) break;
        const uint64_t row[5] = {0x7f0000000000ull + ((uint64_t)k << 36), 0x7e0000000000ull + ((uint64_t)k << 36), (uint64_t)k << 40, n, vshift};
        runs.insert(runs.end(), row, row + 5);
        first[k] = (uint32_t)tiles;
        tiles += (n + 1023) / 1024;
    }
    uint64_t sum = 0;
    BuRunCursor cur = bu_no_run();
    for (uint32_t r = 0; r < k; r++) {
        const uint32_t nt = (uint32_t)((runs[5 * r + 3] + 1023) / 1024);
        const uint32_t ts[4] = {first[r], first[r] + nt / 2, first[r] + nt - 1, first[r] + nt};
        for (uint32_t t : ts) {
            if (t >= tiles) continue;
            if (!bu_cursor_holds(cur, t)) {
                const uint32_t q = bu_run_of_tile(first.data(), BU_MULTI_RUNS + 32, t);
                cur = bu_run_cursor(BuRunRec{runs[5 * q], runs[5 * q + 1], runs[5 * q + 2], (uint32_t)runs[5 * q + 3], (uint32_t)runs[5 * q + 4]}, first[q], 1024u);
            }
            const BuMultiTile d = bu_tile_of(cur, t, 1024u, 16u, 0u);
            for (uint32_t l = 0; l < 1024u; l++) {
                const uint32_t off = bu_lane_off(false, d.width, l);
                sum += d.in + off + bu_lane_block(d, off);
            }
        }
    }
    printf("clean %u runs %llu\n", k, (unsigned long long)sum);
    return 0;
}
#endif
