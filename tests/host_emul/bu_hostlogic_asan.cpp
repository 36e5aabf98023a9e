// TEST-ONLY: the product's host-side container parser + BasisLZ decoder (csrc/bu_basis.hpp, the exact code that ships
// inside libbasisu_hip.so) compiled with AddressSanitizer + UBSan, plus a corrupt-file fuzz loop.  GPU ASan is not
// available on the pool, and this code is what faces untrusted `.basis` bytes, so it gets the sanitizer treatment.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>

#include <thread>
#include <vector>

#include "bu_basis.hpp"
#include "bu_file_layout.hpp"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

// The index buffer and the slice table of whatever slice table the file has (csrc/bu_file_layout.hpp): every entry's indices lie inside the
// buffer, and the kernels' lookup finds every unit in the entry of the image whose [unit0, unit0 + units_of) holds it (all units of a
// table of ordinary size, the first and last of every entry of a hostile one that claims millions).
static bu_status check_etc1s_layout(const bu_host::BuFilePlan& p)
{
    BuEtc1sFileLayout l;
    const bu_status st = bu_etc1s_file_layout(p, l);
    if (st) return st;
    const uint32_t n = (uint32_t)(l.descs.size() - 1);
    bool ok = l.descs.size() >= 1 && l.descs[n].unit0 == l.n_units && l.words <= 0xFFFFFFFFull;
    const auto held = [&](uint32_t u) {
        const BuEtc1sSlice& d = l.descs[bu_etc1s_unit_slice(l.descs.data(), n, u)];
        return d.image < l.unit0.size() && l.unit0[d.image] <= u && u - l.unit0[d.image] < l.units_of[d.image];
    };
    for (uint32_t s = 0; ok && s < n; s++) {
        const BuEtc1sSlice& d = l.descs[s];
        ok = d.n_blocks && (size_t)d.idx_ofs + d.n_blocks <= l.words && (!p.alpha_pairs || (size_t)d.aidx_ofs + d.n_blocks <= l.words) &&
             d.unit0 == l.unit0[d.image] && held(d.unit0) && held(d.unit0 + l.units_of[d.image] - 1);
    }
    for (uint32_t u = 0; ok && l.n_units <= 65536 && u < l.n_units; u++) ok = held(u);
    if (!ok) {
        fprintf(stderr, "the ETC1S layout of %zu images breaks an invariant\n", p.images.size());
        abort();
    }
    return BU_OK;
}

// plan + (for ETC1S) full host decode of every slice, as bu_read_to does before any upload
// report: print, per slice, which form produced decode_slice's result (the fast loop, or the exact loop after the fast one refused) and
// whether the two-thread form decoded it, gave up or was not allowed to start (split_ok() false) -- tests/test_lz_shape_cases.py reads it
static int process(const uint8_t* f, size_t len, int target, bool report = false)
{
    bu_host::BuFilePlan p;
    bu_status st = bu_host::bu_plan_file((bu_read_target)target, f, len, p);
    if (st) return st;
    if (!p.etc1s) return 0;
    st = check_etc1s_layout(p);
    if (st) return st;
    bu_host::BasisLz lz;
    st = bu_host::bu_make_lz(f, len, p.h, lz);
    if (report) printf("codebooks and tables: status=%d\n", (int)st);
    if (st) return st;
    // sequential, as the reference does it ...
    std::vector<std::vector<uint32_t>> seq(p.slices.size()), par(p.slices.size());
    bu_status seq_st = BU_OK;
    size_t seq_decoded = 0;  // slices the sequential loop got through without an error
    for (size_t k = 0; k < p.slices.size() && !seq_st; k++) {
        const bu_slice_desc& s = p.slices[k];
        seq[k].assign((size_t)s.num_blocks_x * s.num_blocks_y + 1, 0);
        seq_st = lz.decode_slice(s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, seq[k].data());
        if (!seq_st) seq_decoded = k + 1;
        // decode_slice is the fast loop with the exact loop (round 1's, status for status the oracle's) as its fallback: compare the two
        // DIRECTLY on every slice -- the exact loop's status is the verdict, and wherever the fast loop claims a regular stream its indices
        // are the exact loop's; rows it published before giving up are final and must match too
        {
            const size_t n = (size_t)s.num_blocks_x * s.num_blocks_y;
            std::vector<uint32_t> ex(n + 1, 0), fa(n + 1, 0);
            const bu_status ex_st = lz.decode_slice_exact(s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, ex.data());
            if (ex_st != seq_st) {
                fprintf(stderr, "decode_slice status %d, decode_slice_exact %d in slice %zu\n", (int)seq_st, (int)ex_st, k);
                abort();
            }
            if (!ex_st && ex != seq[k]) {
                fprintf(stderr, "decode_slice differs from decode_slice_exact in slice %zu\n", k);
                abort();
            }
            bool fast_ok = false;
            if (s.num_blocks_x && s.num_blocks_y) {
                std::atomic<uint32_t> rows{0};
                fast_ok = lz.decode_slice_fast(s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, fa.data(), &rows);
                if (fast_ok && (ex_st != BU_OK || fa != ex)) {
                    fprintf(stderr, "decode_slice_fast accepts slice %zu and disagrees with the exact loop (status %d)\n", k, (int)ex_st);
                    abort();
                }
                if (!ex_st) {  // rows published before a give-up (or all of them) are the exact loop's
                    const size_t pub = (size_t)rows.load() * s.num_blocks_x;
                    if (pub > n || !std::equal(fa.begin(), fa.begin() + (long)pub, ex.begin())) {
                        fprintf(stderr, "rows published by decode_slice_fast differ from the exact loop in slice %zu\n", k);
                        abort();
                    }
                }
            }
            if (report) printf("slice %zu: decode_slice=%s status=%d\n", k, fast_ok ? "fast" : "exact", (int)seq_st);
        }
    }
    if (report) printf("split_ok=%d\n", lz.split_ok() ? 1 : 0);
    // ... and on 4 threads, as bu_read_to does it (threading forced: these files are tiny): same status, same indices
    std::vector<bu_host::SliceJob> jobs;
    for (size_t k = 0; k < p.slices.size(); k++) {
        const bu_slice_desc& s = p.slices[k];
        par[k].assign((size_t)s.num_blocks_x * s.num_blocks_y + 1, 0);
        jobs.push_back({s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, par[k].data(), BU_OK});
    }
    // ... and every slice on two threads (slice_lex + slice_resolve, the streamed front door's form for the first slice): where both
    // halves report a regular stream the indices are the sequential loop's; they may only give up where that loop is the judge
    if (lz.split_ok()) {
        for (size_t k = 0; k < p.slices.size(); k++) {
            const bu_slice_desc& s = p.slices[k];
            const size_t n = (size_t)s.num_blocks_x * s.num_blocks_y;
            std::vector<uint32_t> tok_ep(n + 1), out(n + 1, 0);
            std::vector<uint16_t> tok_sel(n + 1);
            std::atomic<uint32_t> rows_lexed{0}, rows_done{0};
            std::atomic<bool> failed{false};
            bool res_ok = false;
            std::thread th([&] { res_ok = lz.slice_resolve(s.num_blocks_x, s.num_blocks_y, tok_ep.data(), tok_sel.data(), out.data(), rows_lexed, failed, &rows_done, nullptr); });
            const bool lex_ok = lz.slice_lex(s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, tok_ep.data(), tok_sel.data(), rows_lexed, failed);
            th.join();
            if (report) printf("slice %zu: two-thread=%s\n", k, lex_ok && res_ok ? "lex+resolve" : "gave-up");
            if (lex_ok && res_ok) {
                // (slices behind the first failing one were never decoded by the sequential loop: nothing to compare with)
                const bool have_seq = seq_decoded > k;
                if (have_seq && out != seq[k]) {
                    fprintf(stderr, "two-thread decode differs in slice %zu\n", k);
                    abort();
                }
            } else if (seq_st == BU_OK && s.num_blocks_x && s.num_blocks_y) {
                fprintf(stderr, "two-thread decode gave up on slice %zu of a file the sequential loop accepts\n", k);
                abort();
            }
        }
    }
    const bu_status par_st = bu_host::decode_slices(lz, jobs, 4, 0);
    if (par_st != seq_st) {
        fprintf(stderr, "parallel decode status %d != sequential %d\n", (int)par_st, (int)seq_st);
        abort();
    }
    if (!seq_st)
        for (size_t k = 0; k < p.slices.size(); k++)
            if (seq[k] != par[k]) {
                fprintf(stderr, "parallel decode differs in slice %zu\n", k);
                abort();
            }
    // ... and decode_slices with its defaults, as the one-launch path calls it: a file this small takes its sequential loop
    for (size_t k = 0; k < p.slices.size(); k++) std::fill(par[k].begin(), par[k].end(), 0u);
    const bu_status def_st = bu_host::decode_slices(lz, jobs);
    if (def_st != seq_st) {
        fprintf(stderr, "decode_slices status %d != sequential %d\n", (int)def_st, (int)seq_st);
        abort();
    }
    if (!seq_st)
        for (size_t k = 0; k < p.slices.size(); k++)
            if (seq[k] != par[k]) {
                fprintf(stderr, "decode_slices differs in slice %zu\n", k);
                abort();
            }
    return seq_st;
}

// The worker pool under the pattern that once deadlocked it: many parked threads (a wide job first), then thousands of narrow jobs
// whose copies finish at once -- a copy that parked again used to swallow the wake-up meant for the next helper, and the job
// waited for a copy that never started.  Also the split begin() / end() form with the caller doing something else meanwhile.
static int pool_stress(int rounds)
{
    std::atomic<long> sum{0};
    const std::function<void()> wide = [&] { sum.fetch_add(1); };
    bu_host::pool().run(bu_host::Pool::capacity(), wide);
    for (int r = 0; r < rounds; r++) {
        std::atomic<int> next{0}, done{0};
        const std::function<void()> narrow = [&] {
            for (int k; (k = next.fetch_add(1)) < 5;) done.fetch_add(1);
        };
        if (r & 1) {
            bu_host::pool().run(3, narrow);
        } else {
            bu_host::pool().begin(3, narrow);
            narrow();
            bu_host::pool().end();
        }
        if (done.load() != 5) return 1;
    }
    return 0;
}

// The fast slice loops' bit window (bu_host::BitWindow) against the exact loop's BitReader, bit for bit: random byte strings of 0 .. 40
// bytes (shorter than one 8-byte load, and long enough for both the load and the byte tail), a random sequence of take(1 .. 17) with a
// refill whenever fewer than 17 bits are held, and of vlc(4) / vlc(7) including the "more than 32 bits" refusal, read on to 64 bits and
// more past the end: the zeros there are what the fuzz only reaches indirectly.  Every fourth string is all ones, whose vlc's all refuse.
static void bit_window_check(int strings)
{
    long refusals = 0;
    for (int s = 0; s < strings; s++) {
        const size_t len = rnd() % 41;
        uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);  // exact size: ASan sees any over-read
        for (size_t i = 0; i < len; i++) bytes[i] = (s & 3) == 3 ? 0xFF : (uint8_t)rnd();
        bu_host::BitWindow w(bytes, len);
        bu_host::BitReader r(bytes, len);
        for (size_t used = 0; used < 8 * len + 64;) {
            const unsigned op = rnd() % 8;
            if (op < 6) {
                const unsigned n = 1 + rnd() % 17;
                if (w.have < 17) w.refill();
                const uint32_t got = w.take(n), want = r.read(n);
                if (got != want) {
                    fprintf(stderr, "BitWindow::take(%u) = %u, BitReader::read = %u at bit %zu of %zu bytes\n", n, got, want, used, len);
                    abort();
                }
                used += n;
            } else {
                const unsigned chunk = op == 6 ? 4 : 7;
                uint32_t got = 0, want = 0;
                const bool got_ok = w.vlc(chunk, &got), want_ok = bu_host::BasisLz::vlc(r, chunk, &want);
                if (got_ok != want_ok || (got_ok && got != want)) {
                    fprintf(stderr, "BitWindow::vlc(%u) = %d %u, BasisLz::vlc = %d %u at bit %zu of %zu bytes\n", chunk, (int)got_ok, got, (int)want_ok, want, used, len);
                    abort();
                }
                refusals += !got_ok;
                used += chunk + 1;  // (at least)
            }
        }
        free(bytes);
    }
    if (!refusals) {
        fprintf(stderr, "no vlc refused in %d strings\n", strings);
        abort();
    }
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "--pool-stress")) {
        const int st = pool_stress(atoi(argv[2]));
        printf("pool stress %s\n", st ? "FAILED" : "ok");
        return st;
    }
    if (argc < 3) return 2;
    bit_window_check(4000);
    const int iters = atoi(argv[2]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> base;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) base.insert(base.end(), buf, buf + n);
    fclose(fp);
    int ok = 0, bad = 0;
    if (process(base.data(), base.size(), BU_READ_RGBA, true) != 0) return 3;  // the pristine file must parse
    for (int it = 0; it < iters; it++) {
        std::vector<uint8_t> g = base;
        const int kind = rnd() % 4;
        const int flips = 1 + rnd() % 4;
        for (int k = 0; k < flips; k++) {
            size_t pos = kind == 0 ? rnd() % 77 : (kind == 1 ? 77 + rnd() % (g.size() > 200 ? 123 : 1) : rnd() % g.size());
            if (pos >= g.size()) pos = g.size() - 1;
            g[pos] ^= (uint8_t)(1u << (rnd() % 8));
        }
        if (kind == 3 && g.size() > 100) g.resize(77 + rnd() % (g.size() - 77));  // truncation
        // re-seal both CRCs so the mutation reaches the parsers behind them
        if (g.size() >= 77) {
            const uint16_t dc = bu_host::crc16(g.data() + 77, g.size() - 77, 0);
            g[12] = (uint8_t)dc;
            g[13] = (uint8_t)(dc >> 8);
            const uint16_t hc = bu_host::crc16(g.data() + 8, 69, 0);
            g[6] = (uint8_t)hc;
            g[7] = (uint8_t)(hc >> 8);
        }
        // heap copy of exact size so ASan sees any over-read of the file buffer
        uint8_t* exact = (uint8_t*)malloc(g.size() ? g.size() : 1);
        memcpy(exact, g.data(), g.size());
        const int st = process(exact, g.size(), (it & 1) ? BU_READ_RGBA : BU_READ_ETC1);
        free(exact);
        st ? bad++ : ok++;
    }
    printf("fuzz done: %d parsed, %d rejected\n", ok, bad);
    return 0;
}
