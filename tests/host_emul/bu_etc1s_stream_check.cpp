// TEST-ONLY: the scheduler of the streamed ETC1S front door (csrc/bu_etc1s_stream.hpp, the exact text that ships inside libbasisu_hip.so) on the CPU,
// built with AddressSanitizer + UBSan and with ThreadSanitizer.  A recording sink stands where the driver's three HIP lambdas stand: it checks the order
// of the calls, that the bands of an image are ascending and contiguous, and -- the property the GPU relies on -- that at the moment of a launch every
// index word of the launched units is the sequential decode's.  The sink can also fail its n-th launch, which no test may do to a real device.
//   bu_etc1s_stream_check FILE ROUNDS     the file, then ROUNDS damaged copies (CRCs re-sealed), each through every form
//   bu_etc1s_stream_check --pure           the pure pieces (item order, band rule, status order, sizes) on hand-made inputs
//   bu_etc1s_stream_check --rule band AVAIL LAUNCHED FINISHED | --rule split NBLK     a rule with the shipped constants: prints 0 or 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "bu_etc1s_stream.hpp"

#define REQUIRE(cond, ...)                \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            abort();                      \
        }                                 \
    } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

// ---- the sequential reading of a file: what the streamed read has to arrive at --------------------------------------------------------
struct Reference {
    bu_host::BuFilePlan p;
    BuEtc1sFileLayout l;
    bool crc_bad = false;
    bu_status st_tables = BU_OK, st_cb = BU_OK;
    bu_host::BasisLz lz;                     // tables, then codebooks, one after the other
    std::vector<std::vector<uint32_t>> idx;  // per slice the scheduler decodes (file order: colour, then its alpha), nblk words
    std::vector<bu_status> st;
    bu_status status = BU_OK;  // in the reference's order: CRC, codebooks, tables, first failing slice
};

// false: the file never reaches the scheduler (the plan, the bounds of the codebooks and tables or the layout refuse it: the driver's own first lines)
static bool read_sequentially(const uint8_t* f, size_t len, bu_read_target target, Reference& r)
{
    using bu_host::in_file;
    if (bu_host::bu_plan_file(target, f, len, r.p, false) || !r.p.etc1s || r.p.images.empty()) return false;
    const bu_basis_header& h = r.p.h;
    if (!in_file(len, h.endpoint_cb_file_ofs, h.endpoint_cb_file_size) || !in_file(len, h.selector_cb_file_ofs, h.selector_cb_file_size) ||
        !in_file(len, h.tables_file_ofs, h.tables_file_size) || !in_file(len, h.extended_file_ofs, h.extended_file_size))
        return false;
    if (bu_etc1s_file_layout(r.p, r.l)) return false;
    r.crc_bad = bu_host::crc16(f + 77, len - 77, 0) != h.data_crc16;
    r.st_tables = r.lz.init_tables(h.total_selectors, h.total_selectors, f + h.tables_file_ofs, h.tables_file_size, h.tex_type == 3);
    try {
        r.st_cb = r.lz.init_codebooks(f + h.endpoint_cb_file_ofs, h.endpoint_cb_file_size, f + h.selector_cb_file_ofs, h.selector_cb_file_size);
    } catch (...) {
        r.st_cb = BU_ERR_BOUNDS;
    }
    r.status = r.crc_bad ? BU_ERR_DATA_CRC : r.st_cb ? r.st_cb : r.st_tables;
    const size_t per_img = r.p.alpha_pairs ? 2 : 1;
    for (size_t k = 0; k < r.p.images.size(); k++)
        for (size_t a = 0; a < per_img; a++) {
            const bu_slice_desc& s = r.p.slices[r.p.first_slice[k] + a];
            r.idx.emplace_back((size_t)s.num_blocks_x * s.num_blocks_y, 0u);
            bu_status st = BU_ERR_ARGUMENT;  // (tables or codebooks failed: no slice is decoded)
            if (!r.st_tables && !r.st_cb) {
                try {
                    st = r.lz.decode_slice(s.num_blocks_x, s.num_blocks_y, f + s.file_ofs, s.file_size, r.idx.back().data());
                } catch (...) {
                    st = BU_ERR_BOUNDS;
                }
                if (st && !r.status) r.status = st;
            }
            r.st.push_back(st);
        }
    return true;
}

// The reader of a launch is the GPU, no thread of this process: a slice that is decoded again after its two-thread attempt gave up writes the rows it
// has published a second time, with the same values, while a band over them may be in flight.  The comparison therefore reads the index buffer outside
// ThreadSanitizer's view, by value, as the device does; every access of the scheduler itself stays instrumented.
__attribute__((no_sanitize("thread"), noinline)) static bool same_words(const uint32_t* a, const uint32_t* b, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (((const volatile uint32_t*)a)[i] != b[i]) return false;
    return true;
}

// ---- the recording sink -----------------------------------------------------------------------------------------------------------------
struct Recorder {
    const Reference& ref;
    const uint32_t* h_idx;
    long fail_at;  // this launch (counted from 1) returns BU_ERR_HIP; 0: none
    std::mutex m;
    std::set<std::thread::id> bound;
    int codebook_calls = 0;
    long launches = 0;
    bool failed = false;
    std::vector<uint32_t> ended;  // units of image k launched so far

    Recorder(const Reference& r, const uint32_t* idx, long fail) : ref(r), h_idx(idx), fail_at(fail), ended(r.p.images.size(), 0) {}
    bu_status bind()
    {
        std::lock_guard<std::mutex> g(m);
        REQUIRE(!failed, "bind() after a call of the sink had failed");
        bound.insert(std::this_thread::get_id());
        return BU_OK;
    }
    bu_status codebooks(const bu_host::BasisLz& z)
    {
        std::lock_guard<std::mutex> g(m);
        REQUIRE(bound.count(std::this_thread::get_id()), "codebooks() on a thread that has not called bind()");
        REQUIRE(++codebook_calls == 1 && launches == 0, "codebooks() a second time, or after a launch");
        REQUIRE(!ref.st_cb && !ref.st_tables, "codebooks() although the codebooks (%d) or the tables (%d) failed", (int)ref.st_cb, (int)ref.st_tables);
        REQUIRE(z.endpoints == ref.lz.endpoints && z.selectors == ref.lz.selectors, "codebooks() sees other codebooks than a sequential init_codebooks");
        return BU_OK;
    }
    bu_status launch(uint32_t u0, uint32_t u1)
    {
        std::lock_guard<std::mutex> g(m);
        REQUIRE(!failed, "launch() after a launch had failed");
        REQUIRE(bound.count(std::this_thread::get_id()), "launch() on a thread that has not called bind()");
        REQUIRE(codebook_calls == 1, "launch() before codebooks()");
        REQUIRE(u0 < u1, "launch(%u, %u) is empty", u0, u1);
        const BuEtc1sFileLayout& l = ref.l;
        size_t k = 0;
        while (k < l.unit0.size() && !(l.unit0[k] <= u0 && u0 - l.unit0[k] < l.units_of[k])) k++;
        REQUIRE(k < l.unit0.size() && u1 - l.unit0[k] <= l.units_of[k], "launch(%u, %u) lies in no image", u0, u1);
        REQUIRE(u0 == l.unit0[k] + ended[k], "launch(%u, %u): image %zu's previous band ended at unit %u", u0, u1, k, l.unit0[k] + ended[k]);
        ended[k] = u1 - l.unit0[k];
        const size_t per_img = ref.p.alpha_pairs ? 2 : 1, b0 = (size_t)(u0 - l.unit0[k]) * 64;
        for (size_t a = 0; a < per_img; a++) {
            const size_t job = k * per_img + a;
            if (ref.st[job]) continue;  // (its own sequential decode fails: the call will, whatever is launched meanwhile)
            const size_t nblk = ref.idx[job].size(), b1 = std::min<size_t>(nblk, (size_t)ended[k] * 64);
            REQUIRE(b0 < nblk, "launch(%u, %u) starts behind image %zu's last block", u0, u1, k);
            REQUIRE(same_words(h_idx + (a ? l.aidx_ofs[k] : l.idx_ofs[k]) + b0, ref.idx[job].data() + b0, b1 - b0),
                    "launch(%u, %u): the %s indices of image %zu are not the sequential decode's at this moment", u0, u1, a ? "alpha" : "colour", k);
        }
        if (++launches == fail_at) {
            failed = true;
            return BU_ERR_HIP;
        }
        return BU_OK;
    }
};

// ---- one streamed read of a file the Reference describes ---------------------------------------------------------------------------------
// tokens = false: no token buffer (the driver's malloc failed): every slice takes the ordinary loop.  Returns the launches the sink saw.
static long stream_once(const uint8_t* f, size_t len, const Reference& ref, size_t split_min, size_t band_blocks, bool tokens, long fail_at, const char* form)
{
    const bu_basis_header& h = ref.p.h;
    bu_host::BasisLz lz;
    const bu_status st_tables = lz.init_tables(h.total_selectors, h.total_selectors, f + h.tables_file_ofs, h.tables_file_size, h.tex_type == 3);
    REQUIRE(st_tables == ref.st_tables, "%s: init_tables gives %d, then %d", form, (int)ref.st_tables, (int)st_tables);
    std::vector<uint32_t> h_idx(ref.l.words ? ref.l.words : 16, 0xDEADBEEFu);
    const bool may_split = bu_etc1s_may_split(st_tables, lz, true);
    const size_t tok_bytes = tokens ? bu_etc1s_stream_tok_bytes(ref.p, may_split, split_min) : 0;
    void* const tok = tok_bytes ? malloc(tok_bytes) : nullptr;  // (of the exact size: ASan sees a token written behind it)
    Recorder rec(ref, h_idx.data(), fail_at);
    BuEtc1sSink sink;
    sink.bind = [&] { return rec.bind(); };
    sink.codebooks = [&](const bu_host::BasisLz& z) { return rec.codebooks(z); };
    sink.launch = [&](uint32_t u0, uint32_t u1) { return rec.launch(u0, u1); };
    BuLap lap{false};
    BuEtc1sStreamResult res;
    bu_etc1s_stream(f, len, ref.p, ref.l, lz, st_tables, true, h.data_crc16, h_idx.data(), tok, tok_bytes, may_split, sink, lap, res, split_min, band_blocks);
    const bu_status st = bu_etc1s_stream_status(true, st_tables, res);
    free(tok);
    // a launch that failed decides unless the CRC (or, which cannot be: no launch then, codebooks or tables) failed
    const bu_status want = rec.failed && !ref.crc_bad ? BU_ERR_HIP : ref.status;
    REQUIRE(st == want, "%s: status %d, sequentially %d%s", form, (int)st, (int)want, rec.failed ? " (a launch failed)" : "");
    if (st == BU_OK) {
        const size_t per_img = ref.p.alpha_pairs ? 2 : 1;
        for (size_t k = 0; k < ref.p.images.size(); k++) {
            REQUIRE(rec.ended[k] == ref.l.units_of[k], "%s: image %zu launched to unit %u of %u", form, k, rec.ended[k], ref.l.units_of[k]);
            for (size_t a = 0; a < per_img; a++) {
                const std::vector<uint32_t>& want_idx = ref.idx[k * per_img + a];
                REQUIRE(std::equal(want_idx.begin(), want_idx.end(), h_idx.begin() + (a ? ref.l.aidx_ofs[k] : ref.l.idx_ofs[k])),
                        "%s: the index buffer differs from the sequential decode in image %zu", form, k);
            }
        }
    }
    return rec.launches;
}

// every form of the scheduler over one file; false: the file does not reach it
static bool check_file(const uint8_t* f, size_t len, bu_read_target target, bool& good)
{
    Reference ref;
    if (!read_sequentially(f, len, target, ref)) return false;
    good = ref.status == BU_OK;
    stream_once(f, len, ref, BU_ETC1S_STREAM_MIN_BLOCKS, BU_ETC1S_BAND_BLOCKS, true, 0, "default thresholds");
    const long n = stream_once(f, len, ref, 1, 64, true, 0, "every slice on two threads, bands of one unit");
    stream_once(f, len, ref, 1, 64, false, 0, "no token buffer, bands of one unit");
    // a launch fails: the call says so, every thread has stopped and the pool is free -- the clean call right after goes through
    if (n) {
        stream_once(f, len, ref, 1, 64, true, 1 + rnd() % n, "a launch fails");
        stream_once(f, len, ref, 1, 64, true, 0, "the call after a failed launch");
        stream_once(f, len, ref, BU_ETC1S_STREAM_MIN_BLOCKS, BU_ETC1S_BAND_BLOCKS, true, 1, "the first launch fails, default thresholds");
        stream_once(f, len, ref, BU_ETC1S_STREAM_MIN_BLOCKS, BU_ETC1S_BAND_BLOCKS, true, 0, "the call after a failed launch, default thresholds");
    }
    return true;
}

// ---- the pure pieces on hand-made inputs ---------------------------------------------------------------------------------------------
static int pure()
{
    typedef std::vector<std::pair<int, size_t>> Order;
    const auto order_of = [](std::initializer_list<bool> splits) {
        std::vector<BuEtc1sStreamJob> jobs(splits.size());
        size_t k = 0;
        for (bool s : splits) jobs[k++].split = s;
        Order o;
        for (const BuEtc1sItem& it : bu_etc1s_stream_items(jobs)) o.push_back({(int)it.kind, it.job});
        return o;
    };
    const int R = BU_ITEM_RESOLVE, F = BU_ITEM_FEED, C = BU_ITEM_CODEBOOKS, K = BU_ITEM_CRC, S = BU_ITEM_SLICE, L = BU_ITEM_LEX;
    REQUIRE(order_of({}) == (Order{{C, 0}, {F, 0}, {K, 0}}), "item order: no slice");
    REQUIRE(order_of({false}) == (Order{{C, 0}, {F, 0}, {K, 0}}), "item order: one ordinary slice (the caller's)");
    REQUIRE(order_of({true}) == (Order{{R, 0}, {C, 0}, {F, 0}, {K, 0}}), "item order: one two-thread slice");
    REQUIRE(order_of({true, false, true, false}) == (Order{{R, 0}, {C, 0}, {F, 0}, {K, 0}, {S, 1}, {L, 2}, {R, 2}, {S, 3}}), "item order: mixed");
    REQUIRE(order_of({false, true, true}) == (Order{{C, 0}, {F, 0}, {K, 0}, {L, 1}, {R, 1}, {L, 2}, {R, 2}}), "item order: a lexer in front of its resolver");

    REQUIRE(!bu_etc1s_band_due(0, 0, true) && !bu_etc1s_band_due(5, 5, true) && !bu_etc1s_band_due(4, 5, true), "band rule: nothing new");
    REQUIRE(bu_etc1s_band_due(6, 5, true), "band rule: a finished image's rest goes at once");
    REQUIRE(!bu_etc1s_band_due(255, 0, false) && bu_etc1s_band_due(256, 0, false) && bu_etc1s_band_due(356, 100, false) && !bu_etc1s_band_due(355, 100, false),
            "band rule: 16384 blocks are 256 units");
    REQUIRE(bu_etc1s_band_due(1, 0, false, 64) && !bu_etc1s_band_due(1, 0, false, 65) && bu_etc1s_band_due(2, 0, false, 65), "band rule: a given band size");

    const bu_status E1 = BU_ERR_BOUNDS, E2 = BU_ERR_ARGUMENT, E3 = BU_ERR_HIP, E4 = BU_ERR_LENGTH;
    BuEtc1sStreamResult r;
    r.st_slices = {BU_OK, E4, E1};
    REQUIRE(bu_etc1s_stream_status(true, BU_OK, r) == E4, "status: the first failing slice in file order");
    r.st_feed = E3;
    REQUIRE(bu_etc1s_stream_status(true, BU_OK, r) == E3, "status: the feeder before the slices");
    REQUIRE(bu_etc1s_stream_status(true, E2, r) == E2, "status: the tables before the feeder");
    r.st_cb = E1;
    REQUIRE(bu_etc1s_stream_status(true, E2, r) == E1, "status: the codebooks before the tables");
    r.crc_ok = false;
    REQUIRE(bu_etc1s_stream_status(true, E2, r) == BU_ERR_DATA_CRC, "status: the payload CRC before everything");
    REQUIRE(bu_etc1s_stream_status(false, E2, r) == E1, "status: no CRC pending, none reported");
    REQUIRE(bu_etc1s_stream_status(true, BU_OK, BuEtc1sStreamResult()) == BU_OK, "status: nothing failed");

    REQUIRE(bu_etc1s_tok_bytes(0) == 64 && bu_etc1s_tok_bytes(1) == 128 && bu_etc1s_tok_bytes(10) == 128 && bu_etc1s_tok_bytes(11) == 192 &&
                bu_etc1s_tok_bytes(32768) == 196672,
            "token bytes: six per block, a spare line, whole lines");
    REQUIRE(!bu_etc1s_slice_splits(true, 32767) && bu_etc1s_slice_splits(true, 32768) && !bu_etc1s_slice_splits(false, (size_t)1 << 20) &&
                bu_etc1s_slice_splits(true, 1, 1) && !bu_etc1s_slice_splits(true, 0, 1),
            "split rule");
    printf("pure pieces ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--pure")) return pure();
    if (argc == 6 && !strcmp(argv[1], "--rule") && !strcmp(argv[2], "band"))
        return printf("%d\n", (int)bu_etc1s_band_due((uint32_t)atol(argv[3]), (uint32_t)atol(argv[4]), atoi(argv[5]) != 0)) < 0;
    if (argc == 4 && !strcmp(argv[1], "--rule") && !strcmp(argv[2], "split")) return printf("%d\n", (int)bu_etc1s_slice_splits(true, (size_t)atoll(argv[3]))) < 0;
    if (argc != 3) return 2;
    const int rounds = atoi(argv[2]);
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint8_t> base;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0) base.insert(base.end(), buf, buf + n);
    fclose(fp);
    bool good = false;
    for (bu_read_target target : {BU_READ_RGBA, BU_READ_ETC1})  // (RGBA: an alpha file's slices in pairs; ETC1: every slice an image)
        if (!check_file(base.data(), base.size(), target, good) || !good) return 3;  // the pristine file must stream
    int read = 0, failed = 0, rejected = 0;
    for (int it = 0; it < rounds; it++) {
        std::vector<uint8_t> g = base;
        const int kind = rnd() % 4;
        const int flips = 1 + rnd() % 4;
        for (int k = 0; k < flips; k++) {
            size_t pos = kind == 0 ? rnd() % 77 : (kind == 1 ? 77 + rnd() % (g.size() > 200 ? 123 : 1) : rnd() % g.size());
            if (pos >= g.size()) pos = g.size() - 1;
            g[pos] ^= (uint8_t)(1u << (rnd() % 8));
        }
        if (kind == 3 && g.size() > 100) g.resize(77 + rnd() % (g.size() - 77));  // truncation
        // re-seal both CRCs so the mutation reaches the parsers behind them (one payload CRC in eight stays broken: it has to win)
        if (g.size() >= 77) {
            const uint16_t dc = (uint16_t)(bu_host::crc16(g.data() + 77, g.size() - 77, 0) ^ (rnd() % 8 ? 0 : 1));
            g[12] = (uint8_t)dc;
            g[13] = (uint8_t)(dc >> 8);
            const uint16_t hc = bu_host::crc16(g.data() + 8, 69, 0);
            g[6] = (uint8_t)hc;
            g[7] = (uint8_t)(hc >> 8);
        }
        // heap copy of exact size so ASan sees any over-read of the file buffer
        uint8_t* exact = (uint8_t*)malloc(g.size() ? g.size() : 1);
        memcpy(exact, g.data(), g.size());
        if (!check_file(exact, g.size(), (it & 1) ? BU_READ_RGBA : BU_READ_ETC1, good)) rejected++;
        else good ? read++ : failed++;
        free(exact);
    }
    printf("stream check done: %d read, %d failed as they do sequentially, %d never reached the scheduler\n", read, failed, rejected);
    return 0;
}
