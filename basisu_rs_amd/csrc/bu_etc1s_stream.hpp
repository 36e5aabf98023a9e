// Host-side scheduler of the streamed ETC1S front door (bu_read_etc1s_streamed, bu_capi_file.hpp): which slice is decoded where and by whom, and
// when a band of finished units may be launched.  The device enters through BuEtc1sSink and nothing else.  No HIP in here:
// tests/host_emul/bu_etc1s_stream_check.cpp compiles it as it is, with a recording sink, under ASan / UBSan and ThreadSanitizer.
//
// A slice's symbol stream is serial (one host core: 1.86 ms of BASELINE config 4's 2.6), and everything else used to queue up in
// front of and behind it: payload CRC 0.12 ms, codebooks 0.19 ms, upload + kernel + download 0.4 ms.  Here they run BESIDE it:
//   * the slice loop needs the four Huffman tables and the codebook SIZES, never the codebook entries: the tables are parsed first
//     (tens of microseconds), then pool threads decode the codebooks, run the payload CRC and decode the slices, all at once;
//   * the decoders write their indices into a page-locked buffer the kernels read directly over PCIe (no upload), and publish
//     finished block rows; the feeder launches the whole-file kernel over each band of finished 64-block units, so the
//     band's results travel to the (page-locked) output while the next rows are decoded.
// Errors keep the reference's order: CRC (basis.rs:338-341) before codebooks (mod.rs:69-76) before tables (:77-83) before slices
// (first failing slice in file order); work already launched for a file that fails is drained and its output discarded.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include "bu_basis.hpp"
#include "bu_file_layout.hpp"

constexpr size_t BU_ETC1S_STREAM_MIN_BLOCKS = 32768, BU_ETC1S_BAND_BLOCKS = 16384;

// BU_TRACE: the time since the previous lap, one line per step of a call
struct BuLap {
    const bool on;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* what)
    {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[bu_read_to] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    }
};

// The device side of a streamed read.  Each returns a status; a non-zero one ends the feeder and stops the decoders.
struct BuEtc1sSink {
    std::function<bu_status()> bind;                                // by a thread before it calls either of the others
    std::function<bu_status(const bu_host::BasisLz&)> codebooks;   // once, when both codebooks are decoded, before the first launch
    std::function<bu_status(uint32_t, uint32_t)> launch;           // the units [u0, u1) of one image, indices final
};

// What the scheduler leaves for bu_etc1s_stream_status
struct BuEtc1sStreamResult {
    bool crc_ok = true;
    bu_status st_cb = BU_OK, st_feed = BU_OK;
    std::vector<bu_status> st_slices;  // file order
};

// ---- the jobs ----------------------------------------------------------------------------------------------------------------------
// A slice of split_min blocks and more is decoded on TWO threads (bu_host::BasisLz::slice_lex / slice_resolve):
// one walks the bit stream and leaves a token pair per block, the other turns tokens into indices one row behind (endpoint
// prediction, selector history, the stores the GPU reads) -- the symbol loop of a slice is bound by one host core's instruction
// throughput, and this takes a quarter off it (1.55 -> 1.2 ms end to end for BASELINE config 4).  Any irregularity ends both
// halves, and whichever of the two finishes second decodes the slice again with the ordinary loops, which decide the status.
struct BuEtc1sStreamJob {
    size_t nbx = 0, nby = 0;
    const uint8_t* data = nullptr;
    size_t len = 0;
    uint32_t* idx = nullptr;
    std::atomic<uint32_t> rows{0};
    std::atomic<int> done{0};
    bu_status st = BU_OK;
    // the two-thread form
    bool split = false;
    uint32_t* tok_ep = nullptr;
    uint16_t* tok_sel = nullptr;
    std::atomic<uint32_t> rows_lexed{0};
    std::atomic<bool> split_failed{false};
    std::atomic<int> halves_done{0};
    bool lex_ok = false, res_ok = false;
};

// the two-thread form needs whole tables (BasisLz::split_ok) and the caller's leave
inline bool bu_etc1s_may_split(bu_status st_tables, const bu_host::BasisLz& lz, bool allowed) { return st_tables == BU_OK && lz.split_ok() && allowed; }
inline bool bu_etc1s_slice_splits(bool may_split, size_t nblk, size_t split_min = BU_ETC1S_STREAM_MIN_BLOCKS) { return may_split && nblk >= split_min; }
// a two-thread slice's tokens: 4 bytes (tok_ep) + 2 (tok_sel) per block, whole 64-byte lines
inline size_t bu_etc1s_tok_bytes(size_t nblk) { return (nblk * 6 + 127) & ~(size_t)63; }

// the token buffer a file's two-thread slices need
inline size_t bu_etc1s_stream_tok_bytes(const bu_host::BuFilePlan& p, bool may_split, size_t split_min = BU_ETC1S_STREAM_MIN_BLOCKS)
{
    size_t bytes = 0;
    for (size_t k = 0; k < p.images.size(); k++)
        for (size_t a = 0; a < (p.alpha_pairs ? 2u : 1u); a++) {
            const bu_slice_desc& s = p.slices[p.first_slice[k] + a];
            if (bu_etc1s_slice_splits(may_split, (size_t)s.num_blocks_x * s.num_blocks_y, split_min)) bytes += bu_etc1s_tok_bytes((size_t)s.num_blocks_x * s.num_blocks_y);
        }
    return bytes;
}

namespace {  // (BuEtc1sFileLayout's)

// The job table, file order (colour slice, then its alpha slice): which slice, where its indices go, whether it splits.  tok_buf of tok_cap
// bytes takes the tokens; a slice whose tokens it cannot hold (no memory: tok_buf == nullptr) takes the ordinary loop.
inline void bu_etc1s_stream_jobs(const uint8_t* file, const bu_host::BuFilePlan& p, const BuEtc1sFileLayout& l, uint32_t* h_idx, bool may_split, size_t split_min,
                                 void* tok_buf, size_t tok_cap, std::vector<BuEtc1sStreamJob>& jobs)
{
    const size_t n_img = p.images.size(), per_img = p.alpha_pairs ? 2 : 1;
    jobs = std::vector<BuEtc1sStreamJob>(n_img * per_img);
    uint8_t* t = static_cast<uint8_t*>(tok_buf);
    for (size_t k = 0; k < n_img; k++)
        for (size_t a = 0; a < per_img; a++) {
            const bu_slice_desc& s = p.slices[p.first_slice[k] + a];
            BuEtc1sStreamJob& j = jobs[k * per_img + a];
            j.nbx = s.num_blocks_x;
            j.nby = s.num_blocks_y;
            j.data = file + s.file_ofs;
            j.len = s.file_size;
            j.idx = h_idx + (a ? l.aidx_ofs[k] : l.idx_ofs[k]);
            const size_t nblk = j.nbx * j.nby;
            if (!bu_etc1s_slice_splits(may_split, nblk, split_min) || !t || bu_etc1s_tok_bytes(nblk) > tok_cap) continue;
            j.split = true;
            j.tok_ep = reinterpret_cast<uint32_t*>(t);
            j.tok_sel = reinterpret_cast<uint16_t*>(t + nblk * 4);
            t += bu_etc1s_tok_bytes(nblk);
            tok_cap -= bu_etc1s_tok_bytes(nblk);
        }
}

// ---- the work items behind the calling thread's own start on slice 0 ------------------------------------------------------------------
// Who does what: the CALLING thread starts on the first slice at once (all of it, or its bit-serial half) -- the symbol stream
// of the (first) slice is the critical path, and a parked pool thread takes tens of microseconds to wake up.  The pool threads
// pull work items from one counter, in this order: the first slice's resolver half (its lexer is already running), the codebooks,
// the feeder role (it launches bands of finished units through the sink until everything is launched), the payload
// CRC, then the other slices -- a two-thread slice as two items, lexer first, so that whoever pulls a resolver item knows its
// lexer has been claimed by a thread that never waits for anything.  The calling thread joins the queue when its own slice is
// done; if no pool thread ever took the feeder role it runs it last, when everything is decoded.
enum BuEtc1sItemKind { BU_ITEM_RESOLVE, BU_ITEM_FEED, BU_ITEM_CODEBOOKS, BU_ITEM_CRC, BU_ITEM_SLICE, BU_ITEM_LEX };
struct BuEtc1sItem {
    BuEtc1sItemKind kind;
    size_t job;
};
inline std::vector<BuEtc1sItem> bu_etc1s_stream_items(const std::vector<BuEtc1sStreamJob>& jobs)
{
    std::vector<BuEtc1sItem> items;
    if (!jobs.empty() && jobs[0].split) items.push_back({BU_ITEM_RESOLVE, 0});
    items.push_back({BU_ITEM_CODEBOOKS, 0});
    items.push_back({BU_ITEM_FEED, 0});
    items.push_back({BU_ITEM_CRC, 0});
    for (size_t k = 1; k < jobs.size(); k++) {
        if (jobs[k].split) {
            items.push_back({BU_ITEM_LEX, k});
            items.push_back({BU_ITEM_RESOLVE, k});
        } else
            items.push_back({BU_ITEM_SLICE, k});
    }
    return items;
}

// The band rule: `avail` whole units of an image lie inside the rows its slices have finished, `launched` of them are with the GPU.  The rest
// goes now when the image is finished, or when it makes a band of band_blocks blocks.
inline bool bu_etc1s_band_due(uint32_t avail, uint32_t launched, bool finished, size_t band_blocks = BU_ETC1S_BAND_BLOCKS)
{
    return avail > launched && (finished || (size_t)(avail - launched) * 64 >= band_blocks);
}

// The status of a streamed read once the pool has joined, in the reference's order.
inline bu_status bu_etc1s_stream_status(bool crc_pending, bu_status st_tables, const BuEtc1sStreamResult& r)
{
    if (crc_pending && !r.crc_ok) return BU_ERR_DATA_CRC;
    if (r.st_cb) return r.st_cb;
    if (st_tables) return st_tables;
    if (r.st_feed) return r.st_feed;  // (a device error: it stopped the decoders, whose statuses mean nothing then)
    for (const bu_status st : r.st_slices)
        if (st) return st;
    return BU_OK;
}

// ---- what the threads of one read share ---------------------------------------------------------------------------------------------
struct BuEtc1sStream {
    typedef BuEtc1sStreamJob Job;
    const uint8_t* file;
    size_t len;
    const bu_host::BuFilePlan& p;
    const BuEtc1sFileLayout& l;
    bu_host::BasisLz& lz;  // the tables; BU_ITEM_CODEBOOKS adds the codebooks
    bu_status st_tables;
    bool crc_pending;
    uint16_t crc_want;
    const BuEtc1sSink& sink;
    size_t band_blocks;
    BuEtc1sStreamResult& r;
    std::vector<Job> jobs;
    // abort: nothing that is still running can matter any more (a codebook / table / device error, or the scheduler is on its way
    // out): decoders stop at the next row.  slice_failed: some slice failed -- the feeder stops launching, but the OTHER slices
    // decode on: the call reports the first failing slice in file order, and an earlier slice may still fail too.
    std::atomic<bool> abort{false}, slice_failed{false}, feeder_taken{false};
    std::atomic<int> cb_done{0};

    // launches every image's units band by band as its slices publish rows, until all are launched or a flag says stop
    bu_status feeder()
    {
        const size_t n_img = p.images.size(), per_img = p.alpha_pairs ? 2 : 1;
        bu_status fs = sink.bind();  // (a pool thread has no current device yet)
        if (fs) return fs;
        for (unsigned spin = 0; !cb_done.load(std::memory_order_acquire); spin++) {
            if (abort.load(std::memory_order_relaxed)) return BU_OK;
            if (spin > 64) std::this_thread::yield();
        }
        if (r.st_cb != BU_OK || st_tables != BU_OK) return BU_OK;  // (reported by the caller, in the reference's order)
        if ((fs = sink.codebooks(lz))) return fs;
        std::vector<uint32_t> launched(n_img, 0);  // units of image k already handed to the GPU
        for (unsigned spin = 0;; spin++) {
            bool all = true, progressed = false;
            for (size_t k = 0; k < n_img; k++) {
                if (l.units_of[k] == 0 || launched[k] == l.units_of[k]) continue;
                // finished units of image k: whole 64-block units inside the rows BOTH of its slices have finished
                uint32_t avail = l.units_of[k];
                bool finished = true;
                for (size_t a2 = 0; a2 < per_img; a2++) {
                    Job& j = jobs[k * per_img + a2];
                    if (j.done.load(std::memory_order_acquire)) continue;
                    finished = false;
                    const size_t blocks = (size_t)j.rows.load(std::memory_order_acquire) * j.nbx;
                    avail = std::min<uint32_t>(avail, (uint32_t)(blocks / 64));
                }
                if (bu_etc1s_band_due(avail, launched[k], finished, band_blocks)) {
                    const bu_status ls = sink.launch(l.unit0[k] + launched[k], l.unit0[k] + avail);
                    if (ls) return ls;
                    launched[k] = avail;
                    progressed = true;
                }
                if (launched[k] != l.units_of[k]) all = false;
            }
            if (all || abort.load(std::memory_order_relaxed) || slice_failed.load(std::memory_order_relaxed)) return BU_OK;
            if (!progressed && spin > 16) std::this_thread::yield();
        }
    }
    // (a job runs on a pool thread: an exception -- std::bad_alloc from a vector sized by a hostile file -- must become a status there,
    // it cannot unwind through the pool)
    // publish_rows = false: the slice is decoded AGAIN after a two-thread attempt gave up (settle_split).  The resolver has already published
    // rows -- final ones, which this pass writes again with the same values -- and the feeder may have launched bands over them: the row
    // counter must not fall back to 1 and climb a second time, so this pass publishes nothing and the feeder picks the rest up from `done`.
    void run_slice(Job& j, bool publish_rows = true)
    {
        if (st_tables == BU_OK && !abort.load(std::memory_order_relaxed)) {
            try {
                j.st = lz.decode_slice(j.nbx, j.nby, j.data, j.len, j.idx, publish_rows ? &j.rows : nullptr, &abort);
            } catch (...) {
                j.st = BU_ERR_BOUNDS;
            }
        } else
            j.st = BU_ERR_ARGUMENT;  // never reported: an earlier error decides
        if (j.st) slice_failed.store(true, std::memory_order_relaxed);
        j.done.store(1, std::memory_order_release);
    }
    // the halves of a two-thread slice; the one that finishes second settles the slice
    void settle_split(Job& j)
    {
        if (j.halves_done.fetch_add(1, std::memory_order_acq_rel) != 1) return;
        if (j.lex_ok && j.res_ok) {
            j.st = BU_OK;
            j.done.store(1, std::memory_order_release);
        } else {
            run_slice(j, false);  // an irregular stream (or an abort): the ordinary loops, from the slice's first bit
        }
    }
    void run_lex(Job& j)
    {
        try {
            j.lex_ok = lz.slice_lex(j.nbx, j.nby, j.data, j.len, j.tok_ep, j.tok_sel, j.rows_lexed, j.split_failed);
        } catch (...) {
            j.lex_ok = false;
        }
        if (!j.lex_ok) j.split_failed.store(true, std::memory_order_release);
        settle_split(j);
    }
    void run_resolve(Job& j)
    {
        try {
            j.res_ok = lz.slice_resolve(j.nbx, j.nby, j.tok_ep, j.tok_sel, j.idx, j.rows_lexed, j.split_failed, &j.rows, &abort);
        } catch (...) {
            j.res_ok = false;
        }
        if (!j.res_ok) j.split_failed.store(true, std::memory_order_release);
        settle_split(j);
    }
    // one work item; true: this thread has been the feeder -- everything is launched (or stopped), nothing is left that it should start on
    bool run_item(const BuEtc1sItem& it, bool on_caller)
    {
        switch (it.kind) {
        case BU_ITEM_FEED: {
            // (the calling thread leaves the role to a pool thread: it would stop pulling items for as long as bands are pending;
            // it runs the feeder itself at the very end if nobody else did)
            if (on_caller || feeder_taken.exchange(true)) break;
            bu_status fs;
            try {
                fs = feeder();
            } catch (...) {
                fs = BU_ERR_HIP;
            }
            if (fs) {
                r.st_feed = fs;
                abort.store(true, std::memory_order_relaxed);
            }
            return true;
        }
        case BU_ITEM_CODEBOOKS:  // the first kernel launch waits for them
            try {
                r.st_cb = lz.init_codebooks(file + p.h.endpoint_cb_file_ofs, p.h.endpoint_cb_file_size, file + p.h.selector_cb_file_ofs, p.h.selector_cb_file_size);
            } catch (...) {
                r.st_cb = BU_ERR_BOUNDS;
            }
            if (r.st_cb) abort.store(true, std::memory_order_relaxed);
            cb_done.store(1, std::memory_order_release);
            break;
        case BU_ITEM_CRC:
            // (the serial form: bu_host::crc16 cuts large inputs into pieces for the pool -- which this call is holding)
            if (crc_pending) r.crc_ok = (uint16_t)~bu_host::crc16_raw(file + 77, len - 77, 0xFFFF) == crc_want;
            break;
        case BU_ITEM_SLICE: run_slice(jobs[it.job]); break;
        case BU_ITEM_LEX: run_lex(jobs[it.job]); break;
        case BU_ITEM_RESOLVE: run_resolve(jobs[it.job]); break;
        }
        return false;
    }
};

// ---- the scheduler -------------------------------------------------------------------------------------------------------------------
// lz holds the tables (init_tables gave st_tables) and takes the codebooks here.  The slices' indices go to h_idx as `l` lays them out; tok_buf
// (tok_cap bytes, bu_etc1s_stream_tok_bytes) takes the tokens of two-thread slices.  Returns when every thread has stopped and the pool is free;
// bu_etc1s_stream_status reads r.
inline void bu_etc1s_stream(const uint8_t* file, size_t len, const bu_host::BuFilePlan& p, const BuEtc1sFileLayout& l, bu_host::BasisLz& lz, bu_status st_tables,
                            bool crc_pending, uint16_t crc_want, uint32_t* h_idx, void* tok_buf, size_t tok_cap, bool may_split, const BuEtc1sSink& sink, BuLap& lap,
                            BuEtc1sStreamResult& r, size_t split_min = BU_ETC1S_STREAM_MIN_BLOCKS, size_t band_blocks = BU_ETC1S_BAND_BLOCKS)
{
    const bool trace = lap.on;
    BuEtc1sStream s{file, len, p, l, lz, st_tables, crc_pending, crc_want, sink, band_blocks, r};
    std::vector<BuEtc1sStreamJob>& jobs = s.jobs;
    bu_etc1s_stream_jobs(file, p, l, h_idx, may_split, split_min, tok_buf, tok_cap, jobs);
    const std::vector<BuEtc1sItem> items = bu_etc1s_stream_items(jobs);
    std::atomic<size_t> next{0};
    const std::thread::id caller = std::this_thread::get_id();
    // BU_TRACE: when every item started and ended, relative to this point
    struct ItemLog {
        double t0 = 0, t1 = 0;
    };
    std::vector<ItemLog> item_log(trace ? items.size() + 1 : 0);
    const auto t_items = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_items).count(); };
    const std::function<void()> work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < items.size();) {
            struct Stamp {
                ItemLog* l;
                decltype(since)& now;
                Stamp(ItemLog* l_, decltype(since)& n) : l(l_), now(n)
                {
                    if (l) l->t0 = now();
                }
                ~Stamp()
                {
                    if (l) l->t1 = now();
                }
            } stamp(trace ? &item_log[i] : nullptr, since);
            if (s.run_item(items[i], std::this_thread::get_id() == caller)) return;
        }
    };
    const unsigned helpers = bu_host::pool().begin((unsigned)std::min<size_t>(items.size(), bu_host::Pool::capacity()), work);
    (void)helpers;
    struct PoolEnd {  // the pool is released on every path out of this function, after the jobs have seen the abort flag
        std::atomic<bool>& abort;
        bool armed = true;
        ~PoolEnd()
        {
            if (armed) {
                abort.store(true);
                bu_host::pool().end();
            }
        }
    } pool_end{s.abort};
    if (!jobs.empty()) {
        if (jobs[0].split) s.run_lex(jobs[0]);
        else s.run_slice(jobs[0]);
    }
    lap(!jobs.empty() && jobs[0].split ? "slice 0 lexed (resolver on a pool thread)" : "slice 0 decoded");
    work();  // whatever is still in the queue (the feeder item is skipped by this thread)
    pool_end.armed = false;
    bu_host::pool().end();  // every item has finished; the feeder, if a pool thread took the role, has launched everything (or seen a flag)
    if (!s.feeder_taken.exchange(true)) {  // nobody fed the GPU meanwhile: everything is decoded, launch it now
        try {
            r.st_feed = s.feeder();
        } catch (...) {
            r.st_feed = BU_ERR_HIP;
        }
    }
    lap("pool joined, bands launched");
    if (trace) {
        static const char* const names[] = {"resolve", "feed", "codebooks", "crc", "slice", "lex"};
        for (size_t i = 0; i < items.size(); i++)
            fprintf(stderr, "[bu_read_to]   item %2zu %-9s job %2zu (%5zu x %5zu)  %7.3f .. %7.3f ms\n", i, names[items[i].kind], items[i].job,
                    items[i].kind >= BU_ITEM_SLICE || items[i].kind == BU_ITEM_RESOLVE ? jobs[items[i].job].nbx : (size_t)0,
                    items[i].kind >= BU_ITEM_SLICE || items[i].kind == BU_ITEM_RESOLVE ? jobs[items[i].job].nby : (size_t)0, item_log[i].t0, item_log[i].t1);
    }
    r.st_slices.clear();
    for (const BuEtc1sStreamJob& j : jobs) r.st_slices.push_back(j.st);
}

}  // namespace
