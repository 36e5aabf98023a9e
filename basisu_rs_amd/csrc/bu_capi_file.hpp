// C ABI, whole-file level: the crate's public read_to_* API (src/lib.rs:20-22, src/basis.rs) -- container parse, CRC and BasisLZ
// decode on the host (bu_basis.hpp), block work through the kernels; the UASTC file writer.
// Part of the single translation unit bu_hip.hip.
#pragma once
extern "C" {

// ---- whole-file level (basis.rs) --------------------------------------------------------------------
bu_status bu_basis_read_header(const uint8_t* file, size_t len, bu_basis_header* out)
{
    if (!file || !out) return BU_ERR_ARGUMENT;
    return bu_host::read_header(file, len, out);
}

static bu_status bu_basis_read_slice_descs_impl(const uint8_t* file, size_t len, const bu_basis_header* header, bu_slice_desc* out, size_t max_descs,
                                              size_t* n_descs)
{
    if (!file || !header) return BU_ERR_ARGUMENT;
    std::vector<bu_slice_desc> v;
    bu_status st = bu_host::read_slice_descs(file, len, header, v);
    if (st) return st;
    if (n_descs) *n_descs = v.size();
    if (out) {
        if (v.size() > max_descs) return BU_ERR_OUTPUT_SIZE;
        for (size_t i = 0; i < v.size(); i++) out[i] = v[i];
    }
    return BU_OK;
}

uint16_t bu_basis_crc16(const uint8_t* data, size_t len, uint16_t crc) { return bu_host::crc16(data, len, crc); }

using bu_host::BuFilePlan;
using bu_host::bu_plan_file;
using bu_host::bu_make_lz;

// the slice-level target a UASTC file's slices are transcoded to (BU_READ_UASTC never gets here: plain copies)
static bu_target bu_read_block_target(bu_read_target target)
{
    switch (target) {
    case BU_READ_RGBA: return BU_TARGET_RGBA32;
    case BU_READ_ASTC: return BU_TARGET_ASTC;
    case BU_READ_BC7: return BU_TARGET_BC7;
    case BU_READ_ETC1: return BU_TARGET_ETC1;
    case BU_READ_BC4: return BU_TARGET_BC4_R;
    case BU_READ_BC5: return BU_TARGET_BC5_RG;
    case BU_READ_EAC_R11: return BU_TARGET_EAC_R11;
    case BU_READ_EAC_RG11: return BU_TARGET_EAC_RG11;
    case BU_READ_BC1: return BU_TARGET_BC1_RGB;
    case BU_READ_BC3: return BU_TARGET_BC3_RGBA;
    default: return BU_TARGET_ETC2;
    }
}

// the read target whose block target `target` is (bu_read_block_target inverted); false: `target` is no bu_target
static bool bu_block_read_target(bu_target target, bu_read_target* out)
{
    for (int t = (int)BU_READ_RGBA; t <= (int)BU_READ_BC3; t++)
        if (t != (int)BU_READ_UASTC && t != 10 && bu_read_block_target((bu_read_target)t) == target) {
            *out = (bu_read_target)t;
            return true;
        }
    return false;
}

// etc1s_six: the call is bu_read_file_query (bu_plan_file)
static bu_status bu_read_query_impl(bu_read_target target, const uint8_t* file, size_t len, size_t* n_images, size_t* out_bytes, bool etc1s_six = false)
{
    BuFilePlan p;
    bu_status st = bu_plan_file(target, file, len, p, true, etc1s_six);
    if (st) return st;
    if (n_images) *n_images = p.images.size();
    if (out_bytes) *out_bytes = p.out_bytes;
    return BU_OK;
}

static bu_status bu_basislz_decode_impl(const uint8_t* file, size_t len, uint32_t slice_index, uint32_t* endpoints_out, uint8_t* selectors_out,
                                       uint32_t* idx_out)
{
    if (!file) return BU_ERR_ARGUMENT;
    bu_basis_header h;
    bu_status st = bu_host::read_header(file, len, &h);
    if (st) return st;
    if (h.tex_format != 0) return BU_ERR_UNSUPPORTED;
    std::vector<bu_slice_desc> slices;
    st = bu_host::read_slice_descs(file, len, &h, slices);
    if (st) return st;
    bu_host::BasisLz lz;
    st = bu_make_lz(file, len, h, lz);
    if (st) return st;
    if (endpoints_out) memcpy(endpoints_out, lz.endpoints.data(), lz.endpoints.size() * 4);
    if (selectors_out) memcpy(selectors_out, lz.selectors.data(), lz.selectors.size());
    if (idx_out) {
        if (slice_index >= slices.size()) return BU_ERR_ARGUMENT;
        const bu_slice_desc& s = slices[slice_index];
        if (!bu_host::in_file(len, s.file_ofs, s.file_size)) return BU_ERR_BOUNDS;
        st = lz.decode_slice(s.num_blocks_x, s.num_blocks_y, file + s.file_ofs, s.file_size, idx_out);
    }
    return st;
}

// The whole-file ETC1S kernel (bu_etc1s_kernels.hpp) of a slot (bu_etc1s_slot's numbering: 0 ETC1, 1 RGBA32, 2.. the six targets) over
// the 64-block units [u0, u1) of the slices d_descs describes, on the context stream; both codebooks of n_cb entries.  The caller
// asks hipGetLastError.
static void bu_etc1s_file_launch(bu_context* ctx, unsigned slot, unsigned grid, const uint32_t* d_idx, const BuEtc1sSlice* d_descs, uint32_t n_slices,
                                 uint32_t u0, uint32_t u1, const uint32_t* d_ep, const uint2* d_sel, uint32_t n_cb, uint8_t* d_out, uint64_t* d_status)
{
    typedef void (*Fn)(const uint32_t*, const BuEtc1sSlice*, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, const uint2*, uint32_t, uint8_t*,
                       unsigned long long*, const BuTablesAll*);
    static const Fn kernels[8] = {&bu_etc1s_file_kernel<false>,
                                  &bu_etc1s_file_kernel<true>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_BC4>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_BC5>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_R11>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_RG11>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_BC1>,
                                  &bu_etc1s_file_target_kernel<BU_TGT_BC3>};
    hipLaunchKernelGGL(kernels[slot], dim3(grid), dim3(BU_WG), 0, ctx->stream, d_idx, d_descs, n_slices, u0, u1, d_ep, n_cb, d_sel, n_cb, d_out,
                       reinterpret_cast<unsigned long long*>(d_status), ctx->d_tables);
}

// the slot of an ETC1S file's kernel: the plan's block target for the six (bu_read_file_to), else RGBA32 or ETC1
static unsigned bu_etc1s_file_slot(const BuFilePlan& p, bu_read_target target)
{
    return p.etc1s_six ? bu_etc1s_target_slot(bu_read_block_target(target)) : target == BU_READ_RGBA ? 1u : 0u;
}

// ---- streamed ETC1S front door -------------------------------------------------------------------------------------------------
// The device half of a streamed read: buffers up, the slices decoded and their bands launched by the scheduler of bu_etc1s_stream.hpp (which
// says why and in what order) through a sink of this context's stream, results and status words down.
static bu_status bu_read_etc1s_streamed(bu_context* ctx, bu_read_target target, const uint8_t* file, size_t len, const BuFilePlan& p, uint8_t* out,
                                        bool crc_pending, uint16_t crc_want, BuLap& lap)
{
    using bu_host::in_file;
    const bu_basis_header& h = p.h;
    // (the pool is not taken yet: the pooled CRC)
    const auto leave = [&](bu_status s) { return (crc_pending && bu_host::crc16(file + 77, len - 77, 0) != crc_want) ? BU_ERR_DATA_CRC : s; };
    if (!in_file(len, h.endpoint_cb_file_ofs, h.endpoint_cb_file_size) || !in_file(len, h.selector_cb_file_ofs, h.selector_cb_file_size) ||
        !in_file(len, h.tables_file_ofs, h.tables_file_size) || !in_file(len, h.extended_file_ofs, h.extended_file_size))
        return leave(BU_ERR_BOUNDS);
    bu_host::BasisLz lz;
    // total_selectors for both codebooks: basis.rs:289-291
    const bu_status st_tables = lz.init_tables(h.total_selectors, h.total_selectors, file + h.tables_file_ofs, h.tables_file_size, h.tex_type == 3);
    lap("tables");
    const size_t n_img = p.images.size();
    BuEtc1sFileLayout l;
    bu_status st = bu_etc1s_file_layout(p, l);
    if (st) return leave(st);

    BuStagedCall call(ctx, n_img);
    if ((st = call.begin()) || (st = bu_reserve_h_idx(ctx, (l.words ? l.words : 16) * 4))) return st;
    void* d_idx_view = nullptr;
    if (!bu_device_view(ctx->h_idx, &d_idx_view)) return BU_ERR_HIP;
    void* d_out = nullptr;
    const size_t n_cb = h.total_selectors;
    // both codebooks, the status words, then one descriptor per image (+ sentinel)
    enum { EP, SEL, STATUS, DESCS };
    if ((st = call.output(out, p.out_bytes, p.out_bytes, true, 16, &d_out)) ||
        (st = call.aux(BuAuxLayout({n_cb * 4, n_cb * 8, 8 * n_img, l.descs.size() * sizeof(BuEtc1sSlice)}), STATUS)) || (st = call.status_reset()))
        return st;
    BU_HIP(ctx, hipMemcpyAsync(call.region<void>(DESCS), l.descs.data(), l.descs.size() * sizeof(BuEtc1sSlice), hipMemcpyHostToDevice, ctx->stream));
    lap("reserve");

    const bool may_split = bu_etc1s_may_split(st_tables, lz, !getenv("BU_ETC1S_ONE_THREAD"));
    bu_reserve_lex(ctx, bu_etc1s_stream_tok_bytes(p, may_split));
    BuEtc1sSink sink;
    sink.bind = [&]() -> bu_status {
        BU_HIP(ctx, hipSetDevice(ctx->device));
        return BU_OK;
    };
    sink.codebooks = [&](const bu_host::BasisLz& z) -> bu_status {
        if (!z.endpoints.empty()) BU_HIP(ctx, hipMemcpyAsync(call.region<void>(EP), z.endpoints.data(), z.endpoints.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!z.selectors.empty()) BU_HIP(ctx, hipMemcpyAsync(call.region<void>(SEL), z.selectors.data(), z.selectors.size(), hipMemcpyHostToDevice, ctx->stream));
        return BU_OK;
    };
    sink.launch = [&](uint32_t u0, uint32_t u1) -> bu_status {
        const unsigned grid = bu_grid_for((size_t)(u1 - u0) * 64, ctx->cu_count);
        bu_etc1s_file_launch(ctx, bu_etc1s_file_slot(p, target), grid, static_cast<const uint32_t*>(d_idx_view), call.region<const BuEtc1sSlice>(DESCS),
                             (uint32_t)(l.descs.size() - 1), u0, u1, call.region<const uint32_t>(EP), call.region<const uint2>(SEL), (uint32_t)n_cb,
                             static_cast<uint8_t*>(d_out), call.d_status);
        BU_HIP(ctx, hipGetLastError());
        return BU_OK;
    };
    BuEtc1sStreamResult res;
    bu_etc1s_stream(file, len, p, l, lz, st_tables, crc_pending, crc_want, static_cast<uint32_t*>(ctx->h_idx), ctx->lex_buf, ctx->lex_cap, may_split, sink, lap, res);
    if ((st = bu_etc1s_stream_status(crc_pending, st_tables, res)) || (st = call.finish())) return st;
    lap("last band + synchronise");
    return call.status(nullptr);
}

// ---- UASTC file to BU_READ_UASTC: plain copies, no device work (uastc.rs:85-87) ---------------------------------------------------
static bu_status bu_read_uastc_copy(const uint8_t* file, const BuFilePlan& p, uint8_t* out)
{
    for (size_t k = 0; k < p.images.size(); k++) {
        const bu_slice_desc& s = p.slices[p.first_slice[k]];
        if (s.file_size) memcpy(out + p.images[k].offset, file + s.file_ofs, s.file_size);
    }
    return BU_OK;
}

// ---- ETC1S file in one launch (files below BU_ETC1S_STREAM_MIN_BLOCKS, BU_ETC1S_ONE_LAUNCH) ---------------------------------------
// The symbol streams of all slices are decoded on the host cores before anything is uploaded; index buffer, codebooks and slice table go up
// on the context stream, ONE launch serves the whole file (basis.rs:42-58 / 103-123 walk the slices one by one; one status word per image),
// and a single synchronisation ends the call.  The device output buffer mirrors `out`.
static bu_status bu_read_etc1s_one_launch(bu_context* ctx, bu_read_target target, const uint8_t* file, size_t len, const BuFilePlan& p, uint8_t* out, BuLap& lap)
{
    const size_t n_img = p.images.size();
    bu_host::BasisLz lz;
    bu_status st = bu_make_lz(file, len, p.h, lz);
    if (st) return st;
    lap("codebooks + tables");
    BuEtc1sFileLayout l;
    if ((st = bu_etc1s_file_layout(p, l))) return st;
    std::vector<uint32_t> idx_all(l.words ? l.words : 1, 0);
    std::vector<bu_host::SliceJob> jobs;  // file order: colour slice, then its alpha slice
    jobs.reserve(n_img * (p.alpha_pairs ? 2 : 1));
    for (size_t k = 0; k < n_img; k++)
        for (size_t a = 0; a < (p.alpha_pairs ? 2u : 1u); a++) {
            const bu_slice_desc& s = p.slices[p.first_slice[k] + a];
            jobs.push_back({s.num_blocks_x, s.num_blocks_y, file + s.file_ofs, s.file_size, idx_all.data() + (a ? l.aidx_ofs[k] : l.idx_ofs[k]), BU_OK});
        }
    st = bu_host::decode_slices(lz, jobs);  // host cores in parallel; the symbol stream is serial only within a slice
    if (st) return st;
    lap("slice symbol streams");
    const size_t total_in = l.words * 4;
    BuStagedCall call(ctx, n_img);
    const void* d_in = nullptr;
    void* d_out = nullptr;
    // a page-locked `out` (bu_host_alloc) receives the kernels' stores directly over PCIe: no device output buffer, no download.
    // Behind the codebooks: the status words, then one descriptor per image (+ sentinel)
    enum { EP, SEL, STATUS, DESCS };
    // (d_in is reserved in front of the status reset, the indices go up behind it)
    if ((st = call.begin()) || (st = call.input(nullptr, total_in, false, 16, nullptr)) || (st = call.output(out, p.out_bytes, p.out_bytes, true, 16, &d_out)) ||
        (st = call.aux(BuAuxLayout({lz.endpoints.size() * 4, lz.selectors.size(), 8 * n_img, l.descs.size() * sizeof(BuEtc1sSlice)}), STATUS)) ||
        (st = call.status_reset()) || (st = call.input(idx_all.data(), total_in, false, 16, &d_in)))
        return st;
    if (!lz.endpoints.empty()) BU_HIP(ctx, hipMemcpyAsync(call.region<void>(EP), lz.endpoints.data(), lz.endpoints.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    if (!lz.selectors.empty()) BU_HIP(ctx, hipMemcpyAsync(call.region<void>(SEL), lz.selectors.data(), lz.selectors.size(), hipMemcpyHostToDevice, ctx->stream));
    BU_HIP(ctx, hipMemcpyAsync(call.region<void>(DESCS), l.descs.data(), l.descs.size() * sizeof(BuEtc1sSlice), hipMemcpyHostToDevice, ctx->stream));
    if (l.n_units) {
        const unsigned grid = bu_grid_for((size_t)l.n_units * 64, ctx->cu_count);
        bu_etc1s_file_launch(ctx, bu_etc1s_file_slot(p, target), grid, static_cast<const uint32_t*>(d_in), call.region<const BuEtc1sSlice>(DESCS),
                             (uint32_t)(l.descs.size() - 1), 0u, l.n_units, call.region<const uint32_t>(EP), call.region<const uint2>(SEL),
                             (uint32_t)lz.endpoints.size(), static_cast<uint8_t*>(d_out), call.d_status);
        BU_HIP(ctx, hipGetLastError());
    }
    lap("reserve + enqueue");
    BU_HIP(ctx, hipGetLastError());
    if ((st = call.finish())) return st;
    lap("download + synchronise");
    return call.status(nullptr);
}

// ---- UASTC file through the kernels -------------------------------------------------------------------------------------------------
// Every run of slices (bu_file_layout.hpp) is staged at an aligned offset of one device buffer with one upload, the device output buffer
// mirrors `out`, all launches go to the context stream back to back (one status word per image) -- large runs with a mapped output in
// pieces on two streams -- and a single synchronisation ends the call.
// crc_deferred: the payload CRC (0.7 ms per 16 MiB on the host cores -- as long as upload, kernel and download together) is computed ON THE
// DEVICE over the slice bytes the call uploads anyway (bu_crc16_pieces_kernel, one register per 64 KiB piece) and folded at the end
// (bu_crc_fold), which clears the flag; an earlier error return leaves it set.
static bu_status bu_read_uastc_runs(bu_context* ctx, bu_read_target target, const uint8_t* file, size_t len, const BuFilePlan& p, uint8_t* out, bool& crc_deferred,
                                    uint16_t crc_want, BuLap& lap)
{
    const size_t n_img = p.images.size();
    BuUastcFileLayout l;
    bu_uastc_file_layout(p, l);
    std::vector<BuCrcSeg> crc_segs;         // uploaded file ranges whose 64 KiB pieces the device registers
    std::vector<uint16_t> crc_parts(crc_deferred ? l.total_in / BU_CRC_PIECE + 1 : 1, 0);  // landing area of the CRC registers: in front of the call, outlives its drain
    size_t crc_pieces = 0;
    BuStagedCall call(ctx, n_img);
    bu_status st;
    void* d_out_all = nullptr;
    // a page-locked `out` (bu_host_alloc) receives the kernels' stores directly over PCIe: no device output buffer, no download
    enum { STATUS, CRC };
    if ((st = call.begin()) || (st = call.input(nullptr, l.total_in, false, 16, nullptr)) || (st = call.output(out, p.out_bytes, p.out_bytes, true, 16, &d_out_all)) ||
        (st = call.aux(BuAuxLayout({8 * n_img, 2 * crc_parts.size()}), STATUS)))
        return st;
    const bool direct_out = call.out_mapped;
    uint8_t* const d_in = static_cast<uint8_t*>(ctx->d_in);  // (only reserved above: the runs go up one by one below)
    uint8_t* const d_out = static_cast<uint8_t*>(d_out_all);
    uint64_t* const d_status = call.d_status;
    uint16_t* const d_crc = call.region<uint16_t>(CRC);
    // registers of the whole 64 KiB pieces of an uploaded range, on the stream that carries its upload
    auto crc_enqueue = [&](const uint8_t* d_range, size_t file_ofs, size_t nbytes, hipStream_t ps) {
        if (!crc_deferred) return;
        const size_t np = nbytes / BU_CRC_PIECE;
        if (np) hipLaunchKernelGGL(bu_crc16_pieces_kernel, dim3((unsigned)np), dim3(256), 0, ps, reinterpret_cast<const uint4*>(d_range), d_crc + crc_pieces, ctx->d_crc_tables);
        crc_segs.push_back({file_ofs, nbytes, crc_pieces, np});
        crc_pieces += np;
    };
    if ((st = call.status_reset())) return st;
    int used_extra = 0;  // own streams 0..used_extra-1 carry pieces (forked behind the status reset, joined on the host)
    const char* const fixed_piece_mib = getenv("BU_RUN_PIECE_MIB");
    const bu_target bt = bu_read_block_target(target);
    for (const BuFileRun& r : l.runs) {
        if (r.bytes == 0) continue;
        const uint8_t* const src = file + r.file_ofs;
        uint8_t* const d_run = d_in + r.in_off;
        uint8_t* const d_run_out = d_out + p.images[r.first].offset;
        const size_t piece_bytes = bu_run_piece_bytes(r.bytes, fixed_piece_mib);
        const bool pieced = bu_run_is_pieced(target, direct_out, piece_bytes, r.bytes);
        if (pieced) {
            constexpr int n_ps = 2;  // streams that carry pieces: the context's internal one and one of its own
            if ((st = bu_ctx_streams(ctx, n_ps - 1))) return st;
            if (used_extra < n_ps - 1) {
                BU_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));  // the status words are reset on the context stream
                for (; used_extra < n_ps - 1; used_extra++) BU_HIP(ctx, hipStreamWaitEvent(ctx->extra_streams[used_extra], ctx->ev0, 0));
            }
            const size_t obytes = bu_target_block_bytes(bt);
            size_t piece_no = 0;
            for (size_t done = 0; done < r.bytes; done += piece_bytes, piece_no++) {
                const size_t nbytes = r.bytes - done < piece_bytes ? r.bytes - done : piece_bytes;
                const size_t lane = piece_no % (size_t)n_ps;
                hipStream_t ps = lane ? ctx->extra_streams[lane - 1].load(std::memory_order_acquire) : ctx->stream;
                BU_HIP(ctx, hipMemcpyAsync(d_run + done, src + done, nbytes, hipMemcpyHostToDevice, ps));
                crc_enqueue(d_run + done, r.file_ofs + done, nbytes, ps);
                if ((st = bu_launch_uastc(ctx, bt, d_run + done, nbytes / 16, d_run_out + (done / 16) * obytes, 1, done / 16, d_status + r.first, ps, BU_ZEROCOPY_GRID)))
                    return st;
            }
        } else {
            BU_HIP(ctx, hipMemcpyAsync(d_run, src, r.bytes, hipMemcpyHostToDevice, ctx->stream));
            crc_enqueue(d_run, r.file_ofs, r.bytes, ctx->stream);
        }
        if (target == BU_READ_RGBA) {  // image geometry differs per slice: one launch each
            for (size_t k = r.first; k <= r.last; k++) {
                const bu_slice_desc& s = p.slices[p.first_slice[k]];
                if ((st = bu_launch_uastc(ctx, bt, d_in + l.in_off[k], s.file_size / 16, d_out + p.images[k].offset, s.num_blocks_x ? s.num_blocks_x : 1, 0, d_status + k,
                                          ctx->stream, direct_out ? BU_ZEROCOPY_GRID : 0)))
                    return st;
            }
        } else if (!pieced) {  // block-linear: the run's outputs are contiguous from its first image's offset on
            if ((st = bu_launch_uastc(ctx, bt, d_run, r.bytes / 16, d_run_out, 1, 0, d_status + r.first, ctx->stream, direct_out ? BU_ZEROCOPY_GRID : 0))) return st;
        }
    }
    lap("reserve + enqueue");
    // the status words (and the CRC registers of the pieces) are read on the context stream: it must see the other streams' kernels.  Joined on the
    // HOST -- a cross-stream event wait costs 70-80 us on this runtime, a wait for streams that are nearly done costs nothing
    for (int i = 0; i < used_extra; i++) BU_HIP(ctx, hipStreamSynchronize(ctx->extra_streams[i]));
    BU_HIP(ctx, hipGetLastError());
    if ((st = call.finish(crc_parts.data(), d_crc, 2 * crc_pieces))) return st;
    lap("download + synchronise");
    if (crc_deferred) {  // the reference checks the CRC before anything else behind the header (basis.rs:338-341): before the status words
        crc_deferred = false;
        const bool crc_ok = bu_crc_fold(file, len, crc_segs, crc_parts.data(), crc_want);
        lap("data CRC fold");
        if (!crc_ok) return BU_ERR_DATA_CRC;
    }
    return call.status(nullptr);
}

// etc1s_six: the call is bu_read_file_to (bu_plan_file)
static bu_status bu_read_to_impl(bu_context* ctx, bu_read_target target, const uint8_t* file, size_t len, bu_basis_header* header_out, bu_image* images,
                                size_t max_images, size_t* n_images, uint8_t* out, size_t out_bytes, bool etc1s_six = false)
{
    if (!ctx || !out) return BU_ERR_ARGUMENT;
    BuLap lap{getenv("BU_TRACE") != nullptr};
    // The reference checks the payload CRC before anything else behind the header (basis.rs:338-341), so a CRC failure takes precedence
    // over every later error, and nothing is reported as success before it is known.  Two kinds of file defer it past the plan: large
    // UASTC files (bu_read_uastc_runs: on the device) and ETC1S files of some size (bu_read_etc1s_streamed: on a pool thread beside the
    // entropy decode).  A path that returns with the CRC still deferred -- an early error, the one-launch path -- has it settled on the host.
    bool crc_deferred = false;
    uint16_t crc_want = 0;
    {
        bu_basis_header h0;
        if (file && len >= ((size_t)1 << 20) && bu_host::read_header(file, len, &h0) == BU_OK && h0.tex_format == 1 && target != BU_READ_UASTC) {
            crc_deferred = true;
            crc_want = h0.data_crc16;
        }
        if (file && len >= ((size_t)64 << 10) && !getenv("BU_ETC1S_ONE_LAUNCH") && bu_host::read_header(file, len, &h0) == BU_OK && h0.tex_format == 0) {
            crc_deferred = true;
            crc_want = h0.data_crc16;
        }
    }
    auto settle = [&](bu_status s) {  // the status to report once the deferred CRC is known
        if (crc_deferred) {
            crc_deferred = false;
            if (bu_host::crc16(file + 77, len - 77, 0) != crc_want) return BU_ERR_DATA_CRC;
        }
        return s;
    };
    BuFilePlan p;
    bu_status st = bu_plan_file(target, file, len, p, !crc_deferred, etc1s_six);
    lap("plan (parse + CRCs)");
    if (st) return settle(st);
    if (header_out) *header_out = p.h;
    if (n_images) *n_images = p.images.size();
    if (out_bytes < p.out_bytes || (images && p.images.size() > max_images)) return settle(BU_ERR_OUTPUT_SIZE);
    if (images) std::copy(p.images.begin(), p.images.end(), images);
    if (p.images.empty()) return settle(BU_OK);
    if (!p.etc1s) return settle(target == BU_READ_UASTC ? bu_read_uastc_copy(file, p, out) : bu_read_uastc_runs(ctx, target, file, len, p, out, crc_deferred, crc_want, lap));
    size_t total_blocks = 0;
    for (size_t k = 0; k < p.images.size(); k++) total_blocks += (size_t)p.slices[p.first_slice[k]].num_blocks_x * p.slices[p.first_slice[k]].num_blocks_y;
    if (total_blocks >= BU_ETC1S_STREAM_MIN_BLOCKS && !getenv("BU_ETC1S_ONE_LAUNCH")) {
        const bool pending = crc_deferred;
        crc_deferred = false;  // settled inside (on a pool thread); nothing is left for settle()
        return bu_read_etc1s_streamed(ctx, target, file, len, p, out, pending, crc_want, lap);
    }
    return settle(bu_read_etc1s_one_launch(ctx, target, file, len, p, out, lap));
}

// C++ exceptions must not cross the C ABI (a ctypes or Rust caller would be terminated): vectors sized from untrusted
// file fields can throw std::bad_alloc, thread creation std::system_error.  A file that asks for more memory than
// exists is reported like any other out-of-bounds field.
#define BU_GUARDED(call)                 \
    try {                                \
        return call;                     \
    } catch (const std::bad_alloc&) {    \
        return BU_ERR_BOUNDS;            \
    } catch (...) {                      \
        return BU_ERR_HIP;               \
    }
bu_status bu_basis_read_slice_descs(const uint8_t* file, size_t len, const bu_basis_header* header, bu_slice_desc* out, size_t max_descs,
                                    size_t* n_descs)
{
    BU_GUARDED(bu_basis_read_slice_descs_impl(file, len, header, out, max_descs, n_descs))
}
bu_status bu_read_query(bu_read_target target, const uint8_t* file, size_t len, size_t* n_images, size_t* out_bytes)
{
    BU_GUARDED(bu_read_query_impl(target, file, len, n_images, out_bytes))
}
bu_status bu_basislz_decode(const uint8_t* file, size_t len, uint32_t slice_index, uint32_t* endpoints_out, uint8_t* selectors_out,
                            uint32_t* idx_out)
{
    BU_GUARDED(bu_basislz_decode_impl(file, len, slice_index, endpoints_out, selectors_out, idx_out))
}
bu_status bu_read_to(bu_context* ctx, bu_read_target target, const uint8_t* file, size_t len, bu_basis_header* header_out, bu_image* images,
                     size_t max_images, size_t* n_images, uint8_t* out, size_t out_bytes)
{
    BU_GUARDED(bu_read_to_impl(ctx, target, file, len, header_out, images, max_images, n_images, out, out_bytes))
}
// The file calls keyed by block format: a UASTC file, and ETC1 / RGBA32 of an ETC1S file, are bu_read_to's with the read target whose
// block target this is; the six targets of an ETC1S file are planned with the flag.
bu_status bu_read_file_query(bu_target target, const uint8_t* file, size_t len, size_t* n_images, size_t* out_bytes)
{
    bu_read_target rt;
    if (!bu_block_read_target(target, &rt)) return BU_ERR_ARGUMENT;
    BU_GUARDED(bu_read_query_impl(rt, file, len, n_images, out_bytes, true))
}
bu_status bu_read_file_to(bu_context* ctx, bu_target target, const uint8_t* file, size_t len, bu_basis_header* header_out, bu_image* images,
                          size_t max_images, size_t* n_images, uint8_t* out, size_t out_bytes)
{
    bu_read_target rt;
    if (!bu_block_read_target(target, &rt)) return BU_ERR_ARGUMENT;
    BU_GUARDED(bu_read_to_impl(ctx, rt, file, len, header_out, images, max_images, n_images, out, out_bytes, true))
}
#undef BU_GUARDED

bu_status bu_basis_write_uastc(const bu_slice_desc* descs, const uint8_t* const* slice_data, const size_t* slice_bytes, size_t n_slices,
                               uint16_t header_flags, uint8_t tex_type, uint8_t* out, size_t out_cap, size_t* out_len)
{
    if ((n_slices && (!descs || !slice_data || !slice_bytes)) || n_slices >= (1u << 24)) return BU_ERR_ARGUMENT;
    size_t total = 77 + 23 * n_slices;
    for (size_t i = 0; i < n_slices; i++) total += slice_bytes[i];
    if (out_len) *out_len = total;
    if (!out) return BU_OK;
    if (out_cap < total || total > 0xFFFFFFFFull) return BU_ERR_OUTPUT_SIZE;
    auto put = [&](size_t pos, uint32_t v, int n) { for (int k = 0; k < n; k++) out[pos + k] = (uint8_t)(v >> (8 * k)); };
    memset(out, 0, 77 + 23 * n_slices);
    size_t ofs = 77 + 23 * n_slices;
    uint32_t n_images = 0;
    for (size_t i = 0; i < n_slices; i++) {
        const size_t d = 77 + 23 * i;
        put(d, descs[i].image_index, 3);
        out[d + 3] = descs[i].level_index;
        out[d + 4] = descs[i].flags;
        put(d + 5, descs[i].orig_width, 2);
        put(d + 7, descs[i].orig_height, 2);
        put(d + 9, descs[i].num_blocks_x, 2);
        put(d + 11, descs[i].num_blocks_y, 2);
        put(d + 13, (uint32_t)ofs, 4);
        put(d + 17, (uint32_t)slice_bytes[i], 4);
        put(d + 21, bu_host::crc16(slice_data[i], slice_bytes[i], 0), 2);
        if (slice_bytes[i]) memcpy(out + ofs, slice_data[i], slice_bytes[i]);
        ofs += slice_bytes[i];
        if (descs[i].image_index + 1 > n_images) n_images = descs[i].image_index + 1;
    }
    put(0, 0x4273, 2);   // sig
    put(2, 0x13, 2);     // ver
    put(4, 77, 2);       // header_size
    put(8, (uint32_t)(total - 77), 4);
    put(12, bu_host::crc16(out + 77, total - 77, 0), 2);
    put(14, (uint32_t)n_slices, 3);
    put(17, n_images, 3);
    out[20] = 1;         // UASTC4x4
    put(21, header_flags, 2);
    out[23] = tex_type;
    put(65, 77, 4);      // slice_desc_file_ofs
    put(6, bu_host::crc16(out + 8, 77 - 8, 0), 2);
    return BU_OK;
}


}  // extern "C"
