// The ETC1S back-end kernels: codebook indices -> ETC1, RGBA32 and the six targets of bu_etc1s_targets.hpp, per slice, per file and per rectangle.
// The per-block code (index split and check, ETC1 block, palettes, RGBA32 block, target blocks) is bu_etc1s_targets.hpp's, which
// the CPU tests compile for the host; this header holds what only the device has: loads, codebook reads, stores and the status word.
// (Included by bu_hip.hip after bu_kernels.hpp: bu_report, bu_st_stream.)
#pragma once

namespace {

// blocks from which the LDS-staged kernels are launched, and the LDS one CU can give a workgroup (160 KiB less a margin)
constexpr size_t BU_ETC1S_STAGED_MIN = (size_t)1 << 19, BU_ETC1S_LDS_MAX = 152 * 1024;

// Both codebooks as a kernel reads them.  STAGED: the LDS copies s_ep / s_sel, one word per entry (s_sel holds the half of the
// selector entry the target reads); else the global codebooks, SEL_Y picking the entry's second word (ETC1) over its texel rows.
template <bool STAGED, bool SEL_Y = false>
struct BuEtc1sBooks {
    const uint32_t *s_ep, *s_sel, *endpoints;
    const uint2* selectors;
    __device__ __forceinline__ uint32_t endpoint(uint32_t e) const { return STAGED ? s_ep[e] : endpoints[e]; }
    __device__ __forceinline__ uint32_t selector(uint32_t s) const { return STAGED ? s_sel[s] : SEL_Y ? selectors[s].y : selectors[s].x; }
};

// Zeroes the block's output words o; an index out of range is reported in the status word and leaves them so.  True for a good block.
template <int W>
__device__ __forceinline__ bool bu_etc1s_good(const BuEtc1sIndex& k, unsigned long long* status, unsigned long long i, uint32_t (&o)[W])
{
#pragma unroll
    for (int j = 0; j < W; j++) o[j] = 0;
    if (k.bad) bu_report(status, i, BU_ERR_INDEX_RANGE);
    return !k.bad;
}

// the palette words and selector rows of a block with good indices (bu_etc1s_palettes; pal = the etc1s_pal table in LDS)
template <typename Books>
__device__ __forceinline__ void bu_etc1s_fetch(const Books& cb, const uint32_t* pal, const BuEtc1sIndex& k, bool has_a, uint32_t& pr, uint32_t& pg,
                                               uint32_t& pb, uint32_t& pa, uint32_t& rows, uint32_t& arows)
{
    const uint32_t ep = cb.endpoint(k.e);
    rows = cb.selector(k.s);
    uint32_t aep = 0;
    arows = 0;
    if (has_a) {
        aep = cb.endpoint(k.ae);
        arows = cb.selector(k.as);
    }
    bu_etc1s_palettes(pal, ep, aep, pr, pg, pb, pa);
}

// ETC1 of block i with the index word ix (basis_lz/mod.rs:163-181)
template <typename Books>
__device__ __forceinline__ uint2 bu_etc1s_etc1_lane(const Books& cb, uint32_t ix, uint32_t n_ep, uint32_t n_sel, unsigned long long* status, size_t i)
{
    const BuEtc1sIndex k = bu_etc1s_index(ix, false, 0u, n_ep, n_sel);
    uint32_t o[2];
    if (bu_etc1s_good(k, status, i, o)) bu_etc1s_etc1_block(cb.endpoint(k.e), cb.selector(k.s), o);
    return make_uint2(o[0], o[1]);
}

// RGBA32 of block i (basis_lz/mod.rs:122-146, + the alpha pass :139-143 fused), stored as its four rows of the image `img` of nbx
// blocks per row
template <typename Books, typename I>
__device__ __forceinline__ void bu_etc1s_rgba_lane(const Books& cb, const uint32_t* pal, const BuEtc1sIndex& k, bool has_a, unsigned long long* status,
                                                   I i, I nbx, uint4* img)
{
    uint32_t px[16];
    if (bu_etc1s_good(k, status, i, px)) {
        uint32_t pr, pg, pb, pa, rows, arows;
        bu_etc1s_fetch(cb, pal, k, has_a, pr, pg, pb, pa, rows, arows);
        bu_etc1s_block_rgba(pr, pg, pb, pa, rows, has_a, arows, px);
    }
    const I by = i / nbx, bx = i - by * nbx;
#pragma unroll
    for (int r = 0; r < 4; r++) bu_st_stream(img + (size_t)(4 * by + r) * nbx + bx, make_uint4(px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]));
}

// ---- small slices: the codebooks gathered through the L2 ------------------------------------------------------------------------
__global__ __launch_bounds__(BU_WG) void bu_etc1s_etc1_kernel(const uint32_t* __restrict__ idx, size_t n_blocks,
                                                              const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                              const uint2* __restrict__ selectors, uint32_t n_sel,
                                                              uint2* __restrict__ out, unsigned long long* status)
{
    const BuEtc1sBooks<false, true> cb = {nullptr, nullptr, endpoints, selectors};
    const size_t stride = (size_t)gridDim.x * BU_WG;
    for (size_t i = (size_t)blockIdx.x * BU_WG + threadIdx.x; i < n_blocks; i += stride) {
        const uint32_t ix = __builtin_nontemporal_load(idx + i);  // streamed once; the codebook gathers stay cached
        bu_st_stream(out + i, bu_etc1s_etc1_lane(cb, ix, n_ep, n_sel, status, i));
    }
}

__global__ __launch_bounds__(BU_WG) void bu_etc1s_rgba_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ aidx,
                                                              unsigned nbx, size_t n_blocks, const uint32_t* __restrict__ endpoints,
                                                              uint32_t n_ep, const uint2* __restrict__ selectors, uint32_t n_sel,
                                                              uint4* __restrict__ out, unsigned long long* status,
                                                              const BuTablesAll* __restrict__ tables)
{
    __shared__ uint32_t pal_lut[256];
    pal_lut[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
    static_assert(BU_WG == 256, "one palette word per thread");
    __syncthreads();
    const BuEtc1sBooks<false> cb = {nullptr, nullptr, endpoints, selectors};
    const size_t stride = (size_t)gridDim.x * BU_WG;
    for (size_t i = (size_t)blockIdx.x * BU_WG + threadIdx.x; i < n_blocks; i += stride) {
        const uint32_t ix = __builtin_nontemporal_load(idx + i);
        const uint32_t ax = aidx ? __builtin_nontemporal_load(aidx + i) : 0u;
        bu_etc1s_rgba_lane(cb, pal_lut, bu_etc1s_index(ix, aidx != nullptr, ax, n_ep, n_sel), aidx != nullptr, status, i, (size_t)nbx, out);
    }
}

// ---- large slices: both codebooks staged in LDS -------------------------------------------------------------------------------
// One persistent 1024-thread workgroup per CU (two where they fit) copies the endpoint codebook (4 B per entry) and the half of the
// selector codebook its target reads (4 B per entry: texel rows for RGBA32, ETC1 selector bytes for ETC1) into dynamic LDS and
// walks the slice with LDS lookups.  Against the L2 gather above (tools/exp/etc1s_sweep.py, 4096 + 8192 entries, cold rotation):
// 2^18 blocks 4.3 / 5.4 us against 4.3 / 5.0 (ETC1 / RGBA32: launch-bound either way), 2^20 6.7 / 16.0 against 10.3 / 23.3,
// 2^22 15.8 / 56.1 against 38.7 / 91.8, 2^24 41.6 / 218 against 147 / 366 us (ETC1 at 4.8 TB/s, RGBA32 at 5.2 TB/s): the gather
// is bound by the L2's random 4- and 8-byte reads, not by HBM.  The launcher takes this kernel from 2^19 blocks up.
template <bool RGBA>
__global__ __launch_bounds__(1024) void bu_etc1s_staged_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ aidx, unsigned nbx,
                                                               size_t n_blocks, const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                               const uint2* __restrict__ selectors, uint32_t n_sel, uint8_t* __restrict__ out,
                                                               unsigned long long* status, const BuTablesAll* __restrict__ tables)
{
    extern __shared__ uint32_t bu_etc1s_lds[];
    uint32_t* s_ep = bu_etc1s_lds;
    uint32_t* s_sel = bu_etc1s_lds + n_ep;
    uint32_t* pal_lut = s_sel + n_sel;
    const size_t stride = (size_t)gridDim.x * 1024, first = (size_t)blockIdx.x * 1024 + threadIdx.x;
    // ETC1, index array 8-byte and output 16-byte aligned: FOUR blocks per lane and step, a wave on 256 consecutive blocks -- the
    // lane's blocks 2L, 2L+1 and 128+2L, 128+2L+1, so that both of its 8-byte index loads and both of its 16-byte result stores
    // are contiguous across the wave (512 B / 1 KiB per instruction; four CONSECUTIVE blocks per lane make every store
    // instruction write half of each cache line: 2^22 blocks 16 -> 31 us) -- with the next step's indices already in flight.
    // The first loads are issued BEFORE the codebooks are staged, so their latency hides behind the staging.
    const bool vec4 = !RGBA && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const size_t n256 = vec4 ? n_blocks / 256 : 0, wstride = stride / 64, wfirst = first / 64;  // 256-block chunks; waves
    const uint2* idx2 = reinterpret_cast<const uint2*>(idx);
    const unsigned lane = threadIdx.x & 63u;
    bu_v2u curA = {0, 0}, curB = {0, 0};
    uint32_t cur = 0, acur = 0;
    if (vec4) {
        if (wfirst < n256) {
            curA = __builtin_nontemporal_load(reinterpret_cast<const bu_v2u*>(idx2 + wfirst * 128 + lane));
            curB = __builtin_nontemporal_load(reinterpret_cast<const bu_v2u*>(idx2 + wfirst * 128 + 64 + lane));
        }
    } else if (first < n_blocks) {
        cur = __builtin_nontemporal_load(idx + first);
        if (RGBA && aidx) acur = __builtin_nontemporal_load(aidx + first);
    }
    // staging, 16 bytes per load where the source allows (selectors: two 8-byte entries, of which the target keeps 4 bytes each)
    if ((reinterpret_cast<uintptr_t>(endpoints) & 15u) == 0) {
        for (uint32_t i = threadIdx.x; i < n_ep / 4; i += 1024) reinterpret_cast<uint4*>(s_ep)[i] = reinterpret_cast<const uint4*>(endpoints)[i];
        for (uint32_t i = (n_ep & ~3u) + threadIdx.x; i < n_ep; i += 1024) s_ep[i] = endpoints[i];
    } else {
        for (uint32_t i = threadIdx.x; i < n_ep; i += 1024) s_ep[i] = endpoints[i];
    }
    if ((reinterpret_cast<uintptr_t>(selectors) & 15u) == 0 && (n_ep & 1u) == 0) {
        for (uint32_t i = threadIdx.x; i < n_sel / 2; i += 1024) {
            const uint4 two = reinterpret_cast<const uint4*>(selectors)[i];
            reinterpret_cast<uint2*>(s_sel)[i] = RGBA ? make_uint2(two.x, two.z) : make_uint2(two.y, two.w);
        }
        if ((n_sel & 1u) && threadIdx.x == 0) s_sel[n_sel - 1] = RGBA ? selectors[n_sel - 1].x : selectors[n_sel - 1].y;
    } else {
        for (uint32_t i = threadIdx.x; i < n_sel; i += 1024) s_sel[i] = RGBA ? selectors[i].x : selectors[i].y;
    }
    if (RGBA && threadIdx.x < 256) pal_lut[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
    __syncthreads();
    const BuEtc1sBooks<true> cb = {s_ep, s_sel, nullptr, nullptr};
    auto etc1_block = [&](uint32_t ix, size_t i) { return bu_etc1s_etc1_lane(cb, ix, n_ep, n_sel, status, i); };
    if (vec4) {
        for (size_t w = wfirst; w < n256; w += wstride) {
            const size_t wn = w + wstride;
            bu_v2u nxtA = {0, 0}, nxtB = {0, 0};
            if (wn < n256) {
                nxtA = __builtin_nontemporal_load(reinterpret_cast<const bu_v2u*>(idx2 + wn * 128 + lane));
                nxtB = __builtin_nontemporal_load(reinterpret_cast<const bu_v2u*>(idx2 + wn * 128 + 64 + lane));
            }
            const size_t i0 = w * 256 + 2 * lane;
            const uint2 a = etc1_block(curA.x, i0), b = etc1_block(curA.y, i0 + 1), c = etc1_block(curB.x, i0 + 128), d = etc1_block(curB.y, i0 + 129);
            uint4* o4 = reinterpret_cast<uint4*>(out) + w * 128 + lane;
            bu_st_stream(o4, make_uint4(a.x, a.y, b.x, b.y));
            bu_st_stream(o4 + 64, make_uint4(c.x, c.y, d.x, d.y));
            curA = nxtA;
            curB = nxtB;
        }
        // the last n_blocks % 256 blocks
        const size_t t = 256 * n256 + first;
        if (t < n_blocks) bu_st_stream(reinterpret_cast<uint2*>(out) + t, etc1_block(__builtin_nontemporal_load(idx + t), t));
        return;
    }
    for (size_t i = first; i < n_blocks; i += stride) {
        const size_t in = i + stride;
        uint32_t nxt = 0, anxt = 0;
        if (in < n_blocks) {
            nxt = __builtin_nontemporal_load(idx + in);
            if (RGBA && aidx) anxt = __builtin_nontemporal_load(aidx + in);
        }
        if constexpr (!RGBA) bu_st_stream(reinterpret_cast<uint2*>(out) + i, etc1_block(cur, i));
        else
            bu_etc1s_rgba_lane(cb, pal_lut, bu_etc1s_index(cur, aidx != nullptr, acur, n_ep, n_sel), aidx != nullptr, status, i, (size_t)nbx,
                               reinterpret_cast<uint4*>(out));
        cur = nxt;
        acur = anxt;
    }
}

// ---- ETC1S -> BC1 / BC3 / BC4 / BC5 / EAC R11 / EAC RG11 (bu_etc1s_targets.hpp) ---------------------------
// One lane per block and step, grid-stride, the next step's indices in flight.  STAGED = false: the L2 gather of the kernels above,
// 256-thread workgroups, the palette table in LDS.  STAGED = true: one persistent 1024-thread workgroup per CU with both codebooks
// (endpoint words, selector rows) and the palette table in dynamic LDS, as bu_etc1s_staged_kernel<true> lays them out.  A wave's 64
// lanes hold 64 consecutive blocks, so each result store instruction writes 512 B (8-byte targets) or 1 KiB contiguous: whole cache
// lines for an output aligned to them.  Index errors report as the RGBA32 kernels do and leave a zero block.
template <int TARGET, bool STAGED>
__global__ __launch_bounds__(STAGED ? 1024 : BU_WG) void bu_etc1s_target_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ aidx,
                                                                                size_t n_blocks, const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                                                const uint2* __restrict__ selectors, uint32_t n_sel,
                                                                                void* __restrict__ out, unsigned long long* status,
                                                                                const BuTablesAll* __restrict__ tables)
{
    constexpr unsigned WGS = STAGED ? 1024u : (unsigned)BU_WG;
    extern __shared__ uint32_t bu_etc1s_tgt_lds[];
    __shared__ uint32_t s_pal_static[STAGED ? 1 : 256];
    uint32_t* s_ep = bu_etc1s_tgt_lds;
    uint32_t* s_sel = bu_etc1s_tgt_lds + n_ep;
    uint32_t* pal = STAGED ? s_sel + n_sel : s_pal_static;
    const size_t stride = (size_t)gridDim.x * WGS, first = (size_t)blockIdx.x * WGS + threadIdx.x;
    uint32_t cur = 0, acur = 0;
    if (first < n_blocks) {
        cur = __builtin_nontemporal_load(idx + first);
        if (aidx) acur = __builtin_nontemporal_load(aidx + first);
    }
    if constexpr (STAGED) {
        for (uint32_t i = threadIdx.x; i < n_ep; i += WGS) s_ep[i] = endpoints[i];
        for (uint32_t i = threadIdx.x; i < n_sel; i += WGS) s_sel[i] = selectors[i].x;
    }
    if (threadIdx.x < 256) pal[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
    __syncthreads();
    const BuEtc1sBooks<STAGED> cb = {s_ep, s_sel, endpoints, selectors};
    const BuTables& T = tables->t;  // (R11 / RG11: the EAC tables, read through the scalar cache in the table search)
    for (size_t i = first; i < n_blocks; i += stride) {
        const size_t in = i + stride;
        uint32_t nxt = 0, anxt = 0;
        if (in < n_blocks) {
            nxt = __builtin_nontemporal_load(idx + in);
            if (aidx) anxt = __builtin_nontemporal_load(aidx + in);
        }
        const BuEtc1sIndex k = bu_etc1s_index(cur, aidx != nullptr, acur, n_ep, n_sel);
        uint32_t o[4];
        if (bu_etc1s_good(k, status, i, o)) {
            uint32_t pr, pg, pb, pa, rows, arows;
            bu_etc1s_fetch(cb, pal, k, aidx != nullptr, pr, pg, pb, pa, rows, arows);
            bu_etc1s_target_block<TARGET>(T, pr, pg, pb, rows, aidx != nullptr, pa, arows, o);
        }
        if constexpr (bu_out_words(TARGET) == 2) bu_st_stream(reinterpret_cast<uint2*>(out) + i, make_uint2(o[0], o[1]));
        else bu_st_stream(reinterpret_cast<uint4*>(out) + i, make_uint4(o[0], o[1], o[2], o[3]));
        cur = nxt;
        acur = anxt;
    }
}

// ---- whole-file ETC1S launches (bu_read_to): every slice of the file in ONE launch -----------------------------------
// The host concatenates the per-slice index arrays (each padded to a multiple of 64 words) and describes the slices in a
// small table; a wave owns one 64-block unit, finds its slice by a scalar binary search over the units' prefix and then
// does exactly what the per-slice kernels do.  One status word per image, as the sequential drivers report.
// (BuEtc1sSlice, the table's entry, and bu_etc1s_unit_slice, the search, are bu_etc1s_targets.hpp's: the CPU tests compile them too.)
template <bool RGBA>
__global__ __launch_bounds__(BU_WG) void bu_etc1s_file_kernel(const uint32_t* __restrict__ idx, const BuEtc1sSlice* __restrict__ slices, uint32_t n_slices,
                                                              uint32_t unit_begin, uint32_t n_units, const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                              const uint2* __restrict__ selectors, uint32_t n_sel, uint8_t* __restrict__ out,
                                                              unsigned long long* status, const BuTablesAll* __restrict__ tables)
{
    __shared__ uint32_t pal_lut[RGBA ? 256 : 1];
    if constexpr (RGBA) {
        pal_lut[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
        __syncthreads();
    }
    const BuEtc1sBooks<false, !RGBA> cb = {nullptr, nullptr, endpoints, selectors};
    const uint32_t lane = threadIdx.x & 63u, wpg = BU_WG / 64;
    // units [unit_begin, n_units) of the file: the streamed front door launches the bands of a slice as their rows are decoded
    for (uint32_t unit = unit_begin + blockIdx.x * wpg + (threadIdx.x >> 6); unit < n_units; unit += gridDim.x * wpg) {
        // largest s with slices[s].unit0 <= unit (unit is wave-uniform: the search runs on the scalar unit)
        uint32_t lo = 0, hi = n_slices;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint32_t)__builtin_amdgcn_readfirstlane((int)slices[mid].unit0) <= unit) lo = mid;
            else hi = mid;
        }
        const BuEtc1sSlice sd = slices[lo];
        const uint32_t i = (unit - sd.unit0) * 64u + lane;
        if (i >= sd.n_blocks) continue;
        const uint32_t ix = __builtin_nontemporal_load(idx + sd.idx_ofs + i);
        if constexpr (!RGBA) {
            bu_st_stream(reinterpret_cast<uint2*>(out + sd.out_ofs) + i, bu_etc1s_etc1_lane(cb, ix, n_ep, n_sel, status + sd.image, i));
        } else {
            const bool has_a = sd.aidx_ofs != 0xFFFFFFFFu;
            const uint32_t ax = has_a ? __builtin_nontemporal_load(idx + sd.aidx_ofs + i) : 0u;
            bu_etc1s_rgba_lane(cb, pal_lut, bu_etc1s_index(ix, has_a, ax, n_ep, n_sel), has_a, status + sd.image, i, sd.nbx,
                               reinterpret_cast<uint4*>(out + sd.out_ofs));
        }
    }
}

// The six targets of bu_etc1s_targets.hpp over a whole file (bu_read_file_to): the structure of bu_etc1s_file_kernel<true> -- a wave
// per 64-block unit, the palette table in LDS, codebooks gathered through the L2 -- with bu_etc1s_target_kernel's block code and ONE
// result store per lane at out + out_ofs: a wave writes 512 B (8-byte targets) or 1 KiB contiguous.  The unit number is made scalar
// first, so the search of bu_etc1s_unit_slice and the descriptor are scalar loads.  A slice with aidx_ofs set has an alpha slice
// (A = 255 without one); its indices are checked whether TARGET reads A or not, as bu_etc1s_transcode does.
template <int TARGET>
__global__ __launch_bounds__(BU_WG) void bu_etc1s_file_target_kernel(const uint32_t* __restrict__ idx, const BuEtc1sSlice* __restrict__ slices,
                                                                     uint32_t n_slices, uint32_t unit_begin, uint32_t n_units,
                                                                     const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                                     const uint2* __restrict__ selectors, uint32_t n_sel, uint8_t* __restrict__ out,
                                                                     unsigned long long* status, const BuTablesAll* __restrict__ tables)
{
    __shared__ uint32_t pal_lut[256];
    pal_lut[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
    static_assert(BU_WG == 256, "one palette word per thread");
    __syncthreads();
    const BuEtc1sBooks<false> cb = {nullptr, nullptr, endpoints, selectors};
    const BuTables& T = tables->t;  // (R11 / RG11: the EAC tables, read through the scalar cache in the table search)
    const uint32_t lane = threadIdx.x & 63u, wpg = BU_WG / 64;
    for (uint32_t u = unit_begin + blockIdx.x * wpg + (threadIdx.x >> 6); u < n_units; u += gridDim.x * wpg) {
        const uint32_t unit = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
        const BuEtc1sSlice sd = slices[bu_etc1s_unit_slice(slices, n_slices, unit)];
        const uint32_t i = (unit - sd.unit0) * 64u + lane;
        if (i >= sd.n_blocks) continue;
        const bool has_a = sd.aidx_ofs != 0xFFFFFFFFu;
        const uint32_t ix = __builtin_nontemporal_load(idx + sd.idx_ofs + i);
        const uint32_t ax = has_a ? __builtin_nontemporal_load(idx + sd.aidx_ofs + i) : 0u;
        const BuEtc1sIndex k = bu_etc1s_index(ix, has_a, ax, n_ep, n_sel);
        uint32_t o[4];
        if (bu_etc1s_good(k, status + sd.image, i, o)) {
            uint32_t pr, pg, pb, pa, rows, arows;
            bu_etc1s_fetch(cb, pal_lut, k, has_a, pr, pg, pb, pa, rows, arows);
            bu_etc1s_target_block<TARGET>(T, pr, pg, pb, rows, has_a, pa, arows, o);
        }
        if constexpr (bu_out_words(TARGET) == 2) bu_st_stream(reinterpret_cast<uint2*>(out + sd.out_ofs) + i, make_uint2(o[0], o[1]));
        else bu_st_stream(reinterpret_cast<uint4*>(out + sd.out_ofs) + i, make_uint4(o[0], o[1], o[2], o[3]));
    }
}

// ---- rectangles of slices into pitched surfaces (bu_etc1s_transcode_rects_device; table, units and address mapping: bu_etc1s_rect_plan.hpp) -------------
// TARGET: BU_TGT_ETC1, BU_TGT_RGBA or one of the six.  The structure of bu_etc1s_file_target_kernel -- a wave per 64-block unit, the unit number made scalar
// first, the palette table in LDS (ETC1 needs none), codebooks gathered through the L2, nontemporal index loads -- over the units of the jobs of `table`, a
// kernel argument: the search for a unit's job and its descriptor are scalar loads from the argument segment.  A lane holds the block of its row and column of
// the unit (clipped lanes sit out) and stores it at the job's pitch: one store, RGBA32 four.  Every address is rebuilt from the table's integers, so the index
// loads name the global address space themselves (bu_st_stream does); a job with an alpha slice has its indices checked whether TARGET reads A or not.
typedef const uint32_t __attribute__((address_space(1))) * bu_global_u32;
template <int TARGET>
__global__ __launch_bounds__(BU_WG) void bu_etc1s_rects_kernel(const BuEtc1sRectTable table, uint32_t n_units, const uint32_t* __restrict__ endpoints, uint32_t n_ep,
                                                               const uint2* __restrict__ selectors, uint32_t n_sel, unsigned long long* status,
                                                               const BuTablesAll* __restrict__ tables)
{
    static_assert(sizeof(BuEtc1sRectTable) + 4 + 4 + 8 + 4 + 4 + 8 + 8 + 8 <= 4096 && BU_ETC1S_RECTS_OTHER_ARGS == 48,
                  "the job table and the other arguments share the 4 KiB of kernel arguments");
    constexpr bool ETC1 = TARGET == BU_TGT_ETC1, RGBA = TARGET == BU_TGT_RGBA;
    constexpr uint32_t ROW_BYTES = bu_rect_row_bytes(TARGET), ROWS = bu_rect_rows_per_block(TARGET);
    __shared__ uint32_t pal_lut[ETC1 ? 1 : 256];
    if constexpr (!ETC1) {
        pal_lut[threadIdx.x] = tables->t.etc1s_pal[threadIdx.x];
        static_assert(BU_WG == 256, "one palette word per thread");
        __syncthreads();
    }
    const BuEtc1sBooks<false, ETC1> cb = {nullptr, nullptr, endpoints, selectors};
    const uint32_t lane = threadIdx.x & 63u, wpg = BU_WG / 64;
    for (uint32_t uv = blockIdx.x * wpg + (threadIdx.x >> 6); uv < n_units; uv += gridDim.x * wpg) {
        const uint32_t unit = (uint32_t)__builtin_amdgcn_readfirstlane((int)uv);
        const uint32_t r = bu_etc1s_rect_unit_job(table.first_unit, unit);
        const BuEtc1sRectUnit u = bu_etc1s_rect_unit(table.job[r], unit - table.first_unit[r], ROW_BYTES, ROWS);
        if (!bu_etc1s_rect_has(u, lane)) continue;
        const uint32_t off = bu_etc1s_rect_idx(u, lane);
        const unsigned long long i = u.base + off;
        const uint64_t dst = bu_etc1s_rect_dst(u, lane, ROW_BYTES, ROWS);
        const uint32_t ix = __builtin_nontemporal_load((bu_global_u32)u.idx + off);
        if constexpr (ETC1) {
            bu_st_stream(reinterpret_cast<uint2*>(dst), bu_etc1s_etc1_lane(cb, ix, n_ep, n_sel, status, i));
        } else {
            const bool has_a = u.aidx != 0;
            const uint32_t ax = has_a ? __builtin_nontemporal_load((bu_global_u32)u.aidx + off) : 0u;
            const BuEtc1sIndex k = bu_etc1s_index(ix, has_a, ax, n_ep, n_sel);
            uint32_t o[RGBA ? 16 : 4];
            if (bu_etc1s_good(k, status, i, o)) {
                uint32_t pr, pg, pb, pa, rows, arows;
                bu_etc1s_fetch(cb, pal_lut, k, has_a, pr, pg, pb, pa, rows, arows);
                if constexpr (RGBA) bu_etc1s_block_rgba(pr, pg, pb, pa, rows, has_a, arows, o);
                else bu_etc1s_target_block<TARGET>(tables->t, pr, pg, pb, rows, has_a, pa, arows, o);
            }
            if constexpr (RGBA) {
#pragma unroll
                for (int y = 0; y < 4; y++)
                    bu_st_stream(reinterpret_cast<uint4*>(dst + (uint64_t)y * u.pitch), make_uint4(o[4 * y], o[4 * y + 1], o[4 * y + 2], o[4 * y + 3]));
            } else {
                if constexpr (bu_out_words(TARGET) == 2) bu_st_stream(reinterpret_cast<uint2*>(dst), make_uint2(o[0], o[1]));
                else bu_st_stream(reinterpret_cast<uint4*>(dst), make_uint4(o[0], o[1], o[2], o[3]));
            }
        }
    }
}

}  // namespace
