// gfx950 kernels of the block-transcode path: the one-lane-per-block kernel, the mode-sorted kernel (every UASTC target), the
// status-word reset, the CRC, sleep and copy kernels (the ETC1S codebook-lookup kernels: bu_etc1s_kernels.hpp).
// Part of the single translation unit bu_hip.hip (included there; not a stand-alone header).
#pragma once
namespace {

// (BU_WG, BU_SORT_MIN_BLOCKS, bu_dyn_tile, BU_RECT_W, BU_MULTI_RUNS, BU_RUN_STRIPS: bu_launch_plan.hpp)
// ------------------------------------------------------------------------------------------------
// LDS image of the tables of TARGET: [BuBc7Tables (BC7 only)][BuTables up to the end of the target's ranges]
constexpr unsigned bu_lds_front(int target) { return target == 1 ? (unsigned)sizeof(BuBc7Tables) : 0u; }
constexpr unsigned bu_lds_table_bytes(int target) { return bu_lds_front(target) + bu_table_bytes(target); }
// stage the parts of the table blob TARGET reads (bu_table_range; BC7: its own tables in front), 16 bytes per thread per step
template <int WGS, int TARGET>
__device__ __forceinline__ void bu_stage_tables_n(uint4* dst, const BuTablesAll* __restrict__ src)
{
    constexpr BuTableRange R = bu_table_range(TARGET);
    constexpr int F = (int)bu_lds_front(TARGET) / 16;
    // (for BC7 the image is the blob from its first byte; for the others it starts at BuTablesAll::t)
    const uint4* s = reinterpret_cast<const uint4*>(TARGET == 1 ? reinterpret_cast<const void*>(src) : reinterpret_cast<const void*>(&src->t));
    uint4* d = dst;
    for (int i = threadIdx.x; i < F + (int)(R.hi / 16); i += WGS)
        if (i < F || i >= F + (int)(R.lo / 16)) d[i] = s[i];
    if constexpr (R.lo2 < R.hi2) {
        for (int i = F + R.lo2 / 16 + threadIdx.x; i < F + (int)(R.hi2 / 16); i += WGS) d[i] = s[i];
    }
}

// System scope: the status word may live in page-locked HOST memory (the blocking entry points hand the kernels a word the host reads
// directly once the streams are idle: no reset launch in front, no copy behind -- bu_range_begin); for a word in device memory the
// scope changes nothing.  Only a failing block ever gets here.
__device__ __forceinline__ void bu_report(unsigned long long* status, unsigned long long block, int st)
{
    if (status) (void)__hip_atomic_fetch_min(status, (block << 8) | (unsigned long long)st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Every block is read once and every result written once: non-temporal (streaming) accesses keep the 32 MiB of a 4096^2
// atlas from being allocated in L2 / Infinity Cache with normal retention.  Measured on the BC7 headline: 14.4 -> 13.7 us.
typedef unsigned int bu_v4u __attribute__((ext_vector_type(4)));
typedef unsigned int bu_v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 bu_ld_stream(const uint4* p)
{
    const bu_v4u r = __builtin_nontemporal_load(reinterpret_cast<const bu_v4u*>(p));
    return make_uint4(r.x, r.y, r.z, r.w);
}
// The same load through a pointer to the GLOBAL address space.  The multi-run layouts rebuild a run's addresses from integers (the run record comes out of
// LDS), and a load through such a pointer is a flat_load: a 64-bit vector address, counted on lgkmcnt as well as vmcnt, so that no counted wait is possible
// while one is pending.  Every run lies in device memory (hipMalloc'ed or mapped host memory: global either way), so the load may say so.
__device__ __forceinline__ uint4 bu_ld_stream_global(const uint4* p)
{
    typedef const bu_v4u __attribute__((address_space(1))) * bu_global_v4u;
    const bu_v4u r = __builtin_nontemporal_load((bu_global_v4u)p);
    return make_uint4(r.x, r.y, r.z, r.w);
}
// The scalar-base form (bu_multi_addr.hpp): a wave-uniform 64-bit address plus a 32-bit byte offset per lane.  Written as a byte pointer into the global address
// space indexed by an unsigned 32-bit value, it compiles to  global_load_dwordx4 v[..], v_off, s[b:b+1] nt  -- no 64-bit vector arithmetic in front of the access.
typedef const char __attribute__((address_space(1))) * bu_global_bytes;
__device__ __forceinline__ uint4 bu_ld_stream_global(uint64_t base, uint32_t off)
{
    typedef const bu_v4u __attribute__((address_space(1))) * bu_global_v4u;
    const bu_v4u r = __builtin_nontemporal_load((bu_global_v4u)((bu_global_bytes)base + off));
    return make_uint4(r.x, r.y, r.z, r.w);
}
// (the compiler's own stores below say "global" for the same reason: every output lies in device memory, and in the multi-run kernels nothing else says so)
typedef bu_v4u __attribute__((address_space(1))) * bu_global_out_v4u;
typedef bu_v2u __attribute__((address_space(1))) * bu_global_out_v2u;
// Output stores.  BU_ST_MODE selects the cache policy (experiment knob).  A/B inside one run (tools/exp/ab.sh), 2^20 blocks:
//   0 nontemporal (nt)            copy 7.15  BC7 10.93  ETC1 25.1  RGBA32 21.2 us
//   1 plain                            7.07      12.70       25.9         23.1     (results linger dirty in L2)
//   2 write-through (sc1)              7.16      10.88       24.9         20.6
//   3 sc0 sc1                          7.13      10.86       24.8         20.7
//   4 sc1 nt  <- shipped               6.99      10.70       24.75        20.6
#ifndef BU_ST_MODE
#define BU_ST_MODE 4
#endif
#if BU_ST_MODE == 2
#define BU_ST_BITS " sc1"
#elif BU_ST_MODE == 3
#define BU_ST_BITS " sc0 sc1"
#elif BU_ST_MODE == 4
#define BU_ST_BITS " sc1 nt"
#endif
__device__ __forceinline__ void bu_st_stream(uint4* p, const uint4 v)
{
    bu_v4u r;
    r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
#if BU_ST_MODE == 0
    __builtin_nontemporal_store(r, (bu_global_out_v4u)p);
#elif BU_ST_MODE == 1
    *(bu_global_out_v4u)p = r;
#else
    // hipcc does not model an asm store: the s_nop 1 keeps its next instruction from overwriting the data registers before
    // the store has read them (two wait states behind a store of more than 8 bytes on gfx940+)
    asm volatile("global_store_dwordx4 %0, %1, off" BU_ST_BITS "\n\ts_nop 1" ::"v"(p), "v"(r) : "memory");
#endif
}
__device__ __forceinline__ void bu_st_stream(uint2* p, const uint2 v)
{
    bu_v2u r;
    r.x = v.x; r.y = v.y;
    // 8-byte stores stay nontemporal: an sc1 store narrower than 16 bytes is one fabric write per lane
    // (ETC1S -> ETC1 at 2^18 blocks: 4.7 -> 6.2 us with sc1 nt)
#if BU_ST_MODE == 1
    *(bu_global_out_v2u)p = r;
#else
    __builtin_nontemporal_store(r, (bu_global_out_v2u)p);
#endif
}
// The same two stores in the scalar-base form of the multi-run layouts: wave-uniform base, 32-bit byte offset per lane; each in its own cache policy.
typedef char __attribute__((address_space(1))) * bu_global_out_bytes;
__device__ __forceinline__ void bu_st_stream(uint64_t base, uint32_t off, const uint4 v)
{
    bu_v4u r;
    r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
#if BU_ST_MODE == 0
    __builtin_nontemporal_store(r, (bu_global_out_v4u)((bu_global_out_bytes)base + off));
#elif BU_ST_MODE == 1
    *(bu_global_out_v4u)((bu_global_out_bytes)base + off) = r;
#else
    asm volatile("global_store_dwordx4 %0, %1, %2" BU_ST_BITS "\n\ts_nop 1" ::"v"(off), "v"(r), "s"(base) : "memory");  // (the s_nop: as above)
#endif
}
__device__ __forceinline__ void bu_st_stream(uint64_t base, uint32_t off, const uint2 v)
{
    bu_v2u r;
    r.x = v.x; r.y = v.y;
#if BU_ST_MODE == 1
    *(bu_global_out_v2u)((bu_global_out_bytes)base + off) = r;
#else
    __builtin_nontemporal_store(r, (bu_global_out_v2u)((bu_global_out_bytes)base + off));
#endif
}

// UASTC -> {ASTC, BC7, ETC1, ETC2, RGBA32, BC4, BC5, EAC R11, EAC RG11}: replaces the loop of uastc.rs:157-165 / 96-107
template <int TARGET>
__global__ __launch_bounds__(BU_WG) void bu_uastc_kernel(const uint4* __restrict__ in, void* __restrict__ out, size_t n_blocks,
                                                         unsigned bpr, unsigned long long base, unsigned long long* status,
                                                         const BuTablesAll* __restrict__ tables)
{
    __shared__ uint4 t_store[bu_lds_table_bytes(TARGET) / 16];  // the blob as far as TARGET reads it (BC7: its own tables in front)
    BuTables& T = *reinterpret_cast<BuTables*>(t_store + bu_lds_front(TARGET) / 16);
    const size_t stride = (size_t)gridDim.x * BU_WG;
    size_t idx = (size_t)blockIdx.x * BU_WG + threadIdx.x;
    // first block load is issued before the table copy so both are in flight together
    uint4 v = idx < n_blocks ? bu_ld_stream(in + idx) : make_uint4(0, 0, 0, 0);
    bu_stage_tables_n<BU_WG, TARGET>(t_store, tables);
    __syncthreads();
    while (idx < n_blocks) {
        const size_t next = idx + stride;
        const uint4 vn = next < n_blocks ? in[next] : make_uint4(0, 0, 0, 0);
        BuBlk b;
        b.w[0] = v.x;
        b.w[1] = v.y;
        b.w[2] = v.z;
        b.w[3] = v.w;
        const uint32_t mode = T.mode_lut[v.x & 127u];
        uint32_t o[TARGET == BU_TGT_RGBA ? 16 : 4];
#pragma unroll
        for (int i = 0; i < (TARGET == BU_TGT_RGBA ? 16 : 4); i++) o[i] = 0;
        const int st = bu_block_any<TARGET>(T, mode, b, o);
        if (st) {
            bu_report(status, base + idx, st);
#pragma unroll
            for (int i = 0; i < (TARGET == BU_TGT_RGBA ? 16 : 4); i++) o[i] = 0;
        }
        if constexpr (bu_out_words(TARGET) == 2) {  // ETC1, BC4, EAC R11
            reinterpret_cast<uint2*>(out)[idx] = make_uint2(o[0], o[1]);
        } else if constexpr (TARGET == BU_TGT_RGBA) {
            const size_t by = idx / bpr, bx = idx - by * bpr;
            uint4* img = reinterpret_cast<uint4*>(out);
#pragma unroll
            for (int r = 0; r < 4; r++) img[(4 * by + r) * (size_t)bpr + bx] = make_uint4(o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]);
        } else {
            reinterpret_cast<uint4*>(out)[idx] = make_uint4(o[0], o[1], o[2], o[3]);
        }
        v = vn;
        idx = next;
    }
}

// ------------------------------------------------------------------------------------------------
// Mode-sorted kernel (every target; RGBA32 returns its 64 B per block through an LDS row tile).
//
// The per-mode code paths are straight-line and short (100-260 VALU each for BC7) but there are 19 of
// them: a wave whose 64 lanes hold a random mix of modes executes all 19 serially (measured: 69 us
// per 4096x4096 atlas vs a 7 us copy).  So each workgroup first sorts its tile of BU_TILE blocks by
// mode through LDS (counting sort: one LDS atomic per block), cuts every mode's run into chunks of
// <= 64 blocks, and each wave then transcodes whole chunks with a wave-uniform mode (scalar branch,
// no exec-mask divergence).  Results go back to LDS at the sorted slot and leave in original order,
// so global loads and stores stay fully coalesced (1 KiB per wave instruction).
//   LDS per workgroup: tile 16 B x BU_TILE + the target's tables + (ETC, RGBA32) 1 B x BU_TILE status + counters.
// Environment knobs read by the host code (diagnostics, not configuration): BU_TRACE (phase times of bu_read_to on stderr, and
// for the streamed ETC1S front door when every work item started and ended), BU_RUN_PIECE_MIB (piece size of the two-stream upload
// pipeline, 0 = off), BU_ETC1S_ONE_LAUNCH (ETC1S files: decode everything, then one launch -- the round-3 path),
// BU_ETC1S_ONE_THREAD (streamed ETC1S front door: every slice's symbol loop on one thread); round 6: BU_STREAM_MODE=plain | cumask (how the context's own
// streams are created: never / always with CU masks instead of by the hardware-queue check, bu_streams.hpp), BU_ENQUEUE_THREADS=0 (the pipelined batch call
// enqueues from the calling thread alone), BU_TILE_TICKETS=0 (every persistent launch walks fixed shares of the tiles).
// inclusive add-scan over lanes 0..31 (and 32..63) with DPP row shifts: 5 VALU, no LDS round trips
__device__ __forceinline__ uint32_t bu_scan32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1 and 3
    return v;
}

// RECT: a tile is a BU_RECT_W x (tile / BU_RECT_W) RECTANGLE of the block grid (64 x 16 for the 1024-block tiles) instead of a strip
// of consecutive blocks (the launcher picks it when blocks_per_row is a multiple of 64 and the slice is whole rows of such tiles,
// bu_launch_uastc).  Texture content is coherent in two dimensions: a 1024-block strip of a 4096-px-wide image cuts an 8 x 8-block
// region of one UASTC mode into eight runs of eight, a rectangle keeps it whole -- fewer, fuller runs per tile, fewer partly
// filled chunks (mode-coherent atlas: BC7 -5...-10 %).  64 blocks wide: a wave's load / store instruction is still one contiguous
// KiB (32-wide tiles, two 512-byte segments per instruction, cost the uniform-random atlas +3 % on BC7).  Nothing else changes (the
// sort works on the index inside the tile).  A compile-time variant: as a run-time switch the extra index arithmetic cost the
// strip path 4 % (round 2).  BU_RECT_W = 64.
// MULTI (LAYOUT 2): the launch covers SEVERAL runs of blocks at unrelated addresses (slices of a texture array in separate
// allocations); tiles never straddle runs.  The run table travels IN THE KERNEL ARGUMENTS (bu_uastc_multi_kernel: no device
// buffer, no copy, nothing to free behind the launch): per run its input, output, block-index base, size and the number of its
// first tile.  A workgroup finds the run of tile t by comparing t with 64 first-tile numbers at a time (one vector load and a
// ballot per wave) and reads that run's record with scalar loads.  A loop over small slices becomes one launch
// (bu_uastc_transcode_batch_device); more than BU_MULTI_RUNS runs go out as several launches.
struct BuRunDesc {
    const uint4* in;  // the run's first block
    void* out;        // its output
    uint64_t base;    // block-index base of the run (status words)
    uint32_t n;       // blocks in the run
    uint32_t vshift;  // BU_RUN_STRIPS: tiles are strips of 1024 consecutive blocks; else the run is whole 64 x 16-block rectangles of a (virtual) grid
                      // 64 << vshift blocks wide (bu_launch_runs: a power of two, the run a multiple of 16 rows of it)
};
struct BuRunTable {
    BuRunDesc run[BU_MULTI_RUNS];
    uint32_t first_tile[BU_MULTI_RUNS + 32];  // ascending; entries past the last run hold 0xFFFFFFFF (128 entries: two 64-lane loads)
};
static_assert(sizeof(BuRunDesc) == 32 && sizeof(BuRunTable) <= 3968, "the run table must fit the 4 KiB of kernel arguments beside the other parameters");
// What a workgroup carries from tile to tile beside the blocks: `d` describes the tile being sorted, transcoded and written back, `l` the tile whose blocks are being
// LOADED (the same tile, or with PREFETCH the next one: its loads are in flight while `d`'s tile is transcoded).
//   one slice (STRIP, RECT): nothing.  A tile is its number and every address hangs on the launch's `in` / `out` / `base`, so these kernels carry nothing of the other
//     layouts' and compile to what they were
//   RECTS: BuRectTile, the tile's corner in its job's slice and surface (bu_rect_plan.hpp)
//   MULTI: BuMultiTile -- the tile, the run being walked and every address derived from them (bu_multi_addr.hpp) -- and beside the two tiles
//     off: the 32-bit byte offsets of this thread's BPT blocks from the corner of `l`.  They hang on the thread and the run's width alone and are computed anew only
//       where the walk reaches a run of another width (`off_width`: the width they were computed for) -- never per tile, never per access.  `d` uses the same ones
//       for its stores, except in the one tile per change of width in which `l` is already in the next run (bu_uastc_sorted_body, `so`)
//     cur: the run of the tile last looked up, in uniform registers.  The next tile lies in the same run nearly every time (a 2^20-block run is 1024 tiles): its
//       descriptor is then scalar arithmetic on `cur`, with no LDS read, no ballot and no readfirstlane between the scatter and the prefetch loads
struct BuNoTile {};
template <class TILE>
struct BuWalk {
    TILE d = {}, l = {};
};
template <int BPT>
struct BuMultiWalk : BuWalk<BuMultiTile> {
    uint32_t off[BPT] = {};
    uint32_t off_width = 0xFFFFFFFFu;  // (no run has this width)
    BuRunCursor cur = bu_no_run();
};
enum { BU_LAYOUT_STRIP = 0, BU_LAYOUT_RECT = 1, BU_LAYOUT_MULTI = 2,
       BU_LAYOUT_MULTI_WHOLE = 3,    // MULTI with every run tiled as whole rectangles (BuRunDesc::vshift): no lane ever lacks a block, and the validity tests fold away as in RECT
       BU_LAYOUT_RECTS = 4 };        // several RECTANGLES cut out of slices, each stored at a pitch of its own (bu_uastc_rects_kernel below; table and address mapping: bu_rect_plan.hpp)
// one set of tile tickets (kernel, `ticket`): eight counters BU_TICKET_STRIDE words apart, then the count of workgroups that have left
constexpr unsigned BU_TICKET_STRIDE = 32, BU_TICKET_DONE = 8 * BU_TICKET_STRIDE, BU_TICKET_WORDS = 9 * BU_TICKET_STRIDE;
// WGS threads per workgroup, BPT blocks per thread: tile = WGS * BPT blocks.  PREFETCH: a workgroup that walks several tiles
// loads tile k+1 while it transcodes tile k (BPT more uint4 registers).
template <int TARGET, int WGS, int BPT, bool PREFETCH, int LAYOUT>
__device__ __forceinline__ void bu_uastc_sorted_body(const uint4* __restrict__ in, void* __restrict__ out, unsigned n_blocks,
                                                     unsigned bpr, unsigned long long base, unsigned long long* status,
                                                     const BuTablesAll* __restrict__ tables, unsigned cus, unsigned tile_rt,
                                                     const BuRunTable* __restrict__ runs, unsigned* __restrict__ ticket = nullptr,
                                                     const BuRectTable* __restrict__ rects = nullptr)
{
    // Static priority by residency generation.  Workgroups are dealt breadth-first (b, b + CUs, b + 2 CUs, ... share a CU:
    // tools/exp/census.hip), and the instruction arbiter serves the OLDEST wave first, so the four tiles of a CU finish
    // 1.5 us apart and the last one runs its latency-bound chain with the vector units nearly idle (phase stamps,
    // profiles/r02_*stamps*).  Raising the later generations' priority makes them catch up while the older ones fill
    // the gaps: BC7 10.51 -> 10.2 us, ASTC 9.74 -> 9.47, RGBA32 20.4 -> 19.95 in an A/B run.  Speed only: any placement is correct.
    // cus = 0 switches it off: RGBA32 launches in which the workgroups do not all walk the same number of tiles (786 432
    // blocks: the one-tile workgroups of the second generation would run ahead of the two-tile ones, 15.75 against 14.24 us).
    // Round 3, on the leaner kernels: generation priorities 0, 3, 2, 1 beat 0, 1, 2, 3 for BC7 (9.13 -> 8.96 us) and ASTC (9.0 -> 8.8),
    // not for RGBA32 (15.85 -> 16.0); no priorities 9.14 / 9.04 / 17.4 (profiles/r03_ab_wave_priorities.txt).
    if (cus != 0) {  // (comparisons, not blockIdx / cus: a scalar division is ~25 instructions in front of the first load)
        constexpr bool ROT = TARGET == BU_TGT_BC7 || TARGET == BU_TGT_ASTC;
        if (blockIdx.x >= 3 * cus) __builtin_amdgcn_s_setprio(ROT ? 1 : 3);
        else if (blockIdx.x >= 2 * cus) __builtin_amdgcn_s_setprio(2);
        else if (blockIdx.x >= cus) __builtin_amdgcn_s_setprio(ROT ? 3 : 1);
    }
    constexpr int BU_WG = WGS, BU_BPT = BPT, BU_TILE = WGS * BPT;
    __shared__ uint4 t_store[bu_lds_table_bytes(TARGET) / 16];  // the blob as far as TARGET reads it (BC7: its own tables in front)
    BuTables& T = *reinterpret_cast<BuTables*>(t_store + bu_lds_front(TARGET) / 16);
    // RGBA32 through LDS: four pixel rows of 16 B per block, stored row-major by row index so that both the
    // sorted-order writes and the original-order reads are 16-byte strided (no bank conflicts).  The sorted input tile
    // lives IN row 0 of that output tile: a lane reads its block from slot s and later overwrites exactly slot s with
    // the block's first pixel row, so no other lane's input is ever clobbered -- 64 KiB instead of 80 per 1024 blocks,
    // which is what lets two workgroups share a CU.
    constexpr bool RECT = LAYOUT == BU_LAYOUT_RECT, MULTI = LAYOUT == BU_LAYOUT_MULTI || LAYOUT == BU_LAYOUT_MULTI_WHOLE;
    constexpr bool WHOLE = RECT || LAYOUT == BU_LAYOUT_MULTI_WHOLE;  // every tile of the launch holds BU_TILE blocks
    // RECTS: the tiles of several rectangles (a table in the kernel arguments, as MULTI's), each 2^tshift x (BU_TILE >> tshift) blocks of its rectangle, clipped at the
    // rectangle's right and bottom edge, loaded at the slice's pitch and stored at the output's.  Only where a block comes from, whether a lane has one and where its
    // result goes differ from the other layouts; the sort, the chunk phase and the block code do not know.
    constexpr bool RECTS = LAYOUT == BU_LAYOUT_RECTS;
    static_assert(!RECTS || (BU_TILE == (int)BU_RECTS_TILE && PREFETCH), "the host numbers 1024-block tiles of rectangles; one compiled shape");
    constexpr uint32_t RECTS_ROW_BYTES = bu_rect_row_bytes(TARGET), RECTS_ROWS = bu_rect_rows_per_block(TARGET);
    constexpr bool BU_ALIAS = TARGET == BU_TGT_RGBA;
    // two RGBA32 workgroups must fit the 160 KiB of a CU: output tile + table blob + status bytes + counters / chunk list
    static_assert(!BU_ALIAS || bu_lds_table_bytes(TARGET) + 4 * BU_TILE * 16 + BU_TILE + 1536 <= 80 * 1024,
                  "the RGBA32 workgroup no longer fits twice per CU: shrink BuTables or stage it per target in LDS too");
    __shared__ uint4 sblk_store[BU_ALIAS ? 1 : BU_TILE];
    __shared__ uint4 sout[BU_ALIAS ? 4 * BU_TILE : 1];
    uint4* const sblk = BU_ALIAS ? sout : sblk_store;
    // BC7 and ASTC carry a failing block's status inside its result slot (a valid block of either format has a non-zero first
    // byte: BC7's unary mode prefix, ASTC's block mode / void-extent marker), the other targets in a byte per block
    constexpr bool INBLOCK = TARGET == BU_TGT_BC7 || TARGET == BU_TGT_ASTC;
    __shared__ uint8_t sst[INBLOCK ? 16 : BU_TILE];
    // counters and the chunk ticket are double-buffered by tile parity: the buffer of tile t+1 is cleared during tile t,
    // after everyone has finished with its previous use (tile t-1), so no barrier is spent on the reset
    __shared__ uint32_t cnt[2][32], next_chunk[2];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    // Blocks per tile.  The exclusive ETC shape is one workgroup per CU on tiles of up to 4096 blocks; with a fixed tile a slice of
    // 1.5 tiles per CU takes as long as one of 2 (1.5 Mi blocks 33.4 us, 2 Mi 34.2).  There the launcher sizes the tile so
    // that every CU gets the same number of equal tiles (`tile_rt` <= BU_TILE, a multiple of 64); threads past the end of
    // a shorter tile sit out like threads past the end of the slice.  Every other shape passes tile_rt = BU_TILE and
    // compiles to what it was.
    constexpr bool DYN_TILE = bu_dyn_tile(TARGET, BU_TILE) && LAYOUT != BU_LAYOUT_RECT;
    const unsigned tile_blocks = DYN_TILE ? tile_rt : (unsigned)BU_TILE;
    const unsigned n_tiles = (n_blocks + tile_blocks - 1) / tile_blocks;  // 32-bit indices: the host splits launches above 2^26 blocks
    auto in_tile = [&](unsigned l) { return !DYN_TILE || l < tile_blocks; };
    static_assert(!RECT || BU_TILE % BU_RECT_W == 0, "rectangular tiles are BU_RECT_W blocks wide and of fixed size");
    // slice index of block l of tile t.  RECT: `tile_rt` carries ceil(2^32 / tiles per row) + 0 (bu_launch_uastc), which makes
    // t / tpr one s_mul_hi_u32 (exact for t, tpr < 2^16: at most 2^26 blocks per launch, rows below 2^21 blocks)
    const unsigned tpr = RECT ? bpr / BU_RECT_W : 1u;  // tiles per row of tiles
    auto tile_xy = [&](unsigned t, unsigned& ty, unsigned& tx) {
        ty = (unsigned)(((unsigned long long)t * tile_rt) >> 32);
        tx = t - ty * tpr;
    };
    auto gidx = [&](unsigned t, unsigned l) {
        if constexpr (RECT) {
            unsigned ty, tx;
            tile_xy(t, ty, tx);  // (wave-uniform: scalar)
            return ((unsigned)(BU_TILE / BU_RECT_W) * ty + l / BU_RECT_W) * bpr + BU_RECT_W * tx + (l % BU_RECT_W);
        } else {
            return t * tile_blocks + l;
        }
    };
    // RECT launches hold whole tiles only: every lane of every tile has a block (keys are 0..19, never the "no block" 31), and the
    // validity tests below fold away
    auto has_block = [&](uint32_t k) { return WHOLE || k < 20u; };
    unsigned tile = blockIdx.x;
    // Tile tickets (`ticket` != nullptr): a persistent workgroup's FIRST tile is its block index; every further tile is the next number off a
    // counter in device memory instead of tile + gridDim.x -- workgroups that run ahead (a cheaper mode mix, a luckier HBM channel, a CU they
    // share with fewer others) take more tiles, and the launch ends when the tiles do, not when the slowest fixed share does.
    // EIGHT counters, 128 bytes apart, workgroup b draws from counter b % 8 and its k-th ticket is tile gridDim.x + 8 k + b % 8 (every tile >=
    // gridDim.x exactly once): a device-scope atomic on one address completes once per ~12 ns on this chip (eight XCDs, one coherence point:
    // one counter for a 2^25-block launch = 32 768 tickets = 390 us, profiles/r06_ab_tile_tickets.txt), eight counters are not a bottleneck.
    // Thread 0 draws the ticket one whole tile ahead of its use (the atomic's round trip lies under a tile's work) and hands it to the workgroup
    // through LDS at barrier (1).  ticket[BU_TICKET_DONE] counts the workgroups that have left; the last one zeroes all nine words for the next
    // launch on the same stream (the host hands every stream its own set: launches of one stream never overlap).
    __shared__ uint32_t s_next_tile[2];
    // thread 0: the counter value drawn for the tile behind the next one.  It stays RAW until it is handed over: arithmetic on it right behind the
    // atomic would make the wave wait for the atomic's round trip on the spot, with the whole workgroup behind it at the next barrier
    uint32_t my_draw = 0;
    unsigned* const my_counter = ticket ? ticket + (blockIdx.x & 7u) * BU_TICKET_STRIDE : nullptr;
    auto tile_of_draw = [&](uint32_t d) { return gridDim.x + 8u * d + (blockIdx.x & 7u); };
    if (ticket && tid == 0) my_draw = atomicAdd(my_counter, 1u);
    // w.d / w.l: the tile being sorted, transcoded and written back / the tile being loaded (BuWalk; wave-uniform: scalar).  The one-slice layouts have no descriptor.
    // MULTI: every access of a tile is a wave-uniform 64-bit base (the tile's corner: w.d.in / w.d.out, scalar arithmetic per tile) plus the lane's 32-bit byte
    // offset from that corner (w.off)
    using Tile = std::conditional_t<MULTI, BuMultiTile, std::conditional_t<RECTS, BuRectTile, BuNoTile>>;
    std::conditional_t<MULTI, BuMultiWalk<BPT>, BuWalk<Tile>> w;
    constexpr uint32_t OUT_BYTES = TARGET == BU_TGT_RGBA ? 16u : (uint32_t)bu_out_words(TARGET) * 4u;  // bytes of one result store
    // MULTI, persistent grid: the run table is copied to LDS once per workgroup (3.9 KiB) and every later look-up reads it there.  From the kernel
    // arguments a look-up is two vector loads, a ballot and dependent scalar loads -- a microsecond of round trips between the scatter and the prefetch
    // loads of EVERY tile, with the workgroup waiting at barrier (2) behind it (8 % of a multi-run launch over 2^20-block slices)
    constexpr bool RUNS_IN_LDS = (MULTI || RECTS) && PREFETCH;
    __shared__ uint4 s_runs[RUNS_IN_LDS ? (RECTS ? sizeof(BuRectTable) : sizeof(BuRunTable)) / 16 : 1];  // (16 bytes in every other instantiation)
    const BuRunTable* R = runs;  // the table the look-ups read: the kernel arguments until the copy is complete (the first barrier), LDS from then on
    const BuRectTable* Q = rects;  // RECTS: the job table, read where `R` is
    if constexpr (RUNS_IN_LDS && RECTS) {
        for (unsigned i = tid; i < sizeof(BuRectTable) / 16; i += WGS) s_runs[i] = reinterpret_cast<const uint4*>(rects)[i];
    } else if constexpr (RUNS_IN_LDS) {
        static_assert(sizeof(BuRunTable) % 16 == 0, "copied in 16-byte pieces");
        for (unsigned i = tid; i < sizeof(BuRunTable) / 16; i += WGS) s_runs[i] = reinterpret_cast<const uint4*>(runs)[i];
    }
    auto uni32 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    auto uni64 = [&](uint64_t x) { return (uint64_t)uni32((uint32_t)x) | ((uint64_t)uni32((uint32_t)(x >> 32)) << 32); };
    // the descriptor of tile t into w.l (nothing behind the last tile, nothing at all in the one-slice layouts)
    auto look_up = [&](unsigned t) {
        if constexpr (MULTI) {
            if (t < n_tiles) {
                if (!bu_cursor_holds(w.cur, t)) {
                    // runs 0..r start at or before tile t: r = (number of first-tile entries <= t) - 1; the unused entries are ~0
                    uint32_t r = 0;
                    // (this path is rare: the lane's address into the first-tile numbers is formed HERE, from a value the compiler cannot trace back to `lane`, or it
                    //  is hoisted out of the tile loop and holds a register -- in the 64-VGPR kernels a spill slot -- for the whole walk)
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));
#pragma unroll
                    for (unsigned c = 0; c < BU_MULTI_RUNS + 32; c += 64) {
                        const uint32_t cnt = (uint32_t)__popcll(__ballot(R->first_tile[c + ln] <= t));
                        if (cnt) r = c + cnt - 1u;
                    }
                    r = (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
                    // (the record comes back in vector registers -- an LDS read --, but every lane read the same one: made scalar here, so that everything derived
                    //  from it is scalar too.  The pointers are rebuilt from integers, so the compiler no longer knows their address space either: the block loads say
                    //  "global" themselves (bu_ld_stream_global), the result stores are asm global stores in any case)
                    const BuRunDesc rv = R->run[r];
                    const BuRunRec rd = {uni64(reinterpret_cast<uint64_t>(rv.in)), uni64(reinterpret_cast<uint64_t>(rv.out)), uni64(rv.base), uni32(rv.n), uni32(rv.vshift)};
                    w.cur = bu_run_cursor(rd, uni32(R->first_tile[r]), (uint32_t)BU_TILE);
                }
                w.l = bu_tile_of(w.cur, t, (uint32_t)BU_TILE, OUT_BYTES, TARGET == BU_TGT_RGBA ? bpr : 0u);
                if (w.l.width != w.off_width) {  // (uniform: the walk has reached a run of another width)
                    w.off_width = w.l.width;
#pragma unroll
                    for (int j = 0; j < BPT; j++) w.off[j] = bu_lane_off(WHOLE, w.l.width, (unsigned)(j * WGS) + tid);
                }
            }
        } else if constexpr (RECTS) {  // tile t belongs to the last job whose first tile is <= t (first_tile[0] = 0: there is one)
            if (t < n_tiles) {
                static_assert(BU_RECT_JOBS == 64, "one first-tile number per lane");
                const uint32_t r = uni32((uint32_t)__popcll(__ballot(Q->first_tile[lane] <= t)) - 1u);
                const BuRectDesc jv = Q->job[r];  // (every lane reads the same record: made scalar, as MULTI's)
                const BuRectDesc jd = {uni64(jv.in), uni64(jv.out), uni64(jv.pitch), uni64(jv.base), uni32(jv.in_bpr), uni32(jv.w), uni32(jv.h), uni32(jv.tpr)};
                w.l = bu_rect_tile(jd, t - uni32(Q->first_tile[r]), RECTS_ROW_BYTES, RECTS_ROWS);
            }
        }
    };
    auto advance = [&] { w.d = w.l; };  // the tile that was loaded is the one to sort
    look_up(tile);
    advance();
    // has block l of tile t, described by d, a block?  (WHOLE: every lane of every tile has one, and the validity tests fold away)
    auto has_blk = [&](const Tile& d, unsigned t, unsigned l) {
        if constexpr (WHOLE) return true;
        else if constexpr (RECTS) return bu_rect_has(d, l);
        else if constexpr (MULTI) return l < d.n;
        else return t * tile_blocks + l < n_blocks && in_tile(l);
    };
    // block j * WGS + tid of tile t, the tile described by w.l, loaded (MULTI: it lies w.off[j] bytes behind the tile's corner; one slice: `in` is a kernel
    // argument, global already); ld_or_zero: zeros where the lane has none or the walk has ended
    auto ld_blk = [&](unsigned t, int j) {
        if constexpr (MULTI) return bu_ld_stream_global(w.l.in, w.off[j]);
        else if constexpr (RECTS) return bu_ld_stream_global(reinterpret_cast<const uint4*>(bu_rect_src(w.l, (unsigned)(j * WGS) + tid)));
        else return bu_ld_stream(in + gidx(t, (unsigned)(j * WGS) + tid));
    };
    // (`&`, not `&&`: one lane mask per load, no uniform branch around each of them)
    auto ld_or_zero = [&](unsigned t, int j) { return ((t < n_tiles) & has_blk(w.l, t, (unsigned)(j * WGS) + tid)) ? ld_blk(t, j) : make_uint4(0, 0, 0, 0); };
    // Table staging.  The staged 16-byte pieces of the LDS image are numbered 0..TVT-1: BC7's own tables, then the target's one or
    // two ranges of the common blob; piece i sits at t_store[tdst(i)] and comes from the same index of the image's source in device
    // memory.  Every thread issues ALL its table loads back to back (round 2 ran a load / wait / store loop: a second L2 round
    // trip per 8 KiB of tables in front of the first barrier) and, where the image is small, BEFORE the tile's block loads.
    // Images above 16 KiB (ETC: 26.6 KiB) go tile loads first, only key_lut (128 B: all the sort phases read) staged up front, the
    // rest held in registers until the first tile's rank atomics are out (A/B: ETC1 19.45 -> 19.0 us in round 2; tables first
    // 19.2 -> 19.8 in round 3).
    constexpr BuTableRange TR = bu_table_range(TARGET);
    constexpr bool SPLIT = bu_lds_table_bytes(TARGET) > 16384;
    constexpr int TF = (int)bu_lds_front(TARGET) / 16, TV1 = (int)(TR.hi - TR.lo) / 16, TV2 = TR.lo2 < TR.hi2 ? (int)(TR.hi2 - TR.lo2) / 16 : 0;
    constexpr int TVT = TF + TV1 + TV2, TVN = (TVT + WGS - 1) / WGS;
    const uint4* const tsrc = reinterpret_cast<const uint4*>(TARGET == BU_TGT_BC7 ? reinterpret_cast<const void*>(tables) : reinterpret_cast<const void*>(&tables->t));
    auto tdst = [&](int i) { return i < TF ? i : (i < TF + TV1 ? (int)(TR.lo / 16) + i : TF + (int)(TR.lo2 / 16) + (i - TF - TV1)); };
    uint4 tv[TVN];
    if constexpr (!SPLIT) {
#pragma unroll
        for (int k = 0; k < TVN; k++) {
            const int i = k * WGS + (int)tid;
            tv[k] = i < TVT ? tsrc[tdst(i)] : make_uint4(0, 0, 0, 0);
        }
    }
    uint4 v[BU_BPT];
#pragma unroll
    for (int j = 0; j < BU_BPT; j++) v[j] = RECT ? ld_blk(tile, j) : ld_or_zero(tile, j);  // (RECT: the grid is at most n_tiles)
    if constexpr (!SPLIT) {
#pragma unroll
        for (int k = 0; k < TVN; k++) {
            const int i = k * WGS + (int)tid;
            if (i < TVT) t_store[tdst(i)] = tv[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < TVN; k++) {
            const int i = k * WGS + (int)tid;
            tv[k] = i < TVT ? tsrc[tdst(i)] : make_uint4(0, 0, 0, 0);
        }
        static_assert(offsetof(BuTables, key_lut) % 4 == 0 && sizeof(T.key_lut[0]) == 128, "the target's key_lut is staged as 32 dwords");
        if (tid < 32) reinterpret_cast<uint32_t*>(T.key_lut[bu_cost_row(TARGET)])[tid] = reinterpret_cast<const uint32_t*>(tables->t.key_lut[bu_cost_row(TARGET)])[tid];
    }
    bool tables_staged = !SPLIT;
    if (tid < 64) (&cnt[0][0])[tid] = 0;
    if (tid < 2) next_chunk[tid] = 0;
    __syncthreads();
    if constexpr (RUNS_IN_LDS && RECTS) Q = reinterpret_cast<const BuRectTable*>(s_runs);
    else if constexpr (RUNS_IN_LDS) R = reinterpret_cast<const BuRunTable*>(s_runs);
    unsigned par = 0;
    unsigned next_of_loop = 0;
    // STORES_LAST (the multi-run BC7 / ASTC kernels with PREFETCH): a tile's result stores are the LAST thing its iteration issues.  vmcnt counts loads and stores in issue order and
    // the compiler does not count the asm stores of bu_st_stream, so whatever is waited for behind them -- the prefetched blocks `vn`, the drawn ticket -- also
    // waits for their write-through acknowledgement with nothing of the wave's in flight.  Phase D therefore takes the results out of LDS, then consumes what is
    // in flight (the next tile's sort keys out of `vn`, thread 0's next tile out of `my_draw`: they cross the loop edge in `key` / `drawn_tile`), then stores;
    // nothing waits on those stores until the same point of the next tile.  BPT x 4 more live registers at that point.  ASTC takes it in the whole-tile layouts
    // only: its 512 x 2 kernels are held to 64 VGPRs (__launch_bounds__(512, 8)), and its 256 x 4 strip kernel would go from 79 to 97 VGPRs -- four workgroups
    // per CU where the launcher counts on five.  Every target whose results do not travel as one uint4 per block keeps the plain tail too.
    // The ONE-SLICE kernels keep the plain tail as well, all of them: a lone atlas runs bu_uastc_sorted_kernel<BC7, 512, 2, prefetch, RECT> as one-tile workgroups, which
    // have no next tile and pay for this order (results out of LDS first, keys of an empty `vn`) in front of their only stores: 8.41 -> 8.61 us per 2^20-block atlas.
    // The multi-run kernels run as one-tile workgroups only between one tile per CU and one grid of tiles (bu_plan_multi_kernel).
    constexpr bool STORES_LAST = PREFETCH && MULTI && (TARGET == BU_TGT_BC7 || (TARGET == BU_TGT_ASTC && WGS == 256 && WHOLE));
    // sort key of thread block j of tile t, described by d, whose first word is x: the position of its mode in BU_COST_ORDER; 31 where the lane has no block
    auto key_of = [&](const Tile& d, unsigned t, int j, uint32_t x) { return has_blk(d, t, (unsigned)(j * BU_WG) + tid) ? (uint32_t)T.key_lut[bu_cost_row(TARGET)][x & 127u] : 31u; };
    uint32_t next_key[STORES_LAST ? BU_BPT : 1];  // STORES_LAST: the keys of the tile about to be sorted, taken in phase D of the tile before it
    uint32_t drawn_tile = 0;  // thread 0, STORES_LAST: tile_of_draw(my_draw), taken before the stores went out
    if constexpr (STORES_LAST) {
        if (tile < n_tiles) {
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) next_key[j] = key_of(w.d, tile, j, v[j].x);
        }
        if (ticket && tid == 0) drawn_tile = tile_of_draw(my_draw);
        // Nothing of the prologue is still in flight here in practice (the table pieces were stored to LDS before the barrier above, the first tile's keys and the first
        // draw have just been used) -- but every one of those uses sits behind a condition, and the compiler's wait-count bookkeeping is path-insensitive: it would carry
        // "a load into these registers may be pending" into the loop and wait for vmcnt(0) at the first write to one of them in EVERY iteration, which lands a few
        // instructions behind the previous tile's stores.  One full wait here, outside the loop, clears its books.  (vmcnt(0), the other counters untouched)
        __builtin_amdgcn_s_waitcnt(0x0F70);
    }
    for (; tile < n_tiles; tile = next_of_loop, par ^= 1u) {
        // ---- A: sort key + rank within the key (counting sort, pass 1) ----
        // key = position of the block's mode in BU_COST_ORDER (runs are laid out heaviest code path first).
        // Rank within the key = one LDS atomic per block.  64 lanes adding to ONE counter serialise, though, and that is
        // exactly what coherent textures produce (flat regions: long runs of one mode).  A wave whose loads are each of a
        // single mode therefore takes an aggregated path -- one atomic of 64 by lane 0 per load, rank = lane id -- chosen
        // by a wave-uniform branch; every other wave runs the plain per-lane atomics unchanged.
        uint32_t key[BU_BPT], pos[BU_BPT];
        bool uniform = true;
#pragma unroll
        for (int j = 0; j < BU_BPT; j++) {
            key[j] = STORES_LAST ? next_key[j] : key_of(w.d, tile, j, v[j].x);
            uniform = uniform && (__ballot(key[j] == (uint32_t)__builtin_amdgcn_readfirstlane(key[j])) == ~0ull) && has_block(key[j]);
        }
        if (uniform) {
            uint32_t lead[BU_BPT];
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) lead[j] = lane == 0 ? atomicAdd(&cnt[par][key[j]], 64u) : 0u;
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) pos[j] = (uint32_t)__builtin_amdgcn_readfirstlane(lead[j]) + lane;
        } else {
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) pos[j] = atomicAdd(&cnt[par][key[j]], 1u);  // lanes past the end hit the dummy counter 31: no exec-mask region, the atomics issue back to back
        }
        if (ticket && tid == 0) s_next_tile[par] = STORES_LAST ? drawn_tile : tile_of_draw(my_draw);
        if (!tables_staged) {  // (key_lut is rewritten with the bytes it already holds)
#pragma unroll
            for (int k = 0; k < TVN; k++) {
                const int i = k * WGS + (int)tid;
                if (i < TVT) t_store[tdst(i)] = tv[k];
            }
            tables_staged = true;
        }
        __syncthreads();  // (1) every rank is final; the tables are in LDS
        // ---- B: run starts and the chunk map, derived by EVERY wave for itself ----
        // Lane k < 20 holds run k: blocks in the low half, 64-block chunks in the high half of one word; a DPP scan gives
        // every run's first slot and first chunk number.  No wave waits for another one here (the round-1 kernel had one
        // wave build a chunk list in LDS while seven stood at a barrier).
        const uint32_t run_c = lane < 20u ? cnt[par][lane] : 0u;
        const uint32_t run_pk = run_c | (((run_c + 63u) >> 6) << 16);
        const uint32_t run_incl = bu_scan32(run_pk), run_excl = run_incl - run_pk;  // lanes 20..31 carry the totals
        const uint32_t nc = (uint32_t)__builtin_amdgcn_readlane((int)run_incl, 31) >> 16;
        if (tid < 32) cnt[par ^ 1u][tid] = 0;  // the other parity: last read in B of the previous tile, next written in A of the next one
        if (tid == 0) next_chunk[par ^ 1u] = 0;
        // ---- scatter into sorted order (counting sort, pass 2) ----
        uint32_t dest[BU_BPT];
#pragma unroll
        for (int j = 0; j < BU_BPT; j++) {
            const uint32_t st = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(key[j] << 2), (int)run_excl) & 0xFFFFu;
            dest[j] = has_block(key[j]) ? st + pos[j] : 0u;
            if (has_block(key[j])) sblk[dest[j]] = v[j];
        }
        // prefetch the next tile while this one is transcoded
        const unsigned ntile = ticket ? (unsigned)__builtin_amdgcn_readfirstlane((int)s_next_tile[par]) : tile + gridDim.x;
        next_of_loop = ntile;
        uint4 vn[BU_BPT];
        if constexpr (PREFETCH) {
            look_up(ntile);
            if constexpr (MULTI && WHOLE) {
                // every lane of every tile has a block: the loads hang on the one uniform condition and issue back to back under it
                if (ntile < n_tiles) {
#pragma unroll
                    for (int j = 0; j < BU_BPT; j++) vn[j] = ld_blk(ntile, j);
                } else {
#pragma unroll
                    for (int j = 0; j < BU_BPT; j++) vn[j] = make_uint4(0, 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int j = 0; j < BU_BPT; j++) vn[j] = ld_or_zero(ntile, j);
            }
        }
        if (ticket && tid == 0 && ntile < n_tiles) my_draw = atomicAdd(my_counter, 1u);  // (for the tile after the next: needed one tile from now)
        __syncthreads();  // (2) the sorted tile is complete
        // ---- C: whole chunks, wave-uniform mode ----
        // dynamic chunk scheduling: waves take the next chunk as they free up (one LDS atomic per chunk).  The claim for the
        // FOLLOWING chunk is issued before the current one is transcoded, so its LDS round trip hides under the transcode.
        uint32_t c_next = 0;
        if (lane == 0) c_next = atomicAdd(&next_chunk[par], 1u);
        for (;;) {
            const uint32_t c = __builtin_amdgcn_readfirstlane(c_next);
            if (c >= nc) break;
            if (lane == 0) c_next = atomicAdd(&next_chunk[par], 1u);
            // chunk c belongs to the first run whose inclusive chunk count exceeds c
            const uint32_t r = (uint32_t)__builtin_ctzll(__ballot((run_incl >> 16) > c));
            const uint32_t r_pk = (uint32_t)__builtin_amdgcn_readlane((int)run_pk, (int)r), r_ex = (uint32_t)__builtin_amdgcn_readlane((int)run_excl, (int)r);
            const uint32_t k64 = (c - (r_ex >> 16)) << 6;
            const uint32_t s0 = (r_ex & 0xFFFFu) + k64, left = (r_pk & 0xFFFFu) - k64, count = left < 64u ? left : 64u;
            const bool active = lane < count;
            const uint32_t slot = s0 + (active ? lane : 0u);
            const uint4 bv = sblk[slot];
            BuBlk b;
            b.w[0] = bv.x;
            b.w[1] = bv.y;
            b.w[2] = bv.z;
            b.w[3] = bv.w;
            constexpr int NO = TARGET == BU_TGT_RGBA ? 16 : 4;
            uint32_t o[NO];
#pragma unroll
            for (int i = 0; i < NO; i++) o[i] = 0;
            int st = BU_ST_BAD_MODE;
            if (active) {
                switch (r) {  // the run number IS the sort key: run k holds mode BU_COST_ORDER[k] (run 19: invalid mode codes)
#define BU_CASE(k) \
    case k: st = bu_block_mode<TARGET, BU_COST_ORDER[bu_cost_row(TARGET)][k]>(T, b, o); break;
                    BU_CASE(0) BU_CASE(1) BU_CASE(2) BU_CASE(3) BU_CASE(4) BU_CASE(5) BU_CASE(6) BU_CASE(7) BU_CASE(8) BU_CASE(9)
                    BU_CASE(10) BU_CASE(11) BU_CASE(12) BU_CASE(13) BU_CASE(14) BU_CASE(15) BU_CASE(16) BU_CASE(17) BU_CASE(18)
#undef BU_CASE
                default: break;
                }
                // (a failing block leaves o[] at the zeros it was initialised with: every path checks before it writes)
                if constexpr (TARGET == BU_TGT_RGBA) {
#pragma unroll
                    for (int r2 = 0; r2 < 4; r2++) sout[r2 * BU_TILE + slot] = make_uint4(o[4 * r2], o[4 * r2 + 1], o[4 * r2 + 2], o[4 * r2 + 3]);
                    sst[slot] = (uint8_t)st;
                } else if constexpr (INBLOCK) {
                    sblk[slot] = make_uint4(o[0], o[1], o[2], o[3] | (uint32_t)st);  // (a failing block's o[] is all zeros)
                } else {
                    sblk[slot] = make_uint4(o[0], o[1], o[2], o[3]);
                    sst[slot] = (uint8_t)st;
                }
            }
        }
        __syncthreads();  // (3) every result is in LDS
        // ---- D: results leave in original order ----
        // MULTI: the lane offsets of the tile being written back.  With PREFETCH the look-up for the next tile has already run: if that tile lies in a run of another
        // width, w.off belongs to it, and this tile's offsets are computed once more (a uniform branch, taken once per change of width)
        [[maybe_unused]] uint32_t so[MULTI ? BU_BPT : 1];
        if constexpr (MULTI) {
#pragma unroll
            for (int j = 0; j < BPT; j++) so[j] = w.off[j];
            if (w.d.width != w.off_width) {
#pragma unroll
                for (int j = 0; j < BPT; j++) so[j] = bu_lane_off(WHOLE, w.d.width, (unsigned)(j * WGS) + tid);
            }
        }
        // The layouts differ in which block of the call thread block j is (status words) and in where its result goes -- 16 bytes, 8 bytes, or pixel row r of RGBA32's
        // four: at the job's pitch (RECTS), from the tile's corner by the lane's offset (MULTI), by the block's index in the slice (one slice)
        auto blk_of = [&](int j) -> unsigned long long {
            if constexpr (RECTS) return w.d.base + bu_rect_idx(w.d, (unsigned)(j * BU_WG) + tid);
            else if constexpr (MULTI) return w.d.base + bu_lane_block(w.d, so[j]);
            else return base + gidx(tile, (unsigned)(j * BU_WG) + tid);
        };
        auto put16 = [&](int j, const uint4 r) {
            if constexpr (RECTS) bu_st_stream(reinterpret_cast<uint4*>(bu_rect_dst(w.d, (unsigned)(j * BU_WG) + tid, RECTS_ROW_BYTES, RECTS_ROWS)), r);
            else if constexpr (MULTI) bu_st_stream(w.d.out, so[j], r);
            else bu_st_stream(reinterpret_cast<uint4*>(out) + gidx(tile, (unsigned)(j * BU_WG) + tid), r);
        };
        auto put8 = [&](int j, const uint2 r) {
            if constexpr (RECTS) bu_st_stream(reinterpret_cast<uint2*>(bu_rect_dst(w.d, (unsigned)(j * BU_WG) + tid, RECTS_ROW_BYTES, RECTS_ROWS)), r);
            else if constexpr (MULTI) bu_st_stream(w.d.out, so[j] >> 1, r);
            else bu_st_stream(reinterpret_cast<uint2*>(out) + gidx(tile, (unsigned)(j * BU_WG) + tid), r);
        };
        auto put_row = [&](int j, int r, const uint4 px) {
            const unsigned l = (unsigned)(j * BU_WG) + tid;
            if constexpr (RECTS) {
                bu_st_stream(reinterpret_cast<uint4*>(bu_rect_dst(w.d, l, RECTS_ROW_BYTES, RECTS_ROWS) + (uint64_t)r * w.d.pitch), px);
            } else if constexpr (MULTI) {
                bu_st_stream(w.d.out, bu_lane_off_rgba(w.d, so[j], bpr) + (uint32_t)r * bpr * 16u, px);
            } else {
                unsigned by, bx;
                if constexpr (RECT) {  // block row and column straight from the tile coordinates: no division
                    unsigned ty, tx;
                    tile_xy(tile, ty, tx);
                    by = (unsigned)(BU_TILE / BU_RECT_W) * ty + l / BU_RECT_W;
                    bx = BU_RECT_W * tx + (l % BU_RECT_W);
                } else {
                    by = gidx(tile, l) / bpr;
                    bx = gidx(tile, l) - by * bpr;
                }
                bu_st_stream(reinterpret_cast<uint4*>(out) + (size_t)((4 * by + r) * bpr + bx), px);
            }
        };
        // BC7, ASTC: thread block j's result out of its slot; no valid block of these formats starts with a zero byte: word 3 is then the status, reported and cleared
        auto take_inblock = [&](int j) {
            uint4 r = sblk[dest[j]];
            if ((r.x & 0xFFu) == 0u) {
                bu_report(status, blk_of(j), (int)r.w);
                r.w = 0;
            }
            return r;
        };
        if constexpr (STORES_LAST) {
            uint4 r[BU_BPT];
            bool has[BU_BPT];
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) {
                has[j] = has_block(key[j]);
                if (has[j]) r[j] = take_inblock(j);
            }
            // everything this wave still has in flight is consumed HERE, in front of the stores (the asm stores clobber memory: the LDS reads of key_lut stay
            // on this side of them, and so does the compiler's wait for `vn`)
            // (on EVERY path, needed or not -- behind the last tile `vn` is zeros and the draw is stale: the compiler's wait-count bookkeeping is path-insensitive,
            //  and a use under a condition would leave "may still be pending" standing, to be waited for at the next write to these registers: behind the stores)
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) next_key[j] = key_of(w.l, ntile, j, vn[j].x);
            drawn_tile = tile_of_draw(my_draw);   // (every lane, with or without tickets: thread 0's is the one that counts, and only under tickets.  These few
                                                  //  instructions and the key look-ups of a zero `vn` behind a workgroup's last tile are work done to steer the
                                                  //  wait-count pass; tests/test_multi_kernel_address_space.py holds what they buy)
            asm volatile("" : "+v"(drawn_tile));  // (plain arithmetic: pinned in front of the stores by hand)
#pragma unroll
            for (int j = 0; j < BU_BPT; j++)
                if (has[j]) put16(j, r[j]);
        } else {
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) {
                if (!has_block(key[j])) continue;
                if constexpr (INBLOCK) {
                    put16(j, take_inblock(j));
                } else {
                    const uint32_t st = sst[dest[j]];
                    if (st) bu_report(status, blk_of(j), (int)st);
                    if constexpr (TARGET == BU_TGT_RGBA) {
#pragma unroll
                        for (int r = 0; r < 4; r++) put_row(j, r, sout[r * BU_TILE + dest[j]]);
                    } else {
                        const uint4 r = sblk[dest[j]];
                        if constexpr (bu_out_words(TARGET) == 2) put8(j, make_uint2(r.x, r.y));
                        else put16(j, r);
                    }
                }
            }
        }
        // the tile that has been loaded -- ahead of time with PREFETCH, only now without -- becomes the tile to sort
        if constexpr (PREFETCH) {
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) v[j] = vn[j];
        } else {
            look_up(ntile);
#pragma unroll
            for (int j = 0; j < BU_BPT; j++) v[j] = ld_or_zero(ntile, j);
        }
        advance();
        // no barrier here: the next tile's scatter into `sblk` sits behind its barrier (1), which every wave reaches only
        // after its reads of this tile's results have completed
    }
    if (ticket && tid == 0) {  // the last workgroup out resets the set (every other one has drawn its last ticket by then)
        if (atomicAdd(ticket + BU_TICKET_DONE, 1u) == gridDim.x - 1u) {
            for (unsigned k = 0; k < 8; k++) atomicExch(ticket + k * BU_TICKET_STRIDE, 0u);
            atomicExch(ticket + BU_TICKET_DONE, 0u);
        }
    }
}

// MINW: minimum waves per SIMD the register allocation must leave room for (the second __launch_bounds__ argument)
template <int TARGET, int WGS, int BPT, int MINW, bool PREFETCH, int LAYOUT>
__global__ __launch_bounds__(WGS, MINW) void bu_uastc_sorted_kernel(const uint4* __restrict__ in, void* __restrict__ out, unsigned n_blocks,
                                                                unsigned bpr, unsigned long long base, unsigned long long* status,
                                                                const BuTablesAll* __restrict__ tables, unsigned cus, unsigned tile_rt,
                                                                unsigned* __restrict__ ticket)
{
    static_assert(LAYOUT != BU_LAYOUT_MULTI && LAYOUT != BU_LAYOUT_MULTI_WHOLE, "several runs per launch: bu_uastc_multi_kernel");
    bu_uastc_sorted_body<TARGET, WGS, BPT, PREFETCH, LAYOUT>(in, out, n_blocks, bpr, base, status, tables, cus, tile_rt, nullptr, ticket);
}

// several runs in one launch (layout MULTI): n_tiles 1024-block tiles over the runs of `table` (a kernel argument, by value).
// PREFETCH: the launch is a persistent grid whose workgroups walk many tiles (batches of large slices): the next tile's blocks -- of
// whatever run it belongs to -- are loaded while the current tile is transcoded, as in the one-slice kernel.
// WHOLE: every run of the table is tiled as whole rectangles (the host checked: BuRunDesc::vshift of all of them)
// (ASTC, 512 threads: the register allocation is held to the 64 VGPRs at which FOUR such workgroups fit a CU -- left alone it takes 66, three fit, and a persistent grid of four
//  per CU runs its fourth behind the others: 64 ragged slices of ~2^20 blocks 6.7 -> see profiles/r06_ab_astc_64_vgprs.txt)
// (ETC1 / ETC2 and the channel targets also as 512 x 4 on 2048-block tiles -- the host then numbers 2048-block tiles -- under the shared shape's __launch_bounds__(512, 4): two workgroups per CU)
constexpr bool bu_multi_etc_2048(int target, int tile) { return bu_etc_family(target) && tile == 2048; }
template <int TARGET, int WGS, int BPT, bool PREFETCH = false, bool WHOLE = false>
__global__ __launch_bounds__(WGS, (TARGET == BU_TGT_ASTC && WGS == 512) ? 8 : bu_multi_etc_2048(TARGET, WGS * BPT) ? 4 : 1) void bu_uastc_multi_kernel(
    const BuRunTable table, unsigned n_tiles, unsigned bpr, unsigned long long* status, const BuTablesAll* __restrict__ tables, unsigned* __restrict__ ticket)
{
    static_assert(WGS * BPT == 1024 || bu_multi_etc_2048(TARGET, WGS * BPT), "the host numbers 1024-block tiles (ETC1 / ETC2 large batches: 2048-block ones)");
    static_assert(sizeof(BuRunTable) + 40 <= 4096, "the run table and the other arguments share the 4 KiB of kernel arguments");
    bu_uastc_sorted_body<TARGET, WGS, BPT, PREFETCH, WHOLE ? BU_LAYOUT_MULTI_WHOLE : BU_LAYOUT_MULTI>(nullptr, nullptr, n_tiles * (unsigned)(WGS * BPT), bpr, 0ull, status, tables, 0u,
                                                                                                        (unsigned)(WGS * BPT), &table, ticket);
}

// rectangles of slices into pitched surfaces in one launch (layout RECTS; bu_uastc_transcode_rects_device): n_tiles tiles over the jobs of `table` (a kernel
// argument, by value; copied to LDS once per workgroup), a persistent grid in the multi-run launch's 512 x 2 shape with the next tile's loads in flight.  One
// instantiation per target; no tile tickets.  (ASTC is NOT held to 64 VGPRs here as its multi-run kernel of this shape is: that bound costs it a spill.)
template <int TARGET>
__global__ __launch_bounds__(512) void bu_uastc_rects_kernel(const BuRectTable table, unsigned n_tiles, unsigned long long* status, const BuTablesAll* __restrict__ tables)
{
    static_assert(sizeof(BuRectTable) + 24 <= 4096, "the job table and the other arguments share the 4 KiB of kernel arguments");
    bu_uastc_sorted_body<TARGET, 512, 2, true, BU_LAYOUT_RECTS>(nullptr, nullptr, n_tiles * BU_RECTS_TILE, 0u, 0ull, status, tables, 0u, BU_RECTS_TILE, nullptr, nullptr, &table);
}

// status words back to "no failing block".  A kernel, not hipMemsetAsync: the reset is part of what callers capture into
// hipGraphs, and a captured 8-byte memset node replayed as zeros on ROCm 7.2 (tests/test_gpu_round2.py, graph test).
__global__ void bu_status_reset_kernel(unsigned long long* words, unsigned n)
{
    for (unsigned i = threadIdx.x; i < n; i += blockDim.x) words[i] = ~0ull;
}

// ---- CRC-16/GENIBUS of an uploaded file range (basis.rs:364-372; the data CRC of basis.rs:338-341) ----------------------------
// The CRC is linear over GF(2): register(A || B) = register(A) * x^(8|B|) + register(B).  One workgroup covers a 64 KiB piece:
// every thread runs the table-driven register over its own 256 bytes (slicing by four, tables in LDS), multiplies it by
// x^(8 * bytes behind it inside the piece) and the workgroup XORs the 256 contributions.  The host folds the pieces' registers
// (and the few bytes the device never sees: slice table, gaps, tails) in file order -- bu_crc_fold, bu_file_layout.hpp, which has BU_CRC_PIECE.
struct BuCrcTables {
    uint16_t t[4][256];  // t[k][b]: register after byte b followed by k zero bytes
    uint16_t pw[256];    // pw[k] = x^(8 * 256 * k) mod P
};

__device__ __forceinline__ uint32_t bu_crc_gf_mul(uint32_t a, uint32_t b)  // a * b mod x^16 + x^12 + x^5 + 1
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        r ^= (r & 0x10000u) ? 0x11021u : 0u;
        r ^= ((b >> i) & 1u) ? a : 0u;
    }
    return r & 0xFFFFu;
}

__global__ __launch_bounds__(256) void bu_crc16_pieces_kernel(const uint4* __restrict__ data, uint16_t* __restrict__ partial,
                                                              const BuCrcTables* __restrict__ tables)
{
    __shared__ BuCrcTables C;
    __shared__ uint32_t red[4];
    static_assert(sizeof(BuCrcTables) % 16 == 0, "copied in 16-byte pieces");
    for (unsigned i = threadIdx.x; i < sizeof(BuCrcTables) / 16; i += 256) reinterpret_cast<uint4*>(&C)[i] = reinterpret_cast<const uint4*>(tables)[i];
    __syncthreads();
    const uint4* p = data + (size_t)blockIdx.x * (BU_CRC_PIECE / 16) + threadIdx.x * 16;
    uint32_t s = 0;
#pragma unroll 4
    for (int i = 0; i < 16; i++) {
        const uint4 v = p[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {  // bytes in memory order: b0 = low byte of the little-endian word
            const uint32_t x = w[k];
            s = (uint32_t)C.t[3][((s >> 8) ^ x) & 255u] ^ (uint32_t)C.t[2][(s ^ (x >> 8)) & 255u] ^ (uint32_t)C.t[1][(x >> 16) & 255u] ^ (uint32_t)C.t[0][x >> 24];
        }
    }
    uint32_t c = bu_crc_gf_mul(s, C.pw[255u - threadIdx.x]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (uint16_t)(red[0] ^ red[1] ^ red[2] ^ red[3]);
}

// one wave that does nothing for `ticks` ticks of the constant 100 MHz clock (bu_context_probe_streams: kernels of different streams that
// sit on different hardware queues sleep side by side, kernels of streams that share a queue one after the other)
__global__ __launch_bounds__(64) void bu_sleep_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// uint4 -> uint4 copy (measurement only): the practical ceiling any 16 B in / 16 B out kernel is compared with -- one pass per thread, every load in flight before
// the first store, nontemporal both ways.  The shape is the fastest of tools/exp/copy_big.hip at the size (profiles/r06_copy_ceiling_by_size.txt): 1024 threads x one
// element from 2^22 elements on (2^25: 164.5 us = 6.5 TB/s = 0.82 of the data sheet; 256 x 4: 166, 512 x 4 -- this kernel until round 6 -- 173.6, plain loads and
// stores 181), 256 x 4 below (2^20: 6.7 us against 7.0 / 7.1).
template <int WG, int EPT>
__global__ __launch_bounds__(WG) void bu_copy_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, size_t n)
{
    const size_t base = (size_t)blockIdx.x * (WG * EPT) + threadIdx.x;
    uint4 v[EPT];
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const size_t i = base + (size_t)k * WG;
        if (i < n) v[k] = bu_ld_stream(in + i);
    }
#pragma unroll
    for (int k = 0; k < EPT; k++) {
        const size_t i = base + (size_t)k * WG;
        if (i < n) {
            bu_v4u r;
            r.x = v[k].x; r.y = v[k].y; r.z = v[k].z; r.w = v[k].w;
            __builtin_nontemporal_store(r, reinterpret_cast<bu_v4u*>(out + i));
        }
    }
}

}  // namespace
