// TEST-ONLY: the protocol of the blocking host-pointer entry points (csrc/bu_context.hpp + csrc/bu_staged_call.hpp, the shipped text) on the CPU,
// under ASan / UBSan (tests/test_staged_call.py), where its error paths can be reached.  The HIP runtime is the dozen functions below: device
// memory is malloc'ed, a device-to-host copy is RECORDED and performed at the next synchronise of the stream -- so a copy whose destination died
// before that synchronise writes freed memory and ASan says so -- page-locked memory is a table of ranges, and call number k can be made to fail.
// A model driver uses every step of the staged call.  Never part of the product library; nothing links against the HIP runtime.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "bu_file_layout.hpp"  // (BuAuxLayout; the public header)
struct BuTablesAll;
struct BuCrcTables;
#include "bu_context.hpp"
#include "bu_staged_call.hpp"

// ---- the runtime ----------------------------------------------------------------------------------------------------------------------
namespace {
struct Copy { void* dst; const void* src; size_t n; };
struct Range { const uint8_t* base; size_t n; };
std::vector<std::string> calls;  // every runtime call and the launch, in order
std::vector<Copy> pending;       // device-to-host copies of the one stream, not performed yet
std::vector<Range> page_locked;
int failable_calls = 0, fail_at = 0;  // fail_at = k > 0: the k-th call that can fail does
const char* failed_call = nullptr;
const void *output_host = nullptr, *extra_host = nullptr;  // where the model driver's staged output and its extra range land: a download is named by its destination

hipError_t call(const char* name, bool can_fail = true)
{
    calls.push_back(name);
    if (can_fail && ++failable_calls == fail_at) {
        failed_call = name;
        return hipErrorUnknown;
    }
    return hipSuccess;
}
void reset_runtime(int fail_k)
{
    calls.clear();
    failable_calls = 0;
    fail_at = fail_k;
    failed_call = nullptr;
}
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            abort();                                                         \
        }                                                                    \
    } while (0)
}  // namespace

const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "injected failure"; }
hipError_t hipGetLastError(void) { return call("hipGetLastError", false); }
hipError_t hipSetDevice(int) { return call("hipSetDevice"); }
hipError_t hipMalloc(void** p, size_t n)
{
    const hipError_t e = call("hipMalloc");
    if (e == hipSuccess) *p = malloc(n);
    return e;
}
hipError_t hipFree(void* p)
{
    const hipError_t e = call("hipFree");
    if (e == hipSuccess) free(p);
    return e;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned)
{
    const hipError_t e = call("hipHostMalloc");
    if (e == hipSuccess) *p = malloc(n);
    return e;
}
hipError_t hipHostFree(void* p)
{
    const hipError_t e = call("hipHostFree");
    if (e == hipSuccess) free(p);
    return e;
}
// a pointer into a page-locked range is its own device view; anything else is unregistered (a query, never made to fail: that only means "pageable")
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p)
{
    (void)call("hipPointerGetAttributes", false);
    memset(a, 0, sizeof(*a));
    a->type = hipMemoryTypeUnregistered;
    for (const Range& r : page_locked)
        if (static_cast<const uint8_t*>(p) >= r.base && static_cast<const uint8_t*>(p) < r.base + r.n) {
            a->type = hipMemoryTypeHost;
            a->devicePointer = const_cast<void*>(p);
            a->hostPointer = const_cast<void*>(p);
        }
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t)
{
    const hipError_t e = call(kind != hipMemcpyDeviceToHost ? "hipMemcpyAsync H2D"
                              : dst == output_host          ? "hipMemcpyAsync D2H output"
                              : dst == extra_host           ? "hipMemcpyAsync D2H extra"
                                                            : "hipMemcpyAsync D2H status");
    if (e != hipSuccess) return e;
    if (kind == hipMemcpyDeviceToHost) pending.push_back({dst, src, n});
    else memcpy(dst, src, n);  // (everything enqueued before it has run: uploads, the reset and the launch run where they are enqueued)
    return e;
}
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t)
{
    const hipError_t e = call("hipMemsetAsync");
    if (e == hipSuccess) memset(dst, v, n);
    return e;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    const hipError_t e = call("hipStreamSynchronize");
    if (e != hipSuccess) return e;
    for (const Copy& c : pending) memcpy(c.dst, c.src, c.n);
    pending.clear();
    return e;
}

// ---- the model driver: every step of the staged call around one launch stand-in -----------------------------------------------------------
namespace {
constexpr uint8_t KEY = 0x5A;
struct Job {
    const uint8_t* in;
    uint8_t* out;
    size_t n;
    std::vector<uint64_t> reports;  // what the launch leaves in the status words, one per image
    size_t align = 16;
    bool in_mapped = false, out_mapped = false;  // (out: what the call did)
    uint32_t extra = 0;                          // (out: the extra landing range)
};

bu_status model_driver(bu_context* ctx, Job& j, uint64_t* first_bad)
{
    uint32_t extra = 0;  // landing range of the driver's own: in front of the call, so it outlives the drain
    bu_status st;
    output_host = j.out;
    extra_host = &extra;
    {
        BuStagedCall call(ctx, j.reports.size());
        const void* d_in = nullptr;
        void* d_out = nullptr;
        enum { KEYS, STATUS, EXTRA };
        if ((st = call.begin()) || (st = call.input(j.in, j.n, true, j.align, &d_in)) || (st = call.output(j.out, j.n + 64, j.n, true, j.align, &d_out)) ||
            (st = call.aux(BuAuxLayout({1, 8 * j.reports.size(), 4}), STATUS)))
            return st;
        j.in_mapped = call.in_mapped;
        j.out_mapped = call.out_mapped;
        BU_HIP(ctx, hipMemcpyAsync(call.region<void>(KEYS), &KEY, 1, hipMemcpyHostToDevice, ctx->stream));
        if ((st = call.status_reset())) return st;
        // the launch: reads the input and the key, writes the output, reports, leaves a register
        calls.push_back("launch");
        for (size_t k = 0; k < j.reports.size(); k++) {
            CHECK(call.d_status[k] == BU_STATUS_WORD_CLEAR);
            call.d_status[k] = j.reports[k];
        }
        for (size_t i = 0; i < j.n; i++) static_cast<uint8_t*>(d_out)[i] = static_cast<const uint8_t*>(d_in)[i] ^ *call.region<uint8_t>(KEYS);
        *call.region<uint32_t>(EXTRA) = 0xC0FFEEu;
        if ((st = call.finish(&extra, call.region<void>(EXTRA), 4))) return st;
        st = call.status(first_bad);
    }
    j.extra = extra;
    return st;
}

struct Ctx {
    bu_context c;
    Ctx()
    {
        c.device = 0;
        c.stream = reinterpret_cast<hipStream_t>(this);  // (a handle: nobody looks behind it)
        c.d_status = static_cast<unsigned long long*>(malloc(64));
    }
    ~Ctx()
    {
        free(c.d_status);
        free(c.d_in);
        free(c.d_out);
        free(c.d_aux);
    }
};

// buffers of a scenario: 256-aligned, `shift` bytes in; page-locked where asked
struct Buffers {
    uint8_t *in_base, *out_base, *in, *out;
    size_t n;
    Buffers(size_t n_, bool lock_in, bool lock_out, size_t shift = 0) : n(n_)
    {
        in_base = static_cast<uint8_t*>(aligned_alloc(256, (n + shift + 255) & ~(size_t)255));
        out_base = static_cast<uint8_t*>(aligned_alloc(256, (n + shift + 255) & ~(size_t)255));
        in = in_base + shift;
        out = out_base + shift;
        for (size_t i = 0; i < n; i++) in[i] = (uint8_t)(i * 7 + 3);
        memset(out, 0xEE, n);
        page_locked.clear();
        if (lock_in) page_locked.push_back({in_base, n + shift});
        if (lock_out) page_locked.push_back({out_base, n + shift});
    }
    ~Buffers()
    {
        page_locked.clear();
        free(in_base);
        free(out_base);
    }
    bool right() const
    {
        for (size_t i = 0; i < n; i++)
            if (out[i] != (uint8_t)(in[i] ^ KEY)) return false;
        return true;
    }
};

size_t last_of(const char* name)  // (the last call whose name begins with `name`)
{
    size_t at = 0;
    for (size_t i = 0; i < calls.size(); i++)
        if (calls[i].compare(0, strlen(name), name) == 0) at = i + 1;
    return at;  // 1-based; 0: never
}

// ---- (a) the call order ---------------------------------------------------------------------------------------------------------------
void check_order()
{
    const std::vector<std::string> want[4] = {
        // pageable in, pageable out
        {"hipSetDevice", "hipPointerGetAttributes", "hipMalloc", "hipMemcpyAsync H2D", "hipPointerGetAttributes", "hipMalloc", "hipMalloc", "hipMemcpyAsync H2D",
         "hipMemsetAsync", "launch", "hipMemcpyAsync D2H status", "hipMemcpyAsync D2H extra", "hipMemcpyAsync D2H output", "hipStreamSynchronize"},
        // mapped in
        {"hipSetDevice", "hipPointerGetAttributes", "hipPointerGetAttributes", "hipMalloc", "hipMalloc", "hipMemcpyAsync H2D", "hipMemsetAsync", "launch",
         "hipMemcpyAsync D2H status", "hipMemcpyAsync D2H extra", "hipMemcpyAsync D2H output", "hipStreamSynchronize"},
        // mapped out
        {"hipSetDevice", "hipPointerGetAttributes", "hipMalloc", "hipMemcpyAsync H2D", "hipPointerGetAttributes", "hipMalloc", "hipMemcpyAsync H2D", "hipMemsetAsync",
         "launch", "hipMemcpyAsync D2H status", "hipMemcpyAsync D2H extra", "hipStreamSynchronize"},
        // both mapped
        {"hipSetDevice", "hipPointerGetAttributes", "hipPointerGetAttributes", "hipMalloc", "hipMemcpyAsync H2D", "hipMemsetAsync", "launch", "hipMemcpyAsync D2H status",
         "hipMemcpyAsync D2H extra", "hipStreamSynchronize"}};
    for (int m = 0; m < 4; m++) {
        Ctx ctx;
        Buffers b(65, m & 1, m & 2);
        Job j{b.in, b.out, b.n, {BU_STATUS_WORD_CLEAR, BU_STATUS_WORD_CLEAR}};
        reset_runtime(0);
        CHECK(model_driver(&ctx.c, j, nullptr) == BU_OK);
        CHECK(calls == want[m]);
        CHECK(j.in_mapped == bool(m & 1) && j.out_mapped == bool(m & 2) && b.right() && j.extra == 0xC0FFEEu && pending.empty());
    }
    printf("order ok\n");
}

// ---- (b) a failure at every call --------------------------------------------------------------------------------------------------------
// grow: the context has served a small call, and this one needs larger buffers (bu_reserve frees before it allocates)
int check_failures(int mapping, bool grow)
{
    const size_t n = grow ? ((size_t)1 << 20) + 65 : 65;
    int n_calls = 0;
    for (int k = 0;; k++) {  // k = 0: the clean run, which counts the calls
        Ctx ctx;
        if (grow) {
            Buffers small(65, mapping & 1, mapping & 2);
            Job j{small.in, small.out, small.n, {BU_STATUS_WORD_CLEAR}};
            reset_runtime(0);
            CHECK(model_driver(&ctx.c, j, nullptr) == BU_OK);
        }
        Buffers b(n, mapping & 1, mapping & 2);
        Job j{b.in, b.out, b.n, {BU_STATUS_WORD_CLEAR, BU_STATUS_WORD_CLEAR, BU_STATUS_WORD_CLEAR}};
        reset_runtime(k);
        const bu_status st = model_driver(&ctx.c, j, nullptr);
        fail_at = 0;
        if (k == 0) {
            CHECK(st == BU_OK && b.right());
            n_calls = failable_calls;
            continue;
        }
        if (k > n_calls) break;
        CHECK(st == BU_ERR_HIP && failed_call);
        CHECK(strstr(ctx.c.err, std::string(failed_call).substr(0, strcspn(failed_call, " ")).c_str()) && strstr(ctx.c.err, "injected failure"));
        // nothing is in flight once the call has returned: every enqueued copy was followed by a synchronise that ran while its landing area was alive
        CHECK(pending.empty());
        CHECK(last_of("hipMemcpyAsync D2H") == 0 || last_of("hipStreamSynchronize") > last_of("hipMemcpyAsync D2H"));
        CHECK(ctx.c.lock.try_lock());
        ctx.c.lock.unlock();
        // the same context serves the next call
        memset(b.out, 0xEE, b.n);
        reset_runtime(0);
        CHECK(model_driver(&ctx.c, j, nullptr) == BU_OK && b.right() && j.extra == 0xC0FFEEu && pending.empty());
    }
    CHECK(n_calls >= 5);
    return n_calls;
}

// ---- (c) the status words ---------------------------------------------------------------------------------------------------------------
void check_status()
{
    struct Case { std::vector<uint64_t> reports; bu_status want; uint64_t bad; };
    const uint64_t clear = BU_STATUS_WORD_CLEAR;
    const Case cases[] = {{{clear}, BU_OK, 99},
                          {{clear, clear, clear}, BU_OK, 99},
                          {{clear, (uint64_t)5 << 8 | BU_ERR_INVALID_PATTERN, (uint64_t)1 << 8 | BU_ERR_INVALID_MODE}, BU_ERR_INVALID_PATTERN, 5},
                          {{(uint64_t)7 << 8 | BU_ERR_INDEX_RANGE, clear}, BU_ERR_INDEX_RANGE, 7},
                          {{clear, clear, (uint64_t)0x123456789 << 8 | BU_ERR_INVALID_MODE}, BU_ERR_INVALID_MODE, 0x123456789},
                          {{clear, 0, (uint64_t)1 << 8 | BU_ERR_INVALID_MODE}, BU_ERR_ARGUMENT, 99}};  // (a word nobody reset or reported)
    for (const Case& c : cases) {
        Ctx ctx;
        Buffers b(65, false, false);
        Job j{b.in, b.out, b.n, c.reports};
        uint64_t bad = 99;
        reset_runtime(0);
        CHECK(model_driver(&ctx.c, j, &bad) == c.want && bad == c.bad && b.right() && pending.empty());
    }
    printf("status ok\n");
}

// ---- (d) a page-locked buffer whose device view is not aligned as the step asks is staged -------------------------------------------------
void check_alignment()
{
    struct Case { size_t shift, align; bool mapped; };
    // (8 bytes in: refused by bu_device_view itself, the kernels move 16-byte vectors; 16 and 64 bytes in: by the step's own alignment)
    const Case cases[] = {{0, 16, true}, {8, 16, false}, {8, 4, false}, {16, 16, true}, {16, 64, false}, {64, 64, true}, {64, 256, false}};
    for (const Case& c : cases) {
        Ctx ctx;
        Buffers b(65, true, true, c.shift);
        Job j{b.in, b.out, b.n, {BU_STATUS_WORD_CLEAR}, c.align};
        reset_runtime(0);
        CHECK(model_driver(&ctx.c, j, nullptr) == BU_OK && b.right() && pending.empty());
        CHECK(j.in_mapped == c.mapped && j.out_mapped == c.mapped);
        // staged: both device buffers and the aux buffer, an upload and three downloads; mapped: the aux buffer and two downloads
        size_t mallocs = 0, d2h = 0;
        for (const std::string& s : calls) mallocs += s == "hipMalloc", d2h += s.compare(0, 18, "hipMemcpyAsync D2H") == 0;
        CHECK(mallocs == (c.mapped ? 1u : 3u) && d2h == (c.mapped ? 2u : 3u));
    }
    printf("alignment ok\n");
}
}  // namespace

int main()
{
    check_order();
    int total = 0;
    for (int mapping = 0; mapping < 4; mapping++)
        for (int grow = 0; grow < 2; grow++) total += check_failures(mapping, grow != 0);
    printf("failures ok: %d injected\n", total);
    check_status();
    check_alignment();
    printf("staged call check done\n");
    return 0;
}
