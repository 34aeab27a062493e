// abi_context.cpp -- context life cycle, options, streams, introspection (include/cfmm_amd.h).
#include "path_rig.h"

#include <cstdlib>
#include <cstring>

using namespace cfmm;

namespace cfmm {

thread_local std::string g_create_error = "";

// Kernel arguments in device memory: measured 22.2 vs 24.9 us per config-3 step and 7.0 vs 9.1 us per config-2
// step against host-memory kernargs (r01).  The HIP runtime reads the variable when it initialises, so it is
// set when this library is loaded -- unless the caller has decided otherwise (an existing value is kept).
__attribute__((constructor)) static void cfmm_default_environment() { setenv("HIP_FORCE_DEV_KERNARG", "1", 0); }

int fail(const cfmm_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

// Every raw create and destroy of the library's own resources, each the only caller of its HIP function: device arrays
// (DevBuf, devbuf.h), pinned memory, events and streams (PinnedBuf, Event, Stream, hostres.h).  The hooks build counts the
// live ones per family (read-only options "debug_live_allocs" / "_pinned" / "_events" / "_streams"; tests/test_gpu_ownership.py).
enum { kLiveAllocs, kLivePinned, kLiveEvents, kLiveStreams, kLiveFamilies };
#ifdef CFMM_TEST_HOOKS
static std::atomic<int64_t> g_live[kLiveFamilies];
static void count(int family, int by) { g_live[family] += by; }
#else
static void count(int, int) {}
#endif

// a failed create leaves *p null and no sticky error behind
template <class T>
static hipError_t created(hipError_t e, T* p, int family)
{
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
    } else {
        count(family, 1);
    }
    return e;
}

static std::atomic<uint64_t> g_resource_epoch{1};
uint64_t resource_epoch() { return g_resource_epoch.load(std::memory_order_relaxed); }
static void moved() { g_resource_epoch.fetch_add(1, std::memory_order_relaxed); }

hipError_t dev_alloc(void** p, size_t bytes) { moved(); return created(hipMalloc(p, bytes), p, kLiveAllocs); }
hipError_t dev_alloc_fine(void** p, size_t bytes) { moved(); return created(hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained), p, kLiveAllocs); }
void dev_free(void* p) { moved(); (void)hipFree(p); count(kLiveAllocs, -1); }

hipError_t pinned_alloc(void** h, void** d, size_t bytes, bool mapped)
{
    *d = nullptr;
    moved();
    const hipError_t e = created(hipHostMalloc(h, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault), h, kLivePinned);
    if (e == hipSuccess && mapped && hipHostGetDevicePointer(d, *h, 0) != hipSuccess) {
        (void)hipGetLastError();
        *d = nullptr;
    }
    return e;
}
void pinned_free(void* h) { moved(); (void)hipHostFree(h); count(kLivePinned, -1); }

hipError_t event_create(hipEvent_t* e, unsigned flags) { return created(hipEventCreateWithFlags(e, flags), e, kLiveEvents); }
void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); count(kLiveEvents, -1); }

hipError_t stream_create(hipStream_t* s) { return created(hipStreamCreateWithFlags(s, hipStreamNonBlocking), s, kLiveStreams); }
void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); count(kLiveStreams, -1); }

int HostStage::alloc(const cfmm_ctx* c, int n_tokens)
{
    n = n_tokens;
    gran_off = (size_t)((2 * n + 2 + 15) & ~15);
    flag_off = gran_off + 2 * (size_t)((n + 1 + 7) & ~7);
    const int rc = buf.alloc(c, flag_off + 16, true);
    if (rc == CFMM_OK) std::memset(buf.host(), 0, buf.size() * sizeof(double));
    return rc;
}

// optional: without a large BAR (or with CFMM_AMD_ARMED=0, or when the self-check fails) the buffer stays empty
void ArmState::alloc(int device, int n_tokens, int n_padded)
{
    n = n_tokens;
    n_pad = n_padded;
    int large_bar = 0;
    const char* env = std::getenv("CFMM_AMD_ARMED");
    if ((env && env[0] == '0') || hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess || large_bar == 0) return;
    const size_t words = (size_t)n_pad + 8;
    if (!buf.alloc_fine(words)) return;
    // self-check: what the host stores must be what the device holds
    std::vector<double> probe(words), back(words, 0.0);
    for (size_t j = 0; j < words; ++j) probe[j] = 1.0 + (double)j;
    std::memcpy(buf.get(), probe.data(), words * sizeof(double));
    __builtin_ia32_sfence();
    if (hipMemcpy(back.data(), buf.get(), words * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess || back != probe) {
        (void)hipGetLastError();
        buf.reset();
        return;
    }
    std::memset(buf.get(), 0, words * sizeof(double));
    __builtin_ia32_sfence();
}

int KernelTimer::harvest(cfmm_ctx* c, int64_t* sweep_launches, double* sweep_ms_out, int64_t* reduce_launches, double* reduce_ms_out)
{
    for (auto& p : pending) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, p.a, p.b));
        if (p.what == 0) { sweep_n++; sweep_ms += ms; }
        else { reduce_n++; reduce_ms += ms; }
    }
    pending.clear();
    used = 0;
    if (sweep_launches) *sweep_launches = sweep_n;
    if (sweep_ms_out) *sweep_ms_out = sweep_ms;
    if (reduce_launches) *reduce_launches = reduce_n;
    if (reduce_ms_out) *reduce_ms_out = reduce_ms;
    sweep_n = reduce_n = 0;
    sweep_ms = reduce_ms = 0;
    return CFMM_OK;
}

} // namespace cfmm

extern "C" {

const char* cfmm_version(void) { return "cfmm_amd 0.6.0 (gfx950)"; }

const char* cfmm_last_error(const cfmm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int cfmm_ctx_create(int device_id, int32_t n_tokens, cfmm_ctx** out)
{
    if (!out) return fail(nullptr, CFMM_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (n_tokens < 1) return fail(nullptr, CFMM_ERR_INVALID_ARG, "n_tokens must be >= 1");
    if (n_tokens > (1 << 26))
        return fail(nullptr, CFMM_ERR_UNSUPPORTED, "n_tokens %d exceeds the supported maximum %d", n_tokens, 1 << 26);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, CFMM_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= count)
        return fail(nullptr, CFMM_ERR_INVALID_ARG, "device_id %d out of range [0, %d)", device_id, count);
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CFMM_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 only", device_id,
                    prop.gcnArchName);
    HIP_TRY(nullptr, hipSetDevice(device_id));

    cfmm_ctx* c = new cfmm_ctx();
    c->device = device_id;
    c->n = n_tokens;
    c->n_pad = n_pad_of(n_tokens);
    auto bail = [&](int code) {
        g_create_error = c->err;
        cfmm_ctx_destroy(c);
        return code;
    };
#define HIP_TRY_C(expr)                                                                               \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            fail(c, CFMM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));                     \
            return bail(CFMM_ERR_HIP);                                                                \
        }                                                                                             \
    } while (0)
    if (c->own_stream.create(c) != CFMM_OK) return bail(CFMM_ERR_HIP);
    c->stream = c->own_stream.get();
    if (c->d_v.alloc(c, (size_t)c->n) != CFMM_OK || c->d_out.alloc(c, (size_t)c->n + 1) != CFMM_OK || c->stage.alloc(c, c->n) != CFMM_OK)
        return bail(CFMM_ERR_HIP);
    c->arm.alloc(c->device, c->n, c->n_pad);
    // the dynamic-LDS ceiling is a per-function, process-wide attribute: always raise it to the
    // full 160 KiB so that contexts with different n_tokens cannot shrink each other's limit
    HIP_TRY_C(prepare_kernels(160 * 1024));
#undef HIP_TRY_C
    *out = c;
    return CFMM_OK;
}

int cfmm_ctx_create_multi(int32_t n_devices, const int32_t* device_ids, int32_t n_tokens, cfmm_ctx** out)
{
    if (!out) return fail(nullptr, CFMM_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (n_devices < 1 || n_devices > 64 || !device_ids)
        return fail(nullptr, CFMM_ERR_INVALID_ARG, "n_devices must be in [1, 64] and device_ids non-null");
    if (n_tokens > kMaxLdsTokens)
        return fail(nullptr, CFMM_ERR_UNSUPPORTED, "multi-device contexts are limited to n_tokens <= %d", kMaxLdsTokens);
    cfmm_ctx* c = new cfmm_ctx();
    c->device = -1;
    c->n = n_tokens;
    c->n_pad = n_pad_of(n_tokens);
    c->workers.reset(new Workers());
    c->workers->rc.assign((size_t)n_devices, CFMM_OK);
    for (int d = 0; d < n_devices; ++d) {
        cfmm_ctx* child = nullptr;
        int rc = cfmm_ctx_create(device_ids[d], n_tokens, &child);   // validates the ordinal, the arch, n_tokens
        if (rc != CFMM_OK) {
            cfmm_ctx_destroy(c);
            return rc;   // g_create_error already holds the message
        }
        for (int e = 0; e < d; ++e)
            if (device_ids[e] == device_ids[d]) c->shards_distinct = false;
        c->shards.push_back(child);
    }
    *out = c;
    return CFMM_OK;
}

int32_t cfmm_device_count(const cfmm_ctx* c) { return c ? (c->shards.empty() ? 1 : (int32_t)c->shards.size()) : 0; }

void cfmm_ctx_destroy(cfmm_ctx* c)
{
    if (!c) return;
    if (c->workers) {
        Workers& w = *c->workers;
        {
            std::lock_guard<std::mutex> lk(w.mu);
            w.quit.store(true);
            w.cv.notify_all();
        }
        for (auto& t : w.threads) t.join();
    }
    if (is_parent(c)) {
        for (cfmm_ctx* child : c->shards) cfmm_ctx_destroy(child);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    armed_cancel(c);
    if (c->stream && c->stream != c->own_stream.get()) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream.get());
    rccl_release(c);          // a communicator created by cfmm_rccl_init_rank goes with the context
    delete c;                 // every member releases what it owns, the own stream last (ctx.h)
}

int cfmm_set_stream(cfmm_ctx* c, void* hip_stream)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    CFMM_SINGLE_ONLY(c, "cfmm_set_stream");
    c->stream = static_cast<hipStream_t>(hip_stream); // NULL is HIP's default (null) stream
    c->desc_dirty = true;   // (the descriptors are uploaded in stream order: again on the new stream)
    return CFMM_OK;
}

int cfmm_reset_stream(cfmm_ctx* c)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    CFMM_SINGLE_ONLY(c, "cfmm_reset_stream");
    c->stream = c->own_stream.get();
    c->desc_dirty = true;
    return CFMM_OK;
}

static int64_t* option_slot(cfmm_ctx* c, const char* key)
{
    if (!key) return nullptr;
    struct { const char* name; int64_t* slot; } table[] = {
        {"max_grid", &c->geo.max_grid}, {"block", &c->geo.block}, {"bin_copies", &c->geo.bin_copies},
        {"time_kernels", &c->opt_time_kernels}, {"geomean_exact", &c->geo.geomean_exact},
        {"fuse_segments", &c->geo.fuse_segments}, {"zero_copy", &c->opt_zero_copy},
        {"alternate", &c->opt_alternate}, {"pack", &c->geo.pack}, {"compact_trades", &c->opt_compact_trades},
        {"fast_math", &c->opt_fast_math}, {"armed", &c->opt_armed}, {"arm_timeout_ms", &c->opt_arm_timeout_ms},
        {"cost_geomean", &c->geo.cost_geomean}, {"cost_univ3", &c->geo.cost_univ3}, {"host_flag", &c->opt_host_flag},
        {"stop_in_noise", &c->opt_stop_in_noise}, {"multi_threads", &c->opt_multi_threads},
        {"dev_prices_in_window", &c->opt_dev_prices_in_window}, {"univ3_heads", &c->opt_univ3_heads}, {"direct_small", &c->geo.direct_small}, {"stream_stores", &c->opt_stream_stores},
        {"find_lds", &c->opt_find_lds}, {"lean_kernels", &c->opt_lean_kernels}, {"size_max_blocks", &c->opt_size_max_blocks},
        {"split_max_blocks", &c->opt_split_max_blocks}, {"order_max_blocks", &c->opt_order_max_blocks},
#ifdef CFMM_TEST_HOOKS
        {"debug_stall_ms", &c->opt_debug_stall_ms},
#endif
    };
    for (auto& t : table)
        if (!std::strcmp(key, t.name)) return t.slot;
    return nullptr;
}

int cfmm_set_option(cfmm_ctx* c, const char* key, int64_t value)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int64_t* slot = option_slot(c, key);
    if (!slot) return fail(c, CFMM_ERR_INVALID_ARG, "unknown option '%s'", key ? key : "(null)");
    if (slot == &c->geo.max_grid && value < 0) return fail(c, CFMM_ERR_INVALID_ARG, "max_grid must be >= 0 (0 = auto)");
    if (slot == &c->geo.block && !(value == 0 || value == kMidBlock || value == kBigBlock))
        return fail(c, CFMM_ERR_INVALID_ARG, "block must be 0 (auto), %d or %d", kMidBlock, kBigBlock);
    if (slot == &c->geo.bin_copies && !(value == 0 || value == 1 || value == 2))
        return fail(c, CFMM_ERR_INVALID_ARG, "bin_copies must be 0 (auto), 1 (shared) or 2 (per wavefront)");
    if (slot == &c->opt_stream_stores && !(value == 0 || value == 1 || value == 2))
        return fail(c, CFMM_ERR_INVALID_ARG, "stream_stores must be 0 (auto), 1 (write-through) or 2 (non-temporal)");
    if (slot == &c->opt_size_max_blocks && value < 1) return fail(c, CFMM_ERR_INVALID_ARG, "size_max_blocks must be >= 1");
    if (slot == &c->opt_split_max_blocks && value < 1) return fail(c, CFMM_ERR_INVALID_ARG, "split_max_blocks must be >= 1");
    if (slot == &c->opt_order_max_blocks && value < 1) return fail(c, CFMM_ERR_INVALID_ARG, "order_max_blocks must be >= 1");
    *slot = value;
    c->desc_dirty = true;   // pack, compact_trades, block, max_grid, fuse_segments, bin_copies, stream_stores, univ3_heads, geomean_exact, cost_*: all copied
    if (slot != &c->opt_multi_threads)
        for (cfmm_ctx* child : c->shards) {
            int rc = cfmm_set_option(child, key, value);
            if (rc != CFMM_OK) return fail(c, rc, "%s", child->err.c_str());
        }
    if (slot == &c->geo.max_grid || slot == &c->geo.block || slot == &c->geo.fuse_segments ||
        slot == &c->geo.geomean_exact || slot == &c->geo.pack ||
        slot == &c->geo.cost_geomean || slot == &c->geo.cost_univ3 || slot == &c->geo.direct_small)
        c->geometry_dirty = true;
    return CFMM_OK;
}

int cfmm_get_option(const cfmm_ctx* c, const char* key, int64_t* value)
{
    if (!c || !value) return CFMM_ERR_INVALID_ARG;
    if (key && !std::strcmp(key, "peer_seq")) {   // read-only: sharded sweeps performed on the current peer buffers
        *value = (int64_t)c->peer_seq;            // (cfmm_set_peers' `seq` to continue from; ranks re-align on the maximum)
        return CFMM_OK;
    }
    if (key && !std::strcmp(key, "pool_update_regrows")) {   // read-only: compactions + regrows of UniV3 tick arrays (cfmm_pools_set_prices)
        *value = c->pool_update_regrows;
        for (const cfmm_ctx* child : c->shards) *value += child->pool_update_regrows;
        return CFMM_OK;
    }
    if (key && !std::strcmp(key, "lean_launches")) {   // read-only: sweep launches that took a lean kernel (sweep_core.h sweep_body<..., LEAN>)
        *value = c->lean_launches;
        for (const cfmm_ctx* child : c->shards) *value += child->lean_launches;
        return CFMM_OK;
    }
    if (key && !std::strcmp(key, "compact_walks_ns")) {   // read-only: the span of the latest compact_walks launch timed under "time_kernels"
        *value = c->shards.empty() ? c->upd.compact_ns : c->shards[0]->upd.compact_ns;
        return CFMM_OK;
    }
    // read-only, cfmm_quote / cfmm_quote_dev: the span of the latest call's kernel timed under "time_kernels".  A parent
    // reports the longest span among the shards its latest call touched (abi_quote.cpp multi_quote).  After cfmm_quote_dev
    // the span is not known until the kernel has run: the read waits for it and stores it, the one thing a getter changes
    if (key && !std::strcmp(key, "quote_ns")) return quote_ns(const_cast<cfmm_ctx*>(c), value);
    // read-only, cfmm_quote_rate / cfmm_quote_path_rate and their _dev forms: the same of the latest call of any of the four
    if (key && !std::strcmp(key, "rate_ns")) return rate_ns(const_cast<cfmm_ctx*>(c), value);
    // read-only, cfmm_quote_to_rate / cfmm_quote_to_rate_dev: the same of the latest call of either
    if (key && !std::strcmp(key, "limit_ns")) return limit_ns(const_cast<cfmm_ctx*>(c), value);
    // read-only, cfmm_swap: the sum of the kernel spans of the latest call's waves timed under "time_kernels" (a parent: the
    // longest among the shards that call touched), and the number of that call's swaps that were not applied (NaN answers)
    if (key && !std::strcmp(key, "swap_ns")) { *value = c->swap.ns; return CFMM_OK; }
    if (key && !std::strcmp(key, "swap_refused")) { *value = c->swap.refused; return CFMM_OK; }
    if (key && !std::strcmp(key, "swap_launches")) { *value = c->swap.launches; return CFMM_OK; }
    // read-only, cfmm_size_path / cfmm_size_path_dev: the latest call's kernel launches (a parent: its cfmm_quote_path calls), and under
    // "time_kernels" its kernel's span (a parent: the sum of its rounds' "quote_ns"); after cfmm_size_path_dev the read waits, as "quote_ns"
    if (key && !std::strcmp(key, "size_launches")) { *value = c->size.launches; return CFMM_OK; }
    cfmm_ctx* const m = const_cast<cfmm_ctx*>(c);   // (a getter that waits for a timed _dev call's span stores it)
    if (key && !std::strcmp(key, "size_ns")) return m->size.read_ns(m, value);
    // read-only, cfmm_split_paths / cfmm_split_paths_out and their _dev forms: the same two of the latest call of either split entry
    if (key && !std::strcmp(key, "split_launches")) { *value = c->split.launches; return CFMM_OK; }
    if (key && !std::strcmp(key, "split_ns")) return m->split.read_ns(m, value);
    // read-only, cfmm_find_path / cfmm_find_path_out (whichever was called last): the latest call's kernel launches, and under
    // "time_kernels" the sums of the spans of its layer launches (find_relax / find_out_relax) and of its walk launches (claim +
    // advance)
    if (key && !std::strcmp(key, "find_launches")) { *value = c->find.launches; return CFMM_OK; }
    if (key && !std::strcmp(key, "find_relax_ns")) { *value = c->find.relax_ns; return CFMM_OK; }
    if (key && !std::strcmp(key, "find_walk_ns")) { *value = c->find.walk_ns; return CFMM_OK; }
    for (int k = 0; k < 3 && key; ++k) {   // ... and layer by layer: "find_relax_ns_3" is layer 3's find_relax
        static const char* const names[3] = {"find_relax_ns_", "find_claim_ns_", "find_advance_ns_"};
        const size_t len = std::strlen(names[k]);
        if (!std::strncmp(key, names[k], len) && key[len] >= '1' && key[len] <= '0' + CFMM_MAX_PATH_HOPS && !key[len + 1]) {
            *value = c->find.layer_ns[k][key[len] - '1'];
            return CFMM_OK;
        }
    }
    for (int k = 0; k < 2 && key; ++k) {   // ... and round by round: "find_round_relax_ns_2" is the second round of cfmm_find_disjoint_paths
        static const char* const names[2] = {"find_round_relax_ns_", "find_round_walk_ns_"};
        const size_t len = std::strlen(names[k]);
        if (!std::strncmp(key, names[k], len) && key[len] >= '1' && key[len] <= '0' + CFMM_MAX_SPLIT_PATHS && !key[len + 1]) {
            *value = c->find.round_ns[k][key[len] - '1'];
            return CFMM_OK;
        }
    }
    // read-only, cfmm_select_trades: its two geometry constants, and the three kernel spans of the latest call timed under
    // option "time_kernels" (a parent reports its first shard's)
    if (key && !std::strcmp(key, "select_block_pools")) { *value = kSelBlock; return CFMM_OK; }
    if (key && !std::strcmp(key, "select_scan_chunk")) { *value = kSelScanChunk; return CFMM_OK; }
    for (int k = 0; k < 3; ++k) {
        static const char* const names[3] = {"select_flag_ns", "select_scan_ns", "select_emit_ns"};
        if (key && !std::strcmp(key, names[k])) {
            *value = c->shards.empty() ? c->sel.ns[k] : c->shards[0]->sel.ns[k];
            return CFMM_OK;
        }
    }
#ifdef CFMM_TEST_HOOKS
    for (int k = 0; k < kLiveFamilies; ++k) {   // read-only, process-wide: resources of one family created and not yet released
        static const char* const names[kLiveFamilies] = {"debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams"};
        if (key && !std::strcmp(key, names[k])) {
            *value = g_live[k].load();
            return CFMM_OK;
        }
    }
#endif
    int64_t* slot = option_slot(const_cast<cfmm_ctx*>(c), key);
    if (!slot) return fail(c, CFMM_ERR_INVALID_ARG, "unknown option '%s'", key ? key : "(null)");
    *value = *slot;
    return CFMM_OK;
}

int64_t cfmm_pools_count(const cfmm_ctx* c)
{
    if (!c) return 0;
    int64_t m = 0;
    for (auto& s : c->segs) m += s.m;
    for (auto& ps : c->psegs) m += ps.m;
    return m;
}

int32_t cfmm_n_tokens(const cfmm_ctx* c) { return c ? c->n : 0; }

int cfmm_kernel_times(cfmm_ctx* c, int64_t* sweep_launches, double* sweep_ms, int64_t* reduce_launches,
                      double* reduce_ms)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {   // totals over the shards
        int64_t sn = 0, rn = 0;
        double sm = 0, rm = 0;
        for (cfmm_ctx* child : c->shards) {
            int64_t a = 0, b = 0;
            double x = 0, y = 0;
            int rc = cfmm_kernel_times(child, &a, &x, &b, &y);
            if (rc != CFMM_OK) return fail(c, rc, "%s", child->err.c_str());
            sn += a; rn += b; sm += x; rm += y;
        }
        if (sweep_launches) *sweep_launches = sn;
        if (sweep_ms) *sweep_ms = sm;
        if (reduce_launches) *reduce_launches = rn;
        if (reduce_ms) *reduce_ms = rm;
        return CFMM_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return c->timer.harvest(c, sweep_launches, sweep_ms, reduce_launches, reduce_ms);
}

int32_t cfmm_segment_count(const cfmm_ctx* c)
{
    return c ? (int32_t)(c->shards.empty() ? c->segs.size() : c->psegs.size()) : 0;
}

int cfmm_segment_info(const cfmm_ctx* c, int32_t seg, int32_t* kind, int64_t* m, int32_t* block, int32_t* grid)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {   // kind and size of the whole segment; launch geometry of shard 0's block
        if (seg < 0 || seg >= (int32_t)c->psegs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
        const int cs = child_segment(c, seg, 0);
        if (cs >= 0) {
            int rc = cfmm_segment_info(c->shards[0], cs, kind, nullptr, block, grid);
            if (rc != CFMM_OK) return rc;
        }
        if (kind) *kind = c->psegs[(size_t)seg].kind;
        if (m) *m = c->psegs[(size_t)seg].m;
        return CFMM_OK;
    }
    if (seg < 0 || seg >= (int32_t)c->segs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    int rc = ensure_geometry(const_cast<cfmm_ctx*>(c));
    if (rc != CFMM_OK) return rc;
    const Segment& s = c->segs[(size_t)seg];
    if (kind) *kind = s.kind;
    if (m) *m = s.m;
    if (block) *block = s.block;
    if (grid) *grid = s.grid;
    return CFMM_OK;
}

} // extern "C"
