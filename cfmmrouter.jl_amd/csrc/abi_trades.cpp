// abi_trades.cpp -- what a materialising sweep leaves behind (include/cfmm_amd.h): the trades r.Δs / r.Λs of
// src/router.jl:7-8 as host arrays (cfmm_get_trades*) or device arrays (cfmm_trades_dev), update_reserves!
// (src/router.jl:127-132) on the device, and the pool state read-back.
#include "ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

// Device arrays in the reference's layout ({Δ₁, Δ₂} / {Λ₁, Λ₂} per pool) for the trades currently on the device:
// the plain buffers themselves, or the expansion of the compact records (one kernel, asynchronous on the stream).
int expanded_trades(cfmm_ctx* c, const double2** dD, const double2** dL)
{
    if (!c->trades_compact) {
        *dD = c->d_delta.get();
        *dL = c->d_lambda.get();
        return CFMM_OK;
    }
    const size_t rows = (size_t)c->trade_rows;
    if (rows > c->d_xdelta.size() || rows > c->d_xlambda.size()) {
        c->x_valid = false;
        int rc;
        if ((rc = c->d_xdelta.grow(c, rows)) || (rc = c->d_xlambda.grow(c, rows))) return rc;
    }
    if (!c->x_valid && c->have_trades) {
        hipError_t e = launch_expand_trades(c->d_delta.get(), c->d_lambda.get(), c->d_over.get(), c->d_xdelta.get(), c->d_xlambda.get(),
                                            c->trade_rows, c->stream);
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "expand launch failed: %s", hipGetErrorString(e));
        c->x_valid = true;
    }
    *dD = c->d_xdelta.get();
    *dL = c->d_xlambda.get();
    return CFMM_OK;
}

// D2H of trade rows [row0, row0 + count) into Delta / Lambda ([count][2] each, either may be null).
// Round 2 copied the 16-byte records into a pageable vector and decoded them on one thread (8 ms per 1M pools, and two
// more full copies whenever a single pool had used the overflow rows).  Now the records are expanded on the DEVICE
// (expand_trades: 0.03 ms per 1M pools, overflow rows included) and the two result arrays stream to the host in 1 MiB
// chunks through pinned double buffers: kThreads workers, each with its own stream, overlap the PCIe copies with the
// copies from the pinned slots into the caller's (pageable) arrays -- the part that bounds the call.
int download_trades(cfmm_ctx* c, int64_t row0, int64_t count, double* Delta, double* Lambda)
{
    if (count == 0 || (!Delta && !Lambda)) return CFMM_OK;
    const double2 *dD = nullptr, *dL = nullptr;
    int rc = expanded_trades(c, &dD, &dL);
    if (rc != CFMM_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the sweep and the expansion have completed
    if (count < 2 * TradeStaging::kChunkRows) {     // small ranges: plain copies
        if (Delta) HIP_TRY(c, hipMemcpy(Delta, dD + row0, (size_t)count * sizeof(double2), hipMemcpyDeviceToHost));
        if (Lambda) HIP_TRY(c, hipMemcpy(Lambda, dL + row0, (size_t)count * sizeof(double2), hipMemcpyDeviceToHost));
        return CFMM_OK;
    }
    rc = c->tstage.ensure(c);
    if (rc != CFMM_OK) return rc;
    struct Chunk { const double2* src; double* dst; int64_t rows; };
    std::vector<Chunk> chunks;
    for (int arr = 0; arr < 2; ++arr) {
        const double2* src = (arr == 0 ? dD : dL) + row0;
        double* dst = arr == 0 ? Delta : Lambda;
        if (!dst) continue;
        for (int64_t r = 0; r < count; r += TradeStaging::kChunkRows)
            chunks.push_back({src + r, dst + 2 * r, std::min<int64_t>(TradeStaging::kChunkRows, count - r)});
    }
    TradeStaging& t = c->tstage;
    const int device = c->device;
    std::vector<hipError_t> errs((size_t)TradeStaging::kThreads, hipSuccess);
    auto work = [&](int k) {
        hipError_t e = hipSetDevice(device);
        // chunks k, k + T, k + 2T, ...: the copy of the next chunk is in flight while this one is moved out of its slot
        std::vector<size_t> mine;
        for (size_t j = (size_t)k; j < chunks.size(); j += TradeStaging::kThreads) mine.push_back(j);
        auto issue = [&](size_t idx) {
            const Chunk& ch = chunks[mine[idx]];
            const int s = (int)(idx % TradeStaging::kSlots);
            hipError_t ee = hipMemcpyAsync(t.slot[k][s].host(), ch.src, (size_t)ch.rows * sizeof(double2), hipMemcpyDeviceToHost, t.stream[k].get());
            if (ee == hipSuccess) ee = hipEventRecord(t.done[k][s].get(), t.stream[k].get());
            return ee;
        };
        if (e == hipSuccess && !mine.empty()) e = issue(0);
        for (size_t idx = 0; idx < mine.size() && e == hipSuccess; ++idx) {
            if (idx + 1 < mine.size()) e = issue(idx + 1);
            if (e != hipSuccess) break;
            const int s = (int)(idx % TradeStaging::kSlots);
            e = hipEventSynchronize(t.done[k][s].get());
            if (e != hipSuccess) break;
            const Chunk& ch = chunks[mine[idx]];
            std::memcpy(ch.dst, t.slot[k][s].host(), (size_t)ch.rows * sizeof(double2));
        }
        if (e != hipSuccess) (void)hipStreamSynchronize(t.stream[k].get());
        errs[(size_t)k] = e;
    };
    std::vector<std::thread> helpers;
    for (int k = 1; k < TradeStaging::kThreads; ++k) helpers.emplace_back(work, k);
    work(0);
    for (auto& th : helpers) th.join();
    for (hipError_t e : errs)
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "trade download failed: %s", hipGetErrorString(e));
    return CFMM_OK;
}

// Rows [first, first + count) of a weighted segment's coin-major [n_coins][m] array, transposed into the caller's
// [count][n_coins] rows (the reference's per-pool vectors, coins in Ai order).
int download_coin_major(cfmm_ctx* c, const double* src, int64_t m, int nc, int64_t first, int64_t count, double* dst)
{
    if (!dst || count == 0) return CFMM_OK;
    std::vector<double> col((size_t)count);
    for (int k = 0; k < nc; ++k) {
        HIP_TRY(c, hipMemcpy(col.data(), src + (size_t)k * (size_t)m + (size_t)first, (size_t)count * sizeof(double),
                             hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < count; ++i) dst[(size_t)i * (size_t)nc + (size_t)k] = col[(size_t)i];
    }
    return CFMM_OK;
}

int download_segment(cfmm_ctx* c, const Segment& s, int64_t first, int64_t count, double* Delta, double* Lambda)
{
    if (!ragged_kind(s.kind)) return download_trades(c, s.trade_off + first, count, Delta, Lambda);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = download_coin_major(c, s.nc.D.get(), s.m, s.n_coins, first, count, Delta);
    return rc != CFMM_OK ? rc : download_coin_major(c, s.nc.L.get(), s.m, s.n_coins, first, count, Lambda);
}

} // namespace

extern "C" {

int cfmm_get_trades_range(cfmm_ctx* c, int32_t seg, int64_t first, int64_t count, double* Delta, double* Lambda)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) return multi_get_trades_range(c, seg, first, count, Delta, Lambda);
    if (!c->have_trades) return fail(c, CFMM_ERR_STATE, "no materialised trades: call cfmm_find_arb first");
    if (seg < 0 || seg >= (int32_t)c->segs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    const Segment& s = c->segs[(size_t)seg];
    if (first < 0 || count < 0 || first + count > s.m) return fail(c, CFMM_ERR_INVALID_ARG, "row range out of bounds");
    if (count == 0) return CFMM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    return download_segment(c, s, first, count, Delta, Lambda);
}

int cfmm_get_trades(cfmm_ctx* c, double* Delta, double* Lambda)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->have_trades) return fail(c, CFMM_ERR_STATE, "no materialised trades: call cfmm_find_arb first");
    if (c->m_total == 0) return CFMM_OK;
    if (!c->shards.empty()) {
        for (size_t k = 0; k < c->psegs.size(); ++k) {
            const auto& ps = c->psegs[k];
            const int rc = multi_get_trades_range(c, (int32_t)k, 0, ps.m, Delta ? Delta + ps.flat_off : nullptr,
                                                  Lambda ? Lambda + ps.flat_off : nullptr);
            if (rc != CFMM_OK) return rc;
        }
        return CFMM_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->any_ragged) return download_trades(c, 0, c->trade_rows, Delta, Lambda);
    // ragged layout (cfmm_trades_len): segment after segment, n_coins doubles per pool
    for (const Segment& s : c->segs) {
        const int rc = download_segment(c, s, 0, s.m, Delta ? Delta + s.flat_off : nullptr, Lambda ? Lambda + s.flat_off : nullptr);
        if (rc != CFMM_OK) return rc;
    }
    return CFMM_OK;
}

// Three launches on the context's stream behind the sweep (select_kernels.h), one synchronisation, then exactly
// min(count, capacity) rows of every requested output come back.  Reads the trades; changes nothing the other calls see.
int cfmm_select_trades(cfmm_ctx* c, int32_t seg, const double* v, double min_value, int64_t capacity, int64_t* count, int64_t* idx,
                       double* Delta, double* Lambda, double* value)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) return multi_select_trades(c, seg, v, min_value, capacity, count, idx, Delta, Lambda, value);
    if (!c->have_trades) return fail(c, CFMM_ERR_STATE, "no materialised trades: call cfmm_find_arb first");
    if (seg < 0 || seg >= (int32_t)c->segs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    if (capacity < 0 || !count) return fail(c, CFMM_ERR_INVALID_ARG, "cfmm_select_trades: capacity must be >= 0 and count non-null");
    if (!v) {
        if ((int)c->trade_v.size() != c->n)
            return fail(c, CFMM_ERR_STATE, "cfmm_select_trades: v is null and the trades come from cfmm_sweep_dev, whose prices the "
                                           "library has not seen: pass the prices to value the trades at");
        v = c->trade_v.data();
    }
    const Segment& s = c->segs[(size_t)seg];
    *count = 0;
    if (s.m == 0) return CFMM_OK;
    const bool ragged = ragged_kind(s.kind);
    const int nc = ragged ? s.n_coins : 2;
    const size_t blocks = (size_t)select_blocks(s.m);
    const int64_t rows = std::min(capacity, s.m);   // what the emit may write
    const bool emit = rows > 0 && (idx || Delta || Lambda || value);
    HIP_TRY(c, hipSetDevice(c->device));
    SelectScratch& sc = c->sel;
    int rc;
    if ((rc = sc.mask.grow(c, blocks * (kSelBlock / 64))) || (rc = sc.counts.grow(c, blocks)) || (rc = sc.base.grow(c, blocks)) ||
        (rc = sc.v.grow(c, (size_t)c->n)))
        return rc;
    if (emit && ((idx && (rc = sc.idx.grow(c, (size_t)rows))) || (Delta && (rc = sc.D.grow(c, (size_t)rows * nc))) ||
                 (Lambda && (rc = sc.L.grow(c, (size_t)rows * nc))) || (value && (rc = sc.value.grow(c, (size_t)rows)))))
        return rc;
    if ((rc = sc.total.grow(c, 16, true)) != CFMM_OK) return rc;   // (its own 128-byte line)
    if (!sc.total.dev()) {
        sc.total.reset();
        return fail(c, CFMM_ERR_HIP, "cfmm_select_trades: pinned host memory is not device-mapped");
    }
    const bool timed = c->opt_time_kernels != 0;
    hipEvent_t sel_ev[6] = {};
    for (int k = 0; k < 6 && timed; ++k) {
        if ((rc = sc.ev[k].create(c, hipEventDefault)) != CFMM_OK) return rc;
        sel_ev[k] = sc.ev[k].get();
    }
    // the prices: uploaded per call (n doubles; a pageable source is staged by the runtime before the call returns)
    HIP_TRY(c, hipMemcpyAsync(sc.v.get(), v, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SelectArgs a{};
    a.m = s.m;
    a.n_coins = nc;
    a.v = sc.v.get();
    a.min_value = min_value;
    if (ragged) {
        a.ncD = s.nc.D.get();
        a.ncL = s.nc.L.get();
        a.nctok = s.nc.tok.get();
    } else {
        a.Delta = c->d_delta.get() + s.trade_off;
        a.Lambda = c->d_lambda.get() + s.trade_off;
        a.Over = c->d_over.get() + s.trade_off;
        a.compact = c->trades_compact;
        a.pk = s.pk.get();
        a.Ai = s.Ai.get();
    }
    a.mask = sc.mask.get();
    a.counts = sc.counts.get();
    a.base = sc.base.get();
    a.capacity = rows;
    a.out_idx = idx ? sc.idx.get() : nullptr;
    a.out_D = Delta ? sc.D.get() : nullptr;
    a.out_L = Lambda ? sc.L.get() : nullptr;
    a.out_value = value ? sc.value.get() : nullptr;
    *sc.total.host() = -1;
    hipError_t e = launch_select_count(a, ragged, sc.total.dev(), c->stream, timed ? sel_ev : nullptr);
    if (e == hipSuccess && emit) e = launch_select_emit(a, ragged, c->stream, timed ? sel_ev : nullptr);
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "select launch failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t total = *static_cast<volatile long long*>(sc.total.host());
    if (total < 0 || total > s.m) return fail(c, CFMM_ERR_HIP, "cfmm_select_trades: the count did not arrive");
    if (timed)
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            sc.ns[k] = 0;
            if (k == 2 && !emit) continue;
            HIP_TRY(c, hipEventElapsedTime(&ms, sel_ev[2 * k], sel_ev[2 * k + 1]));
            sc.ns[k] = (int64_t)((double)ms * 1e6);
        }
    *count = total;
    const size_t w = (size_t)std::min(total, rows);   // rows to copy back: exactly these, and nothing when there are none
    if (!emit || w == 0) return CFMM_OK;
    if (idx) HIP_TRY(c, hipMemcpy(idx, sc.idx.get(), w * sizeof(long long), hipMemcpyDeviceToHost));
    if (Delta) HIP_TRY(c, hipMemcpy(Delta, sc.D.get(), w * nc * sizeof(double), hipMemcpyDeviceToHost));
    if (Lambda) HIP_TRY(c, hipMemcpy(Lambda, sc.L.get(), w * nc * sizeof(double), hipMemcpyDeviceToHost));
    if (value) HIP_TRY(c, hipMemcpy(value, sc.value.get(), w * sizeof(double), hipMemcpyDeviceToHost));
    return CFMM_OK;
}

int64_t cfmm_trades_len(const cfmm_ctx* c)
{
    if (!c) return 0;
    int64_t len = 0;
    for (const Segment& s : c->segs) len += s.m * (ragged_kind(s.kind) ? s.n_coins : 2);
    for (const auto& ps : c->psegs) len += ps.m * ps.n_coins;
    return len;
}

int cfmm_trades_dev(cfmm_ctx* c, const double** d_delta, const double** d_lambda)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    CFMM_SINGLE_ONLY(c, "cfmm_trades_dev");
    int rc = ensure_geometry(c);
    if (rc != CFMM_OK) return rc;
    if (c->any_ragged)
        return fail(c, CFMM_ERR_UNSUPPORTED, "cfmm_trades_dev: the market has weighted or Curve pools, whose trades are ragged and kept "
                                             "per segment (use cfmm_get_trades / cfmm_get_trades_range)");
    HIP_TRY(c, hipSetDevice(c->device));
    // device consumers get the reference's layout: the compact records of the latest materialising sweep are
    // expanded (asynchronously, on the context's stream) into {Δ₁, Δ₂} / {Λ₁, Λ₂} arrays -- call again after
    // every sweep whose trades are wanted
    if (!c->have_trades) c->trades_compact = (c->opt_compact_trades != 0 && !global_bins(c)) ? 1 : 0;
    const double2 *dD = nullptr, *dL = nullptr;
    rc = expanded_trades(c, &dD, &dL);
    if (rc != CFMM_OK) return rc;
    if (d_delta) *d_delta = reinterpret_cast<const double*>(dD);
    if (d_lambda) *d_lambda = reinterpret_cast<const double*>(dL);
    return CFMM_OK;
}

int cfmm_update_reserves(cfmm_ctx* c)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {
        if (!c->have_trades) return fail(c, CFMM_ERR_STATE, "no materialised trades: call cfmm_find_arb / cfmm_route first");
        for (size_t d = 0; d < c->shards.size(); ++d) {
            cfmm_ctx* child = c->shards[d];
            if (child->segs.empty()) continue;
            const int rc = cfmm_update_reserves(child);
            if (rc != CFMM_OK) {
                c->have_trades = c->have_out = false;   // some shards have moved: the trades describe no consistent market any more
                return fail(c, rc, "shard %d: %s", (int)d, child->err.c_str());
            }
        }
        c->have_trades = c->have_out = false;
        return CFMM_OK;
    }
    if (!c->have_trades) return fail(c, CFMM_ERR_STATE, "no materialised trades: call cfmm_find_arb / cfmm_route first");
    bool any_univ3 = false;
    for (const Segment& s : c->segs) any_univ3 = any_univ3 || s.kind == CFMM_KIND_UNIV3;
    if (any_univ3 && (int)c->trade_v.size() != c->n)
        return fail(c, CFMM_ERR_STATE, "UniV3 pools need the prices of the trades: run the materialising sweep through "
                                       "cfmm_find_arb / cfmm_route (host pointer), not cfmm_sweep_dev");
    HIP_TRY(c, hipSetDevice(c->device));
    // Phase 1 (no side effects): the replacement of every UniV3 segment.  The pool's state is its price: find_arb!
    // (src/cfmms.jl:339-395) moves a trading pool to the internal price P = p/γ (price falling, :361) or γ·p (price
    // rising, :381 in the flipped frame), p = v₁/v₂ -- through every fully drained tick and part of the last one -- and
    // leaves a pool inside its no-arbitrage band (:347-349) alone.  P above the first tick means the pool ran out of
    // liquidity on that side and rests at the first tick's upper price.  Tick constants are then re-derived exactly
    // as at upload (compute_at_tick, :294-313).  A failure here leaves the context untouched (the call can be retried).
    struct Fresh {
        UniV3State u;
        int fast_ok = 0;
        std::vector<double> cp;
    };
    std::vector<Fresh> fresh(c->segs.size());   // (releases what it still holds on every early return)
    const double* v = c->trade_v.data();
    for (size_t k = 0; k < c->segs.size(); ++k) {
        Segment& s = c->segs[k];
        if (s.kind != CFMM_KIND_UNIV3) continue;
        const LadderStore::Csr lad = s.lad.csr();   // (re-tightened first when cfmm_pools_set_ticks has replaced ladders)
        std::vector<double>& cp = fresh[k].cp;
        cp = s.h_cp;
        for (int64_t i = 0; i < s.m; ++i) {
            const double g = s.h_gamma[(size_t)i], q = s.h_cp[(size_t)i];
            const double pr = v[s.h_ai[(size_t)(2 * i)]] / v[s.h_ai[(size_t)(2 * i + 1)]];   // :340
            if (g * q <= pr && pr <= q / g) continue;                                        // :347-349
            const double P = pr < g * q ? pr / g : g * pr;
            const double top = lad.lower_ticks[lad.tick_off[i]];
            cp[(size_t)i] = P > top ? top : P;
        }
        const int rc = univ3_build(c, fresh[k].u, fresh[k].fast_ok, s.m, cp.data(), s.h_gamma.data(), s.h_ai.data(),
                                   lad.tick_off, lad.lower_ticks, lad.liquidity);
        if (rc != CFMM_OK) return rc;
    }
    // Phase 2: R <- R + γΔ − Λ for the two-coin families on the device (no host traffic); from the first launch on the
    // trades count as consumed, so that a failure cannot lead to a second application of the same trades.
    c->have_trades = false;
    c->have_out = false;
    DevBuf<int> d_left;   // per segment: 1 = a new reserve left the operand window of the fast arithmetic
    std::vector<int> left(c->segs.size(), 0);
    if (d_left.alloc(c, c->segs.size()) != CFMM_OK ||
        hipMemsetAsync(d_left.get(), 0, c->segs.size() * sizeof(int), c->stream) != hipSuccess) {
        (void)hipGetLastError();
        c->trade_v.clear();
        return fail(c, CFMM_ERR_HIP, "update_reserves: scratch allocation failed");
    }
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < c->segs.size() && e == hipSuccess; ++k) {
        Segment& s = c->segs[k];
        if (s.kind == CFMM_KIND_UNIV3) continue;
        if (ragged_kind(s.kind)) {
            e = launch_update_ncoin(s.kind, s.nc.R.get(), s.nc.q.get(), s.nc.par.get(), s.nc.glg.get(), s.nc.D.get(), s.nc.L.get(),
                                    s.n_coins, s.m, c->stream);
            continue;
        }
        e = launch_update_two_coin(s.R.get(), s.gamma.get(), c->d_delta.get() + s.trade_off, c->d_lambda.get() + s.trade_off,
                                   c->d_over.get() + s.trade_off, c->trades_compact, s.kind == CFMM_KIND_GEOMEAN ? s.lR.get() : nullptr,
                                   s.eta.get(), s.m, d_left.get() + k, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(left.data(), d_left.get(), left.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // also: nothing in flight still reads the old UniV3 constants
    d_left.reset();
    c->trade_v.clear();
    c->x_valid = false;
    if (e != hipSuccess)
        return fail(c, CFMM_ERR_HIP, "update launch failed: %s (two-coin reserves may have moved; the trades are consumed)", hipGetErrorString(e));
    // Phase 3: move in the UniV3 replacements (cannot fail); the move assignment releases exactly what it replaces.
    for (size_t k = 0; k < c->segs.size(); ++k) {
        Segment& s = c->segs[k];
        if (s.kind != CFMM_KIND_UNIV3) {
            if (left[k]) s.fast_ok = 0;
            continue;
        }
        s.u = std::move(fresh[k].u);
        c->desc_dirty = true;   // the sweep descriptors hold the replaced arrays
        s.fast_ok = fresh[k].fast_ok;
        s.h_cp.swap(fresh[k].cp);
    }
    return CFMM_OK;
}

int cfmm_get_reserves(cfmm_ctx* c, int32_t seg, double* R)
{
    if (!c || !R) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {
        if (seg < 0 || seg >= (int32_t)c->psegs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
        const int nd = (int)c->shards.size();
        for (int d = 0; d < nd; ++d) {
            int64_t lo, hi;
            shard_range(c->psegs[(size_t)seg].m, d, nd, lo, hi);
            if (hi == lo) continue;
            const int rc = cfmm_get_reserves(c->shards[(size_t)d], child_segment(c, seg, d), R + c->psegs[(size_t)seg].n_coins * lo);
            if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, c->shards[(size_t)d]->err.c_str());
        }
        return CFMM_OK;
    }
    if (seg < 0 || seg >= (int32_t)c->segs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    const Segment& s = c->segs[(size_t)seg];
    if (s.kind == CFMM_KIND_UNIV3) return fail(c, CFMM_ERR_INVALID_ARG, "UniV3 segments have prices, not reserves: cfmm_get_prices");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ragged_kind(s.kind)) return download_coin_major(c, s.nc.R.get(), s.m, s.n_coins, 0, s.m, R);   // [m][n_coins]
    HIP_TRY(c, hipMemcpy(R, s.R.get(), (size_t)s.m * sizeof(double2), hipMemcpyDeviceToHost));
    return CFMM_OK;
}

int cfmm_get_prices(cfmm_ctx* c, int32_t seg, double* current_price)
{
    if (!c || !current_price) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {
        if (seg < 0 || seg >= (int32_t)c->psegs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
        const int nd = (int)c->shards.size();
        for (int d = 0; d < nd; ++d) {
            int64_t lo, hi;
            shard_range(c->psegs[(size_t)seg].m, d, nd, lo, hi);
            if (hi == lo) continue;
            const int rc = cfmm_get_prices(c->shards[(size_t)d], child_segment(c, seg, d), current_price + lo);
            if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, c->shards[(size_t)d]->err.c_str());
        }
        return CFMM_OK;
    }
    if (seg < 0 || seg >= (int32_t)c->segs.size()) return fail(c, CFMM_ERR_INVALID_ARG, "segment out of range");
    const Segment& s = c->segs[(size_t)seg];
    if (s.kind != CFMM_KIND_UNIV3) return fail(c, CFMM_ERR_INVALID_ARG, "not a UniV3 segment: cfmm_get_reserves");
    std::copy(s.h_cp.begin(), s.h_cp.end(), current_price);
    return CFMM_OK;
}

} // extern "C"
