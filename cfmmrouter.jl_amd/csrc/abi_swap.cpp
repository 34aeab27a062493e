// abi_swap.cpp -- cfmm_swap and cfmm_swap_out: swaps of one segment's pools that MOVE the pools (include/cfmm_amd.h has the
// contracts).  The two directions share every line here, as abi_quote.cpp's do: a Dir names the entry and its given amount
// in the messages and picks the launcher; `given` / `answer` below are amount_in / amount_out of cfmm_swap and amount_out /
// amount_in of cfmm_swap_out, which adds a limit on the answer and a status per swap.  cfmm_swap_limit (include/cfmm_amd_limit.h)
// is the third direction: cfmm_swap's amounts, a limit on the marginal RATE in the place of cfmm_swap_out's limit, a status per
// swap and one more answer, the amount used (`used` below: non-null exactly for this direction; swap_limit_kernels.h).
// Each exact-input swap answers what cfmm_quote answers on the pool as it stands (swap_kernels.h runs quote_one itself) and
// then leaves the pool at R + γΔ − Λ (src/cfmms.jl:26-31; swap_pool.h: the per-kind forms); each exact-output swap answers
// cfmm_quote_out's bits (swap_out_kernels.h runs quote_out_one) and leaves the pool at R_in + γ·in, R_out − want.  The swaps
// of a batch are applied in query order: the host cuts the batch into waves of distinct rows (swap_waves.h) and launches them
// in stream order.  The reserve kinds synchronise once, at the end; UniV3 -- whose state is its price, with records prepared
// on the host -- reads the wave's landing prices back and moves the pools through cfmm_pools_set_prices' own apply path
// (abi_update.cpp univ3_move_prices) before the next wave.  The only memory of the feature is SwapScratch (ctx.h),
// proportional to the swaps of a call and never to the pools.
#include "../../include/cfmm_amd_limit.h"
#include "seg_view.h"
#include "stage_layout.h"
#include "swap_waves.h"
#include "univ3_pool.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

constexpr Dir kForward{false, "cfmm_swap", nullptr, "amount_in"};
constexpr Dir kInverse{true, "cfmm_swap_out", nullptr, "amount_out"};
constexpr Dir kLimited{false, "cfmm_swap_limit", nullptr, "amount_in", true};

// the kernel's view of segment `s` (seg_view.h), taken afresh per wave: a moved UniV3 pool may have regrown the record
// arrays.  The wave's query arrays are filled in by the caller; `left`: the call's window flag.
hipError_t launch_wave(const cfmm_ctx* c, const Dir& dir, const Segment& s, const SwapLimitArgs& w, int* left, hipEvent_t e0, hipEvent_t e1)
{
    const SwapPathSeg p = swap_path_seg(s, left);
    SwapLimitArgs sl = w;
    SwapOutArgs& so = sl.o;
    swap_view(p, so.s);
    const UniV3Pools u = univ3_view(p.s);
    const NCoinPools n = ncoin_view(p.s);
    if (dir.rated) return launch_swap_limit(s.kind, sl, u, n, c->stream, e0, e1);
    return dir.exact_out ? launch_swap_out(s.kind, so, u, n, c->stream, e0, e1) : launch_swap(s.kind, so.s, u, n, c->stream, e0, e1);
}

// One checked call on a single-device context.  limit, status: cfmm_swap_out's (either may be null); cfmm_swap passes neither;
// cfmm_swap_limit passes its rate limits as `limit` (never null), `used`, and a status that may be null.
int swap_single(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                const int32_t* coin_out, const double* given, const double* limit, double* answer, int32_t* status, double* used)
{
    Segment& s = c->segs[(size_t)seg];
    HIP_TRY(c, hipSetDevice(c->device));
    const SwapPlan plan = swap_plan(count, idx);
    const int64_t waves = (int64_t)plan.wave_off.size() - 1;
    const bool univ3 = s.kind == CFMM_KIND_UNIV3;
    const bool flagged = !univ3 && kind_info(s.kind).has_fast;
    const bool timed = c->opt_time_kernels != 0;
    const bool out = dir.exact_out, lim = dir.rated, stat = out || lim;
    SwapScratch& sc = c->swap;
    const size_t n = (size_t)count;
    const SwapStage lay(n, idx != nullptr, univ3, limit != nullptr, stat, lim);
    int rc;
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.amt.grow(c, n)) || (rc = sc.coins.grow(c, 2 * n)) || (rc = sc.out.grow(c, n)) ||
        (idx && (rc = sc.idx.grow(c, n))) || (univ3 && (rc = sc.price.grow(c, n))) || (flagged && (rc = sc.left.grow(c, 1))) ||
        (limit && (rc = sc.limit.grow(c, n))) || (stat && (rc = sc.status.grow(c, n))) || (lim && (rc = sc.used.grow(c, n))) || (timed && (rc = sc.ev.ensure(c, (size_t)waves))))
        return rc;
    // pinned staging, the swaps in launch order
    unsigned long long* st = sc.stage.host();
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st), *h_price = lay.price.in(st), *h_limit = lay.limit.in(st), *h_used = lay.used.in(st);
    int32_t *h_coins = lay.coins.in(st), *h_status = lay.status.in(st);   // coins: [count] coin_in, then [count] coin_out
    long long* h_idx = lay.idx.in(st);
    int* h_left = lay.left.in(st);
    for (size_t j = 0; j < n; ++j) {
        const size_t q = (size_t)plan.perm[j];
        h_amt[j] = given[q];
        h_coins[j] = coin_in[q];
        if (coin_out) h_coins[n + j] = coin_out[q];
        if (idx) h_idx[j] = idx[q];
        if (limit) h_limit[j] = limit[q];
    }
    *h_left = 0;
    armed_cancel(c);
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.coins.get(), h_coins, (coin_out ? 2 : 1) * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(sc.idx.get(), h_idx, n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    if (limit) HIP_TRY(c, hipMemcpyAsync(sc.limit.get(), h_limit, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (flagged) HIP_TRY(c, hipMemsetAsync(sc.left.get(), 0, sizeof(int), c->stream));
    swap_invalidate(c);   // from the first launch on the pools count as moved
    std::vector<char> refused_at(univ3 && !out ? n : 0, 0);   // UniV3, exact input: the landing price was no state a pool can take
    std::vector<int64_t> rows;
    std::vector<double> prices;
    for (int64_t w = 0; w < waves; ++w) {
        const size_t off = (size_t)plan.wave_off[(size_t)w], nw = (size_t)plan.wave_off[(size_t)w + 1] - off;
        SwapLimitArgs sl{};
        SwapOutArgs& so = sl.o;
        SwapArgs& a = so.s;
        a.q.count = (int64_t)nw;
        a.q.idx = idx ? sc.idx.get() + off : nullptr;
        a.q.coin_in = sc.coins.get() + off;
        a.q.coin_out = coin_out ? sc.coins.get() + n + off : nullptr;
        a.q.amount_in = sc.amt.get() + off;
        a.q.amount_out = sc.out.get() + off;
        a.price = univ3 ? sc.price.get() + off : nullptr;
        so.max_in = limit ? sc.limit.get() + off : nullptr;
        so.status = stat ? sc.status.get() + off : nullptr;
        sl.used = lim ? sc.used.get() + off : nullptr;
        const hipError_t e = launch_wave(c, dir, s, sl, sc.left.get(), sc.ev.start((size_t)w, timed), sc.ev.stop((size_t)w, timed));
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "swap launch failed: %s (earlier waves of the call have moved their pools)", hipGetErrorString(e));
        if (!univ3) continue;
        // the wave's landing prices, 8 bytes per swap (exact output: and its statuses -- only an applied swap moves its pool);
        // then the pools move as cfmm_pools_set_prices moves them
        HIP_TRY(c, hipMemcpyAsync(h_price + off, sc.price.get() + off, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (out) HIP_TRY(c, hipMemcpyAsync(h_status + off, sc.status.get() + off, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rows.clear();
        prices.clear();
        for (size_t j = off; j < off + nw; ++j) {
            const int64_t row = idx ? idx[plan.perm[j]] : plan.perm[j];
            double P;
            if (out) {
                if (h_status[j] != CFMM_SWAP_APPLIED) continue;   // (the kernel has tested the price of an applied swap)
            } else if (!finite_pos(h_price[j])) {   // check_univ3_price would refuse it: the pool stays
                refused_at[j] = 1;
                continue;
            }
            if (!univ3_landing(h_price[j], s.lad.lower_ticks(row)[0], s.h_cp[(size_t)row], P)) continue;   // (a == 0, no liquidity: where it was)
            rows.push_back(row);
            prices.push_back(P);
        }
        if ((rc = univ3_move_prices(c, s, rows, prices.data())) != CFMM_OK) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (stat) HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (lim) HIP_TRY(c, hipMemcpyAsync(h_used, sc.used.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (flagged) HIP_TRY(c, hipMemcpyAsync(h_left, sc.left.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (flagged && *h_left) s.fast_ok = 0;   // (never sent back: as cfmm_update_reserves)
    if (timed && (rc = sc.ev.elapsed_ns(c, 0, (size_t)waves, sc.ns)) != CFMM_OK) return rc;
    int64_t refused = 0;
    for (size_t j = 0; j < n; ++j) {
        const bool held = univ3 && !out && refused_at[j];
        const double o = held ? std::nan("") : h_out[j];
        refused += out ? h_status[j] != CFMM_SWAP_APPLIED : o != o;
        answer[plan.perm[j]] = o;
        if (out && status) status[plan.perm[j]] = h_status[j];
        if (lim) {   // (UniV3: a landing price no pool can take refuses the swap here, as cfmm_swap's)
            used[plan.perm[j]] = held ? std::nan("") : h_used[j];
            if (status) status[plan.perm[j]] = held ? CFMM_LIMIT_REFUSED : h_status[j];
        }
    }
    sc.refused = refused;
    sc.launches = waves;
    return CFMM_OK;
}

// A parent: the swaps go to the shards that hold their rows (shard_range: contiguous blocks in device order), each shard's in
// the caller's order -- a row lives on one shard, so per-row order is kept -- and the answers return in query order, as
// multi_quote.  The caller has run every check there is, for every shard, before any shard changes.
int multi_swap(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* given, const double* limit, double* answer, int32_t* status, double* used)
{
    const int nd = (int)c->shards.size();
    const std::vector<ShardBucket> buckets = split_by_shard(c->psegs[(size_t)seg].m, nd, count, idx);
    c->have_trades = c->have_out = false;
    std::vector<double> out, us;
    std::vector<int32_t> st;
    int64_t ns = 0, refused = 0;
    for (int d = 0; d < nd; ++d) {
        const ShardBucket& bk = buckets[(size_t)d];
        if (bk.where.empty()) continue;
        out.resize(bk.where.size());
        st.resize(bk.where.size());
        us.resize(bk.where.size());
        const std::vector<int32_t> ci = gather(bk.where, coin_in), co = gather(bk.where, coin_out);
        const std::vector<double> amt = gather(bk.where, given), lim = gather(bk.where, limit);
        cfmm_ctx* child = c->shards[(size_t)d];
        const int rc = swap_single(child, dir, child_segment(c, seg, d), (int64_t)bk.where.size(), bk.rows.data(), ci.data(),
                                   coin_out ? co.data() : nullptr, amt.data(), limit ? lim.data() : nullptr, out.data(),
                                   status ? st.data() : nullptr, used ? us.data() : nullptr);
        if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s (some shards may have moved)", d, child->err.c_str());
        scatter(bk.where, out.data(), answer);
        if (used) scatter(bk.where, us.data(), used);
        if (status) scatter(bk.where, st.data(), status);
        if (child->opt_time_kernels != 0) ns = std::max(ns, child->swap.ns);
        refused += child->swap.refused;
    }
    c->swap.ns = ns;   // "swap_ns" of a parent: the longest among the shards THIS call touched
    c->swap.refused = refused;
    c->swap.launches = 0;
    for (const cfmm_ctx* child : c->shards) c->swap.launches += child->swap.launches;   // (of the shards' latest calls)
    return CFMM_OK;
}

// every check of either entry, before anything is enqueued; then the call
// (dir.rated: cfmm_swap_limit, whose `limit` is the rate limit and must be there, with `used`)
int swap_host(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
              const int32_t* coin_out, const double* given, const double* limit, double* answer, int32_t* status, double* used)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_quote_seg(c, dir.who, seg, count, seg_count(c));
    if (rc != CFMM_OK) return rc;
    const PathSegInfo si = seg_info(c, seg);
    const bool rated = dir.rated;
    if (rated && count > 0 && (!limit || !used)) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null query array", dir.who);
    {
        // cfmm_swap_limit: +inf is an amount where the swap has a limit > 0 (checked as 0; everything else as it is)
        std::vector<double> amounts;
        if (rated && given && count > 0) {
            amounts.assign(given, given + count);
            for (int64_t q = 0; q < count; ++q)
                if (given[q] == __builtin_inf() && limit[q] > 0.0 && std::isfinite(limit[q])) amounts[(size_t)q] = 0.0;
        }
        if ((rc = check_quote_queries(c, dir.who, dir.given, si.kind, si.m, si.n_coins, count, idx, coin_in, coin_out,
                                      amounts.empty() ? given : amounts.data(), answer)) != CFMM_OK)
            return rc;
    }
    for (int64_t q = 0; limit && q < count; ++q)
        if (!(limit[q] >= 0.0) || !std::isfinite(limit[q]))
            return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: %s must be finite and >= 0", dir.who, (long long)q, rated ? "rate_limit" : "max_amount_in");
    if (count == 0) return CFMM_OK;   // a no-op that invalidates nothing
    return !c->shards.empty() ? multi_swap(c, dir, seg, count, idx, coin_in, coin_out, given, limit, answer, status, used)
                  : swap_single(c, dir, seg, count, idx, coin_in, coin_out, given, limit, answer, status, used);
}

} // namespace

// the trades and outputs on the device describe the market before the swaps: as cfmm_pools_set_* (abi_update.cpp apply)
void cfmm::swap_invalidate(cfmm_ctx* c)
{
    c->have_trades = false;
    c->have_out = false;
    c->x_valid = false;
    c->trade_v.clear();
}

extern "C" int cfmm_swap(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                         const double* amount_in, double* amount_out)
{
    return swap_host(c, kForward, seg, count, idx, coin_in, coin_out, amount_in, nullptr, amount_out, nullptr, nullptr);
}

extern "C" int cfmm_swap_out(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                             const double* amount_out, const double* max_amount_in, double* amount_in, int32_t* status)
{
    return swap_host(c, kInverse, seg, count, idx, coin_in, coin_out, amount_out, max_amount_in, amount_in, status, nullptr);
}

extern "C" int cfmm_swap_limit(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                               const double* amount_in, const double* rate_limit, double* amount_used, double* amount_out, int32_t* status)
{
    return swap_host(c, kLimited, seg, count, idx, coin_in, coin_out, amount_in, rate_limit, amount_out, status, amount_used);
}
