// abi_limit.cpp -- cfmm_quote_to_rate and cfmm_quote_to_rate_dev (include/cfmm_amd_limit.h): the amount that brings a pool's
// marginal rate down to a limit, and what it buys (the inverses: to_rate_pool.h, the kernel: to_rate_kernels.h).  Shaped like
// abi_rate.cpp's single-pool entries, whose checks, staging rule and shard split these take: the query columns and the staging
// are QuoteScratch's (the limits travel where the quotes carry their amounts; every host-pointer call ends synchronised), the
// answers ToRateScratch's (ctx.h).  cfmm_swap_limit, the entry that executes against the limit, is the third direction of
// abi_swap.cpp.
// Read-only.  Scratch is proportional to the queries of a call, never to the pools.
#include "../../include/cfmm_amd_limit.h"
#include "seg_view.h"
#include "shard_split.h"
#include "stage_layout.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

constexpr const char *kWho = "cfmm_quote_to_rate", *kDev = "cfmm_quote_to_rate_dev";

hipError_t launch_for(const cfmm_ctx* c, const Segment& s, const ToRateArgs& q, hipEvent_t e0, hipEvent_t e1)
{
    const PathSeg p = path_seg(s);
    ToRateArgs a = q;
    quote_view(p, a.q);
    return launch_quote_to_rate(s.kind, a, univ3_view(p), ncoin_view(p), c->stream, e0, e1);
}

int to_rate_host(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                 const double* limit, double* amount_in, double* amount_out);

// A parent: abi_rate.cpp's multi_rate.  Everything was checked by the caller.
int multi_to_rate(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                  const double* limit, double* amount_in, double* amount_out)
{
    const int nd = (int)c->shards.size();
    const std::vector<ShardBucket> buckets = split_by_shard(c->psegs[(size_t)seg].m, nd, count, idx);
    std::vector<double> in, out;
    int64_t ns = 0;
    for (int d = 0; d < nd; ++d) {
        const ShardBucket& bk = buckets[(size_t)d];
        if (bk.where.empty()) continue;
        in.resize(bk.where.size());
        out.resize(bk.where.size());
        const std::vector<int32_t> ci = gather(bk.where, coin_in), co = gather(bk.where, coin_out);
        const std::vector<double> lim = gather(bk.where, limit);
        cfmm_ctx* child = c->shards[(size_t)d];
        const int rc = to_rate_host(child, child_segment(c, seg, d), (int64_t)bk.where.size(), bk.rows.data(), ci.data(),
                                    coin_out ? co.data() : nullptr, lim.data(), in.data(), amount_out ? out.data() : nullptr);
        if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, child->err.c_str());
        scatter(bk.where, in.data(), amount_in);
        if (amount_out) scatter(bk.where, out.data(), amount_out);
        if (child->opt_time_kernels != 0) ns = std::max(ns, child->to_rate.ns);
    }
    c->to_rate.ns = ns;   // "limit_ns" of a parent: the longest kernel span among the shards THIS call touched
    return CFMM_OK;
}

// Pinned staging (stage_layout.h RateStage), copied to / from the device arrays in stream order; one synchronisation.
int to_rate_host(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                 const double* limit, double* amount_in, double* amount_out)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_quote_seg(c, kWho, seg, count, seg_count(c));
    if (rc != CFMM_OK) return rc;
    const PathSegInfo si = seg_info(c, seg);
    {
        // cfmm_quote's checks of rows and coins (its amounts: all 0), then the limits
        const std::vector<double> zeros((size_t)std::max<int64_t>(count, 0), 0.0);
        if ((rc = check_quote_queries(c, kWho, "rate_limit", si.kind, si.m, si.n_coins, count, idx, coin_in, coin_out,
                                      limit ? zeros.data() : nullptr, amount_in)) != CFMM_OK)
            return rc;
        for (int64_t q = 0; q < count; ++q)
            if (!(limit[q] > 0.0) || !std::isfinite(limit[q]))
                return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: rate_limit must be finite and > 0", kWho, (long long)q);
    }
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty()) return multi_to_rate(c, seg, count, idx, coin_in, coin_out, limit, amount_in, amount_out);

    const Segment& s = c->segs[(size_t)seg];
    HIP_TRY(c, hipSetDevice(c->device));
    QuoteScratch& sc = c->quote;
    ToRateScratch& ts = c->to_rate;
    const size_t n = (size_t)count;
    const RateStage lay(n, true, idx != nullptr);
    const bool timed = c->opt_time_kernels != 0;
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.amt.grow(c, n)) || (rc = sc.coins.grow(c, 2 * n)) ||
        (rc = ts.out.grow(c, 2 * n)) || (idx && (rc = sc.idx.grow(c, n))) || (timed && (rc = ts.ev.ensure(c, 1))))
        return rc;
    unsigned long long* st = sc.stage.host();
    double *h_lim = lay.amt.in(st), *h_out = lay.out.in(st);   // h_out: [count] amount_in, then [count] amount_out
    int32_t* h_coins = lay.coins.in(st);                        // [count] coin_in, then [count] coin_out
    long long* h_idx = lay.idx.in(st);
    std::memcpy(h_lim, limit, n * sizeof(double));
    std::memcpy(h_coins, coin_in, n * sizeof(int32_t));
    if (coin_out) std::memcpy(h_coins + n, coin_out, n * sizeof(int32_t));
    if (idx) std::memcpy(h_idx, idx, n * sizeof(long long));
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_lim, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.coins.get(), h_coins, (coin_out ? 2 : 1) * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(sc.idx.get(), h_idx, n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    ToRateArgs a{};
    a.q.count = count;
    a.q.idx = idx ? sc.idx.get() : nullptr;
    a.q.coin_in = sc.coins.get();
    a.q.coin_out = coin_out ? sc.coins.get() + n : nullptr;
    a.q.amount_in = sc.amt.get();
    a.amount = ts.out.get();
    a.q.amount_out = amount_out ? ts.out.get() + n : nullptr;
    const hipError_t e = launch_for(c, s, a, ts.ev.start(0, timed), ts.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote to rate launch failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipMemcpyAsync(h_out, ts.out.get(), (amount_out ? 2 : 1) * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (timed) {
        if ((rc = ts.ev.elapsed_ns(c, 0, 1, ts.ns)) != CFMM_OK) return rc;
        ts.dev_timed = false;
    }
    std::memcpy(amount_in, h_out, n * sizeof(double));
    if (amount_out) std::memcpy(amount_out, h_out + n, n * sizeof(double));
    return CFMM_OK;
}

int to_rate_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in, const int32_t* d_coin_out,
                const double* d_limit, double* d_amount_in, double* d_amount_out)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", kDev);
    int rc = check_quote_seg(c, kDev, seg, count, (int64_t)c->segs.size());
    if (rc != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    const Segment& s = c->segs[(size_t)seg];
    if (!d_coin_in || !d_limit || !d_amount_in) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null query array", kDev);
    if (!d_coin_out && ragged_kind(s.kind))
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: coin_out is required on a %s segment", kDev, kind_info(s.kind).name);
    if (s.m <= 0) return fail(c, CFMM_ERR_INVALID_ARG, "%s: the segment has no pools", kDev);
    HIP_TRY(c, hipSetDevice(c->device));
    const bool timed = c->opt_time_kernels != 0;
    ToRateScratch& ts = c->to_rate;
    if (timed && (rc = ts.ev.ensure(c, 1)) != CFMM_OK) return rc;
    ToRateArgs a{};
    a.q.count = count;
    a.q.idx = reinterpret_cast<const long long*>(d_idx);
    a.q.coin_in = d_coin_in;
    a.q.coin_out = d_coin_out;
    a.q.amount_in = d_limit;
    a.q.amount_out = d_amount_out;
    a.amount = d_amount_in;
    const hipError_t e = launch_for(c, s, a, ts.ev.start(0, timed), ts.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote to rate launch failed: %s", hipGetErrorString(e));
    ts.dev_timed = timed;   // the span is read when "limit_ns" is asked for (the call itself does not wait)
    return CFMM_OK;
}

} // namespace

int cfmm_quote_to_rate(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                       const double* rate_limit, double* amount_in, double* amount_out)
{
    return to_rate_host(c, seg, count, idx, coin_in, coin_out, rate_limit, amount_in, amount_out);
}

int cfmm_quote_to_rate_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in, const int32_t* d_coin_out,
                           const double* d_rate_limit, double* d_amount_in, double* d_amount_out)
{
    return to_rate_dev(c, seg, count, d_idx, d_coin_in, d_coin_out, d_rate_limit, d_amount_in, d_amount_out);
}

namespace cfmm {

// read-only option "limit_ns": the span of the latest call's kernel timed under "time_kernels"
int limit_ns(cfmm_ctx* c, int64_t* value)
{
    ToRateScratch& ts = c->to_rate;
    if (ts.dev_timed) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(ts.ev.stop(0)));
        if (const int rc = ts.ev.elapsed_ns(c, 0, 1, ts.ns)) return rc;
        ts.dev_timed = false;
    }
    *value = ts.ns;
    return CFMM_OK;
}

} // namespace cfmm
