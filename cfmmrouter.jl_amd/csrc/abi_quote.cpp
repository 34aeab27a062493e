// abi_quote.cpp -- cfmm_quote / cfmm_quote_dev: exact-input swap quotes of one segment's pools as they stand on the device
// (forward_trade, src/cfmms.jl:398-449, generalised to every kind; the forms: quote_pool.h, the kernel: quote_kernels.h), and
// cfmm_quote_out / cfmm_quote_out_dev, their inverses (exact-output).  The two directions share every line here: a Dir names
// the entry and its given amount in the messages and picks the launcher; `given` / `answer` below are amount_in / amount_out
// of the forward entries and amount_out / amount_in of the inverse ones.
// Read-only: the pool streams are the segment's own arrays, the only memory of the feature is QuoteScratch (ctx.h), which is
// proportional to the queries of a call and never to the pools.
#include "seg_view.h"
#include "stage_layout.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

constexpr Dir kForward{false, "cfmm_quote", "cfmm_quote_dev", "amount_in"};
constexpr Dir kInverse{true, "cfmm_quote_out", "cfmm_quote_out_dev", "amount_out"};

// the kernel's view of segment `s` (seg_view.h: the members of its own kind); the query arrays are filled in by the caller
hipError_t launch_for(const cfmm_ctx* c, const Dir& dir, const Segment& s, const QuoteArgs& q, hipEvent_t e0, hipEvent_t e1)
{
    const PathSeg p = path_seg(s);
    QuoteArgs a = q;
    quote_view(p, a);
    return (dir.exact_out ? launch_quote_out : launch_quote)(s.kind, a, univ3_view(p), ncoin_view(p), c->stream, e0, e1);
}

int quote_host(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* given, double* answer);

// A parent: the queries go to the shards that hold their rows (shard_split.h: contiguous blocks in device order) and the
// answers return in query order, as cfmm_select_trades handles its rows.  Everything was checked by the caller.  One call
// per shard that got any.
int multi_quote(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                const int32_t* coin_out, const double* given, double* answer)
{
    const int nd = (int)c->shards.size();
    const std::vector<ShardBucket> buckets = split_by_shard(c->psegs[(size_t)seg].m, nd, count, idx);
    std::vector<double> out;
    int64_t ns = 0;
    for (int d = 0; d < nd; ++d) {
        const ShardBucket& bk = buckets[(size_t)d];
        if (bk.where.empty()) continue;
        out.resize(bk.where.size());
        const std::vector<int32_t> ci = gather(bk.where, coin_in), co = gather(bk.where, coin_out);
        const std::vector<double> amt = gather(bk.where, given);
        cfmm_ctx* child = c->shards[(size_t)d];
        const int rc = quote_host(child, dir, child_segment(c, seg, d), (int64_t)bk.where.size(), bk.rows.data(), ci.data(),
                                  coin_out ? co.data() : nullptr, amt.data(), out.data());
        if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, child->err.c_str());
        scatter(bk.where, out.data(), answer);
        if (child->opt_time_kernels != 0) ns = std::max(ns, child->quote.ns);
    }
    c->quote.ns = ns;   // "quote_ns" of a parent: the longest kernel span among the shards THIS call touched
    return CFMM_OK;
}

// Pinned staging (stage_layout.h QuoteStage), copied to / from the scratch's device arrays in stream order; one synchronisation.
int quote_host(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* given, double* answer)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_quote_seg(c, dir.who, seg, count, seg_count(c));
    if (rc != CFMM_OK) return rc;
    const PathSegInfo si = seg_info(c, seg);
    if ((rc = check_quote_queries(c, dir.who, dir.given, si.kind, si.m, si.n_coins, count, idx, coin_in, coin_out, given, answer)) != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty()) return multi_quote(c, dir, seg, count, idx, coin_in, coin_out, given, answer);

    const Segment& s = c->segs[(size_t)seg];
    HIP_TRY(c, hipSetDevice(c->device));
    QuoteScratch& sc = c->quote;
    const size_t n = (size_t)count;
    const QuoteStage lay(n, idx != nullptr);
    const bool timed = c->opt_time_kernels != 0;
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.amt.grow(c, n)) || (rc = sc.coins.grow(c, 2 * n)) ||
        (rc = sc.out.grow(c, n)) || (idx && (rc = sc.idx.grow(c, n))) || (timed && (rc = sc.ev.ensure(c, 1))))
        return rc;
    unsigned long long* st = sc.stage.host();
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st);
    int32_t* h_coins = lay.coins.in(st);   // [count] coin_in, then [count] coin_out
    long long* h_idx = lay.idx.in(st);
    std::memcpy(h_amt, given, n * sizeof(double));
    std::memcpy(h_coins, coin_in, n * sizeof(int32_t));
    if (coin_out) std::memcpy(h_coins + n, coin_out, n * sizeof(int32_t));
    if (idx) std::memcpy(h_idx, idx, n * sizeof(long long));
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.coins.get(), h_coins, (coin_out ? 2 : 1) * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(sc.idx.get(), h_idx, n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    QuoteArgs a{};
    a.count = count;
    a.idx = idx ? sc.idx.get() : nullptr;
    a.coin_in = sc.coins.get();
    a.coin_out = coin_out ? sc.coins.get() + n : nullptr;
    a.amount_in = sc.amt.get();
    a.amount_out = sc.out.get();
    const hipError_t e = launch_for(c, dir, s, a, sc.ev.start(0, timed), sc.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote launch failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (timed) {
        if ((rc = sc.ev.elapsed_ns(c, 0, 1, sc.ns)) != CFMM_OK) return rc;
        sc.dev_timed = false;
    }
    std::memcpy(answer, h_out, n * sizeof(double));
    return CFMM_OK;
}

int quote_dev(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
              const int32_t* d_coin_out, const double* d_given, double* d_answer)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text, with the entry's name from the Dir)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", dir.dev);
    int rc = check_quote_seg(c, dir.dev, seg, count, (int64_t)c->segs.size());
    if (rc != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    const Segment& s = c->segs[(size_t)seg];
    if (!d_coin_in || !d_given || !d_answer) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null query array", dir.dev);
    if (!d_coin_out && ragged_kind(s.kind))
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: coin_out is required on a %s segment", dir.dev, kind_info(s.kind).name);
    if (s.m <= 0) return fail(c, CFMM_ERR_INVALID_ARG, "%s: the segment has no pools", dir.dev);
    HIP_TRY(c, hipSetDevice(c->device));
    const bool timed = c->opt_time_kernels != 0;
    QuoteScratch& sc = c->quote;
    if (timed && (rc = sc.ev.ensure(c, 1)) != CFMM_OK) return rc;
    QuoteArgs a{};
    a.count = count;
    a.idx = reinterpret_cast<const long long*>(d_idx);
    a.coin_in = d_coin_in;
    a.coin_out = d_coin_out;
    a.amount_in = d_given;
    a.amount_out = d_answer;
    const hipError_t e = launch_for(c, dir, s, a, sc.ev.start(0, timed), sc.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote launch failed: %s", hipGetErrorString(e));
    sc.dev_timed = timed;   // the span is read when "quote_ns" is asked for (the call itself does not wait)
    return CFMM_OK;
}

} // namespace

int cfmm_quote(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
               const double* amount_in, double* amount_out)
{
    return quote_host(c, kForward, seg, count, idx, coin_in, coin_out, amount_in, amount_out);
}

int cfmm_quote_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                   const int32_t* d_coin_out, const double* d_amount_in, double* d_amount_out)
{
    return quote_dev(c, kForward, seg, count, d_idx, d_coin_in, d_coin_out, d_amount_in, d_amount_out);
}

int cfmm_quote_out(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                   const double* amount_out, double* amount_in)
{
    return quote_host(c, kInverse, seg, count, idx, coin_in, coin_out, amount_out, amount_in);
}

int cfmm_quote_out_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                       const int32_t* d_coin_out, const double* d_amount_out, double* d_amount_in)
{
    return quote_dev(c, kInverse, seg, count, d_idx, d_coin_in, d_coin_out, d_amount_out, d_amount_in);
}

namespace cfmm {

int check_quote_seg(cfmm_ctx* c, const char* who, int32_t seg, int64_t count, int64_t nseg)
{
    if (seg < 0 || seg >= nseg) return fail(c, CFMM_ERR_INVALID_ARG, "%s: segment out of range", who);
    if (count < 0) return fail(c, CFMM_ERR_INVALID_ARG, "%s: count must be >= 0", who);
    return CFMM_OK;
}

// every query of a host-pointer call, before anything is enqueued (cfmm_swap runs the same checks under its own name)
int check_quote_queries(cfmm_ctx* c, const char* who, const char* given_name, int kind, int64_t m, int nc, int64_t count,
                        const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out, const double* given, const double* answer)
{
    if (count > 0 && (!coin_in || !given || !answer)) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null query array", who);
    if (count > 0 && !coin_out && ragged_kind(kind))
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: coin_out is required on a %s segment (query 0)", who, kind_info(kind).name);
    for (int64_t q = 0; q < count; ++q) {
        const int64_t row = idx ? idx[q] : q;
        if (row < 0 || row >= m)
            return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: row %lld out of range (segment has %lld pools)", who,
                        (long long)q, (long long)row, (long long)m);
        const int ci = coin_in[q], co = coin_out ? coin_out[q] : 1 - ci;
        if (ci < 0 || ci >= nc) return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: coin_in %d out of range (pool has %d coins)", who, (long long)q, ci, nc);
        if (co < 0 || co >= nc) return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: coin_out %d out of range (pool has %d coins)", who, (long long)q, co, nc);
        if (ci == co) return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: coin_in and coin_out are both %d", who, (long long)q, ci);
        if (!(given[q] >= 0.0) || !std::isfinite(given[q]))
            return fail(c, CFMM_ERR_INVALID_ARG, "%s: query %lld: %s must be finite and >= 0", who, (long long)q, given_name);
    }
    return CFMM_OK;
}

// read-only option "quote_ns": the span of the latest call's kernel (of either direction) timed under "time_kernels"
int quote_ns(cfmm_ctx* c, int64_t* value)
{
    QuoteScratch& sc = c->quote;
    if (sc.dev_timed) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(sc.ev.stop(0)));
        if (const int rc = sc.ev.elapsed_ns(c, 0, 1, sc.ns)) return rc;
        sc.dev_timed = false;
    }
    *value = sc.ns;
    return CFMM_OK;
}

} // namespace cfmm
