// abi_quote.cpp -- cfmm_quote / cfmm_quote_dev: exact-input swap quotes of one segment's pools as they stand on the device
// (forward_trade, src/cfmms.jl:398-449, generalised to every kind; the forms: quote_pool.h, the kernel: quote_kernels.h), and
// cfmm_quote_out / cfmm_quote_out_dev, their inverses (exact-output).  The two directions share every line here: a Dir names
// the entry and its given amount in the messages and picks the launcher; `given` / `answer` below are amount_in / amount_out
// of the forward entries and amount_out / amount_in of the inverse ones.
// Read-only: the pool streams are the segment's own arrays, the only memory of the feature is QuoteScratch (ctx.h), which is
// proportional to the queries of a call and never to the pools.
#include "ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

struct Dir {
    bool exact_out;
    const char *host, *dev, *given;   // the entries' names and the given amount's, as the messages spell them
};
constexpr Dir kForward{false, "cfmm_quote", "cfmm_quote_dev", "amount_in"};
constexpr Dir kInverse{true, "cfmm_quote_out", "cfmm_quote_out_dev", "amount_out"};

// the kernel's view of segment `s` for `count` queries; the query arrays are filled in by the caller
hipError_t launch_for(const cfmm_ctx* c, const Dir& dir, const Segment& s, const QuoteArgs& q, hipEvent_t e0, hipEvent_t e1)
{
    QuoteArgs a = q;
    a.m = s.m;
    a.n_coins = ragged_kind(s.kind) ? s.n_coins : 2;
    a.R = s.R.get();
    a.w = s.w.get();
    a.gamma = s.gamma.get();
    UniV3Pools u;
    NCoinPools n;
    std::memset(&u, 0, sizeof u);
    std::memset(&n, 0, sizeof n);
    if (s.kind == CFMM_KIND_UNIV3) {
        const UniV3State& st = s.u;
        u.pg = st.pg.get();
        u.cur_a = st.cur_a.get();
        u.cur_b = st.cur_b.get();
        u.cur_c = st.cur_c.get();
        u.curR = st.curR.get();
        u.walk = st.walk.get();
        u.ticks = st.ticks.get();
    } else if (ragged_kind(s.kind)) {
        n.R = s.nc.R.get();
        n.q = s.nc.q.get();
        n.glg = s.nc.glg.get();
        n.par = s.nc.par.get();
        n.n_coins = s.n_coins;
    }
    return (dir.exact_out ? launch_quote_out : launch_quote)(s.kind, a, u, n, c->stream, e0, e1);
}

int check_seg(cfmm_ctx* c, const char* who, int32_t seg, int64_t count, int64_t nseg) { return check_quote_seg(c, who, seg, count, nseg); }

// every query of a host-pointer call, before anything is enqueued
int check_queries(cfmm_ctx* c, const Dir& dir, int kind, int64_t m, int nc, int64_t count, const int64_t* idx, const int32_t* coin_in,
                  const int32_t* coin_out, const double* given, const double* answer)
{
    return check_quote_queries(c, dir.host, dir.given, kind, m, nc, count, idx, coin_in, coin_out, given, answer);
}

int quote_host(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* given, double* answer);

// A parent: the queries go to the shards that hold their rows (shard_range: contiguous blocks in device order) and the
// answers return in query order, as cfmm_select_trades handles its rows.  Everything was checked by the caller.  One pass
// buckets the queries by shard (a binary search on the blocks' ends per query), one call per shard that got any.
int multi_quote(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                const int32_t* coin_out, const double* given, double* answer)
{
    const int64_t m = c->psegs[(size_t)seg].m;
    const int nd = (int)c->shards.size();
    std::vector<int64_t> first((size_t)nd), end((size_t)nd);
    for (int d = 0; d < nd; ++d) shard_range(m, d, nd, first[(size_t)d], end[(size_t)d]);
    struct Bucket {
        std::vector<int64_t> where, rows;
        std::vector<int32_t> ci, co;
        std::vector<double> amt;
    };
    std::vector<Bucket> buckets((size_t)nd);
    for (int64_t q = 0; q < count; ++q) {
        const int64_t row = idx ? idx[q] : q;
        const size_t d = (size_t)(std::upper_bound(end.begin(), end.end(), row) - end.begin());   // first shard whose end > row
        Bucket& bk = buckets[d];
        bk.where.push_back(q);
        bk.rows.push_back(row - first[d]);
        bk.ci.push_back(coin_in[q]);
        if (coin_out) bk.co.push_back(coin_out[q]);
        bk.amt.push_back(given[q]);
    }
    std::vector<double> out;
    int64_t ns = 0;
    for (int d = 0; d < nd; ++d) {
        const Bucket& bk = buckets[(size_t)d];
        if (bk.where.empty()) continue;
        out.resize(bk.where.size());
        cfmm_ctx* child = c->shards[(size_t)d];
        const int rc = quote_host(child, dir, child_segment(c, seg, d), (int64_t)bk.where.size(), bk.rows.data(), bk.ci.data(),
                                  coin_out ? bk.co.data() : nullptr, bk.amt.data(), out.data());
        if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, child->err.c_str());
        for (size_t j = 0; j < bk.where.size(); ++j) answer[bk.where[j]] = out[j];
        if (child->opt_time_kernels != 0) ns = std::max(ns, child->quote.ns);
    }
    c->quote.ns = ns;   // "quote_ns" of a parent: the longest kernel span among the shards THIS call touched
    return CFMM_OK;
}

// Pinned staging: [count] 8-byte words per column -- idx, amounts, {coin_in, coin_out} as two int32 columns packed into
// one, and the answers -- copied to / from the scratch's device arrays in stream order; one synchronisation.
int quote_host(cfmm_ctx* c, const Dir& dir, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* given, double* answer)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const bool parent = !c->shards.empty();
    int rc = check_seg(c, dir.host, seg, count, parent ? (int64_t)c->psegs.size() : (int64_t)c->segs.size());
    if (rc != CFMM_OK) return rc;
    const int kind = parent ? c->psegs[(size_t)seg].kind : c->segs[(size_t)seg].kind;
    const int64_t m = parent ? c->psegs[(size_t)seg].m : c->segs[(size_t)seg].m;
    const int nc = !ragged_kind(kind) ? 2 : (parent ? c->psegs[(size_t)seg].n_coins : c->segs[(size_t)seg].n_coins);
    if ((rc = check_queries(c, dir, kind, m, nc, count, idx, coin_in, coin_out, given, answer)) != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    if (parent) return multi_quote(c, dir, seg, count, idx, coin_in, coin_out, given, answer);

    const Segment& s = c->segs[(size_t)seg];
    HIP_TRY(c, hipSetDevice(c->device));
    QuoteScratch& sc = c->quote;
    const size_t n = (size_t)count;
    const size_t ncol = 3 + (idx ? 1 : 0);                 // amounts, coins, answers (+ idx)
    if ((rc = sc.stage.grow(c, ncol * n, false)) || (rc = sc.amt.grow(c, n)) || (rc = sc.coins.grow(c, 2 * n)) ||
        (rc = sc.out.grow(c, n)) || (idx && (rc = sc.idx.grow(c, n))))
        return rc;
    const bool timed = c->opt_time_kernels != 0;
    for (int k = 0; k < 2 && timed; ++k)
        if ((rc = sc.ev[k].create(c, hipEventDefault)) != CFMM_OK) return rc;
    unsigned long long* st = sc.stage.host();
    double* h_amt = reinterpret_cast<double*>(st);
    int32_t* h_coins = reinterpret_cast<int32_t*>(st + n);   // [count] coin_in, then [count] coin_out
    double* h_out = reinterpret_cast<double*>(st + 2 * n);
    long long* h_idx = reinterpret_cast<long long*>(st + 3 * n);
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
    const hipError_t e = launch_for(c, dir, s, a, timed ? sc.ev[0].get() : nullptr, timed ? sc.ev[1].get() : nullptr);
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote launch failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (timed) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, sc.ev[0].get(), sc.ev[1].get()));
        sc.ns = (int64_t)((double)ms * 1e6);
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
    int rc = check_seg(c, dir.dev, seg, count, (int64_t)c->segs.size());
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
    for (int k = 0; k < 2 && timed; ++k)
        if ((rc = sc.ev[k].create(c, hipEventDefault)) != CFMM_OK) return rc;
    QuoteArgs a{};
    a.count = count;
    a.idx = reinterpret_cast<const long long*>(d_idx);
    a.coin_in = d_coin_in;
    a.coin_out = d_coin_out;
    a.amount_in = d_given;
    a.amount_out = d_answer;
    const hipError_t e = launch_for(c, dir, s, a, timed ? sc.ev[0].get() : nullptr, timed ? sc.ev[1].get() : nullptr);
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
        float ms = 0.f;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(sc.ev[1].get()));
        HIP_TRY(c, hipEventElapsedTime(&ms, sc.ev[0].get(), sc.ev[1].get()));
        sc.ns = (int64_t)((double)ms * 1e6);
        sc.dev_timed = false;
    }
    *value = sc.ns;
    return CFMM_OK;
}

} // namespace cfmm
