// abi_rate.cpp -- cfmm_quote_rate / cfmm_quote_path_rate and their _dev forms (include/cfmm_amd_rate.h): the exact-input quote
// of a pool or a path AND its marginal rate from one read of the pools (the derivatives: rate_pool.h, the kernels:
// rate_kernels.h).  Shaped like abi_quote.cpp and abi_quote_path.cpp, whose checks, staging rule and shard split these
// entries take: the query columns and the staging are QuoteScratch's, the table, the rig and the hop columns PathScratch's
// (every host-pointer call ends synchronised), the answers RateScratch's (ctx.h).
// Read-only.  Scratch is proportional to the queries of a call (count x max_hops for paths), never to the pools.
#include "../../include/cfmm_amd_rate.h"
#include "path_rig.h"
#include "shard_split.h"
#include "stage_layout.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace cfmm;

namespace {

constexpr const char *kWho = "cfmm_quote_rate", *kDev = "cfmm_quote_rate_dev";
constexpr const char *kPathWho = "cfmm_quote_path_rate", *kPathDev = "cfmm_quote_path_rate_dev";

hipError_t launch_for(const cfmm_ctx* c, const Segment& s, const RateArgs& q, hipEvent_t e0, hipEvent_t e1)
{
    const PathSeg p = path_seg(s);
    RateArgs a = q;
    quote_view(p, a.q);
    return launch_quote_rate(s.kind, a, univ3_view(p), ncoin_view(p), c->stream, e0, e1);
}

int rate_host(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
              const double* amount_in, double* amount_out, double* rate);

// A parent: abi_quote.cpp's multi_quote with two answers per query.  Everything was checked by the caller.
int multi_rate(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
               const double* amount_in, double* amount_out, double* rate)
{
    const int nd = (int)c->shards.size();
    const std::vector<ShardBucket> buckets = split_by_shard(c->psegs[(size_t)seg].m, nd, count, idx);
    std::vector<double> out, rt;
    int64_t ns = 0;
    for (int d = 0; d < nd; ++d) {
        const ShardBucket& bk = buckets[(size_t)d];
        if (bk.where.empty()) continue;
        out.resize(bk.where.size());
        rt.resize(bk.where.size());
        const std::vector<int32_t> ci = gather(bk.where, coin_in), co = gather(bk.where, coin_out);
        const std::vector<double> amt = gather(bk.where, amount_in);
        cfmm_ctx* child = c->shards[(size_t)d];
        const int rc = rate_host(child, child_segment(c, seg, d), (int64_t)bk.where.size(), bk.rows.data(), ci.data(),
                                 coin_out ? co.data() : nullptr, amount_in ? amt.data() : nullptr, amount_out ? out.data() : nullptr, rt.data());
        if (rc != CFMM_OK) return fail(c, rc, "shard %d: %s", d, child->err.c_str());
        if (amount_out) scatter(bk.where, out.data(), amount_out);
        scatter(bk.where, rt.data(), rate);
        if (child->opt_time_kernels != 0) ns = std::max(ns, child->rate.ns);
    }
    c->rate.ns = ns;   // "rate_ns" of a parent: the longest kernel span among the shards THIS call touched
    return CFMM_OK;
}

// Pinned staging (stage_layout.h RateStage), copied to / from the device arrays in stream order; one synchronisation.
int rate_host(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
              const double* amount_in, double* amount_out, double* rate)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_quote_seg(c, kWho, seg, count, seg_count(c));
    if (rc != CFMM_OK) return rc;
    const PathSegInfo si = seg_info(c, seg);
    {
        // cfmm_quote's checks; a call without amounts is checked as one whose amounts are all 0
        const std::vector<double> zeros(amount_in ? 0 : (size_t)std::max<int64_t>(count, 0), 0.0);
        const double* answer = rate && (amount_out || !amount_in) ? rate : nullptr;   // (either missing output: "null query array")
        if ((rc = check_quote_queries(c, kWho, "amount_in", si.kind, si.m, si.n_coins, count, idx, coin_in, coin_out,
                                      amount_in ? amount_in : zeros.data(), answer)) != CFMM_OK)
            return rc;
    }
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty()) return multi_rate(c, seg, count, idx, coin_in, coin_out, amount_in, amount_out, rate);

    const Segment& s = c->segs[(size_t)seg];
    HIP_TRY(c, hipSetDevice(c->device));
    QuoteScratch& sc = c->quote;
    RateScratch& rs = c->rate;
    const size_t n = (size_t)count;
    const RateStage lay(n, amount_in != nullptr, idx != nullptr);
    const bool timed = c->opt_time_kernels != 0;
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (amount_in && (rc = sc.amt.grow(c, n))) || (rc = sc.coins.grow(c, 2 * n)) ||
        (rc = rs.out.grow(c, 2 * n)) || (idx && (rc = sc.idx.grow(c, n))) || (timed && (rc = rs.ev.ensure(c, 1))))
        return rc;
    unsigned long long* st = sc.stage.host();
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st);   // h_out: [count] amount_out, then [count] rate
    int32_t* h_coins = lay.coins.in(st);                        // [count] coin_in, then [count] coin_out
    long long* h_idx = lay.idx.in(st);
    if (amount_in) std::memcpy(h_amt, amount_in, n * sizeof(double));
    std::memcpy(h_coins, coin_in, n * sizeof(int32_t));
    if (coin_out) std::memcpy(h_coins + n, coin_out, n * sizeof(int32_t));
    if (idx) std::memcpy(h_idx, idx, n * sizeof(long long));
    if (amount_in) HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.coins.get(), h_coins, (coin_out ? 2 : 1) * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (idx) HIP_TRY(c, hipMemcpyAsync(sc.idx.get(), h_idx, n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    RateArgs a{};
    a.q.count = count;
    a.q.idx = idx ? sc.idx.get() : nullptr;
    a.q.coin_in = sc.coins.get();
    a.q.coin_out = coin_out ? sc.coins.get() + n : nullptr;
    a.q.amount_in = amount_in ? sc.amt.get() : nullptr;
    a.q.amount_out = amount_out ? rs.out.get() : nullptr;
    a.rate = rs.out.get() + n;
    const hipError_t e = launch_for(c, s, a, rs.ev.start(0, timed), rs.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote rate launch failed: %s", hipGetErrorString(e));
    // (one copy back: both halves when the call wants the amounts, else the rates alone)
    if (amount_out) HIP_TRY(c, hipMemcpyAsync(h_out, rs.out.get(), 2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    else HIP_TRY(c, hipMemcpyAsync(h_out + n, rs.out.get() + n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (timed) {
        if ((rc = rs.ev.elapsed_ns(c, 0, 1, rs.ns)) != CFMM_OK) return rc;
        rs.dev_timed = false;
    }
    if (amount_out) std::memcpy(amount_out, h_out, n * sizeof(double));
    std::memcpy(rate, h_out + n, n * sizeof(double));
    return CFMM_OK;
}

int rate_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in, const int32_t* d_coin_out,
             const double* d_amount_in, double* d_amount_out, double* d_rate)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", kDev);
    int rc = check_quote_seg(c, kDev, seg, count, (int64_t)c->segs.size());
    if (rc != CFMM_OK) return rc;
    if (count == 0) return CFMM_OK;
    const Segment& s = c->segs[(size_t)seg];
    if (!d_coin_in || !d_rate || (d_amount_in && !d_amount_out)) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null query array", kDev);
    if (!d_coin_out && ragged_kind(s.kind))
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: coin_out is required on a %s segment", kDev, kind_info(s.kind).name);
    if (s.m <= 0) return fail(c, CFMM_ERR_INVALID_ARG, "%s: the segment has no pools", kDev);
    HIP_TRY(c, hipSetDevice(c->device));
    const bool timed = c->opt_time_kernels != 0;
    RateScratch& rs = c->rate;
    if (timed && (rc = rs.ev.ensure(c, 1)) != CFMM_OK) return rc;
    RateArgs a{};
    a.q.count = count;
    a.q.idx = reinterpret_cast<const long long*>(d_idx);
    a.q.coin_in = d_coin_in;
    a.q.coin_out = d_coin_out;
    a.q.amount_in = d_amount_in;
    a.q.amount_out = d_amount_out;
    a.rate = d_rate;
    const hipError_t e = launch_for(c, s, a, rs.ev.start(0, timed), rs.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "quote rate launch failed: %s", hipGetErrorString(e));
    rs.dev_timed = timed;   // the span is read when "rate_ns" is asked for (the call itself does not wait)
    return CFMM_OK;
}

PathRateStage stage_of(const cfmm_ctx* c, size_t n, size_t nh) { return PathRateStage(table_records(c) * sizeof(PathSeg), n, nh); }

int launch(cfmm_ctx* c, const PathRateArgs& a)
{
    return c->path.launch(c, c->rate.ev, "quote path rate", [&](hipEvent_t e0, hipEvent_t e1) { return launch_quote_path_rate(a, c->stream, e0, e1); });
}

// A parent: abi_quote_path.cpp's multi_path, forward direction, through cfmm_quote_rate -- one call per level and segment that
// has an active path; the poison rule and the left fold of the rates are applied here, in the kernel's order.  Everything was
// checked by the caller; the answers are written only when every call has succeeded.
int multi_path(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
               const int32_t* ci, const int32_t* co, const double* given, double* answer, double* rate, double* hops, double* hop_rate)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t n = (size_t)count, nseg = c->psegs.size(), nh = n * (size_t)max_hops;
    std::vector<double> x(given, given + n), fold(n, nan), hv(hops ? nh : 0, nan), hr(hop_rate ? nh : 0, nan), out, rt;
    std::vector<std::vector<int64_t>> where(nseg), rows(nseg);
    std::vector<std::vector<int32_t>> cis(nseg), cos(nseg);
    std::vector<std::vector<double>> amts(nseg);
    int64_t ns = 0;
    for (int k = 0; k < max_hops; ++k) {
        for (size_t s = 0; s < nseg; ++s) { where[s].clear(); rows[s].clear(); cis[s].clear(); cos[s].clear(); amts[s].clear(); }
        for (size_t p = 0; p < n; ++p) {
            if (k >= n_hops[p]) continue;
            const size_t at = (size_t)k * n + p;
            if (!(x[p] >= 0.0) || !std::isfinite(x[p])) {   // the kernel's rule: what is no amount poisons the hop, amount and rate
                x[p] = nan;
                fold[p] = k == 0 ? nan : fold[p] * nan;
                if (hops) hv[at] = nan;
                if (hop_rate) hr[at] = nan;
                continue;
            }
            const size_t s = (size_t)hop_seg[at];
            where[s].push_back((int64_t)p);
            rows[s].push_back(hop_row[at]);
            cis[s].push_back(ci[at]);
            cos[s].push_back(co[at]);
            amts[s].push_back(x[p]);
        }
        for (size_t s = 0; s < nseg; ++s) {
            if (where[s].empty()) continue;
            out.resize(where[s].size());
            rt.resize(where[s].size());
            const int rc = cfmm_quote_rate(c, (int32_t)s, (int64_t)where[s].size(), rows[s].data(), cis[s].data(), cos[s].data(),
                                           amts[s].data(), out.data(), rt.data());
            if (rc != CFMM_OK) return rc;   // (the message is the inner call's)
            if (c->opt_time_kernels != 0) ns = std::max(ns, c->rate.ns);
            for (size_t j = 0; j < where[s].size(); ++j) {
                const size_t p = (size_t)where[s][j], at = (size_t)k * n + p;
                x[p] = out[j];
                fold[p] = k == 0 ? rt[j] : fold[p] * rt[j];
                if (hops) hv[at] = out[j];
                if (hop_rate) hr[at] = rt[j];
            }
        }
    }
    c->rate.ns = ns;   // "rate_ns" of a parent: the longest span among the calls THIS entry made
    std::memcpy(answer, x.data(), n * sizeof(double));
    std::memcpy(rate, fold.data(), n * sizeof(double));
    if (hops) std::memcpy(hops, hv.data(), nh * sizeof(double));
    if (hop_rate) std::memcpy(hop_rate, hr.data(), nh * sizeof(double));
    return CFMM_OK;
}

int path_host(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
              const int32_t* ci, const int32_t* co, const double* given, double* answer, double* rate, double* hops, double* hop_rate)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    char msg[256] = "";
    const std::vector<PathSegInfo> info = seg_infos(c);
    int rc = check_paths(kPathWho, false, info.data(), (int64_t)info.size(), count, max_hops, n_hops, hop_seg, hop_row, ci, co, given, msg, sizeof msg);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count > 0 && (!answer || !rate)) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", kPathWho);
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty()) return multi_path(c, count, max_hops, n_hops, hop_seg, hop_row, ci, co, given, answer, rate, hops, hop_rate);

    HIP_TRY(c, hipSetDevice(c->device));
    PathScratch& ps = c->path;
    RateScratch& rs = c->rate;
    const size_t n = (size_t)count, H = (size_t)max_hops, nh = n * H;
    const bool any_hops = hops || hop_rate;
    const PathRateStage lay = stage_of(c, n, nh);
    PathRateArgs a{};
    if ((rc = ps.upload_table(c, lay, a.p.nseg)) || (rc = ps.hop_i32.grow(c, n + 3 * nh)) || (rc = ps.hop_row.grow(c, nh)) ||
        (rc = ps.given.grow(c, n)) || (rc = rs.out.grow(c, 2 * n)) || (any_hops && (rc = rs.hops.grow(c, 2 * nh))))
        return rc;
    unsigned long long* st = ps.stage.host();
    int32_t* h_i32 = lay.i32.in(st);
    long long* h_row = lay.row.in(st);
    double *h_given = lay.given.in(st), *h_answer = lay.answer.in(st), *h_hops = lay.hops.in(st);
    std::memcpy(h_i32, n_hops, n * sizeof(int32_t));
    std::memcpy(h_i32 + n, hop_seg, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + nh, ci, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + 2 * nh, co, nh * sizeof(int32_t));
    std::memcpy(h_row, hop_row, nh * sizeof(long long));
    std::memcpy(h_given, given, n * sizeof(double));
    HIP_TRY(c, hipMemcpyAsync(ps.hop_i32.get(), h_i32, (n + 3 * nh) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ps.hop_row.get(), h_row, nh * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ps.given.get(), h_given, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    a.p.count = count;
    a.p.max_hops = max_hops;
    a.p.segs = ps.table.get();
    a.p.n_hops = ps.hop_i32.get();
    a.p.hop_seg = ps.hop_i32.get() + n;
    a.p.hop_coin_in = ps.hop_i32.get() + n + nh;
    a.p.hop_coin_out = ps.hop_i32.get() + n + 2 * nh;
    a.p.hop_row = ps.hop_row.get();
    a.p.given = ps.given.get();
    a.p.answer = rs.out.get();
    a.p.hops = hops ? rs.hops.get() : nullptr;
    a.rate = rs.out.get() + n;
    a.hop_rate = hop_rate ? rs.hops.get() + nh : nullptr;
    if ((rc = launch(c, a)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_answer, rs.out.get(), 2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (hops) HIP_TRY(c, hipMemcpyAsync(h_hops, rs.hops.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (hop_rate) HIP_TRY(c, hipMemcpyAsync(h_hops + nh, rs.hops.get() + nh, nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ps.in_flight = false;
    if (c->opt_time_kernels != 0) {
        if ((rc = rs.ev.elapsed_ns(c, 0, 1, rs.ns)) != CFMM_OK) return rc;
        rs.dev_timed = false;
    }
    std::memcpy(answer, h_answer, n * sizeof(double));
    std::memcpy(rate, h_answer + n, n * sizeof(double));
    if (hops) std::memcpy(hops, h_hops, nh * sizeof(double));
    if (hop_rate) std::memcpy(hop_rate, h_hops + nh, nh * sizeof(double));
    return CFMM_OK;
}

int path_dev(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg, const int64_t* d_hop_row,
             const int32_t* d_ci, const int32_t* d_co, const double* d_given, double* d_answer, double* d_rate, double* d_hops, double* d_hop_rate)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", kPathDev);
    char msg[256] = "";
    int rc = check_path_scalars(kPathDev, count, max_hops, msg, sizeof msg);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    if (!d_n_hops || !d_hop_seg || !d_hop_row || !d_ci || !d_co || !d_given || !d_answer || !d_rate)
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", kPathDev);
    HIP_TRY(c, hipSetDevice(c->device));
    PathRateArgs a{};
    if ((rc = c->path.upload_table(c, stage_of(c, 0, 0), a.p.nseg)) != CFMM_OK) return rc;
    a.p.count = count;
    a.p.max_hops = max_hops;
    a.p.segs = c->path.table.get();
    a.p.n_hops = d_n_hops;
    a.p.hop_seg = d_hop_seg;
    a.p.hop_row = reinterpret_cast<const long long*>(d_hop_row);
    a.p.hop_coin_in = d_ci;
    a.p.hop_coin_out = d_co;
    a.p.given = d_given;
    a.p.answer = d_answer;
    a.p.hops = d_hops;
    a.rate = d_rate;
    a.hop_rate = d_hop_rate;
    if ((rc = launch(c, a)) != CFMM_OK) return rc;
    c->rate.dev_timed = c->opt_time_kernels != 0;   // the span is read when "rate_ns" is asked for (the call does not wait)
    return CFMM_OK;
}

} // namespace

int cfmm_quote_rate(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out,
                    const double* amount_in, double* amount_out, double* rate)
{
    return rate_host(c, seg, count, idx, coin_in, coin_out, amount_in, amount_out, rate);
}

int cfmm_quote_rate_dev(cfmm_ctx* c, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in, const int32_t* d_coin_out,
                        const double* d_amount_in, double* d_amount_out, double* d_rate)
{
    return rate_dev(c, seg, count, d_idx, d_coin_in, d_coin_out, d_amount_in, d_amount_out, d_rate);
}

int cfmm_quote_path_rate(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                         const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_in, double* amount_out, double* rate,
                         double* hop_out, double* hop_rate)
{
    return path_host(c, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, amount_out, rate, hop_out, hop_rate);
}

int cfmm_quote_path_rate_dev(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                             const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                             const double* d_amount_in, double* d_amount_out, double* d_rate, double* d_hop_out, double* d_hop_rate)
{
    return path_dev(c, count, max_hops, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_in, d_amount_out, d_rate,
                    d_hop_out, d_hop_rate);
}

namespace cfmm {

// read-only option "rate_ns": the span of the latest call's kernel (single pool or path) timed under "time_kernels"
int rate_ns(cfmm_ctx* c, int64_t* value)
{
    RateScratch& rs = c->rate;
    if (rs.dev_timed) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(rs.ev.stop(0)));
        if (const int rc = rs.ev.elapsed_ns(c, 0, 1, rs.ns)) return rc;
        rs.dev_timed = false;
    }
    *value = rs.ns;
    return CFMM_OK;
}

} // namespace cfmm
