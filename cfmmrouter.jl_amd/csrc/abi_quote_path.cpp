// abi_quote_path.cpp -- cfmm_quote_path / cfmm_quote_path_out and their _dev forms: an amount carried through a path of up to
// CFMM_MAX_PATH_HOPS pools that may lie in different segments, one launch for all paths (the kernels: quote_path_kernels.h;
// the per-hop forms are cfmm_quote's own, quote_pool.h; the checks: path_checks.h).  As in abi_quote.cpp the two directions
// share every line: `given` / `answer` are amount_in / amount_out of the forward entries and amount_out / amount_in of the
// inverse ones, `hops` is hop_out / hop_in.
// Read-only.  The kernels see the segments through a table of PathSeg records in device memory, rebuilt and uploaded on every
// call by the rig these entries share with cfmm_size_path and cfmm_split_paths (ctx.h PathRig, path_rig.h).
// The only memory of the feature is PathScratch (ctx.h): proportional to count x max_hops, never to the pools.
#include "path_rig.h"
#include "stage_layout.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace cfmm;

namespace {

constexpr Dir kForward{false, "cfmm_quote_path", "cfmm_quote_path_dev", nullptr};
constexpr Dir kInverse{true, "cfmm_quote_path_out", "cfmm_quote_path_out_dev", nullptr};

// the staging of a call of n paths (stage_layout.h PathStage)
PathStage stage_of(const cfmm_ctx* c, size_t n, size_t nh, bool want_hops) { return PathStage(table_records(c) * sizeof(PathSeg), n, nh, want_hops); }

// (the span goes to QuoteScratch's events: "quote_ns")
int launch(cfmm_ctx* c, const Dir& dir, const PathArgs& a)
{
    return c->path.launch(c, c->quote.ev, "quote path",
                          [&](hipEvent_t e0, hipEvent_t e1) { return launch_quote_path(dir.exact_out, a, c->stream, e0, e1); });
}

// A parent: the paths are walked hop level by hop level through the per-segment parent path (cfmm_quote / cfmm_quote_out ->
// multi_quote), one call per level and segment that has an active path; the +inf / NaN rule is applied here.  Everything was
// checked by the caller; the answers are written only when every call has succeeded.
int multi_path(cfmm_ctx* c, const Dir& dir, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
               const int64_t* hop_row, const int32_t* ci, const int32_t* co, const double* given, double* answer, double* hops)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t n = (size_t)count, nseg = c->psegs.size();
    std::vector<double> x(given, given + n), hv(hops ? n * (size_t)max_hops : 0, nan), out;
    std::vector<std::vector<int64_t>> where(nseg), rows(nseg);
    std::vector<std::vector<int32_t>> cis(nseg), cos(nseg);
    std::vector<std::vector<double>> amts(nseg);
    int64_t ns = 0;
    for (int step = 0; step < max_hops; ++step) {
        const int k = dir.exact_out ? max_hops - 1 - step : step;
        for (size_t s = 0; s < nseg; ++s) { where[s].clear(); rows[s].clear(); cis[s].clear(); cos[s].clear(); amts[s].clear(); }
        for (size_t p = 0; p < n; ++p) {
            if (k >= n_hops[p]) continue;
            const size_t at = (size_t)k * n + p;
            if (!(x[p] >= 0.0) || !std::isfinite(x[p])) {   // the kernels' rule: exact output passes +inf / NaN on unevaluated,
                if (!dir.exact_out || x[p] < 0.0) x[p] = nan;   // anything else that is no amount becomes NaN
                if (hops) hv[at] = x[p];
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
            const int rc = (dir.exact_out ? cfmm_quote_out : cfmm_quote)(c, (int32_t)s, (int64_t)where[s].size(), rows[s].data(), cis[s].data(),
                                                                         cos[s].data(), amts[s].data(), out.data());
            if (rc != CFMM_OK) return rc;   // (the message is the inner call's)
            if (c->opt_time_kernels != 0) ns = std::max(ns, c->quote.ns);
            for (size_t j = 0; j < where[s].size(); ++j) {
                const size_t p = (size_t)where[s][j];
                x[p] = out[j];
                if (hops) hv[(size_t)k * n + p] = out[j];
            }
        }
    }
    c->quote.ns = ns;   // "quote_ns" of a parent: the longest span among the calls THIS entry made
    std::memcpy(answer, x.data(), n * sizeof(double));
    if (hops) std::memcpy(hops, hv.data(), hv.size() * sizeof(double));
    return CFMM_OK;
}

// Pinned staging behind the table (stage_layout.h PathStage), copied to / from the scratch's device arrays in stream order; one
// synchronisation.
int path_host(cfmm_ctx* c, const Dir& dir, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
              const int64_t* hop_row, const int32_t* ci, const int32_t* co, const double* given, double* answer, double* hops)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    char msg[256] = "";
    const std::vector<PathSegInfo> info = seg_infos(c);
    int rc = check_paths(dir.who, dir.exact_out, info.data(), (int64_t)info.size(), count, max_hops, n_hops, hop_seg, hop_row, ci, co,
                         given, msg, sizeof msg);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count > 0 && !answer) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", dir.who);
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty()) return multi_path(c, dir, count, max_hops, n_hops, hop_seg, hop_row, ci, co, given, answer, hops);

    HIP_TRY(c, hipSetDevice(c->device));
    PathScratch& ps = c->path;
    const size_t n = (size_t)count, H = (size_t)max_hops, nh = n * H;
    const PathStage lay = stage_of(c, n, nh, hops != nullptr);
    PathArgs a{};
    if ((rc = ps.upload_table(c, lay, a.nseg)) || (rc = ps.hop_i32.grow(c, n + 3 * nh)) || (rc = ps.hop_row.grow(c, nh)) ||
        (rc = ps.given.grow(c, n)) || (rc = ps.answer.grow(c, n)) || (hops && (rc = ps.hops.grow(c, nh))))
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
    a.count = count;
    a.max_hops = max_hops;
    a.segs = ps.table.get();
    a.n_hops = ps.hop_i32.get();
    a.hop_seg = ps.hop_i32.get() + n;
    a.hop_coin_in = ps.hop_i32.get() + n + nh;
    a.hop_coin_out = ps.hop_i32.get() + n + 2 * nh;
    a.hop_row = ps.hop_row.get();
    a.given = ps.given.get();
    a.answer = ps.answer.get();
    a.hops = hops ? ps.hops.get() : nullptr;
    if ((rc = launch(c, dir, a)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_answer, ps.answer.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (hops) HIP_TRY(c, hipMemcpyAsync(h_hops, ps.hops.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ps.in_flight = false;
    if (c->opt_time_kernels != 0) {
        if ((rc = c->quote.ev.elapsed_ns(c, 0, 1, c->quote.ns)) != CFMM_OK) return rc;
        c->quote.dev_timed = false;
    }
    std::memcpy(answer, h_answer, n * sizeof(double));
    if (hops) std::memcpy(hops, h_hops, nh * sizeof(double));
    return CFMM_OK;
}

int path_dev(cfmm_ctx* c, const Dir& dir, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
             const int64_t* d_hop_row, const int32_t* d_ci, const int32_t* d_co, const double* d_given, double* d_answer, double* d_hops)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text, with the entry's name from the Dir)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", dir.dev);
    char msg[256] = "";
    int rc = check_path_scalars(dir.dev, count, max_hops, msg, sizeof msg);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    if (!d_n_hops || !d_hop_seg || !d_hop_row || !d_ci || !d_co || !d_given || !d_answer)
        return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", dir.dev);
    HIP_TRY(c, hipSetDevice(c->device));
    PathArgs a{};
    if ((rc = c->path.upload_table(c, stage_of(c, 0, 0, false), a.nseg)) != CFMM_OK) return rc;
    a.count = count;
    a.max_hops = max_hops;
    a.segs = c->path.table.get();
    a.n_hops = d_n_hops;
    a.hop_seg = d_hop_seg;
    a.hop_row = reinterpret_cast<const long long*>(d_hop_row);
    a.hop_coin_in = d_ci;
    a.hop_coin_out = d_co;
    a.given = d_given;
    a.answer = d_answer;
    a.hops = d_hops;
    if ((rc = launch(c, dir, a)) != CFMM_OK) return rc;
    c->quote.dev_timed = c->opt_time_kernels != 0;   // the span is read when "quote_ns" is asked for (the call does not wait)
    return CFMM_OK;
}

} // namespace

int cfmm_quote_path(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                    const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_in, double* amount_out, double* hop_out)
{
    return path_host(c, kForward, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, amount_out, hop_out);
}

int cfmm_quote_path_out(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                        const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_out,
                        double* amount_in, double* hop_in)
{
    return path_host(c, kInverse, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, amount_in, hop_in);
}

int cfmm_quote_path_dev(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                        const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                        const double* d_amount_in, double* d_amount_out, double* d_hop_out)
{
    return path_dev(c, kForward, count, max_hops, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_in,
                    d_amount_out, d_hop_out);
}

int cfmm_quote_path_out_dev(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                            const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                            const double* d_amount_out, double* d_amount_in, double* d_hop_in)
{
    return path_dev(c, kInverse, count, max_hops, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_out,
                    d_amount_in, d_hop_in);
}
