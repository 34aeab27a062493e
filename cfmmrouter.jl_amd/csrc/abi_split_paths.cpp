// abi_split_paths.cpp -- cfmm_split_paths / cfmm_split_paths_dev (include/cfmm_amd_split.h): an order's amount spread over its
// 1 .. 8 paths by a greedy search of rounds x 64 grid points per path in ONE launch, one wavefront per order (the kernel:
// split_paths_kernels.h; the search's arithmetic: split_grid.h, shared with it; the checks: split_checks.h and path_checks.h).
// And their exact-output twins cfmm_split_paths_out / cfmm_split_paths_out_dev (include/cfmm_amd_split_out.h;
// split_paths_out_kernels.h, split_out_grid.h): the same checks, staging, scratch and launch rule -- `Way` below says which
// entry is running; p.answer / path_out / total then carry the shares of the wanted amount, their costs and the total cost.
// Read-only.  As in abi_size_path.cpp the kernel sees the segments through a table of PathSeg records in device memory, which
// upload_table below REBUILDS FROM THE SEGMENTS' CURRENT ADDRESSES (seg_view.h) AND UPLOADS ON EVERY CALL: a table kept across
// calls would hold a freed address.  The only memory of the feature is SplitScratch (ctx.h): proportional to the orders and to
// n_paths x max_hops, never to the pools.
// A multi-device parent runs the search on the host (multi_split): per round one cfmm_quote_path call of 64 x n_paths paths
// through the parent path, the grid points, the greedy and the status by split_grid.h -- the text the kernel compiles -- so the
// answers are the same bits (the twin: multi_split_out, over cfmm_quote_path_out and split_out_grid.h).
#include "seg_view.h"
#include "split_checks.h"
#include "split_out_grid.h"
#include "stage_layout.h"

#include <cstring>
#include <vector>

using namespace cfmm;

namespace {

// which entry: its names in refusals, what it calls the amount, and its launcher
struct Way {
    const char *who, *who_dev, *amount_name;
    hipError_t (*launch)(const SplitArgs&, int64_t, hipStream_t, hipEvent_t, hipEvent_t);
    bool out;
};
constexpr Way kIn = {"cfmm_split_paths", "cfmm_split_paths_dev", "amount_in", &launch_split_paths, false};
constexpr Way kOut = {"cfmm_split_paths_out", "cfmm_split_paths_out_dev", "amount_out", &launch_split_paths_out, true};

int refuse(cfmm_ctx* c, int rc, const char* msg) { return rc == CFMM_OK ? rc : fail(c, rc, "%s", msg); }

// The staging is free again, the table may be rewritten: the call before has left the device (`done` sits behind its kernel)
int wait_previous(cfmm_ctx* c)
{
    SplitScratch& sc = c->split;
    if (sc.in_flight) HIP_TRY(c, hipEventSynchronize(sc.done.get()));
    sc.in_flight = false;
    return CFMM_OK;
}

SplitStage stage_of(const cfmm_ctx* c, size_t g, size_t n, size_t nh) { return SplitStage(table_records(c) * sizeof(PathSeg), g, n, nh); }

// table (seg_view.h: rebuilt from the segments' current addresses) -> staging -> device, in stream order
int upload_table(cfmm_ctx* c, const SplitStage& lay, int32_t& nrec_out)
{
    SplitScratch& sc = c->split;
    const size_t nrec = table_records(c);
    int rc;
    if ((rc = wait_previous(c)) || (rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.table.grow(c, nrec)) ||
        (rc = sc.done.create(c, hipEventDisableTiming)))
        return rc;
    PathSeg* t = reinterpret_cast<PathSeg*>(lay.table.in(sc.stage.host()));
    build_table(c, t, [](const Segment& s, size_t) { return path_seg(s); });
    HIP_TRY(c, hipMemcpyAsync(sc.table.get(), t, nrec * sizeof(PathSeg), hipMemcpyHostToDevice, c->stream));
    nrec_out = (int32_t)nrec;
    return CFMM_OK;
}

int launch(cfmm_ctx* c, const Way& w, const SplitArgs& a)
{
    SplitScratch& sc = c->split;
    const bool timed = c->opt_time_kernels != 0;
    int rc;
    if (timed && (rc = sc.ev.ensure(c, 1)) != CFMM_OK) return rc;
    const hipError_t e = w.launch(a, c->opt_split_max_blocks, c->stream, sc.ev.start(0, timed), sc.ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "split paths%s launch failed: %s", w.out ? " out" : "", hipGetErrorString(e));
    HIP_TRY(c, hipEventRecord(sc.done.get(), c->stream));
    sc.in_flight = true;
    sc.launches = 1;
    return CFMM_OK;
}

// A parent.  Per round the 64 grid points of every path (point j of path p is path j*n_paths + p of the inner call, whose hop
// arrays repeat the call's 64 times) go through cfmm_quote_path's parent path; the rest is split_grid.h, order by order.
// Everything was checked by the caller; the answers are written only when every call has succeeded.
struct GridPaths {   // the call's hop arrays, 64 times
    std::vector<int32_t> nh, seg, cin, cot;
    std::vector<int64_t> row;
    GridPaths(int64_t n_paths, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* ci,
              const int32_t* co)
    {
        constexpr size_t J = CFMM_SPLIT_POINTS;
        const size_t n = (size_t)n_paths, H = (size_t)max_hops, N = J * n;
        nh.resize(N), seg.resize(H * N), cin.resize(H * N), cot.resize(H * N), row.resize(H * N);
        for (size_t j = 0; j < J; ++j) {
            std::memcpy(&nh[j * n], n_hops, n * sizeof(int32_t));
            for (size_t k = 0; k < H; ++k) {
                std::memcpy(&seg[k * N + j * n], hop_seg + k * n, n * sizeof(int32_t));
                std::memcpy(&row[k * N + j * n], hop_row + k * n, n * sizeof(int64_t));
                std::memcpy(&cin[k * N + j * n], ci + k * n, n * sizeof(int32_t));
                std::memcpy(&cot[k * N + j * n], co + k * n, n * sizeof(int32_t));
            }
        }
    }
};

int multi_split(cfmm_ctx* c, int64_t count, const int64_t* order_first, const double* amount, int64_t n_paths, int32_t max_hops,
                const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* ci, const int32_t* co,
                int32_t rounds, double* path_in, double* path_out, double* total_out, int32_t* status)
{
    constexpr size_t J = CFMM_SPLIT_POINTS;
    constexpr int KMAX = CFMM_MAX_SPLIT_PATHS;
    const size_t n = (size_t)n_paths, N = J * n, G = (size_t)count;
    const GridPaths gp(n_paths, max_hops, n_hops, hop_seg, hop_row, ci, co);
    std::vector<double> base(n, 0.0), rem(amount, amount + G), x(N), y(N);
    std::vector<int> slices(n, 0);
    std::vector<char> any_nan(G, 0), last_flat(G, 0);
    SplitScratch& sc = c->split;
    int64_t ns = 0;
    for (int r = 0; r < rounds; ++r) {
        for (size_t g = 0; g < G; ++g) {
            const double s = split_slice(rem[g]);
            for (size_t p = (size_t)order_first[g]; p < (size_t)order_first[g + 1]; ++p)
                for (size_t j = 0; j < J; ++j) x[j * n + p] = split_point(base[p], s, rem[g], (int)j);
        }
        const int rc = cfmm_quote_path(c, (int64_t)N, max_hops, gp.nh.data(), gp.seg.data(), gp.row.data(), gp.cin.data(), gp.cot.data(),
                                       x.data(), y.data(), nullptr);
        if (rc != CFMM_OK) return rc;   // (the message is the inner call's)
        if (c->opt_time_kernels != 0) ns += c->quote.ns;
        for (size_t g = 0; g < G; ++g) {
            const size_t first = (size_t)order_first[g];
            const int K = (int)(order_first[g + 1] - order_first[g]);
            int cnt[KMAX];
            const int flags = split_greedy(
                K, [&](int k, int at) { return y[(size_t)(at + 1) * n + first + (size_t)k] - y[(size_t)at * n + first + (size_t)k]; }, cnt);
            any_nan[g] = any_nan[g] || (flags & kSplitStepNan) != 0;
            last_flat[g] = (flags & kSplitStepFlat) != 0;
            for (int k = 0; k < K; ++k) slices[first + (size_t)k] = cnt[k];
            if (r + 1 < rounds) {
                double sum = 0.0;
                for (int k = 0; k < K; ++k) {
                    const size_t p = first + (size_t)k;
                    base[p] = x[(size_t)split_back(cnt[k]) * n + p];
                    sum = k == 0 ? base[p] : sum + base[p];
                }
                rem[g] = split_rem(amount[g], sum);
            }
        }
    }
    sc.ns = ns;
    sc.dev_timed = false;
    sc.launches = rounds;
    for (size_t g = 0; g < G; ++g) {
        const size_t first = (size_t)order_first[g];
        const int K = (int)(order_first[g + 1] - order_first[g]);
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            const double yk = y[(size_t)slices[first + (size_t)k] * n + first + (size_t)k];
            total = k == 0 ? yk : total + yk;
        }
        const int32_t st = split_status(any_nan[g] != 0, last_flat[g] != 0, amount[g], total);
        for (int k = 0; k < K; ++k) {
            const size_t p = first + (size_t)k, at = (size_t)slices[p] * n + p;
            path_in[p] = split_written(st, x[at]);
            path_out[p] = split_written(st, y[at]);
        }
        total_out[g] = split_written(st, total);
        status[g] = st;
    }
    return CFMM_OK;
}

// The twin: per round the shares x go through cfmm_quote_path_out's parent path and come back as costs; the greedy, the
// first-bad-step rule, the status and the written values by split_out_grid.h.  `share` is path_amount_out, `cost` path_amount_in.
int multi_split_out(cfmm_ctx* c, int64_t count, const int64_t* order_first, const double* amount, int64_t n_paths, int32_t max_hops,
                    const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* ci, const int32_t* co,
                    int32_t rounds, double* share, double* cost, double* total_in, int32_t* status)
{
    constexpr size_t J = CFMM_SPLIT_POINTS;
    constexpr int KMAX = CFMM_MAX_SPLIT_PATHS;
    const size_t n = (size_t)n_paths, N = J * n, G = (size_t)count;
    const GridPaths gp(n_paths, max_hops, n_hops, hop_seg, hop_row, ci, co);
    std::vector<double> base(n, 0.0), rem(amount, amount + G), x(N), y(N);
    std::vector<int> slices(n, 0), bad(G, kSplitOutClean);
    SplitScratch& sc = c->split;
    int64_t ns = 0;
    for (int r = 0; r < rounds; ++r) {
        for (size_t g = 0; g < G; ++g) {
            const double s = split_slice(rem[g]);
            for (size_t p = (size_t)order_first[g]; p < (size_t)order_first[g + 1]; ++p)
                for (size_t j = 0; j < J; ++j) x[j * n + p] = split_point(base[p], s, rem[g], (int)j);
        }
        const int rc = cfmm_quote_path_out(c, (int64_t)N, max_hops, gp.nh.data(), gp.seg.data(), gp.row.data(), gp.cin.data(), gp.cot.data(),
                                           x.data(), y.data(), nullptr);
        if (rc != CFMM_OK) return rc;   // (the message is the inner call's)
        if (c->opt_time_kernels != 0) ns += c->quote.ns;
        for (size_t g = 0; g < G; ++g) {
            const size_t first = (size_t)order_first[g];
            const int K = (int)(order_first[g + 1] - order_first[g]);
            int cnt[KMAX];
            bad[g] = split_out_greedy(
                K, [&](int k, int at) { return y[(size_t)(at + 1) * n + first + (size_t)k] - y[(size_t)at * n + first + (size_t)k]; }, cnt, bad[g]);
            for (int k = 0; k < K; ++k) slices[first + (size_t)k] = cnt[k];
            if (r + 1 < rounds) {
                double sum = 0.0;
                for (int k = 0; k < K; ++k) {
                    const size_t p = first + (size_t)k;
                    base[p] = x[(size_t)split_back(cnt[k]) * n + p];
                    sum = k == 0 ? base[p] : sum + base[p];
                }
                rem[g] = split_rem(amount[g], sum);
            }
        }
    }
    sc.ns = ns;
    sc.dev_timed = false;
    sc.launches = rounds;
    for (size_t g = 0; g < G; ++g) {
        const size_t first = (size_t)order_first[g];
        const int K = (int)(order_first[g + 1] - order_first[g]);
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            const double yk = y[(size_t)slices[first + (size_t)k] * n + first + (size_t)k];
            total = k == 0 ? yk : total + yk;
        }
        const int32_t st = split_out_status(bad[g], amount[g], total);
        for (int k = 0; k < K; ++k) {
            const size_t p = first + (size_t)k, at = (size_t)slices[p] * n + p;
            share[p] = split_out_written_share(st, x[at]);
            cost[p] = split_out_written_cost(st, y[at]);
        }
        total_in[g] = split_out_written_cost(st, total);
        status[g] = st;
    }
    return CFMM_OK;
}

void fill_args(SplitArgs& a, int64_t count, int64_t n_paths, int32_t max_hops, int32_t rounds)
{
    a.p.count = n_paths;
    a.p.max_hops = max_hops;
    a.p.given = nullptr;
    a.p.hops = nullptr;
    a.orders = count;
    a.rounds = rounds;
}

} // namespace

namespace cfmm {

int split_ns(cfmm_ctx* c, int64_t* value)
{
    SplitScratch& sc = c->split;
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

namespace {

// Both host-pointer entries (path_amount_in / path_amount_out / total_out are cfmm_split_paths' names: the twin's shares, costs
// and total cost stand in the same places).  Pinned staging behind the table (stage_layout.h SplitStage), copied to / from the
// scratch's device arrays in stream order; one synchronisation.
int split_host(cfmm_ctx* c, const Way& w, int64_t count, const int64_t* order_first, const double* amount_in, int64_t n_paths,
               int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
               const int32_t* hop_coin_out, int32_t rounds, double* path_amount_in, double* path_amount_out, double* total_out,
               int32_t* status)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    char msg[256] = "";
    const std::vector<PathSegInfo> info = seg_infos(c);
    int rc = check_split(w.who, info.data(), (int64_t)info.size(), count, order_first, amount_in, n_paths, max_hops, n_hops, hop_seg, hop_row,
                         hop_coin_in, hop_coin_out, rounds, path_amount_in, path_amount_out, total_out, status, msg, sizeof msg, w.amount_name);
    if (rc != CFMM_OK) return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    if (!c->shards.empty())
        return (w.out ? multi_split_out : multi_split)(c, count, order_first, amount_in, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in,
                                                       hop_coin_out, rounds, path_amount_in, path_amount_out, total_out, status);

    HIP_TRY(c, hipSetDevice(c->device));
    SplitScratch& sc = c->split;
    const size_t g = (size_t)count, n = (size_t)n_paths, H = (size_t)max_hops, nh = n * H;
    const SplitStage lay = stage_of(c, g, n, nh);
    SplitArgs a{};
    if ((rc = upload_table(c, lay, a.p.nseg)) || (rc = sc.hop_i32.grow(c, n + 3 * nh)) || (rc = sc.i64.grow(c, nh + g + 1)) ||
        (rc = sc.amount.grow(c, g)) || (rc = sc.out.grow(c, 2 * n + g)) || (rc = sc.status.grow(c, g)))
        return rc;
    unsigned long long* st = sc.stage.host();
    int32_t* h_i32 = lay.i32.in(st);
    long long* h_i64 = lay.row.in(st);
    double *h_amount = lay.amount.in(st), *h_out = lay.out.in(st);
    int32_t* h_status = lay.status.in(st);
    std::memcpy(h_i32, n_hops, n * sizeof(int32_t));
    std::memcpy(h_i32 + n, hop_seg, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + nh, hop_coin_in, nh * sizeof(int32_t));
    std::memcpy(h_i32 + n + 2 * nh, hop_coin_out, nh * sizeof(int32_t));
    std::memcpy(h_i64, hop_row, nh * sizeof(long long));
    std::memcpy(h_i64 + nh, order_first, (g + 1) * sizeof(long long));
    std::memcpy(h_amount, amount_in, g * sizeof(double));
    HIP_TRY(c, hipMemcpyAsync(sc.hop_i32.get(), h_i32, (n + 3 * nh) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.i64.get(), h_i64, (nh + g + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.amount.get(), h_amount, g * sizeof(double), hipMemcpyHostToDevice, c->stream));
    fill_args(a, count, n_paths, max_hops, rounds);
    a.p.segs = sc.table.get();
    a.p.n_hops = sc.hop_i32.get();
    a.p.hop_seg = sc.hop_i32.get() + n;
    a.p.hop_coin_in = sc.hop_i32.get() + n + nh;
    a.p.hop_coin_out = sc.hop_i32.get() + n + 2 * nh;
    a.p.hop_row = sc.i64.get();
    a.order_first = sc.i64.get() + nh;
    a.amount = sc.amount.get();
    a.p.answer = sc.out.get();
    a.path_out = sc.out.get() + n;
    a.total = sc.out.get() + 2 * n;
    a.status = sc.status.get();
    if ((rc = launch(c, w, a)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), (2 * n + g) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), g * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sc.in_flight = false;
    sc.dev_timed = false;
    if (c->opt_time_kernels != 0 && (rc = sc.ev.elapsed_ns(c, 0, 1, sc.ns)) != CFMM_OK) return rc;
    std::memcpy(path_amount_in, h_out, n * sizeof(double));
    std::memcpy(path_amount_out, h_out + n, n * sizeof(double));
    std::memcpy(total_out, h_out + 2 * n, g * sizeof(double));
    std::memcpy(status, h_status, g * sizeof(int32_t));
    return CFMM_OK;
}

// both device-pointer entries
int split_dev(cfmm_ctx* c, const Way& w, int64_t count, const int64_t* d_order_first, const double* d_amount_in, int64_t n_paths,
              int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg, const int64_t* d_hop_row, const int32_t* d_hop_coin_in,
              const int32_t* d_hop_coin_out, int32_t rounds, double* d_path_amount_in, double* d_path_amount_out, double* d_total_out,
              int32_t* d_status)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const char* kWhoDev = w.who_dev;
    if (is_parent(c))   // (CFMM_SINGLE_ONLY's text)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (host-pointer calls only)", kWhoDev);
    char msg[256] = "";
    int rc;
    if ((rc = check_split_scalars(kWhoDev, count, n_paths, max_hops, rounds, msg, sizeof msg)) ||
        (rc = check_split_arrays(kWhoDev, count, d_order_first, d_amount_in, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out,
                                 d_path_amount_in, d_path_amount_out, d_total_out, d_status, msg, sizeof msg)))
        return refuse(c, rc, msg);
    if (count == 0) return CFMM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    SplitArgs a{};
    if ((rc = upload_table(c, stage_of(c, 0, 0, 0), a.p.nseg)) != CFMM_OK) return rc;
    fill_args(a, count, n_paths, max_hops, rounds);
    a.p.segs = c->split.table.get();
    a.p.n_hops = d_n_hops;
    a.p.hop_seg = d_hop_seg;
    a.p.hop_row = reinterpret_cast<const long long*>(d_hop_row);
    a.p.hop_coin_in = d_hop_coin_in;
    a.p.hop_coin_out = d_hop_coin_out;
    a.order_first = reinterpret_cast<const long long*>(d_order_first);
    a.amount = d_amount_in;
    a.p.answer = d_path_amount_in;
    a.path_out = d_path_amount_out;
    a.total = d_total_out;
    a.status = d_status;
    if ((rc = launch(c, w, a)) != CFMM_OK) return rc;
    c->split.dev_timed = c->opt_time_kernels != 0;   // the span is read when "split_ns" is asked for (the call does not wait)
    return CFMM_OK;
}

} // namespace

int cfmm_split_paths(cfmm_ctx* c, int64_t count, const int64_t* order_first, const double* amount_in, int64_t n_paths, int32_t max_hops,
                     const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                     const int32_t* hop_coin_out, int32_t rounds, double* path_amount_in, double* path_amount_out, double* total_out,
                     int32_t* status)
{
    return split_host(c, kIn, count, order_first, amount_in, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds,
                      path_amount_in, path_amount_out, total_out, status);
}

int cfmm_split_paths_out(cfmm_ctx* c, int64_t count, const int64_t* order_first, const double* amount_out, int64_t n_paths, int32_t max_hops,
                         const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                         const int32_t* hop_coin_out, int32_t rounds, double* path_amount_out, double* path_amount_in, double* total_in,
                         int32_t* status)
{
    return split_host(c, kOut, count, order_first, amount_out, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds,
                      path_amount_out, path_amount_in, total_in, status);
}

int cfmm_split_paths_dev(cfmm_ctx* c, int64_t count, const int64_t* d_order_first, const double* d_amount_in, int64_t n_paths,
                         int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg, const int64_t* d_hop_row,
                         const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out, int32_t rounds, double* d_path_amount_in,
                         double* d_path_amount_out, double* d_total_out, int32_t* d_status)
{
    return split_dev(c, kIn, count, d_order_first, d_amount_in, n_paths, max_hops, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in,
                     d_hop_coin_out, rounds, d_path_amount_in, d_path_amount_out, d_total_out, d_status);
}

int cfmm_split_paths_out_dev(cfmm_ctx* c, int64_t count, const int64_t* d_order_first, const double* d_amount_out, int64_t n_paths,
                             int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg, const int64_t* d_hop_row,
                             const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out, int32_t rounds, double* d_path_amount_out,
                             double* d_path_amount_in, double* d_total_in, int32_t* d_status)
{
    return split_dev(c, kOut, count, d_order_first, d_amount_out, n_paths, max_hops, d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in,
                     d_hop_coin_out, rounds, d_path_amount_out, d_path_amount_in, d_total_in, d_status);
}
