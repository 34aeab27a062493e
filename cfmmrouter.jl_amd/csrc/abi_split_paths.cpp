// abi_split_paths.cpp -- cfmm_split_paths / cfmm_split_paths_dev (include/cfmm_amd_split.h): an order's amount spread over its
// 1 .. 8 paths by a greedy search of rounds x 64 grid points per path in ONE launch, one wavefront per order (the kernel:
// split_paths_kernels.h; the search's arithmetic: split_grid.h, shared with it; the checks: split_checks.h and path_checks.h).
// And their exact-output twins cfmm_split_paths_out / cfmm_split_paths_out_dev (include/cfmm_amd_split_out.h;
// split_paths_out_kernels.h, split_out_grid.h): the same checks, staging, scratch and launch rule -- `Way` below says which
// entry is running; p.answer / path_out / total then carry the shares of the wanted amount, their costs and the total cost.
// Read-only.  As in abi_size_path.cpp the kernel sees the segments through a table of PathSeg records in device memory,
// rebuilt and uploaded on every call by the rig of the read-only path entries (ctx.h TimedPathRig, path_rig.h).  The only
// memory of the feature is SplitScratch (ctx.h): proportional to the orders and to n_paths x max_hops, never to the pools.
// A multi-device parent runs the search on the host (multi_split over split_search.h): per round one cfmm_quote_path /
// cfmm_quote_path_out call of 64 x n_paths paths through the parent path, the grid points, the greedy and the status by
// split_grid.h / split_out_grid.h -- the text the kernels compile -- so the answers are the same bits.
#include "path_rig.h"
#include "split_checks.h"
#include "split_search.h"
#include "stage_layout.h"

#include <cstring>
#include <vector>

using namespace cfmm;

namespace {

// which entry: its names in refusals and in the launch error, what it calls the amount, and its launcher
struct Way {
    const char *who, *who_dev, *amount_name, *what;
    hipError_t (*launch)(const SplitArgs&, int64_t, hipStream_t, hipEvent_t, hipEvent_t);
    bool out;
};
constexpr Way kIn = {"cfmm_split_paths", "cfmm_split_paths_dev", "amount_in", "split paths", &launch_split_paths, false};
constexpr Way kOut = {"cfmm_split_paths_out", "cfmm_split_paths_out_dev", "amount_out", "split paths out", &launch_split_paths_out, true};

SplitStage stage_of(const cfmm_ctx* c, size_t g, size_t n, size_t nh) { return SplitStage(table_records(c) * sizeof(PathSeg), g, n, nh); }

int launch(cfmm_ctx* c, const Way& w, const SplitArgs& a)
{
    SplitScratch& sc = c->split;
    const int rc = sc.launch(c, sc.ev, w.what,
                             [&](hipEvent_t e0, hipEvent_t e1) { return w.launch(a, c->opt_split_max_blocks, c->stream, e0, e1); });
    if (rc == CFMM_OK) sc.launches = 1;
    return rc;
}

// A parent.  Per round the 64 grid points of every path go through the parent path of cfmm_quote_path (the twin:
// cfmm_quote_path_out) over the call's hop arrays repeated 64 times; the rest is split_search.h, order by order.  Everything
// was checked by the caller; the answers are written only when every call has succeeded.
int multi_split(cfmm_ctx* c, const Way& w, int64_t count, const int64_t* order_first, const double* amount, int64_t n_paths, int32_t max_hops,
                const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* ci, const int32_t* co,
                int32_t rounds, double* path_x, double* path_y, double* total_y, int32_t* status)
{
    const GridPaths gp(n_paths, max_hops, n_hops, hop_seg, hop_row, ci, co);
    int64_t ns = 0;
    const auto quote = [&](int64_t N, const double* x, double* y) {
        const int rc = (w.out ? cfmm_quote_path_out : cfmm_quote_path)(c, N, max_hops, gp.nh.data(), gp.seg.data(), gp.row.data(), gp.cin.data(),
                                                                       gp.cot.data(), x, y, nullptr);
        if (rc == CFMM_OK && c->opt_time_kernels != 0) ns += c->quote.ns;
        return rc;   // (the message is the inner call's)
    };
    const int rc = w.out ? split_search<SplitOut>(quote, count, order_first, amount, n_paths, rounds, path_x, path_y, total_y, status)
                         : split_search<SplitIn>(quote, count, order_first, amount, n_paths, rounds, path_x, path_y, total_y, status);
    if (rc != CFMM_OK) return rc;
    SplitScratch& sc = c->split;
    sc.ns = ns;
    sc.dev_timed = false;
    sc.launches = rounds;
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
        return multi_split(c, w, count, order_first, amount_in, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds,
                           path_amount_in, path_amount_out, total_out, status);

    HIP_TRY(c, hipSetDevice(c->device));
    SplitScratch& sc = c->split;
    const size_t g = (size_t)count, n = (size_t)n_paths, H = (size_t)max_hops, nh = n * H;
    const SplitStage lay = stage_of(c, g, n, nh);
    SplitArgs a{};
    if ((rc = sc.upload_table(c, lay, a.p.nseg)) || (rc = sc.hop_i32.grow(c, n + 3 * nh)) || (rc = sc.i64.grow(c, nh + g + 1)) ||
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
    if ((rc = c->split.upload_table(c, stage_of(c, 0, 0, 0), a.p.nseg)) != CFMM_OK) return rc;
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
