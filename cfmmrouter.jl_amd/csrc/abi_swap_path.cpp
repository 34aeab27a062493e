// abi_swap_path.cpp -- cfmm_swap_path and, by a direction (Dir), cfmm_swap_path_out: swap paths that MOVE their pools, in
// query order, each path all or nothing (include/cfmm_amd.h and cfmm_amd_path_out.h have the contracts).  The exact-output
// form differs in the kernel it launches (swap_path_out_kernel: the walk from the last hop backwards), the roles of the
// amounts and the names in the messages; every line below serves both, described for the exact-input form.
// A path answers what cfmm_quote_path answers on the market as the applied paths before it left it, and each of its hops
// leaves its pool where cfmm_swap of (that hop, the amount entering it) leaves it (swap_path_kernels.h: pass 1 quotes and
// tests, pass 2 applies).
// And swap_paths_run, THE DRIVER of every executing path entry -- these two and abi_swap_order.cpp's, whose OWNERS (what is
// applied all or nothing) are orders of several paths where here every path is its own.  The host cuts the batch into waves
// of pool-disjoint owners (swap_path_waves.h), uploads the hop arrays ONCE in wave order (swap_fill.h) and launches one kernel
// per wave over its span of them.  It waits between waves only behind a wave with a UniV3 hop -- UniV3's state is its price,
// with records prepared on the host: the wave's owner statuses and landing prices are read back and the pools of the applied
// owners move through cfmm_pools_set_prices' own apply path (abi_update.cpp univ3_move_prices), after which the segment table
// is rebuilt (a moved pool may have regrown the record arrays).  Otherwise it synchronises once, at the end.
// The only memory of the feature is SwapPathScratch (ctx.h): proportional to count x max_hops, never to the pools.
#include "seg_view.h"
#include "stage_layout.h"
#include "../../include/cfmm_amd_order.h"
#include "../../include/cfmm_amd_path_out.h"
#include "swap_path_checks.h"

#include <algorithm>
#include <utility>

using namespace cfmm;

static_assert(CFMM_PATH_APPLIED == 0 && CFMM_SWAP_APPLIED == 0 && CFMM_ORDER_APPLIED == 0, "status 0 is APPLIED in every executing entry");

int cfmm::swap_paths_run(cfmm_ctx* c, bool exact_out, const SwapPathCall& q, SwapWaveLaunch launch)
{
    HIP_TRY(c, hipSetDevice(c->device));
    SwapPathScratch& sc = c->swap_path;
    const size_t G = (size_t)q.orders, n = (size_t)q.n_paths, H = (size_t)q.max_hops, nh = n * H, owners = G ? G : n;
    const size_t so = G ? n : 0;   // where the owners' statuses start in the status column
    const SwapPathPlan plan = swap_wave_plan((int64_t)owners, q.order_first, q.n_paths, q.hop.n_hops, q.hop.seg, q.hop.row, &sc.pools);
    const int64_t waves = (int64_t)plan.wave_off.size() - 1;
    const bool timed = c->opt_time_kernels != 0;
    const size_t nseg = c->segs.size(), nrec = table_records(c);
    const SwapPathStage lay(nrec * sizeof(SwapPathSeg), nrec, n, nh, G);   // the pinned staging (stage_layout.h)
    int rc;
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.table.grow(c, nrec)) || (rc = sc.hop_i32.grow(c, lay.i32.n)) ||
        (rc = sc.i64.grow(c, lay.row.n)) || (rc = sc.amt.grow(c, lay.amt.n)) || (rc = sc.out.grow(c, lay.out.n)) || (rc = sc.hops.grow(c, nh)) ||
        (rc = sc.price.grow(c, nh)) || (rc = sc.status.grow(c, lay.status.n)) || (rc = sc.left.grow(c, nrec)) ||
        (timed && (rc = sc.ev.ensure(c, (size_t)waves))))
        return rc;
    unsigned long long* st = sc.stage.host();
    SwapPathSeg* h_table = reinterpret_cast<SwapPathSeg*>(lay.table.in(st));
    int32_t *h_i32 = lay.i32.in(st), *h_seg = h_i32 + n, *h_status = lay.status.in(st);
    long long *h_row = lay.row.in(st), *h_first = h_row + nh;   // h_first[j] (orders): where the order at position j starts in the launch order
    double *h_amt = lay.amt.in(st), *h_out = lay.out.in(st), *h_hops = lay.hops.in(st), *h_price = lay.price.in(st);
    int* h_left = lay.left.in(st);
    // THE difference between the two kinds of entry, stated once: where the owner at position j of the launch order starts
    // among the paths (a path that is its own owner: at j), and -- `so` above -- where the owners' statuses stand
    const auto first_path = [&](size_t j) { return G ? (size_t)h_first[j] : j; };
    fill_launch_order(plan, q.order_first, n, H, q.hop, q.given, q.limit, h_i32, h_row, h_amt);
    // table (seg_view.h: rebuilt from the segments' current addresses, one window flag per segment) -> staging -> device
    const auto upload_table = [&]() {
        build_table(c, h_table, [&](const Segment& s, size_t i) { return swap_path_seg(s, sc.left.get() + i); });
        HIP_TRY(c, hipMemcpyAsync(sc.table.get(), h_table, nrec * sizeof(SwapPathSeg), hipMemcpyHostToDevice, c->stream));
        return (int)CFMM_OK;
    };
    armed_cancel(c);
    if ((rc = upload_table()) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(sc.hop_i32.get(), h_i32, lay.i32.n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.i64.get(), h_row, lay.row.n * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, (n + (q.limit ? owners : 0)) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(sc.left.get(), 0, nrec * sizeof(int), c->stream));
    swap_invalidate(c);   // from the first launch on the pools count as moved
    bool any_univ3 = false;
    for (const Segment& s : c->segs) any_univ3 = any_univ3 || (s.kind == CFMM_KIND_UNIV3 && s.m > 0);
    std::vector<std::vector<std::pair<int64_t, double>>> moved(any_univ3 ? nseg : 0);   // per UniV3 segment: {row, landing price}
    std::vector<int64_t> rows;
    std::vector<double> prices;
    for (int64_t w = 0; w < waves; ++w) {
        const size_t off = (size_t)plan.wave_off[(size_t)w], nw = (size_t)plan.wave_off[(size_t)w + 1] - off;   // the wave's span of the owners
        const size_t p0 = first_path(off), p1 = first_path(off + nw);                                            // ... and of the paths
        // the paths the launch sees: with orders all of the call, the wave's orders beside them; else the wave's own
        const size_t at = G ? 0 : off;
        SwapOrderArgs a{};
        a.p.count = (int64_t)(G ? n : nw);
        a.p.stride = q.n_paths;
        a.p.max_hops = q.max_hops;
        a.p.nseg = (int32_t)nrec;
        a.p.segs = sc.table.get();
        a.p.n_hops = sc.hop_i32.get() + at;
        a.p.hop_seg = sc.hop_i32.get() + n + at;
        a.p.hop_coin_in = sc.hop_i32.get() + n + nh + at;
        a.p.hop_coin_out = sc.hop_i32.get() + n + 2 * nh + at;
        a.p.hop_row = sc.i64.get() + at;
        a.p.amount_in = sc.amt.get() + at;
        a.p.amount_out = sc.out.get() + at;
        a.p.hops = sc.hops.get() + at;
        a.p.price = sc.price.get() + at;
        a.p.status = sc.status.get() + at;
        if (G) {
            a.orders = (int64_t)nw;
            a.order_first = sc.i64.get() + nh + off;
            a.limit = q.limit ? sc.amt.get() + n + off : nullptr;
            a.total = sc.out.get() + n + off;
            a.status = sc.status.get() + n + off;
        } else {
            a.p.min_out = q.limit ? sc.amt.get() + n + off : nullptr;   // (the limits are the paths' own)
        }
        const hipError_t e = launch(c, exact_out, a, sc.ev.start((size_t)w, timed), sc.ev.stop((size_t)w, timed));
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "%s launch failed: %s (earlier waves of the call have moved their pools)", q.what, hipGetErrorString(e));
        if (!any_univ3) continue;
        // which hop levels of the wave hold a UniV3 hop
        bool level[CFMM_MAX_PATH_HOPS] = {};
        bool some = false;
        for (size_t p = p0; p < p1; ++p)
            for (size_t k = 0; k < (size_t)h_i32[p]; ++k)
                if (c->segs[(size_t)h_seg[k * n + p]].kind == CFMM_KIND_UNIV3) level[k] = some = true;
        if (!some) continue;
        // the wave's owner statuses and landing prices; then the pools of its applied owners move as cfmm_pools_set_prices moves them
        HIP_TRY(c, hipMemcpyAsync(h_status + so + off, sc.status.get() + so + off, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        for (size_t k = 0; k < H; ++k)
            if (level[k]) HIP_TRY(c, hipMemcpyAsync(h_price + k * n + p0, sc.price.get() + k * n + p0, (p1 - p0) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t j = off; j < off + nw; ++j) {
            if (h_status[so + j] != 0) continue;   // (APPLIED is 0)
            for (size_t p = first_path(j); p < first_path(j + 1); ++p)
                for (size_t k = 0; k < (size_t)h_i32[p]; ++k) {
                    const size_t seg = (size_t)h_seg[k * n + p];
                    const Segment& s = c->segs[seg];
                    if (s.kind != CFMM_KIND_UNIV3) continue;
                    const int64_t row = h_row[k * n + p];
                    double P;   // (the landing price is finite and > 0: the kernel has refused the owner otherwise)
                    if (univ3_landing(h_price[k * n + p], s.lad.lower_ticks(row)[0], s.h_cp[(size_t)row], P)) moved[seg].push_back({row, P});
                }
        }
        bool replaced = false;
        for (size_t seg = 0; seg < nseg; ++seg) {
            if (moved[seg].empty()) continue;
            std::sort(moved[seg].begin(), moved[seg].end());   // univ3_move_prices takes its rows ascending (distinct: one wave)
            rows.clear();
            prices.clear();
            for (const auto& rp : moved[seg]) {
                rows.push_back(rp.first);
                prices.push_back(rp.second);
            }
            moved[seg].clear();
            if ((rc = univ3_move_prices(c, c->segs[seg], rows, prices.data())) != CFMM_OK) return rc;
            replaced = true;
        }
        // (the stream is idle up to the moves just enqueued, which do not read the staging's table: it may be rewritten)
        if (replaced && w + 1 < waves && (rc = upload_table()) != CFMM_OK) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), lay.out.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), lay.status.n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (q.hop_ans) HIP_TRY(c, hipMemcpyAsync(h_hops, sc.hops.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_left, sc.left.get(), nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nseg; ++i)
        if (h_left[i]) c->segs[i].fast_ok = 0;   // (never sent back: as cfmm_update_reserves)
    if (timed && (rc = sc.ev.elapsed_ns(c, 0, (size_t)waves, c->swap.ns)) != CFMM_OK) return rc;
    c->swap.refused = scatter_to_caller(plan, q.order_first, n, H, h_out, h_status, h_hops, q.answer, q.path_status, q.hop_ans, q.total, q.status);
    c->swap.launches = waves;
    return CFMM_OK;
}

namespace {

constexpr Dir kForward{false, "cfmm_swap_path", nullptr, nullptr};
constexpr Dir kInverse{true, "cfmm_swap_path_out", nullptr, nullptr};

// One call of either direction.  given / limit / answer / hop_ans: amount_in, min_amount_out, amount_out, hop_out of
// cfmm_swap_path; amount_out, max_amount_in, amount_in, hop_in of cfmm_swap_path_out.
int swap_path_host(cfmm_ctx* c, const Dir& dir, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                   const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* given,
                   const double* limit, double* answer, double* hop_ans, int32_t* status)
{
    const char* who = dir.who;
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // a path's hops may sit on different shards: all-or-nothing across devices is a change of its own
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (a path's hops may sit on different shards)", who);
    char msg[256] = "";
    const std::vector<PathSegInfo> info = seg_infos(c);
    int rc = check_paths(who, dir.exact_out, info.data(), (int64_t)info.size(), count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out,
                         given, msg, sizeof msg);
    if (rc == CFMM_OK) rc = check_swap_paths(who, count, n_hops, hop_seg, hop_row, limit, msg, sizeof msg, dir.exact_out);
    if (rc != CFMM_OK) return fail(c, rc, "%s", msg);
    if (count > 0 && !answer) return fail(c, CFMM_ERR_INVALID_ARG, "%s: null path array", who);
    if (count == 0) return CFMM_OK;   // a no-op that invalidates nothing
    const SwapPathCall q{"swap path", 0, nullptr, count, max_hops, {n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out}, given, limit, answer, hop_ans,
                         status, nullptr, nullptr};
    return swap_paths_run(c, dir.exact_out, q, [](const cfmm_ctx* c, bool exact_out, const SwapOrderArgs& a, hipEvent_t e0, hipEvent_t e1) {
        return (exact_out ? launch_swap_path_out : launch_swap_path)(a.p, c->stream, e0, e1);
    });
}

} // namespace

extern "C" int cfmm_swap_path(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                              const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_in,
                              const double* min_amount_out, double* amount_out, double* hop_out, int32_t* status)
{
    return swap_path_host(c, kForward, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, min_amount_out,
                          amount_out, hop_out, status);
}

extern "C" int cfmm_swap_path_out(cfmm_ctx* c, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                                  const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_out,
                                  const double* max_amount_in, double* amount_in, double* hop_in, int32_t* status)
{
    return swap_path_host(c, kInverse, count, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, max_amount_in,
                          amount_in, hop_in, status);
}
