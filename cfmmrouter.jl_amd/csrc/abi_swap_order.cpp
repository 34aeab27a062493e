// abi_swap_order.cpp -- cfmm_swap_order and, by a direction (Dir), cfmm_swap_order_out (include/cfmm_amd_order.h): orders that
// MOVE their pools, in the caller's order, each order all or nothing ACROSS its 1 .. 8 paths with one limit on its total.
// abi_swap_path.cpp's arrangement, one level up: the host cuts the batch into waves of pool-disjoint ORDERS
// (swap_order_waves.h), uploads the orders and their paths ONCE in wave order -- an order's paths stay together, so a wave is
// one span of the orders and one span of the paths -- and launches one kernel per wave over its span of orders
// (swap_order_kernels.h: eight lanes per order; pass 1 walks and tests every path, the group decides, pass 2 applies).  It
// waits between waves only behind a wave with a UniV3 hop: the wave's order statuses and landing prices are read back and the
// UniV3 pools of the APPLIED ORDERS move through cfmm_pools_set_prices' own apply path (abi_update.cpp univ3_move_prices),
// after which the segment table is rebuilt.  Otherwise it synchronises once, at the end.
// The only memory of the feature is SwapOrderScratch (ctx.h): proportional to the orders and to n_paths x max_hops, never to
// the pools.
#include "seg_view.h"
#include "stage_layout.h"
#include "../../include/cfmm_amd_order.h"
#include "order_checks.h"
#include "swap_order_waves.h"
#include "univ3_pool.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

using namespace cfmm;

static_assert(CFMM_ORDER_APPLIED == kOrderApplied && CFMM_ORDER_LIMIT == kOrderLimit && CFMM_ORDER_REFUSED == kOrderRefused &&
              CFMM_ORDER_UNOBTAINABLE == kOrderUnobtainable && CFMM_ORDER_PATH_HELD == kOrderPathHeld, "the kernel's codes are the header's");

namespace {

constexpr Dir kForward{false, "cfmm_swap_order", nullptr, nullptr};
constexpr Dir kInverse{true, "cfmm_swap_order_out", nullptr, nullptr};

// table (seg_view.h: rebuilt from the segments' current addresses, one window flag per segment) -> staging -> device
int upload_table(cfmm_ctx* c, SwapPathSeg* t)
{
    SwapOrderScratch& sc = c->swap_order;
    build_table(c, t, [&](const Segment& s, size_t i) { return swap_path_seg(s, sc.left.get() + i); });
    HIP_TRY(c, hipMemcpyAsync(sc.table.get(), t, table_records(c) * sizeof(SwapPathSeg), hipMemcpyHostToDevice, c->stream));
    return CFMM_OK;
}

// One call of either direction.  given / limit / answer / hop_ans / total: path_amount_in, min_total_out, path_amount_out,
// hop_out, total_out of cfmm_swap_order; path_amount_out, max_total_in, path_amount_in, hop_in, total_in of cfmm_swap_order_out.
int swap_order_host(cfmm_ctx* c, const Dir& dir, int64_t count, const int64_t* order_first, int64_t n_paths, int32_t max_hops,
                    const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                    const int32_t* hop_coin_out, const double* given, const double* limit, double* answer, double* hop_ans, double* total,
                    int32_t* path_status, int32_t* status)
{
    const char* who = dir.who;
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (is_parent(c))   // an order's hops may sit on different shards: all-or-nothing across devices is a change of its own
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s is not available on a multi-device context (an order's hops may sit on different shards)", who);
    char msg[256] = "";
    const std::vector<PathSegInfo> info = seg_infos(c);
    int rc = check_orders(who, dir.exact_out, info.data(), (int64_t)info.size(), count, order_first, n_paths, max_hops, n_hops, hop_seg, hop_row,
                          hop_coin_in, hop_coin_out, given, limit, answer, total, status, msg, sizeof msg);
    if (rc != CFMM_OK) return fail(c, rc, "%s", msg);
    if (count == 0) return CFMM_OK;   // a no-op that invalidates nothing

    HIP_TRY(c, hipSetDevice(c->device));
    const SwapPathPlan plan = swap_order_plan(count, order_first, n_paths, n_hops, hop_seg, hop_row, &c->swap_order.pools);
    const int64_t waves = (int64_t)plan.wave_off.size() - 1;
    const bool timed = c->opt_time_kernels != 0;
    SwapOrderScratch& sc = c->swap_order;
    const size_t G = (size_t)count, n = (size_t)n_paths, H = (size_t)max_hops, nh = n * H, nseg = c->segs.size(), nrec = table_records(c);
    const SwapOrderStage lay(nrec * sizeof(SwapPathSeg), nrec, G, n, nh);   // the pinned staging (stage_layout.h)
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.table.grow(c, nrec)) || (rc = sc.hop_i32.grow(c, n + 3 * nh)) ||
        (rc = sc.i64.grow(c, nh + G + 1)) || (rc = sc.amt.grow(c, n + G)) || (rc = sc.out.grow(c, n + G)) || (rc = sc.hops.grow(c, nh)) ||
        (rc = sc.price.grow(c, nh)) || (rc = sc.status.grow(c, n + G)) || (rc = sc.left.grow(c, nrec)) ||
        (timed && (rc = sc.ev.ensure(c, (size_t)waves))))
        return rc;
    unsigned long long* st = sc.stage.host();
    SwapPathSeg* h_table = reinterpret_cast<SwapPathSeg*>(lay.table.in(st));
    int32_t *h_i32 = lay.i32.in(st), *h_seg = h_i32 + n, *h_ci = h_i32 + n + nh, *h_co = h_i32 + n + 2 * nh, *h_status = lay.status.in(st);
    long long *h_row = lay.row.in(st), *h_first = h_row + nh;   // h_first[j]: where the order at position j starts in the launch order
    double* h_amt = lay.amt.in(st);   // [n_paths] the given amounts, then [count] the limits
    double *h_out = lay.out.in(st), *h_hops = lay.hops.in(st), *h_price = lay.price.in(st);
    int* h_left = lay.left.in(st);
    // the orders in launch order, each with its paths behind one another; the slots a path does not use are zeroed (never
    // read by the kernel)
    std::memset(h_seg, 0, 3 * nh * sizeof(int32_t));
    std::memset(h_row, 0, nh * sizeof(long long));
    size_t at = 0;
    for (size_t j = 0; j < G; ++j) {
        const size_t g = (size_t)plan.perm[j];
        h_first[j] = (long long)at;
        if (limit) h_amt[n + j] = limit[g];
        for (size_t q = (size_t)order_first[g]; q < (size_t)order_first[g + 1]; ++q, ++at) {
            h_i32[at] = n_hops[q];
            h_amt[at] = given[q];
            for (size_t k = 0; k < (size_t)n_hops[q]; ++k) {
                h_seg[k * n + at] = hop_seg[k * n + q];
                h_row[k * n + at] = hop_row[k * n + q];
                h_ci[k * n + at] = hop_coin_in[k * n + q];
                h_co[k * n + at] = hop_coin_out[k * n + q];
            }
        }
    }
    h_first[G] = (long long)at;   // == n_paths
    armed_cancel(c);
    if ((rc = upload_table(c, h_table)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(sc.hop_i32.get(), h_i32, (n + 3 * nh) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.i64.get(), h_row, (nh + G + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, (n + (limit ? G : 0)) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(sc.left.get(), 0, nrec * sizeof(int), c->stream));
    swap_invalidate(c);   // from the first launch on the pools count as moved
    bool any_univ3 = false;
    for (const Segment& s : c->segs) any_univ3 = any_univ3 || (s.kind == CFMM_KIND_UNIV3 && s.m > 0);
    std::vector<std::vector<std::pair<int64_t, double>>> moved(any_univ3 ? nseg : 0);   // per UniV3 segment: {row, landing price}
    std::vector<int64_t> rows;
    std::vector<double> prices;
    for (int64_t w = 0; w < waves; ++w) {
        const size_t off = (size_t)plan.wave_off[(size_t)w], nw = (size_t)plan.wave_off[(size_t)w + 1] - off;
        const size_t p0 = (size_t)h_first[off], p1 = (size_t)h_first[off + nw];   // the wave's span of the paths
        SwapOrderArgs a{};
        a.p.count = n_paths;
        a.p.stride = n_paths;
        a.p.max_hops = max_hops;
        a.p.nseg = (int32_t)nrec;
        a.p.segs = sc.table.get();
        a.p.n_hops = sc.hop_i32.get();
        a.p.hop_seg = sc.hop_i32.get() + n;
        a.p.hop_coin_in = sc.hop_i32.get() + n + nh;
        a.p.hop_coin_out = sc.hop_i32.get() + n + 2 * nh;
        a.p.hop_row = sc.i64.get();
        a.p.amount_in = sc.amt.get();
        a.p.min_out = nullptr;
        a.p.amount_out = sc.out.get();
        a.p.hops = sc.hops.get();
        a.p.price = sc.price.get();
        a.p.status = sc.status.get();
        a.orders = (int64_t)nw;
        a.order_first = sc.i64.get() + nh + off;
        a.limit = limit ? sc.amt.get() + n + off : nullptr;
        a.total = sc.out.get() + n + off;
        a.status = sc.status.get() + n + off;
        const hipError_t e = launch_swap_order(dir.exact_out, a, c->opt_order_max_blocks, c->stream, sc.ev.start((size_t)w, timed), sc.ev.stop((size_t)w, timed));
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "swap order launch failed: %s (earlier waves of the call have moved their pools)", hipGetErrorString(e));
        if (!any_univ3) continue;
        // which hop levels of the wave hold a UniV3 hop
        bool level[CFMM_MAX_PATH_HOPS] = {};
        bool some = false;
        for (size_t p = p0; p < p1; ++p)
            for (size_t k = 0; k < (size_t)h_i32[p]; ++k)
                if (c->segs[(size_t)h_seg[k * n + p]].kind == CFMM_KIND_UNIV3) level[k] = some = true;
        if (!some) continue;
        // the wave's order statuses and landing prices; then the pools of its applied orders move as cfmm_pools_set_prices moves them
        HIP_TRY(c, hipMemcpyAsync(h_status + n + off, sc.status.get() + n + off, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        for (size_t k = 0; k < H; ++k)
            if (level[k]) HIP_TRY(c, hipMemcpyAsync(h_price + k * n + p0, sc.price.get() + k * n + p0, (p1 - p0) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t j = off; j < off + nw; ++j) {
            if (h_status[n + j] != CFMM_ORDER_APPLIED) continue;
            for (size_t p = (size_t)h_first[j]; p < (size_t)h_first[j + 1]; ++p)
                for (size_t k = 0; k < (size_t)h_i32[p]; ++k) {
                    const size_t seg = (size_t)h_seg[k * n + p];
                    const Segment& s = c->segs[seg];
                    if (s.kind != CFMM_KIND_UNIV3) continue;
                    const int64_t row = h_row[k * n + p];
                    double P = h_price[k * n + p];   // finite and > 0: the kernel has refused the order otherwise
                    const double top = s.lad.lower_ticks(row)[0];   // out of liquidity on that side: the first tick's upper price
                    P = P > top ? top : P;
                    if (std::memcmp(&P, &s.h_cp[(size_t)row], sizeof P) == 0) continue;   // (amount 0, no liquidity: where it was)
                    moved[seg].push_back({row, P});
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
        if (replaced && w + 1 < waves && (rc = upload_table(c, h_table)) != CFMM_OK) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), (n + G) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), (n + G) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (hop_ans) HIP_TRY(c, hipMemcpyAsync(h_hops, sc.hops.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_left, sc.left.get(), nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nseg; ++i)
        if (h_left[i]) c->segs[i].fast_ok = 0;   // (never sent back: as cfmm_update_reserves)
    if (timed && (rc = sc.ev.elapsed_ns(c, 0, (size_t)waves, c->swap.ns)) != CFMM_OK) return rc;
    int64_t refused = 0;
    for (size_t j = 0; j < G; ++j) {
        const size_t g = (size_t)plan.perm[j];
        total[g] = h_out[n + j];
        status[g] = h_status[n + j];
        refused += h_status[n + j] != CFMM_ORDER_APPLIED;
        size_t p = (size_t)h_first[j];
        for (size_t q = (size_t)order_first[g]; q < (size_t)order_first[g + 1]; ++q, ++p) {
            answer[q] = h_out[p];
            if (path_status) path_status[q] = h_status[p];
            if (hop_ans)
                for (size_t k = 0; k < H; ++k) hop_ans[k * n + q] = h_hops[k * n + p];
        }
    }
    c->swap.refused = refused;
    c->swap.launches = waves;
    return CFMM_OK;
}

} // namespace

extern "C" int cfmm_swap_order(cfmm_ctx* c, int64_t count, const int64_t* order_first, int64_t n_paths, int32_t max_hops, const int32_t* n_hops,
                               const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out,
                               const double* path_amount_in, const double* min_total_out, double* path_amount_out, double* hop_out,
                               double* total_out, int32_t* path_status, int32_t* status)
{
    return swap_order_host(c, kForward, count, order_first, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, path_amount_in,
                           min_total_out, path_amount_out, hop_out, total_out, path_status, status);
}

extern "C" int cfmm_swap_order_out(cfmm_ctx* c, int64_t count, const int64_t* order_first, int64_t n_paths, int32_t max_hops,
                                   const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, const int32_t* hop_coin_in,
                                   const int32_t* hop_coin_out, const double* path_amount_out, const double* max_total_in,
                                   double* path_amount_in, double* hop_in, double* total_in, int32_t* path_status, int32_t* status)
{
    return swap_order_host(c, kInverse, count, order_first, n_paths, max_hops, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, path_amount_out,
                           max_total_in, path_amount_in, hop_in, total_in, path_status, status);
}
