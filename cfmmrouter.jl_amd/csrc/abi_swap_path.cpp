// abi_swap_path.cpp -- cfmm_swap_path and, by a direction (Dir), cfmm_swap_path_out: swap paths that MOVE their pools, in
// query order, each path all or nothing (include/cfmm_amd.h and cfmm_amd_path_out.h have the contracts).  The exact-output
// form differs in the kernel it launches (swap_path_out_kernel: the walk from the last hop backwards), the roles of the
// amounts and the names in the messages; every line below serves both, described for the exact-input form.
// A path answers what cfmm_quote_path answers on the market as the applied paths before it left it, and each of its hops
// leaves its pool where cfmm_swap of (that hop, the amount entering it) leaves it (swap_path_kernels.h: pass 1 quotes and
// tests, pass 2 applies).  The host cuts the batch into waves of pool-disjoint paths (swap_path_waves.h), uploads the hop
// arrays ONCE in wave order and launches one kernel per wave over its span of them.  It waits between waves only behind a
// wave with a UniV3 hop -- UniV3's state is its price, with records prepared on the host: the wave's statuses and landing
// prices are read back and the pools of the applied paths move through cfmm_pools_set_prices' own apply path (abi_update.cpp
// univ3_move_prices), after which the segment table is rebuilt (a moved pool may have regrown the record arrays).  Otherwise
// it synchronises once, at the end.
// The only memory of the feature is SwapPathScratch (ctx.h): proportional to count x max_hops, never to the pools.
#include "seg_view.h"
#include "stage_layout.h"
#include "../../include/cfmm_amd_path_out.h"
#include "swap_path_checks.h"
#include "swap_path_waves.h"
#include "univ3_pool.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

using namespace cfmm;

namespace {

constexpr Dir kForward{false, "cfmm_swap_path", nullptr, nullptr};
constexpr Dir kInverse{true, "cfmm_swap_path_out", nullptr, nullptr};

// table (seg_view.h: rebuilt from the segments' current addresses, one window flag per segment) -> staging -> device
int upload_table(cfmm_ctx* c, SwapPathSeg* t)
{
    SwapPathScratch& sc = c->swap_path;
    build_table(c, t, [&](const Segment& s, size_t i) { return swap_path_seg(s, sc.left.get() + i); });
    HIP_TRY(c, hipMemcpyAsync(sc.table.get(), t, table_records(c) * sizeof(SwapPathSeg), hipMemcpyHostToDevice, c->stream));
    return CFMM_OK;
}

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

    HIP_TRY(c, hipSetDevice(c->device));
    const SwapPathPlan plan = swap_path_plan(count, n_hops, hop_seg, hop_row, &c->swap_path.pools);
    const int64_t waves = (int64_t)plan.wave_off.size() - 1;
    const bool timed = c->opt_time_kernels != 0;
    SwapPathScratch& sc = c->swap_path;
    const size_t n = (size_t)count, H = (size_t)max_hops, nh = n * H, nseg = c->segs.size(), nrec = table_records(c);
    const SwapPathStage lay(nrec * sizeof(SwapPathSeg), nrec, n, nh);   // the pinned staging (stage_layout.h)
    if ((rc = sc.stage.grow(c, lay.l.words(), false)) || (rc = sc.table.grow(c, nrec)) ||
        (rc = sc.hop_i32.grow(c, n + 3 * nh)) || (rc = sc.hop_row.grow(c, nh)) || (rc = sc.amt.grow(c, 2 * n)) || (rc = sc.out.grow(c, n)) ||
        (rc = sc.hops.grow(c, nh)) || (rc = sc.price.grow(c, nh)) || (rc = sc.status.grow(c, n)) || (rc = sc.left.grow(c, nrec)) ||
        (timed && (rc = sc.ev.ensure(c, (size_t)waves))))
        return rc;
    unsigned long long* st = sc.stage.host();
    SwapPathSeg* h_table = reinterpret_cast<SwapPathSeg*>(lay.table.in(st));
    int32_t *h_i32 = lay.i32.in(st), *h_seg = h_i32 + n, *h_ci = h_i32 + n + nh, *h_co = h_i32 + n + 2 * nh, *h_status = lay.status.in(st);
    long long* h_row = lay.row.in(st);
    double* h_amt = lay.amt.in(st);   // [count] the given amounts, then [count] the limits
    double *h_out = lay.out.in(st), *h_hops = lay.hops.in(st), *h_price = lay.price.in(st);
    int* h_left = lay.left.in(st);
    // the paths in launch order; the slots a path does not use are zeroed (never read by the kernel)
    std::memset(h_seg, 0, 3 * nh * sizeof(int32_t));
    std::memset(h_row, 0, nh * sizeof(long long));
    for (size_t j = 0; j < n; ++j) {
        const size_t q = (size_t)plan.perm[j];
        h_i32[j] = n_hops[q];
        h_amt[j] = given[q];
        if (limit) h_amt[n + j] = limit[q];
        for (size_t k = 0; k < (size_t)n_hops[q]; ++k) {
            h_seg[k * n + j] = hop_seg[k * n + q];
            h_row[k * n + j] = hop_row[k * n + q];
            h_ci[k * n + j] = hop_coin_in[k * n + q];
            h_co[k * n + j] = hop_coin_out[k * n + q];
        }
    }
    armed_cancel(c);
    if ((rc = upload_table(c, h_table)) != CFMM_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(sc.hop_i32.get(), h_i32, (n + 3 * nh) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.hop_row.get(), h_row, nh * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sc.amt.get(), h_amt, (limit ? 2 : 1) * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(sc.left.get(), 0, nrec * sizeof(int), c->stream));
    swap_invalidate(c);   // from the first launch on the pools count as moved
    bool any_univ3 = false;
    for (const Segment& s : c->segs) any_univ3 = any_univ3 || (s.kind == CFMM_KIND_UNIV3 && s.m > 0);
    std::vector<std::vector<std::pair<int64_t, double>>> moved(any_univ3 ? nseg : 0);   // per UniV3 segment: {row, landing price}
    std::vector<int64_t> rows;
    std::vector<double> prices;
    for (int64_t w = 0; w < waves; ++w) {
        const size_t off = (size_t)plan.wave_off[(size_t)w], nw = (size_t)plan.wave_off[(size_t)w + 1] - off;
        SwapPathArgs a{};
        a.count = (int64_t)nw;
        a.stride = count;
        a.max_hops = max_hops;
        a.nseg = (int32_t)nrec;
        a.segs = sc.table.get();
        a.n_hops = sc.hop_i32.get() + off;
        a.hop_seg = sc.hop_i32.get() + n + off;
        a.hop_coin_in = sc.hop_i32.get() + n + nh + off;
        a.hop_coin_out = sc.hop_i32.get() + n + 2 * nh + off;
        a.hop_row = sc.hop_row.get() + off;
        a.amount_in = sc.amt.get() + off;
        a.min_out = limit ? sc.amt.get() + n + off : nullptr;
        a.amount_out = sc.out.get() + off;
        a.hops = sc.hops.get() + off;
        a.price = sc.price.get() + off;
        a.status = sc.status.get() + off;
        const hipError_t e = (dir.exact_out ? launch_swap_path_out : launch_swap_path)(a, c->stream, sc.ev.start((size_t)w, timed), sc.ev.stop((size_t)w, timed));
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "swap path launch failed: %s (earlier waves of the call have moved their pools)", hipGetErrorString(e));
        if (!any_univ3) continue;
        // which hop levels of the wave hold a UniV3 hop
        bool level[CFMM_MAX_PATH_HOPS] = {};
        bool some = false;
        for (size_t j = off; j < off + nw; ++j)
            for (size_t k = 0; k < (size_t)h_i32[j]; ++k)
                if (c->segs[(size_t)h_seg[k * n + j]].kind == CFMM_KIND_UNIV3) level[k] = some = true;
        if (!some) continue;
        // the wave's statuses and landing prices; then the pools of its applied paths move as cfmm_pools_set_prices moves them
        HIP_TRY(c, hipMemcpyAsync(h_status + off, sc.status.get() + off, nw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        for (size_t k = 0; k < H; ++k)
            if (level[k]) HIP_TRY(c, hipMemcpyAsync(h_price + k * n + off, sc.price.get() + k * n + off, nw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t j = off; j < off + nw; ++j) {
            if (h_status[j] != CFMM_PATH_APPLIED) continue;
            for (size_t k = 0; k < (size_t)h_i32[j]; ++k) {
                const size_t seg = (size_t)h_seg[k * n + j];
                const Segment& s = c->segs[seg];
                if (s.kind != CFMM_KIND_UNIV3) continue;
                const int64_t row = h_row[k * n + j];
                double P = h_price[k * n + j];   // finite and > 0: the kernel has refused the path otherwise
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
    HIP_TRY(c, hipMemcpyAsync(h_out, sc.out.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_status, sc.status.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (hop_ans) HIP_TRY(c, hipMemcpyAsync(h_hops, sc.hops.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_left, sc.left.get(), nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < nseg; ++i)
        if (h_left[i]) c->segs[i].fast_ok = 0;   // (never sent back: as cfmm_update_reserves)
    if (timed && (rc = sc.ev.elapsed_ns(c, 0, (size_t)waves, c->swap.ns)) != CFMM_OK) return rc;
    int64_t refused = 0;
    for (size_t j = 0; j < n; ++j) {
        const size_t q = (size_t)plan.perm[j];
        answer[q] = h_out[j];
        if (status) status[q] = h_status[j];
        refused += h_status[j] != CFMM_PATH_APPLIED;
        if (hop_ans)
            for (size_t k = 0; k < H; ++k) hop_ans[k * n + q] = h_hops[k * n + j];
    }
    c->swap.refused = refused;
    c->swap.launches = waves;
    return CFMM_OK;
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
