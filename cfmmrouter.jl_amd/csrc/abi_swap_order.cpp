// abi_swap_order.cpp -- cfmm_swap_order and, by a direction (Dir), cfmm_swap_order_out (include/cfmm_amd_order.h): orders that
// MOVE their pools, in the caller's order, each order all or nothing ACROSS its 1 .. 8 paths with one limit on its total.
// The checks are here; the call itself is abi_swap_path.cpp's driver (swap_paths_run) with the orders as what is applied all
// or nothing: waves of pool-disjoint ORDERS (swap_order_waves.h), the orders and their paths uploaded ONCE in wave order -- an
// order's paths stay together, so a wave is one span of the orders and one span of the paths -- and one kernel per wave over
// its span of orders (swap_order_kernels.h: eight lanes per order; pass 1 walks and tests every path, the group decides, pass 2
// applies), the UniV3 pools of the APPLIED ORDERS moved between waves.
// The only memory of the feature is SwapPathScratch (ctx.h): proportional to the orders and to n_paths x max_hops, never to
// the pools.
#include "seg_view.h"
#include "../../include/cfmm_amd_order.h"
#include "order_checks.h"

using namespace cfmm;

static_assert(CFMM_ORDER_APPLIED == kOrderApplied && CFMM_ORDER_LIMIT == kOrderLimit && CFMM_ORDER_REFUSED == kOrderRefused &&
              CFMM_ORDER_UNOBTAINABLE == kOrderUnobtainable && CFMM_ORDER_PATH_HELD == kOrderPathHeld, "the kernel's codes are the header's");

namespace {

constexpr Dir kForward{false, "cfmm_swap_order", nullptr, nullptr};
constexpr Dir kInverse{true, "cfmm_swap_order_out", nullptr, nullptr};

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
    const SwapPathCall q{"swap order", count, order_first, n_paths, max_hops, {n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out}, given, limit,
                         answer, hop_ans, path_status, total, status};
    return swap_paths_run(c, dir.exact_out, q, [](const cfmm_ctx* c, bool exact_out, const SwapOrderArgs& a, hipEvent_t e0, hipEvent_t e1) {
        return launch_swap_order(exact_out, a, c->opt_order_max_blocks, c->stream, e0, e1);
    });
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
