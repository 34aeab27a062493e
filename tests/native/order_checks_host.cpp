// order_checks_host.cpp -- csrc/order_checks.h (the checks of cfmm_swap_order / cfmm_swap_order_out) driven by a stand-alone
// host program: no device, no context, no HIP header.  Every refusal of the header is provoked once and its text compared
// word for word.  Built with the address and undefined-behaviour sanitizers and run by tests/test_swap_order_cpu.py.
#include "order_checks.h"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace cfmm;

static char msg[256];

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n  msg: %s\n", __FILE__, __LINE__, #cond, msg); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int E = CFMM_ERR_INVALID_ARG;
    auto is = [&](const char* what) { return std::strcmp(msg, what) == 0; };
    // a market of two segments; three orders of 2, 1 and 3 paths over six paths of at most two hops
    const PathSegInfo segs[2] = {{CFMM_KIND_PRODUCT, 300, 2}, {CFMM_KIND_WEIGHTED, 40, 3}};
    enum { G = 3, P = 6, H = 2 };
    int64_t of[G + 1] = {0, 2, 3, 6};
    int32_t nh[P] = {1, 2, 1, 1, 2, 1};
    int32_t seg[H * P] = {0, 0, 1, 0, 1, 0, /**/ 0, 1, 0, 0, 0, 0};
    int64_t row[H * P] = {17, 4, 5, 17, 6, 8, /**/ 0, 4, 0, 0, 9, 0};
    int32_t ci[H * P] = {0, 1, 2, 0, 1, 0, /**/ 0, 0, 0, 0, 0, 0};
    int32_t co[H * P] = {1, 0, 0, 1, 2, 1, /**/ 0, 2, 0, 0, 1, 0};
    double given[P] = {1.0, 2.0, 0.0, 4.0, 5.0, 6.0}, limit[G] = {0.0, 1.5, 1e300};
    double out[P], total[G];
    int32_t st[G];
    auto call = [&](const char* who, bool exact_out, int64_t count, int64_t n_paths, int32_t max_hops, const double* lim) {
        msg[0] = 0;
        return check_orders(who, exact_out, segs, 2, count, of, n_paths, max_hops, nh, seg, row, ci, co, given, lim, out, total, st, msg, sizeof msg);
    };
    const char *in = "cfmm_swap_order", *ot = "cfmm_swap_order_out";
    REQUIRE(call(in, false, G, P, H, nullptr) == CFMM_OK && msg[0] == 0);
    REQUIRE(call(in, false, G, P, H, limit) == CFMM_OK && msg[0] == 0);
    REQUIRE(call(ot, true, G, P, H, limit) == CFMM_OK && msg[0] == 0);
    REQUIRE(call(in, false, 0, 0, H, nullptr) == CFMM_OK);                                             // an empty call
    // the scalars
    REQUIRE(call(in, false, -1, P, H, nullptr) == E && is("cfmm_swap_order: count must be >= 0"));
    REQUIRE(call(in, false, G, P, 9, nullptr) == E && is("cfmm_swap_order: max_hops must be 1 .. 8 (got 9)"));
    REQUIRE(call(in, false, G, 0, H, nullptr) == E && is("cfmm_swap_order: n_paths must be >= 1 (got 0)"));
    REQUIRE(call(in, false, 0, 4, H, nullptr) == E && is("cfmm_swap_order: 4 paths belong to no order (count is 0)"));
    // null arrays
    msg[0] = 0;
    REQUIRE(check_orders(in, false, segs, 2, G, nullptr, P, H, nh, seg, row, ci, co, given, nullptr, out, total, st, msg, sizeof msg) == E &&
            is("cfmm_swap_order: null order array"));
    REQUIRE(check_orders(in, false, segs, 2, G, of, P, H, nh, seg, row, ci, co, given, nullptr, out, nullptr, st, msg, sizeof msg) == E &&
            is("cfmm_swap_order: null order array"));
    REQUIRE(check_orders(in, false, segs, 2, G, of, P, H, nh, seg, row, ci, co, nullptr, nullptr, out, total, st, msg, sizeof msg) == E &&
            is("cfmm_swap_order: null path array"));
    REQUIRE(check_orders(ot, true, segs, 2, G, of, P, H, nh, seg, row, ci, co, given, nullptr, nullptr, total, st, msg, sizeof msg) == E &&
            is("cfmm_swap_order_out: null path array"));
    // order_first: cfmm_split_paths' checks and texts
    of[0] = 1;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 0: order_first[0] must be 0 (got 1)"));
    of[0] = 0;
    of[2] = 1;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 1: order_first decreases (1 after 2)"));
    of[2] = 2;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 1: 0 paths (an order has 1 .. 8)"));
    of[2] = 7;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 1: its paths end at 7, beyond n_paths 6"));
    of[2] = 3;
    of[3] = 5;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order_first[count] must be n_paths 6 (got 5)"));
    of[3] = 6;
    {
        const int64_t nine[2] = {0, 9};
        const int32_t one[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, z32[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, c1[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
        const int64_t r9[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
        const double a9[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
        double o9[9];
        REQUIRE(check_orders(in, false, segs, 2, 1, nine, 9, 1, one, z32, r9, z32, c1, a9, nullptr, o9, total, st, msg, sizeof msg) == E &&
                is("cfmm_swap_order: order 0: 9 paths (an order has 1 .. 8)"));
    }
    // the paths: cfmm_swap_path's checks, named by order and by the path's number within it
    nh[4] = 3;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: path 1: n_hops 3 out of range (1 .. 2)"));
    nh[4] = 2;
    seg[1 * P + 1] = 2;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 0: path 1, hop 1: segment 2 out of range (the context has 2)"));
    seg[1 * P + 1] = 1;
    row[1 * P + 1] = 40;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 0: path 1, hop 1: row 40 out of range (segment 1 has 40 pools)"));
    row[1 * P + 1] = 4;
    ci[0 * P + 2] = 3;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 1: path 0, hop 0: coin_in 3 out of range (pool has 3 coins)"));
    ci[0 * P + 2] = 2;
    co[0 * P + 5] = 2;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: path 2, hop 0: coin_out 2 out of range (pool has 2 coins)"));
    co[0 * P + 5] = 0;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: path 2, hop 0: coin_in and coin_out are both 0"));
    co[0 * P + 5] = 1;
    for (const double bad : {-1.0, nan, inf, -inf}) {
        given[4] = bad;
        REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: path 1, hop 0: amount_in must be finite and >= 0"));
        REQUIRE(call(ot, true, G, P, H, nullptr) == E && is("cfmm_swap_order_out: order 2: path 1, hop 1: amount_out must be finite and >= 0"));
    }
    given[4] = 5.0;
    // a pool twice in one path (cfmm_swap_path's text), and twice among an order's paths (cfmm_split_paths' text)
    seg[1 * P + 4] = 1;
    row[1 * P + 4] = 6;
    REQUIRE(call(in, false, G, P, H, nullptr) == E &&
            is("cfmm_swap_order: order 2: path 1, hops 0 and 1: row 6 of segment 1 appears twice (a pool may appear only once in a path)"));
    seg[1 * P + 4] = 0;
    row[1 * P + 4] = 8;
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: paths 1 and 2 share pool (segment 0, row 8)"));
    REQUIRE(call(ot, true, G, P, H, nullptr) == E && is("cfmm_swap_order_out: order 2: paths 1 and 2 share pool (segment 0, row 8)"));
    row[1 * P + 4] = 17;   // (order 0's pool: different orders may share pools -- the planner puts them into different waves)
    REQUIRE(call(in, false, G, P, H, nullptr) == E && is("cfmm_swap_order: order 2: paths 0 and 1 share pool (segment 0, row 17)"));
    row[1 * P + 4] = 9;
    row[0 * P + 3] = 4;
    seg[0 * P + 3] = 1;
    ci[0 * P + 3] = 0;
    REQUIRE(call(in, false, G, P, H, nullptr) == CFMM_OK);   // order 2's first path on (1, 4), which order 0 visits too
    // the limits
    for (const double bad : {-1.0, nan, inf, -inf}) {
        double l[G] = {0.0, bad, 2.0};
        REQUIRE(call(in, false, G, P, H, l) == E && is("cfmm_swap_order: order 1: min_total_out must be finite and >= 0"));
        REQUIRE(call(ot, true, G, P, H, l) == E && is("cfmm_swap_order_out: order 1: max_total_in must be finite and >= 0"));
    }
    const double l0[G] = {-0.0, 0.0, 0.0};
    REQUIRE(call(in, false, G, P, H, l0) == CFMM_OK);
    std::printf("ORDER_CHECKS_OK\n");
    return 0;
}
