// split_checks_host.cpp -- csrc/split_checks.h and csrc/split_grid.h driven by a stand-alone host program (no device, no context),
// built with the address and undefined-behaviour sanitizers by tests/test_split_checks_cpu.py.
// First the checks, asserted here.  Then the grid arithmetic, which the test compares with the numpy statement of the contract
// (tests/split_paths_ref.py): the program reads requests from standard input, one per line, every double as the 16 hex digits
// of its bits, and answers each with one line:
//   P <base> <rem>                       ->  P <x_0> ... <x_63>                    split_slice, split_point
//   G <K> <y[0][0]> ... <y[K-1][63]>     ->  G <flags> <n_0> ... <n_7>             split_greedy on increments y[k][n+1] - y[k][n]
//   R <amount> <K> <base_0> ...          ->  R <rem>                               split_rem of the sum in increasing k
//   A <any_nan> <last_flat> <amount> <total> <v>  ->  A <status> <written v>       split_status, split_written
#include "split_checks.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

using namespace cfmm;

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n  msg: %s\n", __FILE__, __LINE__, #cond, msg); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

static double from_hex(const std::string& s)
{
    const uint64_t u = std::strtoull(s.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}
static uint64_t bits(double d)
{
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

static char msg[256];

static int checks()
{
    const char* who = "cfmm_split_paths";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto is = [&](const char* what) { return std::strcmp(msg, what) == 0; };
    // scalars
    REQUIRE(check_split_scalars(who, 3, 5, 8, 1, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_scalars(who, 0, 0, 1, CFMM_MAX_SPLIT_ROUNDS, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_scalars(who, 3, 5, 8, 0, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: rounds must be 1 .. 16 (got 0)"));
    REQUIRE(check_split_scalars(who, 3, 5, 8, 17, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: rounds must be 1 .. 16 (got 17)"));
    REQUIRE(check_split_scalars("cfmm_split_paths_dev", -1, 5, 8, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths_dev: count must be >= 0"));
    REQUIRE(check_split_scalars(who, 3, 5, 9, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: max_hops must be 1 .. 8 (got 9)"));
    REQUIRE(check_split_scalars(who, 3, 0, 8, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: n_paths must be >= 1 (got 0)"));
    REQUIRE(check_split_scalars(who, 0, -2, 8, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: n_paths must be >= 0 (got -2)"));
    // arrays
    int dummy = 0;
    const void* p = &dummy;
    REQUIRE(check_split_arrays(who, 2, p, p, p, p, p, p, p, p, p, p, p, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_arrays(who, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_arrays(who, 2, nullptr, p, p, p, p, p, p, p, p, p, p, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: null order array"));
    REQUIRE(check_split_arrays(who, 2, p, p, p, p, p, p, p, p, p, nullptr, p, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: null order array"));
    REQUIRE(check_split_arrays(who, 2, p, p, p, p, nullptr, p, p, p, p, p, p, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: null path array"));
    // orders
    const int64_t first[5] = {0, 1, 3, 6, 14};
    const double amount[4] = {1.0, 0.0, 5.0, 1e300};
    REQUIRE(check_split_orders(who, 4, first, amount, 14, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_orders(who, 0, nullptr, nullptr, 0, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_split_orders(who, 0, nullptr, nullptr, 2, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: 2 paths belong to no order (count is 0)"));
    {
        const int64_t f[5] = {1, 1, 3, 6, 14};
        REQUIRE(check_split_orders(who, 4, f, amount, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 0: order_first[0] must be 0 (got 1)"));
    }
    {
        const int64_t f[5] = {0, 1, 3, 2, 14};
        REQUIRE(check_split_orders(who, 4, f, amount, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 2: order_first decreases (2 after 3)"));
    }
    {
        const int64_t f[5] = {0, 1, 1, 6, 14};
        REQUIRE(check_split_orders(who, 4, f, amount, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 1: 0 paths (an order has 1 .. 8)"));
    }
    {
        const int64_t f[5] = {0, 1, 3, 5, 14};
        REQUIRE(check_split_orders(who, 4, f, amount, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 3: 9 paths (an order has 1 .. 8)"));
    }
    REQUIRE(check_split_orders(who, 4, first, amount, 13, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 3: its paths end at 14, beyond n_paths 13"));
    REQUIRE(check_split_orders(who, 4, first, amount, 15, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order_first[count] must be n_paths 15 (got 14)"));
    for (const double bad : {-1.0, nan, inf, -inf}) {
        const double a[4] = {1.0, 0.0, bad, 2.0};
        REQUIRE(check_split_orders(who, 4, first, a, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 2: amount_in must be finite and >= 0"));
    }
    // the whole call on a market of two segments: 300 two-coin pools and 40 three-coin pools
    const PathSegInfo segs[2] = {{CFMM_KIND_PRODUCT, 300, 2}, {CFMM_KIND_WEIGHTED, 40, 3}};
    enum { G = 3, P = 6, H = 3 };
    const int64_t of[G + 1] = {0, 3, 4, 6};
    const double am[G] = {10.0, 0.0, 3.0};
    const int32_t nh[P] = {1, 2, 3, 1, 2, 1};
    // hop-major [H][P]
    int32_t seg[H * P] = {0, 0, 1, 0, 0, 1, /**/ 0, 1, 0, 0, 1, 0, /**/ 0, 0, 0, 0, 0, 0};
    int64_t row[H * P] = {17, 4, 5, 17, 8, 9, /**/ 0, 4, 6, 0, 10, 0, /**/ 0, 0, 7, 0, 0, 0};
    int32_t ci[H * P] = {0, 1, 2, 0, 0, 1, /**/ 0, 0, 1, 0, 2, 0, /**/ 0, 0, 0, 0, 0, 0};
    int32_t co[H * P] = {1, 0, 0, 1, 1, 0, /**/ 1, 2, 0, 1, 0, 1, /**/ 1, 1, 1, 1, 1, 1};
    double out[P];
    int32_t st[G];
    auto call = [&](int32_t rounds = 5) {
        return check_split(who, segs, 2, G, of, am, P, H, nh, seg, row, ci, co, rounds, out, out, out, st, msg, sizeof msg);
    };
    REQUIRE(call() == CFMM_OK);                                      // (segment 0 row 17 occurs in orders 0 and 1: other orders may share)
    REQUIRE(call(0) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: rounds must be 1 .. 16 (got 0)"));
    // a bad hop is named by order, path within the order, and hop
    row[1 * P + 4] = 40;
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 2: path 0, hop 1: row 40 out of range (segment 1 has 40 pools)"));
    row[1 * P + 4] = 10;
    ci[2 * P + 2] = 1;
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 0: path 2, hop 2: coin_in and coin_out are both 1"));
    ci[2 * P + 2] = 0;
    {
        int32_t bad_nh[P] = {1, 2, 3, 0, 2, 1};
        REQUIRE(check_split(who, segs, 2, G, of, am, P, H, bad_nh, seg, row, ci, co, 5, out, out, out, st, msg, sizeof msg) == CFMM_ERR_INVALID_ARG &&
                is("cfmm_split_paths: order 1: path 0: n_hops 0 out of range (1 .. 3)"));
    }
    REQUIRE(check_split(who, segs, 0, G, of, am, P, H, nh, seg, row, ci, co, 5, out, out, out, st, msg, sizeof msg) == CFMM_ERR_INVALID_ARG &&
            is("cfmm_split_paths: order 0: path 0, hop 0: segment 0 out of range (the context has 0)"));
    // shared pools: between two paths of an order, and within one path; slots beyond n_hops do not count
    row[0 * P + 0] = 4;                                              // order 0: path 0 hop 0 = (0, 4) = path 1 hop 0
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 0: paths 0 and 1 share pool (segment 0, row 4)"));
    row[0 * P + 0] = 17;
    seg[2 * P + 2] = 1, row[2 * P + 2] = 4, ci[2 * P + 2] = 0, co[2 * P + 2] = 1;   // order 0: path 2 hop 2 = (1, 4) = path 1 hop 1
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 0: paths 1 and 2 share pool (segment 1, row 4)"));
    row[2 * P + 2] = 5;                                              // ... = path 2's own hop 0
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 0: paths 2 and 2 share pool (segment 1, row 5)"));
    seg[2 * P + 2] = 0, row[2 * P + 2] = 7;
    row[1 * P + 5] = 9, seg[1 * P + 5] = 1;                          // order 2: path 1 has one hop: its slot at hop 1 is not looked at
    REQUIRE(call() == CFMM_OK);
    row[0 * P + 5] = 8, seg[0 * P + 5] = 0;                          // order 2: path 1 hop 0 = (0, 8) = path 0 hop 0
    REQUIRE(call() == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths: order 2: paths 0 and 1 share pool (segment 0, row 8)"));
    std::printf("SPLIT_CHECKS_OK\n");
    return 0;
}

int main()
{
    if (checks()) return 1;
    static char line[1 << 16];
    while (std::fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string what, tok;
        if (!(in >> what)) continue;
        std::vector<std::string> t;
        while (in >> tok) t.push_back(tok);
        if (what == "P") {
            REQUIRE(t.size() == 2);
            const double base = from_hex(t[0]), rem = from_hex(t[1]), s = split_slice(rem);
            std::printf("P");
            for (int j = 0; j < CFMM_SPLIT_POINTS; ++j) std::printf(" %016" PRIx64, bits(split_point(base, s, rem, j)));
            std::printf("\n");
        } else if (what == "G") {
            REQUIRE(!t.empty());
            const int K = std::atoi(t[0].c_str());
            REQUIRE(K >= 0 && K <= CFMM_MAX_SPLIT_PATHS && t.size() == 1 + (size_t)K * CFMM_SPLIT_POINTS);
            std::vector<double> y;
            for (size_t i = 1; i < t.size(); ++i) y.push_back(from_hex(t[i]));
            int n[CFMM_MAX_SPLIT_PATHS];
            int asked = 0;
            const int flags = split_greedy(K, [&](int k, int at) {
                ++asked;
                if (k < 0 || k >= K || at < 0 || at > CFMM_SPLIT_POINTS - 2) std::abort();   // never asked beyond the order or the grid
                return y[(size_t)k * CFMM_SPLIT_POINTS + at + 1] - y[(size_t)k * CFMM_SPLIT_POINTS + at];
            }, n);
            REQUIRE(asked == K + CFMM_SPLIT_POINTS - 2);
            std::printf("G %d", flags);
            for (int k = 0; k < CFMM_MAX_SPLIT_PATHS; ++k) std::printf(" %d", n[k]);
            std::printf("\n");
        } else if (what == "R") {
            REQUIRE(t.size() >= 3);
            const int K = std::atoi(t[1].c_str());
            REQUIRE(K >= 1 && K <= CFMM_MAX_SPLIT_PATHS && t.size() == 2 + (size_t)K);
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum = k == 0 ? from_hex(t[2]) : sum + from_hex(t[2 + k]);
            std::printf("R %016" PRIx64 "\n", bits(split_rem(from_hex(t[0]), sum)));
        } else if (what == "A") {
            REQUIRE(t.size() == 5);
            const int32_t st = split_status(t[0] != "0", t[1] != "0", from_hex(t[2]), from_hex(t[3]));
            std::printf("A %d %016" PRIx64 "\n", (int)st, bits(split_written(st, from_hex(t[4]))));
        } else {
            REQUIRE(!"a request is P, G, R or A");
        }
    }
    std::printf("SPLIT_GRID_OK\n");
    return 0;
}
