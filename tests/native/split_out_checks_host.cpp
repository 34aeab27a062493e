// split_out_checks_host.cpp -- csrc/split_out_grid.h (what cfmm_split_paths_out's search has of its own: the ONE text the
// kernel and the multi-device parent compile) and csrc/split_checks.h under the entry's name, driven by a stand-alone host
// program (no device, no context), built with the address and undefined-behaviour sanitizers by
// tests/test_split_out_checks_cpu.py.
// First the checks, asserted here.  Then the greedy and the status rule, which the test compares with the numpy statement of the
// contract (tests/split_paths_out_ref.py): the program reads requests from standard input, one per line, every double as the
// 16 hex digits of its bits, and answers each with one line:
//   G <bad> <K> <c[0][0]> ... <c[K-1][63]>   ->  G <bad> <n_0> ... <n_7>            split_out_greedy on increments c[k][n+1] - c[k][n]
//   A <bad> <amount> <total> <v>             ->  A <status> <share> <cost>          split_out_status, split_out_written_share / _cost
// (the grid points, the step back and the remainder are split_grid.h's, tied to numpy by split_checks_host.cpp)
#include "split_checks.h"
#include "split_out_grid.h"

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
    const char* who = "cfmm_split_paths_out";
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto is = [&](const char* what) { return std::strcmp(msg, what) == 0; };
    static_assert(CFMM_SPLIT_UNOBTAINABLE == 4 && CFMM_SPLIT_UNOBTAINABLE != CFMM_SPLIT_SATURATED, "a status of its own");
    REQUIRE(check_split_scalars(who, 3, 5, 8, 0, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths_out: rounds must be 1 .. 16 (got 0)"));
    const int64_t first[5] = {0, 1, 3, 6, 14};
    const double amount[4] = {1.0, 0.0, 5.0, 1e300};
    REQUIRE(check_split_orders(who, 4, first, amount, 14, msg, sizeof msg, "amount_out") == CFMM_OK);
    for (const double bad : {-1.0, nan, inf, -inf}) {
        const double a[4] = {1.0, 0.0, bad, 2.0};
        REQUIRE(check_split_orders(who, 4, first, a, 14, msg, sizeof msg, "amount_out") == CFMM_ERR_INVALID_ARG &&
                is("cfmm_split_paths_out: order 2: amount_out must be finite and >= 0"));
        REQUIRE(check_split_orders("cfmm_split_paths", 4, first, a, 14, msg, sizeof msg) == CFMM_ERR_INVALID_ARG &&
                is("cfmm_split_paths: order 2: amount_in must be finite and >= 0"));   // (the forward entry's text is as it was)
    }
    // the whole call on a market of two segments: the shared-pool refusal and a bad hop, named by order
    const PathSegInfo segs[2] = {{CFMM_KIND_PRODUCT, 300, 2}, {CFMM_KIND_WEIGHTED, 40, 3}};
    enum { G = 2, P = 4, H = 2 };
    const int64_t of[G + 1] = {0, 3, 4};
    const double am[G] = {10.0, 0.0};
    const int32_t nh[P] = {1, 2, 1, 1};
    int32_t seg[H * P] = {0, 0, 1, 0, /**/ 0, 1, 0, 0};
    int64_t row[H * P] = {17, 4, 5, 17, /**/ 0, 4, 0, 0};
    int32_t ci[H * P] = {0, 1, 2, 0, /**/ 0, 0, 0, 0};
    int32_t co[H * P] = {1, 0, 0, 1, /**/ 1, 2, 1, 1};
    double out[P];
    int32_t st[G];
    auto call = [&](const double* amounts) {
        return check_split(who, segs, 2, G, of, amounts, P, H, nh, seg, row, ci, co, 5, out, out, out, st, msg, sizeof msg, "amount_out");
    };
    REQUIRE(call(am) == CFMM_OK);
    const double neg[G] = {10.0, -0.5};
    REQUIRE(call(neg) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths_out: order 1: amount_out must be finite and >= 0"));
    row[0 * P + 0] = 4;
    REQUIRE(call(am) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths_out: order 0: paths 0 and 1 share pool (segment 0, row 4)"));
    row[0 * P + 0] = 17;
    row[1 * P + 1] = 40;
    REQUIRE(call(am) == CFMM_ERR_INVALID_ARG && is("cfmm_split_paths_out: order 0: path 1, hop 1: row 40 out of range (segment 1 has 40 pools)"));
    // the order of the greedy's arg-min
    REQUIRE(split_out_better(1.0, 3, 2.0, 0) && !split_out_better(2.0, 0, 1.0, 3));
    REQUIRE(split_out_better(1.0, 0, 1.0, 1) && !split_out_better(1.0, 1, 1.0, 0));
    REQUIRE(split_out_better(0.0, 0, -0.0, 1) && split_out_better(-0.0, 0, 0.0, 1));          // equal as numbers: the smaller path
    REQUIRE(split_out_better(inf, 5, nan, 0) && !split_out_better(nan, 0, inf, 5));            // +inf is a number
    REQUIRE(split_out_better(nan, 0, nan, 1) && !split_out_better(nan, 1, nan, 0));
    REQUIRE(split_out_better(1e300, 7, inf, 0));
    std::printf("SPLIT_OUT_CHECKS_OK\n");
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
        if (what == "G") {
            REQUIRE(t.size() >= 2);
            const int bad_in = std::atoi(t[0].c_str()), K = std::atoi(t[1].c_str());
            REQUIRE(bad_in >= kSplitOutClean && bad_in <= kSplitOutNan);
            REQUIRE(K >= 0 && K <= CFMM_MAX_SPLIT_PATHS && t.size() == 2 + (size_t)K * CFMM_SPLIT_POINTS);
            std::vector<double> c;
            for (size_t i = 2; i < t.size(); ++i) c.push_back(from_hex(t[i]));
            int n[CFMM_MAX_SPLIT_PATHS];
            int asked = 0;
            const int bad = split_out_greedy(K, [&](int k, int at) {
                ++asked;
                if (k < 0 || k >= K || at < 0 || at > CFMM_SPLIT_POINTS - 2) std::abort();   // never asked beyond the order or the grid
                return c[(size_t)k * CFMM_SPLIT_POINTS + at + 1] - c[(size_t)k * CFMM_SPLIT_POINTS + at];
            }, n, bad_in);
            REQUIRE(asked == K + CFMM_SPLIT_POINTS - 2);
            std::printf("G %d", bad);
            for (int k = 0; k < CFMM_MAX_SPLIT_PATHS; ++k) std::printf(" %d", n[k]);
            std::printf("\n");
        } else if (what == "A") {
            REQUIRE(t.size() == 4);
            const int32_t st = split_out_status(std::atoi(t[0].c_str()), from_hex(t[1]), from_hex(t[2]));
            const double v = from_hex(t[3]);
            std::printf("A %d %016" PRIx64 " %016" PRIx64 "\n", (int)st, bits(split_out_written_share(st, v)), bits(split_out_written_cost(st, v)));
        } else {
            REQUIRE(!"a request is G or A");
        }
    }
    std::printf("SPLIT_OUT_GRID_OK\n");
    return 0;
}
