// size_checks_host.cpp -- csrc/size_checks.h and csrc/size_grid.h driven by a stand-alone host program (no device, no context),
// built with the address and undefined-behaviour sanitizers by tests/test_size_checks_cpu.py.
// First the checks, asserted here.  Then the grid arithmetic, which the test compares with the numpy statement of the contract
// (tests/size_path_ref.py): the program reads requests from standard input, one per line, every double as the 16 hex digits of
// its bits, and answers each with one line:
//   T <lo> <hi>                    ->  T <x_0> ... <x_63>                 size_trial
//   G <vi> <vo> <x> <y>            ->  G <gain>                           size_gain
//   S <g_0> ... <g_63>             ->  S <j*> <left> <right>              size_better, folded in lane order AND as the kernel's butterfly
//   A <any_nan> <max_in> <x> <y> <g>  ->  A <amount_in> <amount_out> <gain> <status>   size_answer
#include "size_checks.h"

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
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
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

static int checks()
{
    char msg[256];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto has = [&](const char* what) { return std::strstr(msg, what) != nullptr; };
    REQUIRE(check_size_scalars("cfmm_size_path", 3, 8, 1, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_size_scalars("cfmm_size_path", 0, 1, CFMM_MAX_SIZE_ROUNDS, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_size_scalars("cfmm_size_path", 3, 8, 0, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("cfmm_size_path: rounds must be 1 .. 16 (got 0)"));
    REQUIRE(check_size_scalars("cfmm_size_path", 3, 8, 17, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("(got 17)"));
    REQUIRE(check_size_scalars("cfmm_size_path_dev", -1, 8, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("cfmm_size_path_dev: count must be >= 0"));
    REQUIRE(check_size_scalars("cfmm_size_path", 3, 9, 5, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("max_hops must be 1 .. 8"));
    double a[4] = {1.0, 0.0, 5.0, 2.0};
    int32_t st[4];
    REQUIRE(check_size_arrays("cfmm_size_path", 4, a, a, a, a, st, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_size_arrays("cfmm_size_path", 0, nullptr, nullptr, nullptr, nullptr, nullptr, msg, sizeof msg) == CFMM_OK);
    REQUIRE(check_size_arrays("cfmm_size_path", 4, a, a, a, nullptr, st, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("null path array"));
    REQUIRE(check_size_arrays("cfmm_size_path", 4, nullptr, a, a, a, st, msg, sizeof msg) == CFMM_ERR_INVALID_ARG);
    REQUIRE(check_size_arrays("cfmm_size_path", 4, a, a, a, a, nullptr, msg, sizeof msg) == CFMM_ERR_INVALID_ARG);
    REQUIRE(check_size_amounts("cfmm_size_path", 4, a, nullptr, nullptr, msg, sizeof msg) == CFMM_OK);   // 0 is a limit
    double v[4] = {1.0, 2.5, 1e-300, 1e300};
    REQUIRE(check_size_amounts("cfmm_size_path", 4, a, v, v, msg, sizeof msg) == CFMM_OK);
    for (const double bad : {-1.0, nan, inf, -inf}) {
        double lim[4] = {1.0, 0.0, bad, 2.0};
        REQUIRE(check_size_amounts("cfmm_size_path", 4, lim, nullptr, nullptr, msg, sizeof msg) == CFMM_ERR_INVALID_ARG);
        REQUIRE(has("cfmm_size_path: path 2, hop 0: max_amount_in must be finite and >= 0"));
    }
    for (const double bad : {0.0, -0.0, -2.0, nan, inf}) {
        double w[4] = {1.0, bad, 1.0, 1.0};
        REQUIRE(check_size_amounts("cfmm_size_path", 4, a, w, nullptr, msg, sizeof msg) == CFMM_ERR_INVALID_ARG);
        REQUIRE(has("path 1, hop 0: value_in must be finite and > 0"));
        REQUIRE(check_size_amounts("cfmm_size_path", 4, a, nullptr, w, msg, sizeof msg) == CFMM_ERR_INVALID_ARG);
        REQUIRE(has("path 1, hop 0: value_out must be finite and > 0"));
    }
    // the limit is looked at before the values, path by path
    double lim[4] = {1.0, nan, 1.0, 1.0}, w[4] = {0.0, 1.0, 1.0, 1.0};
    REQUIRE(check_size_amounts("cfmm_size_path", 4, lim, w, nullptr, msg, sizeof msg) == CFMM_ERR_INVALID_ARG && has("path 0, hop 0: value_in"));
    std::printf("SIZE_CHECKS_OK\n");
    return 0;
}

// the arg-max as the kernel takes it: lane j starts with (g_j, j) and exchanges with lane j ^ m, m = 1, 2, .. 32
static int butterfly(const std::vector<double>& g)
{
    std::vector<double> bg(g);
    std::vector<int> bj(CFMM_SIZE_POINTS);
    for (int j = 0; j < CFMM_SIZE_POINTS; ++j) bj[j] = j;
    for (int m = 1; m < CFMM_SIZE_POINTS; m <<= 1) {
        const std::vector<double> og(bg);
        const std::vector<int> oj(bj);
        for (int j = 0; j < CFMM_SIZE_POINTS; ++j)
            if (size_better(og[j ^ m], oj[j ^ m], og[j], oj[j])) {
                bg[j] = og[j ^ m];
                bj[j] = oj[j ^ m];
            }
    }
    for (int j = 1; j < CFMM_SIZE_POINTS; ++j)
        if (bj[j] != bj[0]) return -1;   // every lane must end at the same winner
    return bj[0];
}

int main()
{
    if (checks()) return 1;
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string what, tok;
        if (!(in >> what)) continue;
        std::vector<std::string> t;
        while (in >> tok) t.push_back(tok);
        if (what == "T") {
            REQUIRE(t.size() == 2);
            std::printf("T");
            for (int j = 0; j < CFMM_SIZE_POINTS; ++j) std::printf(" %016" PRIx64, bits(size_trial(from_hex(t[0]), from_hex(t[1]), j)));
            std::printf("\n");
        } else if (what == "G") {
            REQUIRE(t.size() == 4);
            std::printf("G %016" PRIx64 "\n", bits(size_gain(from_hex(t[0]), from_hex(t[1]), from_hex(t[2]), from_hex(t[3]))));
        } else if (what == "S") {
            REQUIRE(t.size() == (size_t)CFMM_SIZE_POINTS);
            std::vector<double> g;
            for (const std::string& s : t) g.push_back(from_hex(s));
            int bj = 0;
            for (int j = 1; j < CFMM_SIZE_POINTS; ++j)
                if (size_better(g[j], j, g[bj], bj)) bj = j;
            REQUIRE(butterfly(g) == bj);
            std::printf("S %d %d %d\n", bj, size_left(bj), size_right(bj));
        } else if (what == "A") {
            REQUIRE(t.size() == 5);
            const SizeAnswer s = size_answer(t[0] != "0", from_hex(t[1]), from_hex(t[2]), from_hex(t[3]), from_hex(t[4]));
            std::printf("A %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bits(s.amount_in), bits(s.amount_out), bits(s.gain), (int)s.status);
        } else {
            REQUIRE(!"a request is T, G, S or A");
        }
    }
    std::printf("SIZE_GRID_OK\n");
    return 0;
}
