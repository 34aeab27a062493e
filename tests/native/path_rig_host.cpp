// path_rig_host.cpp -- TEST-ONLY stand-alone host program (tests/test_path_rig_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it; nothing is loaded into Python) over the HIP-free parts of the path entries'
// host side: csrc/stage_layout.h (the one staging layout of the executing path entries), csrc/swap_fill.h (the UniV3 landing
// rule, the columns into launch order and back), csrc/swap_path_waves.h and swap_order_waves.h (the planner and its two namings) and csrc/split_search.h (the parent's
// split search, here over a closed-form quote).  No HIP header, no context, no GPU.
// Output: PATH_RIG_HOST_OK behind the self-checked parts, and for the search one line per direction, rounds and array --
//   SEARCH <in|out> <rounds> <x|y|total|status> <64-bit words in hex>
// -- which the test compares word for word with tests/split_paths_ref.py / split_paths_out_ref.py over the same closed form.
#include "../../cfmmrouter.jl_amd/csrc/split_search.h"
#include "../../cfmmrouter.jl_amd/csrc/stage_layout.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_fill.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_order_waves.h"

#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace cfmm;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);           \
            return 1;                                                    \
        }                                                                \
    } while (0)

// ---- the layout -------------------------------------------------------------------------------------------------------------
// SwapPathStage(table_bytes, nrec, n, nh, g) against what the two layouts it replaces gave (computed once from them, 192 bytes
// per table record): g == 0 is the former SwapPathStage(table_bytes, nrec, n, nh), g > 0 the former
// SwapOrderStage(table_bytes, nrec, g, n, nh).  Nothing moved: old and new words are equal in all four cases.  (The former
// order layout at g == 0 -- never used, count == 0 returns early -- was 34 / 256 words; the path form it now is has 34 / 260.)
int test_layout()
{
    struct Case { size_t nrec, g, n, H, words, off[9]; };   // off: table i32 row amt out hops price status left
    const Case cases[] = {
        {1, 0, 1, 1, 34, {0, 24, 26, 27, 29, 30, 31, 32, 33}},
        {7, 0, 5, 3, 260, {0, 168, 193, 208, 218, 223, 238, 253, 256}},
        {7, 3, 5, 3, 266, {0, 168, 193, 212, 220, 228, 243, 258, 262}},
        {64, 8, 64, 4, 2941, {0, 1536, 1952, 2217, 2289, 2361, 2617, 2873, 2909}},
    };
    for (const Case& k : cases) {
        const size_t nh = k.n * k.H;
        const SwapPathStage s(k.nrec * 192, k.nrec, k.n, nh, k.g);
        const size_t got[9] = {s.table.off, s.i32.off, s.row.off, s.amt.off, s.out.off, s.hops.off, s.price.off, s.status.off, s.left.off};
        CHECK(s.l.words() == k.words);
        for (int i = 0; i < 9; ++i) CHECK(got[i] == k.off[i]);
        CHECK(s.i32.n == k.n + 3 * nh && s.row.n == nh + (k.g ? k.g + 1 : 0) && s.amt.n == k.n + (k.g ? k.g : k.n));
        CHECK(s.out.n == k.n + k.g && s.status.n == k.n + k.g && s.hops.n == nh && s.price.n == nh && s.left.n == k.nrec);
        std::vector<unsigned long long> heap(s.l.words());   // every column written to its end: ASan judges the heap buffer
        std::memset(s.left.in(heap.data()), 0x5a, s.left.n * sizeof(int));
        std::memset(s.status.in(heap.data()), 0x5a, s.status.n * sizeof(int32_t));
        std::memset(s.amt.in(heap.data()), 0x5a, s.amt.n * sizeof(double));
        std::memset(s.row.in(heap.data()), 0x5a, s.row.n * sizeof(long long));
    }
    return 0;
}

// ---- the landing rule -------------------------------------------------------------------------------------------------------
int test_landing()
{
    double to = -1.0;
    CHECK(univ3_landing(1.25, 2.0, 1.0, to) && to == 1.25);                  // below the top tick: moves there
    CHECK(univ3_landing(3.0, 2.0, 1.0, to) && to == 2.0);                    // above it: clamps to the first tick's upper price
    CHECK(!univ3_landing(1.0, 2.0, 1.0, to));                                // the current price bit for bit: stays
    CHECK(!univ3_landing(5.0, 2.0, 2.0, to));                                //   ... also when the clamp lands on it
    CHECK(univ3_landing(-0.0, 2.0, 0.0, to) && std::signbit(to));            // -0.0 against +0.0: different bits, it moves
    CHECK(univ3_landing(0.0, 2.0, -0.0, to) && !std::signbit(to));
    // a pool without liquidity: the kernel's landing price is the price it stands at, whatever the tick above
    const double cp = 0x1.23456789abcdep+3;
    CHECK(!univ3_landing(cp, std::numeric_limits<double>::infinity(), cp, to) && !univ3_landing(cp, cp, cp, to));
    return 0;
}

// ---- the columns into launch order, and back -----------------------------------------------------------------------------------
int test_fill()
{
    // 5 orders over 9 paths of 1 .. 3 hops; order 2 shares a pool with order 0 and order 4 with order 1: two waves
    const size_t G = 5, n = 9, H = 3, nh = n * H;
    const int64_t first[G + 1] = {0, 2, 3, 6, 7, 9};
    const int32_t n_hops[n] = {1, 3, 2, 1, 2, 3, 1, 2, 1};
    std::vector<int32_t> seg(nh, -77), ci(nh, -78), co(nh, -79);   // garbage in the slots a path does not use
    std::vector<int64_t> row(nh, (int64_t)1 << 40);
    for (size_t p = 0; p < n; ++p)
        for (size_t k = 0; k < (size_t)n_hops[p]; ++k) {
            seg[k * n + p] = (int32_t)(k % 2);
            row[k * n + p] = (int64_t)(100 * p + k);   // every hop a pool of its own ...
            ci[k * n + p] = (int32_t)(p + k) % 3;
            co[k * n + p] = (int32_t)(p + k + 1) % 3;
        }
    row[1 * n + 4] = row[0 * n + 0], seg[1 * n + 4] = seg[0 * n + 0];   // ... but path 4 (order 2) meets path 0 (order 0)
    row[0 * n + 8] = row[1 * n + 2], seg[0 * n + 8] = seg[1 * n + 2];   //     and path 8 (order 4) meets path 2 (order 1)
    double given[n], limit[G], plimit[n];
    for (size_t p = 0; p < n; ++p) given[p] = 1.5 + (double)p, plimit[p] = 0.25 * (double)p;
    for (size_t g = 0; g < G; ++g) limit[g] = 10.0 + (double)g;
    const HopCols in{n_hops, seg.data(), row.data(), ci.data(), co.data()};

    const SwapPathPlan plan = swap_order_plan((int64_t)G, first, (int64_t)n, n_hops, seg.data(), row.data());
    CHECK((plan.perm == std::vector<int64_t>{0, 1, 3, 2, 4}) && (plan.wave_off == std::vector<int64_t>{0, 3, 5}));
    const size_t L[n] = {0, 1, 2, 6, 3, 4, 5, 7, 8};        // the paths in launch order
    const long long want_first[G + 1] = {0, 2, 3, 4, 7, 9};
    const SwapPathStage lay(192, 1, n, nh, G);
    std::vector<unsigned long long> st(lay.l.words(), 0x5a5a5a5a5a5a5a5aull);
    int32_t* h_i32 = lay.i32.in(st.data());
    long long* h_i64 = lay.row.in(st.data());
    double* h_amt = lay.amt.in(st.data());
    fill_launch_order(plan, first, n, H, in, given, limit, h_i32, h_i64, h_amt);
    for (size_t at = 0; at < n; ++at) {
        const size_t q = L[at];
        CHECK(h_i32[at] == n_hops[q] && h_amt[at] == given[q]);
        for (size_t k = 0; k < H; ++k) {
            const bool used = k < (size_t)n_hops[q];
            CHECK(h_i32[n + k * n + at] == (used ? seg[k * n + q] : 0) && h_i64[k * n + at] == (used ? row[k * n + q] : 0));
            CHECK(h_i32[n + nh + k * n + at] == (used ? ci[k * n + q] : 0) && h_i32[n + 2 * nh + k * n + at] == (used ? co[k * n + q] : 0));
        }
    }
    for (size_t j = 0; j <= G; ++j) CHECK(h_i64[nh + j] == want_first[j]);
    for (size_t j = 0; j < G; ++j) CHECK(h_amt[n + j] == limit[(size_t)plan.perm[j]]);

    // back: what position p / j of the launch order holds returns to the path / order it came from
    std::vector<double> h_out(n + G), h_hops(nh), answer(n, -1.0), hop_ans(nh, -1.0), total(G, -1.0);
    std::vector<int32_t> h_status(n + G), path_status(n, -1), status(G, -1);
    for (size_t at = 0; at < n; ++at) {
        h_out[at] = 100.0 + (double)L[at];
        h_status[at] = (int32_t)(L[at] % 3);
        for (size_t k = 0; k < H; ++k) h_hops[k * n + at] = 1000.0 * (double)k + (double)L[at];
    }
    for (size_t j = 0; j < G; ++j) {
        h_out[n + j] = 500.0 + (double)plan.perm[j];
        h_status[n + j] = plan.perm[j] == 3 ? 0 : 1 + (int32_t)plan.perm[j];   // only order 3 APPLIED
    }
    const int64_t refused = scatter_to_caller(plan, first, n, H, h_out.data(), h_status.data(), h_hops.data(), answer.data(), path_status.data(),
                                              hop_ans.data(), total.data(), status.data());
    CHECK(refused == 4);
    for (size_t q = 0; q < n; ++q) {
        CHECK(answer[q] == 100.0 + (double)q && path_status[q] == (int32_t)(q % 3));
        for (size_t k = 0; k < H; ++k) CHECK(hop_ans[k * n + q] == 1000.0 * (double)k + (double)q);
    }
    for (size_t g = 0; g < G; ++g) CHECK(total[g] == 500.0 + (double)g && status[g] == (g == 3 ? 0 : 1 + (int32_t)g));

    // the same nine paths, one per order: the path form (no order_first) fills what the order form with an identity
    // order_first fills, and its plan is the order planner's
    int64_t ident[n + 1];
    for (size_t p = 0; p <= n; ++p) ident[p] = (int64_t)p;
    const SwapPathPlan pp = swap_path_plan((int64_t)n, n_hops, seg.data(), row.data());
    const SwapPathPlan po = swap_order_plan((int64_t)n, ident, (int64_t)n, n_hops, seg.data(), row.data());
    CHECK(pp.perm == po.perm && pp.wave_off == po.wave_off && (pp.perm == std::vector<int64_t>{0, 1, 2, 3, 5, 6, 7, 4, 8}));
    const SwapPathStage lp(192, 1, n, nh), lo(192, 1, n, nh, n);
    std::vector<unsigned long long> sp(lp.l.words(), 0x5a5a5a5a5a5a5a5aull), sn(lo.l.words(), 0xa5a5a5a5a5a5a5a5ull);
    fill_launch_order(pp, nullptr, n, H, in, given, plimit, lp.i32.in(sp.data()), lp.row.in(sp.data()), lp.amt.in(sp.data()));
    fill_launch_order(po, ident, n, H, in, given, plimit, lo.i32.in(sn.data()), lo.row.in(sn.data()), lo.amt.in(sn.data()));
    CHECK(std::memcmp(lp.i32.in(sp.data()), lo.i32.in(sn.data()), (n + 3 * nh) * sizeof(int32_t)) == 0);
    CHECK(std::memcmp(lp.row.in(sp.data()), lo.row.in(sn.data()), nh * sizeof(long long)) == 0);
    CHECK(std::memcmp(lp.amt.in(sp.data()), lo.amt.in(sn.data()), 2 * n * sizeof(double)) == 0);
    for (size_t j = 0; j < n; ++j) {
        const size_t q = (size_t)pp.perm[j];
        CHECK(lp.i32.in(sp.data())[j] == n_hops[q] && lp.amt.in(sp.data())[j] == given[q] && lp.amt.in(sp.data())[n + j] == plimit[q]);
        CHECK(lo.row.in(sn.data())[nh + j] == (long long)j);
    }
    // ... and back: the paths' statuses are the owners'
    std::vector<double> o2(n), a2(n, -1.0);
    std::vector<int32_t> s2(n), ps2(n, -1);
    for (size_t j = 0; j < n; ++j) o2[j] = 7.0 + (double)pp.perm[j], s2[j] = pp.perm[j] % 2 ? 2 : 0;
    CHECK(scatter_to_caller(pp, nullptr, n, H, o2.data(), s2.data(), nullptr, a2.data(), ps2.data(), nullptr, nullptr, nullptr) == 4);
    for (size_t q = 0; q < n; ++q) CHECK(a2[q] == 7.0 + (double)q && ps2[q] == (q % 2 ? 2 : 0));
    CHECK(scatter_to_caller(pp, nullptr, n, H, o2.data(), s2.data(), nullptr, a2.data(), nullptr, nullptr, nullptr, nullptr) == 4);
    return 0;
}

// ---- the search over a closed-form quote ---------------------------------------------------------------------------------------
// 6 orders of K = 1, 2, 3, 8, 8, 1 paths (23 paths) of 1 .. 3 constant-product hops with a fee, every operation rounded on
// its own (this file is compiled with -ffp-contract=off); tests/test_path_rig_cpu.py states the same market in numpy.
// Path 4 (of order 2) quotes NaN whatever it is asked.
constexpr int kOrders = 6, kPaths = 23, kNanPath = 4;
constexpr double kGamma = 0.997;
inline int hops_of(int p) { return 1 + p % 3; }
inline double r_in(int p, int k) { return 1000.0 + 37.0 * p + 11.0 * k; }
inline double r_out(int p, int k) { return 900.0 + 29.0 * p + 7.0 * k; }

double quote_forward(int p, double x)
{
    if (p == kNanPath) return std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < hops_of(p); ++k) {
        const double g = kGamma * x, num = r_out(p, k) * g, den = r_in(p, k) + g;
        x = num / den;
    }
    return x;
}
double quote_inverse(int p, double y)   // what to tender for y; +inf where a hop cannot give it
{
    if (p == kNanPath) return std::numeric_limits<double>::quiet_NaN();
    for (int k = hops_of(p) - 1; k >= 0; --k) {
        if (!(y < r_out(p, k))) return std::numeric_limits<double>::infinity();
        const double num = r_in(p, k) * y, den = r_out(p, k) - y, t = num / den;
        y = t / kGamma;
    }
    return y;
}

void print_words(const char* dir, int rounds, const char* what, const std::vector<double>& v)
{
    std::printf("SEARCH %s %d %s", dir, rounds, what);
    for (double d : v) {
        uint64_t w;
        std::memcpy(&w, &d, sizeof w);
        std::printf(" %016" PRIx64, w);
    }
    std::printf("\n");
}
void print_words(const char* dir, int rounds, const char* what, const std::vector<int32_t>& v)   // (as int64 words)
{
    std::printf("SEARCH %s %d %s", dir, rounds, what);
    for (int32_t s : v) std::printf(" %016" PRIx64, (uint64_t)(int64_t)s);
    std::printf("\n");
}

template <class Way>
int run_search(const char* dir, double (*quote_one)(int, double), const double* amount)
{
    const int64_t first[kOrders + 1] = {0, 1, 3, 6, 14, 22, 23};
    for (int rounds : {1, 3, 5}) {
        std::vector<double> x(kPaths, -7.0), y(kPaths, -7.0), total(kOrders, -7.0);
        std::vector<int32_t> status(kOrders, -1);
        int calls = 0;
        const int rc = split_search<Way>(
            [&](int64_t N, const double* in, double* out) {
                ++calls;
                if (N != (int64_t)CFMM_SPLIT_POINTS * kPaths) return (int)CFMM_ERR_INVALID_ARG;
                for (int64_t i = 0; i < N; ++i) out[i] = quote_one((int)(i % kPaths), in[i]);   // point j of path p at j*n_paths + p
                return (int)CFMM_OK;
            },
            kOrders, first, amount, kPaths, rounds, x.data(), y.data(), total.data(), status.data());
        CHECK(rc == CFMM_OK && calls == rounds);
        // every order is decided, none skipped: each status and total, and every path's pair, has been written
        for (int g = 0; g < kOrders; ++g) CHECK(status[g] >= 0 && !(total[g] == -7.0));
        for (int p = 0; p < kPaths; ++p) CHECK(!(x[p] == -7.0) && !(y[p] == -7.0));
        print_words(dir, rounds, "x", x);
        print_words(dir, rounds, "y", y);
        print_words(dir, rounds, "total", total);
        print_words(dir, rounds, "status", status);
    }
    // a failing quote ends the search with its code and writes nothing
    std::vector<double> x(kPaths, -7.0), y(kPaths, -7.0), total(kOrders, -7.0);
    std::vector<int32_t> status(kOrders, -1);
    CHECK(split_search<Way>([](int64_t, const double*, double*) { return (int)CFMM_ERR_HIP; }, kOrders, first, amount, kPaths, 3, x.data(), y.data(),
                            total.data(), status.data()) == CFMM_ERR_HIP);
    CHECK(x[0] == -7.0 && y[kPaths - 1] == -7.0 && total[0] == -7.0 && status[kOrders - 1] == -1);
    return 0;
}

int main()
{
    if (test_layout() || test_landing() || test_fill()) return 1;
    // order 1: amount 0 (CFMM_SPLIT_NONE); order 2 holds the NaN path; exact output: order 4 asks for more than its paths can give
    const double amount_in[kOrders] = {50.0, 0.0, 120.0, 400.0, 1.0e6, 10.0};
    const double amount_out[kOrders] = {50.0, 0.0, 120.0, 400.0, 1.0e6, 10.0};
    if (run_search<SplitIn>("in", quote_forward, amount_in) || run_search<SplitOut>("out", quote_inverse, amount_out)) return 1;
    std::printf("PATH_RIG_HOST_OK\n");
    return 0;
}
