// swap_out_host.cpp -- TEST-ONLY host build of csrc/swap_pool.h + quote_pool.h + univ3_pool.h for cfmm_swap_out: the very
// functions swap_out_kernel runs on the device, applied as the kernel and abi_swap.cpp apply them -- quote_out, the status
// (unobtainable, refused, over the limit, applied: in that order), the move to R_in + γ·in, R_out − want, in query order.
// Only the library functions (log, exp, expm1, ...) differ from the device: the host's libm here.  Also the HIP-free check of
// cfmm_swap_path_out's limits (swap_path_checks.h, exact_out).  Built as a shared object with the Makefile's host flags and
// loaded with ctypes (tests/test_swap_out_precise_cpu.py); with -DSWAP_OUT_HOST_MAIN a stand-alone program for the
// sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/curve_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_path_checks.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/univ3_pool.h"

namespace {
constexpr int32_t kApplied = CFMM_SWAP_APPLIED, kOverLimit = CFMM_SWAP_OVER_LIMIT, kRefused = CFMM_SWAP_REFUSED, kUnobtainable = CFMM_SWAP_UNOBTAINABLE;
}

// One pool of n coins, `steps` exact-output swaps applied in order.  kind: CFMM_KIND_* (0 Product, 1 GeometricMean,
// 3 weighted, 4 Curve, 5 Solidly).  R [n] is the pool's state and moves; w [n] (kinds 1, 3; normalised here as the upload
// does), alpha, beta (kind 4).  max_in: null or [steps].  Per step: in[s] (the answer: +inf, NaN, the would-be quote or the
// quote), status[s], and the state after it in Rs [steps][n].  konst [steps][2]: the refreshed constants of the two coins
// that moved (GeometricMean {Q1, Q2}; weighted / Curve {q_in, q_out}; else, or when nothing moved, 0).
extern "C" int swap_out_host_pool(int kind, int n, double* R, const double* w, double alpha, double beta, double gamma, int steps,
                                  const int32_t* cin, const int32_t* cout, const double* want, const double* max_in, double* in,
                                  int32_t* status, double* Rs, double* konst)
{
    double wn[cfmm::kMaxCoins] = {0}, q[cfmm::kMaxCoins] = {0}, lbeta = 0.0;
    if (kind == 1 || kind == 3) {
        double ws = 0.0;
        for (int k = 0; k < n; ++k) ws += w[k];
        for (int k = 0; k < n; ++k) wn[k] = kind == 3 ? w[k] / ws : w[k];
    }
    if (kind == 4) {   // the upload: q = log R, {α, log β} (curve_solve_lbeta)
        for (int k = 0; k < n; ++k) q[k] = std::log(R[k]);
        lbeta = cfmm::curve_solve_lbeta(alpha, std::log(beta), q, n);
    }
    for (int s = 0; s < steps; ++s) {
        const int ci = cin[s], co = cout[s];
        if (ci < 0 || ci >= n || co < 0 || co >= n || ci == co) return -1;
        const double ri = R[ci], ro = R[co];
        double a;
        switch (kind) {
        case 0: a = cfmm::quote_out_product(ri, ro, gamma, want[s]); break;
        case 5: a = cfmm::quote_out_solidly(ri, ro, gamma, want[s]); break;
        case 1:
        case 3: a = cfmm::quote_out_weighted(ri, ro, wn[ci], wn[co], gamma, want[s]); break;
        case 4: {
            double srho = 0.0;
            for (int k = 0; k < n; ++k) srho += q[k];
            a = cfmm::quote_out_curve(ri, ro, srho, alpha, lbeta, gamma, want[s]);
            break;
        }
        default: return -1;
        }
        konst[2 * s] = konst[2 * s + 1] = 0.0;
        const bool within = !max_in || a <= max_in[s];
        int32_t st = kApplied;
        if (a == std::numeric_limits<double>::infinity()) {
            st = kUnobtainable;
        } else if (want[s] != 0.0) {   // (want == 0 moves nothing: swap_out_kernel's rule)
            const double2 rn = cfmm::swap_reserves(ri, ro, gamma, a, want[s]);
            bool valid = cfmm::swap_reserves_valid(rn, kind == 5);
            double qi = 0.0, qo = 0.0;
            if (kind == 3) {
                qi = cfmm::swap_weighted_q(rn.x, wn[ci]);
                qo = cfmm::swap_weighted_q(rn.y, wn[co]);
            } else if (kind == 4) {
                qi = cfmm::swap_curve_q(rn.x);
                qo = cfmm::swap_curve_q(rn.y);
                if (valid && alpha > 0.0) valid = cfmm::swap_curve_in_range(lbeta, q, 1, n, ci, qi, co, qo);
            }
            if (!valid) {
                a = std::nan("");
                st = kRefused;
            } else if (!within) {
                st = kOverLimit;
            } else {
                R[ci] = rn.x;
                R[co] = rn.y;
                if (kind == 4) { q[ci] = qi; q[co] = qo; }
                if (kind == 1) {
                    const double2 Q = cfmm::swap_geomean_q(gamma, wn[0] / wn[1], R[0], R[1]);
                    qi = Q.x;
                    qo = Q.y;
                }
                konst[2 * s] = qi;
                konst[2 * s + 1] = qo;
            }
        }
        in[s] = a;
        status[s] = st;
        for (int k = 0; k < n; ++k) Rs[s * n + k] = R[k];
    }
    return 0;
}

// One UniV3 pool (cfmm_pools_add_univ3's parametrisation), `steps` exact-output swaps applied in order: per step the answer,
// the status and the price the pool rests at afterwards (swap_univ3_price of the answer, clamped to the first tick's upper
// price as abi_swap.cpp does).  The pool is re-prepared from its price before every step, as the host does.
extern "C" int swap_out_host_univ3(double cp, double gamma, int64_t nt, const double* lt, const double* lq, int steps, const int32_t* cin,
                                   const double* want, const double* max_in, double* in, int32_t* status, double* price)
{
    for (int s = 0; s < steps; ++s) {
        const int64_t ct = cfmm::univ3_current_tick(lt, nt, cp);
        if (ct < 1) return -1;
        cfmm::UniV3PoolRec r;
        std::vector<cfmm::TickRec> ticks;
        cfmm::univ3_prepare_pool(cp, gamma, ct, nt, lt, lq, r, ticks);
        double a = cfmm::quote_out_univ3(r.cur_a, r.cur_b, r.cur_c, r.curR, r.walk, ticks.data(), r.pg.y, cin[s], want[s]);
        const bool within = !max_in || a <= max_in[s];
        int32_t st;
        if (a == std::numeric_limits<double>::infinity()) {
            st = kUnobtainable;
        } else {
            const double P = cfmm::swap_univ3_price(r.pg.x, r.cur_a, r.cur_b, r.cur_c, r.walk, ticks.data(), r.pg.y, cin[s], a);
            if (!cfmm::finite_pos(P)) {
                a = std::nan("");
                st = kRefused;
            } else if (!within) {
                st = kOverLimit;
            } else {
                st = kApplied;
                cp = P > lt[0] ? lt[0] : P;
            }
        }
        in[s] = a;
        status[s] = st;
        price[s] = cp;
    }
    return 0;
}

// cfmm_swap_path_out's checks beyond check_paths
extern "C" int swap_out_host_check(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                                   const double* max_amount_in, char* msg, int64_t len)
{
    return cfmm::check_swap_paths("cfmm_swap_path_out", count, n_hops, hop_seg, hop_row, max_amount_in, msg, (size_t)len, true);
}

#ifdef SWAP_OUT_HOST_MAIN
// a fixed set of sequences through every function above, for the sanitizers: prints the answers
int main()
{
    const int32_t cin[5] = {0, 1, 0, 2, 1}, cout[5] = {1, 0, 2, 0, 0};
    const double want[5] = {3.0, 0.0, 1e30, 0.5, 2.0}, lim[5] = {1e9, 1e9, 1e9, 1e9, 1e-9};
    for (int kind : {0, 1, 3, 4, 5}) {
        const int n = (kind == 3 || kind == 4) ? 3 : 2;
        double R[3] = {100.0, 250.0, 75.0}, w[3] = {0.2, 0.5, 0.3}, in[5], Rs[15], konst[10];
        int32_t ci[5], co[5], st[5];
        for (int s = 0; s < 5; ++s) { ci[s] = cin[s] % n; co[s] = cout[s] % n; if (ci[s] == co[s]) co[s] = (ci[s] + 1) % n; }
        if (swap_out_host_pool(kind, n, R, w, 2.0, 1e6, 0.997, 5, ci, co, want, lim, in, st, Rs, konst)) return 3;
        std::printf("kind %d: %.17g %.17g %.17g %.17g %.17g [%d %d %d %d %d] -> %.17g %.17g\n", kind, in[0], in[1], in[2], in[3], in[4], st[0],
                    st[1], st[2], st[3], st[4], R[0], R[1]);
        if (st[0] != kApplied || st[1] != kApplied || st[2] != kUnobtainable || st[4] != kOverLimit) return 5;
    }
    const double lt[5] = {4.0, 2.0, 1.0, 0.5, 0.25}, lq[5] = {16.0, 0.0, 9.0, 25.0, 4.0};
    const int32_t uc[4] = {0, 1, 1, 0};
    const double uw[4] = {1.5, 0.0, 1e9, 2.0};
    double in[4], price[4];
    int32_t st[4];
    if (swap_out_host_univ3(0.8, 0.997, 5, lt, lq, 4, uc, uw, nullptr, in, st, price)) return 4;
    std::printf("univ3: %.17g %.17g %.17g %.17g [%d %d %d %d] -> %.17g\n", in[0], in[1], in[2], in[3], st[0], st[1], st[2], st[3], price[3]);
    if (st[1] != kApplied || st[2] != kUnobtainable) return 6;
    // the limit check of the path entry: named at hop 0, under the entry's own name
    const int32_t n_hops[2] = {2, 1}, seg[4] = {0, 1, 1, -77};
    const int64_t row[4] = {5, 5, 6, (int64_t)1 << 40};
    char msg[256] = "";
    const double ok_lim[2] = {0.0, 1e300}, bad_lim[2] = {1.0, -1.0};
    if (swap_out_host_check(2, n_hops, seg, row, nullptr, msg, sizeof msg) != CFMM_OK || swap_out_host_check(2, n_hops, seg, row, ok_lim, msg, sizeof msg) != CFMM_OK || msg[0]) return 7;
    if (swap_out_host_check(2, n_hops, seg, row, bad_lim, msg, sizeof msg) != CFMM_ERR_INVALID_ARG ||
        !std::strstr(msg, "cfmm_swap_path_out: path 1, hop 0: max_amount_in must be finite and >= 0"))
        return 8;
    std::printf("%s\nSWAP_OUT_HOST_OK\n", msg);
    return 0;
}
#endif
