// curve_host.cpp -- TEST-ONLY host build of the Curve (StableSwap) per-pool solve: curve_pool.h's curve_solve<N>, the very
// template sweep_ncoin<CurveFamily> runs on the device, for N = 2..8, with the same inputs (log R and log β as the upload
// computes them: curve_solve_lbeta; pools it refuses, curve_in_range at α > 0, are flagged and get NaN trades) and the same turn of log r into trades as curve_pool in sweep_ncoin.h.  Only exp, log and expm1 differ
// from the device (the host's libm here).  Built and loaded (ctypes) by tests/test_curve_precise_cpu.py with the
// Makefile's host flags.
#include <cmath>
#include <cstdint>

#include "../../cfmmrouter.jl_amd/csrc/curve_pool.h"

namespace {

template <int N>
void solve_rows(int64_t m, const double* R_, const double* v_, const double* alpha, const double* beta, const double* gamma,
                double* D, double* L, int32_t* refused)
{
    for (int64_t i = 0; i < m; ++i) {
        double R[N], rho[N], v[N], lr[N];
        for (int k = 0; k < N; ++k) {
            R[k] = R_[i * N + k];
            rho[k] = std::log(R[k]);   // the upload's q = log R
            v[k] = v_[i * N + k];
        }
        const double g = gamma[i], lb = std::log(beta[i]);
        refused[i] = alpha[i] > 0.0 && !cfmm::curve_in_range(lb, rho, N);
        if (refused[i]) {
            for (int k = 0; k < N; ++k) D[i * N + k] = L[i * N + k] = __builtin_nan("");
            continue;
        }
        if (!cfmm::curve_solve<N>(rho, R, v, alpha[i], cfmm::curve_solve_lbeta(alpha[i], lb, rho, N), g, lr)) {
            for (int k = 0; k < N; ++k) D[i * N + k] = L[i * N + k] = 0.0;
            continue;
        }
        const double rg = 1.0 / g;
        for (int k = 0; k < N; ++k) {
            const bool nan_k = lr[k] != lr[k];
            const double em = std::expm1(lr[k] - rho[k]);
            L[i * N + k] = nan_k ? lr[k] : (lr[k] < rho[k] ? -(R[k] * em) : 0.0);
            D[i * N + k] = nan_k ? lr[k] : (lr[k] > rho[k] ? (R[k] * em) * rg : 0.0);
        }
    }
}

} // namespace

// R, v: [m, n] row-major (v = each coin's price); alpha, beta, gamma: [m].  -> D, L [m, n], refused [m] (the upload's
// range check).  Returns 0, or -1 for n outside 2..8.
extern "C" int curve_host_solve(int n, int64_t m, const double* R, const double* v, const double* alpha, const double* beta,
                                const double* gamma, double* D, double* L, int32_t* refused)
{
    switch (n) {
    case 2: solve_rows<2>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 3: solve_rows<3>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 4: solve_rows<4>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 5: solve_rows<5>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 6: solve_rows<6>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 7: solve_rows<7>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    case 8: solve_rows<8>(m, R, v, alpha, beta, gamma, D, L, refused); return 0;
    default: return -1;
    }
}
