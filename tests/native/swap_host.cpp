// swap_host.cpp -- TEST-ONLY host build of csrc/swap_pool.h + quote_pool.h + univ3_pool.h (and the HIP-free wave numbering,
// swap_waves.h): the very functions swap_kernel runs on the device, applied as the kernel and abi_swap.cpp apply them -- the
// quote, the validity test, the move, in query order.  Only the library functions (log, exp, expm1, ...) differ from the
// device: the host's libm here.  Built as a shared object with the Makefile's host flags and loaded with ctypes
// (tests/test_swap_precise_cpu.py); with -DSWAP_HOST_MAIN a stand-alone program for the sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/curve_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_waves.h"
#include "../../cfmmrouter.jl_amd/csrc/univ3_pool.h"

// One pool of n coins, `steps` swaps applied in order.  kind: CFMM_KIND_* (0 Product, 1 GeometricMean, 3 weighted, 4 Curve,
// 5 Solidly).  R [n] is the pool's state and moves; w [n] (kinds 1, 3; normalised here as the upload does), alpha, beta (kind
// 4).  Per step: out[s] (NaN: refused, the pool stays), and the state after it in Rs [steps][n].  konst [steps][2]: the
// refreshed constants of the two coins that moved (GeometricMean {Q1, Q2}; weighted / Curve {q_in, q_out}; else 0).
extern "C" int swap_host_pool(int kind, int n, double* R, const double* w, double alpha, double beta, double gamma, int steps,
                              const int32_t* cin, const int32_t* cout, const double* a, double* out, double* Rs, double* konst)
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
        double o;
        switch (kind) {
        case 0: o = cfmm::quote_product(ri, ro, gamma, a[s]); break;
        case 5: o = cfmm::quote_solidly(ri, ro, gamma, a[s]); break;
        case 1:
        case 3: o = cfmm::quote_weighted(ri, ro, wn[ci], wn[co], gamma, a[s]); break;
        case 4: {
            double srho = 0.0;
            for (int k = 0; k < n; ++k) srho += q[k];
            o = cfmm::quote_curve(ri, ro, srho, alpha, lbeta, gamma, a[s]);
            break;
        }
        default: return -1;
        }
        konst[2 * s] = konst[2 * s + 1] = 0.0;
        if (a[s] != 0.0) {   // (a == 0 moves nothing: swap_kernel's rule)
            const double2 rn = cfmm::swap_reserves(ri, ro, gamma, a[s], o);
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
                o = std::nan("");
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
        out[s] = o;
        for (int k = 0; k < n; ++k) Rs[s * n + k] = R[k];
    }
    return 0;
}

// One UniV3 pool (cfmm_pools_add_univ3's parametrisation), `steps` swaps applied in order: per step the answer and the price
// the pool rests at afterwards (clamped to the first tick's upper price, as abi_swap.cpp does; a price that is not finite
// and > 0 refuses the swap: NaN, the pool stays).  The pool is re-prepared from its price before every step, as the host does.
extern "C" int swap_host_univ3(double cp, double gamma, int64_t nt, const double* lt, const double* lq, int steps, const int32_t* cin,
                               const double* a, double* out, double* price)
{
    for (int s = 0; s < steps; ++s) {
        const int64_t ct = cfmm::univ3_current_tick(lt, nt, cp);
        if (ct < 1) return -1;
        cfmm::UniV3PoolRec r;
        std::vector<cfmm::TickRec> ticks;
        cfmm::univ3_prepare_pool(cp, gamma, ct, nt, lt, lq, r, ticks);
        double o = cfmm::quote_univ3(r.cur_a, r.cur_b, r.cur_c, r.curR, r.walk, ticks.data(), r.pg.y, cin[s], a[s]);
        double P = cfmm::swap_univ3_price(r.pg.x, r.cur_a, r.cur_b, r.cur_c, r.walk, ticks.data(), r.pg.y, cin[s], a[s]);
        if (!cfmm::finite_pos(P)) {
            o = std::nan("");
        } else {
            cp = P > lt[0] ? lt[0] : P;
        }
        out[s] = o;
        price[s] = cp;
    }
    return 0;
}

extern "C" int64_t swap_host_waves(int64_t count, const int64_t* idx, int64_t* wave, int64_t* perm, int64_t* wave_off)
{
    const int64_t waves = cfmm::swap_wave_numbers(count, idx, wave);
    const cfmm::SwapPlan p = cfmm::swap_plan(count, idx);
    for (int64_t j = 0; j < count; ++j) perm[j] = p.perm[(size_t)j];
    for (size_t w = 0; w < p.wave_off.size(); ++w) wave_off[w] = p.wave_off[w];
    return waves;
}

#ifdef SWAP_HOST_MAIN
// a fixed set of sequences through every function above, for the sanitizers: prints the answers
int main()
{
    const int32_t cin[4] = {0, 1, 0, 2}, cout[4] = {1, 0, 2, 0};
    const double a[4] = {3.0, 0.0, 1e30, 0.5};
    for (int kind : {0, 1, 3, 4, 5}) {
        const int n = (kind == 3 || kind == 4) ? 3 : 2;
        double R[3] = {100.0, 250.0, 75.0}, w[3] = {0.2, 0.5, 0.3}, out[4], Rs[12], konst[8];
        int32_t ci[4], co[4];
        for (int s = 0; s < 4; ++s) { ci[s] = cin[s] % n; co[s] = cout[s] % n; if (ci[s] == co[s]) co[s] = (ci[s] + 1) % n; }
        if (swap_host_pool(kind, n, R, w, 2.0, 1e6, 0.997, 4, ci, co, a, out, Rs, konst)) return 3;
        std::printf("kind %d: %.17g %.17g %.17g %.17g -> %.17g %.17g\n", kind, out[0], out[1], out[2], out[3], R[0], R[1]);
    }
    const double lt[5] = {4.0, 2.0, 1.0, 0.5, 0.25}, lq[5] = {16.0, 0.0, 9.0, 25.0, 4.0};
    const int32_t uc[4] = {0, 1, 1, 0};
    const double ua[4] = {1.5, 0.0, 1e9, 2.0};
    double out[4], price[4];
    if (swap_host_univ3(0.8, 0.997, 5, lt, lq, 4, uc, ua, out, price)) return 4;
    std::printf("univ3: %.17g %.17g %.17g %.17g -> %.17g\n", out[0], out[1], out[2], out[3], price[3]);
    const int64_t idx[5] = {5, 2, 5, 5, 2};
    int64_t wave[5], perm[5], off[6];
    const int64_t waves = swap_host_waves(5, idx, wave, perm, off);
    std::printf("waves %lld: %lld %lld %lld %lld %lld\nSWAP_HOST_OK\n", (long long)waves, (long long)wave[0], (long long)wave[1],
                (long long)wave[2], (long long)wave[3], (long long)wave[4]);
    return 0;
}
#endif
