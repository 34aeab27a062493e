// to_rate_host.cpp -- TEST-ONLY host build of csrc/to_rate_pool.h beside csrc/rate_pool.h: the very functions to_rate_kernel runs
// on the device, fed the state as the upload prepares it (tests/native/rate_host.cpp's preparation, line for line).  Only the
// library functions differ from the device: the host's libm here.  Every query answers the amount to the limit, the rate the
// same build's rate function reports AT that amount (the round trip) and, on Curve, the evaluations the search made.
// Two uses (tests/test_to_rate_precise_cpu.py): built as a shared object with the Makefile's host flags and loaded with ctypes;
// and built with -DTO_RATE_HOST_MAIN under the address and undefined-behaviour sanitizers as a stand-alone program that reads
// the queries from a flat binary file and writes its answers to another.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/curve_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/to_rate_pool.h"
#include "../../cfmmrouter.jl_amd/csrc/univ3_pool.h"

extern "C" int to_rate_host_curve_cap(void) { return cfmm::kToRateCurveIters; }

// kind: CFMM_KIND_* (0 Product, 1 GeometricMean, 3 weighted, 4 Curve, 5 Solidly).  R, w: [m, n] row-major (w: weighted
// kinds, else null); alpha, beta: Curve, else null; cin, cout, iters: [m].  Returns 0, or -1 for a kind it does not know.
extern "C" int to_rate_host_pools(int kind, int n, int64_t m, const double* R, const double* w, const double* alpha, const double* beta,
                                  const double* gamma, const int32_t* cin, const int32_t* cout, const double* r, double* amount,
                                  double* rate_back, int32_t* iters)
{
    for (int64_t i = 0; i < m; ++i) {
        const double* Ri = R + i * n;
        const double ri = Ri[cin[i]], ro = Ri[cout[i]], g = gamma[i];
        iters[i] = 0;
        switch (kind) {
        case 0:
            amount[i] = cfmm::to_rate_product(ri, ro, g, r[i]);
            rate_back[i] = cfmm::rate_product(ri, ro, g, amount[i]);
            break;
        case 5:
            amount[i] = cfmm::to_rate_solidly(ri, ro, g, r[i]);
            rate_back[i] = cfmm::rate_solidly(ri, ro, g, amount[i]);
            break;
        case 1:
            amount[i] = cfmm::to_rate_weighted(ri, ro, w[i * n + cin[i]], w[i * n + cout[i]], g, r[i]);
            rate_back[i] = cfmm::rate_weighted(ri, ro, w[i * n + cin[i]], w[i * n + cout[i]], g, amount[i]);
            break;
        case 3: {   // the upload's normalisation (abi_upload.cpp cfmm_pools_add_weighted)
            double ws = 0.0;
            for (int k = 0; k < n; ++k) ws += w[i * n + k];
            amount[i] = cfmm::to_rate_weighted(ri, ro, w[i * n + cin[i]] / ws, w[i * n + cout[i]] / ws, g, r[i]);
            rate_back[i] = cfmm::rate_weighted(ri, ro, w[i * n + cin[i]] / ws, w[i * n + cout[i]] / ws, g, amount[i]);
            break;
        }
        case 4: {   // q = log R, {α, log β} (curve_solve_lbeta), summed in coin order as quote_sum_logs does
            double rho[cfmm::kMaxCoins], srho = 0.0;
            for (int k = 0; k < n; ++k) rho[k] = std::log(Ri[k]);
            for (int k = 0; k < n; ++k) srho += rho[k];
            const double lb = cfmm::curve_solve_lbeta(alpha[i], std::log(beta[i]), rho, n);
            int it = 0;
            amount[i] = cfmm::to_rate_curve(ri, ro, srho, alpha[i], lb, g, r[i], &it);
            iters[i] = it;
            rate_back[i] = cfmm::rate_curve(ri, ro, srho, alpha[i], lb, g, amount[i]);
            break;
        }
        default: return -1;
        }
    }
    return 0;
}

// UniV3: p pools in CSR form (cfmm_pools_add_univ3's parametrisation), q queries {pool, coin in, limit}
extern "C" int to_rate_host_univ3(int64_t p, const double* current_price, const double* gamma, const int64_t* tick_off,
                                  const double* lower_ticks, const double* liquidity, int64_t q, const int64_t* pool, const int32_t* cin,
                                  const double* r, double* amount, double* rate_back)
{
    std::vector<cfmm::UniV3PoolRec> rec((size_t)p);
    std::vector<cfmm::TickRec> ticks;
    for (int64_t i = 0; i < p; ++i) {
        const double* lt = lower_ticks + tick_off[i];
        const int64_t nt = tick_off[i + 1] - tick_off[i];
        const int64_t ct = cfmm::univ3_current_tick(lt, nt, current_price[i]);
        if (ct < 1) return -1;
        cfmm::univ3_prepare_pool(current_price[i], gamma[i], ct, nt, lt, liquidity + tick_off[i], rec[(size_t)i], ticks);
    }
    for (int64_t j = 0; j < q; ++j) {
        if (pool[j] < 0 || pool[j] >= p) return -1;
        const cfmm::UniV3PoolRec& x = rec[(size_t)pool[j]];
        amount[j] = cfmm::to_rate_univ3(x.cur_a, x.cur_b, x.cur_c, x.curR, x.walk, ticks.data(), x.pg.y, cin[j], r[j]);
        rate_back[j] = cfmm::rate_univ3(x.cur_a, x.cur_b, x.cur_c, x.curR, x.walk, ticks.data(), x.pg.y, cin[j], amount[j]);
    }
    return 0;
}

#ifdef TO_RATE_HOST_MAIN
// to_rate_host IN OUT.  IN: tests/native/rate_host.cpp's blocks of 8-byte words with the limits in the place of the amounts.
// OUT: per block the amounts, then the rates at them, as doubles.
namespace {
template <class T> bool rd(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
}
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* outf = std::fopen(argv[2], "wb");
    if (!in || !outf) return 2;
    int64_t head[4];
    long blocks = 0, rows = 0;
    while (std::fread(head, sizeof head, 1, in) == 1) {
        std::vector<double> amount, back;
        if (head[0] == 1) {
            const int kind = (int)head[1], n = (int)head[2];
            const size_t m = (size_t)head[3];
            std::vector<double> R, w, al, be, g, r;
            std::vector<int64_t> ci64, co64;
            bool ok = rd(in, R, m * n) && rd(in, w, (kind == 1 || kind == 3) ? m * n : 0) && rd(in, al, kind == 4 ? m : 0) &&
                      rd(in, be, kind == 4 ? m : 0) && rd(in, g, m) && rd(in, ci64, m) && rd(in, co64, m) && rd(in, r, m);
            if (!ok) return 3;
            std::vector<int32_t> ci(ci64.begin(), ci64.end()), co(co64.begin(), co64.end()), iters(m);
            amount.resize(m);
            back.resize(m);
            if (to_rate_host_pools(kind, n, (int64_t)m, R.data(), w.empty() ? nullptr : w.data(), al.empty() ? nullptr : al.data(),
                                   be.empty() ? nullptr : be.data(), g.data(), ci.data(), co.data(), r.data(), amount.data(), back.data(),
                                   iters.data()))
                return 4;
        } else if (head[0] == 2) {
            const size_t p = (size_t)head[1], q = (size_t)head[2], T = (size_t)head[3];
            std::vector<double> cp, g, lt, lq, r;
            std::vector<int64_t> off, pool, ci64;
            bool ok = rd(in, cp, p) && rd(in, g, p) && rd(in, off, p + 1) && rd(in, lt, T) && rd(in, lq, T) && rd(in, pool, q) &&
                      rd(in, ci64, q) && rd(in, r, q);
            if (!ok) return 3;
            std::vector<int32_t> ci(ci64.begin(), ci64.end());
            amount.resize(q);
            back.resize(q);
            if (to_rate_host_univ3((int64_t)p, cp.data(), g.data(), off.data(), lt.data(), lq.data(), (int64_t)q, pool.data(), ci.data(),
                                   r.data(), amount.data(), back.data()))
                return 4;
        } else {
            return 5;
        }
        if (!amount.empty() && (std::fwrite(amount.data(), sizeof(double), amount.size(), outf) != amount.size() ||
                                std::fwrite(back.data(), sizeof(double), back.size(), outf) != back.size()))
            return 6;
        ++blocks;
        rows += (long)amount.size();
    }
    std::fclose(in);
    std::fclose(outf);
    std::printf("TO_RATE_HOST_OK %ld blocks %ld rows\n", blocks, rows);
    return 0;
}
#endif
