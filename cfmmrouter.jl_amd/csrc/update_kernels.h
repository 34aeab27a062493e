// update_kernels.h -- kernels that rewrite pool state or trade buffers in place: update_reserves! for the two-coin and
// N-coin families (F::q_of: sweep_ncoin.h), the expansion of compact trade records, sparse pool-state updates.
#pragma once

#include "fast_arith.h"

namespace cfmm {

// update_reserves!(r) for the two-coin families -- src/router.jl:127-132 with the update the routing
// problem prescribes (find_arb! docstring, src/cfmms.jl:26-31): R <- (R + γΔ) − Λ, in place, from
// the trades of the latest materialising sweep; GeometricMean segments refresh the exponents'
// v-independent constants {Q1, Q2} (see GeoMeanLogOps) with the same expressions as the upload.
// one pool's trades from the buffers (plain or compact layout, see SweepArgs)
__device__ __forceinline__ void read_trade(const double2* __restrict__ Delta, const double2* __restrict__ Lambda,
                                           const double2* __restrict__ Over, int compact, long long i, double2& d, double2& l)
{
    if (!compact) {
        d = Delta[i];
        l = Lambda[i];
        return;
    }
    const double2 r = Delta[i];
    if (r.y == -1.0) {
        d = Lambda[i];
        l = Over[i];
    } else if (__builtin_signbit(r.x)) {
        d = make_double2(0.0, -r.x);
        l = make_double2(r.y, 0.0);
    } else {
        d = make_double2(r.x, 0.0);
        l = make_double2(0.0, r.y);
    }
}

__global__ __launch_bounds__(256) void update_two_coin(double2* __restrict__ R, const double* __restrict__ gamma,
                                                       const double2* __restrict__ Delta,
                                                       const double2* __restrict__ Lambda,
                                                       const double2* __restrict__ Over, int compact,
                                                       double2* __restrict__ Q, const double* __restrict__ eta, long long m,
                                                       int* __restrict__ left_window)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double g = gamma[i];
    const double2 r = R[i];
    double2 d, l;
    read_trade(Delta, Lambda, Over, compact, i, d, l);
    const double2 rn = make_double2((r.x + g * d.x) - l.x, (r.y + g * d.y) - l.y);
    R[i] = rn;
    // a reserve that leaves the operand window of the fast arithmetic (sweep.h kFastExp) sends the segment back to the
    // compiler's division / square-root sequences
    if (left_window && !(in_fast_window(rn.x) && in_fast_window(rn.y))) *left_window = 1;
    if (Q) {
        const double e = eta[i], lg = log(g), le = log(e), l1 = log(rn.x), l2 = log(rn.y);
        Q[i] = make_double2(((lg + le) + l2) + e * l1, e * ((lg + l1) - le) + l2);
    }
}

__global__ __launch_bounds__(256) void expand_trades(const double2* __restrict__ rec, const double2* __restrict__ ovA,
                                                     const double2* __restrict__ ovB, double2* __restrict__ Delta,
                                                     double2* __restrict__ Lambda, long long m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double2 d, l;
    read_trade(rec, ovA, ovB, 1, i, d, l);
    Delta[i] = d;
    Lambda[i] = l;
}

// update_reserves! for N-coin segments: R <- (R + γΔ) − Λ per coin, q <- the family's constant (F::q_of); par stays (the
// weights, or Curve's α and β: the pool's parameters)
template <class F>
__global__ __launch_bounds__(256) void update_ncoin(double* __restrict__ R, double* __restrict__ q, const double* __restrict__ par,
                                                    const double2* __restrict__ glg, const double* __restrict__ Delta,
                                                    const double* __restrict__ Lambda, int n_coins, long long m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double g = glg[i].x;
    for (int k = 0; k < n_coins; ++k) {
        const long long j = (long long)k * m + i;
        const double rn = (R[j] + g * Delta[j]) - Lambda[j];
        R[j] = rn;
        q[j] = F::q_of(rn, par, j);
    }
}

// Sparse pool-state updates (sweep.h ScatterArgs): one lane moves one 8-byte word of one (pool, column) from the staging
// buffer -- read as one contiguous stream -- to the pool's row of the column; the rows are sorted by the host, so the words of
// neighbouring pools land in the same 128-byte lines where the update is dense.  Plain vector stores.
__global__ __launch_bounds__(256) void scatter_records(ScatterArgs a)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.total) return;
    int c = 0;
    for (int k = 1; k < a.ncols; ++k) c = g >= a.col[k].begin ? k : c;   // (columns in staging order)
    const ScatterCol col = a.col[c];
    const long long local = g - col.begin, j = local / col.width, t = local - j * col.width;
    if (j >= col.rows) return;                                            // (a gap between two columns)
    const long long row = col.dense_base >= 0 ? col.dense_base + j : a.idx[j];
    col.dst[row * col.width + t] = a.stage[g];
}

} // namespace cfmm
