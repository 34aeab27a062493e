// update_kernels.h -- kernels that rewrite pool state or trade buffers in place: update_reserves! for the two-coin and
// N-coin families (F::q_of: sweep_ncoin.h), the expansion of compact trade records, sparse pool-state updates, the
// compaction of a UniV3 segment's tick records.
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

// Compaction of a UniV3 segment's tick records (abi_update.cpp univ3_make_room): every pool's two walk lists -- back to back
// in the old array, walk.y + walk.w + 2 records of 64 bytes from walk.x -- move to the pool's base in a fresh, tight array;
// thr[e] is rewritten from record e's own thr field, the pool's new span goes to the fresh walk array, and the four
// read-ahead thresholds behind the new tail are zeroed.  The host computed the new spans (new_walk: pinned staging, read once).
// kCompactGroup = 16 lanes per pool, 16 bytes per lane and step: a group's step is 256 contiguous bytes = four records = two
// full 128-byte lines on either side (records are 64-byte aligned), the mean list of the 1M-pool market (19 records) takes
// 5 steps, and a wavefront waits for the longest of 4 pools, not of 8 or 16.  Plain vector loads and stores: no atomics, no
// LDS, no block reads what another writes (source and destination are different allocations).
constexpr int kCompactGroup = 16;
__global__ __launch_bounds__(256) void compact_walks(const int4* __restrict__ old_walk, const int4* __restrict__ new_walk,
                                                     int4* __restrict__ walk_out, const TickRec* __restrict__ old_ticks,
                                                     TickRec* __restrict__ ticks, double* __restrict__ thr, long long m,
                                                     long long tail)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) thr[tail + threadIdx.x] = 0.0;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) / kCompactGroup;
    const int lane = (int)threadIdx.x % kCompactGroup;
    if (i >= m) return;
    const int4 wo = old_walk[i], wn = new_walk[i];
    if (lane == 0) walk_out[i] = wn;
    const int pieces = 4 * (wo.y + wo.w + 2);                                  // 16-byte pieces of the pool's records
    const double2* __restrict__ src = reinterpret_cast<const double2*>(old_ticks + wo.x);
    double2* __restrict__ dst = reinterpret_cast<double2*>(ticks + wn.x);
    double* __restrict__ t = thr + wn.x;
    for (int k = lane; k < pieces; k += kCompactGroup) {
        const double2 q = src[k];
        dst[k] = q;
        if ((k & 3) == 2) t[k >> 2] = q.y;                                     // piece 2 of a record is {rout, thr}
    }
}

} // namespace cfmm
