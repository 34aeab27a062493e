// select_kernels.h -- cfmm_select_trades: an order-preserving stream compaction of one segment's trades.  Three launches,
// none of which has a block that waits for another block:
//   select_flag   one lane per pool: does it trade, and is it worth min_value?  One 64-lane ballot per wavefront = one mask
//                 word (1 bit per pool); the block's popcount goes to counts[block]
//   select_scan   ONE block walks counts[] in chunks of kSelScanChunk and carries the running total: exclusive bases per block,
//                 and the grand total, which it also stores to pinned host memory
//   select_emit   a selected lane's slot = base[block] + set bits of the block's earlier wavefronts + set bits below the lane
//                 (mbcnt); lanes whose slot is below `capacity` decode their trade and write idx, the expanded rows and the value
// The value of a pool is its term of the dual acc, value = Σ_k (Λ_k − Δ_k)·v[A_k], summed in coin order from +0.0 with every
// operation rounded on its own (this translation unit is compiled with -ffp-contract=off): the host reproduces it bit for bit.
// RAGGED = false: the two-coin trade buffers (read_trade: plain or compact layout, overflow rows included), tokens from the
// packed records or Ai.  RAGGED = true: the coin-major columns of a weighted / Curve segment, walked coin by coin -- no
// per-coin register arrays, so the two-coin instantiation does not pay for kMaxCoins.
#pragma once

#include "update_kernels.h"

namespace cfmm {

// (SelectArgs, kSelBlock, kSelScanChunk: sweep.h)

// the two tokens of two-coin pool i
__device__ __forceinline__ int2 select_tokens(const SelectArgs& a, long long i)
{
    if (a.pk) {
        const unsigned t = a.pk[i].tok;
        return make_int2((int)(t & 0xffffu), (int)(t >> 16));
    }
    return a.Ai[i];
}

// Pool i of the segment: trades = some entry of Δ or Λ compares != 0.0 (−0.0 does not, NaN does); value as above.
template <bool RAGGED>
__device__ __forceinline__ void select_eval(const SelectArgs& a, long long i, bool& trades, double& value)
{
    double acc = 0.0;
    if (RAGGED) {
        bool any = false;
        for (int k = 0; k < a.n_coins; ++k) {
            const long long j = (long long)k * a.m + i;
            const double d = a.ncD[j], l = a.ncL[j];
            any = any || d != 0.0 || l != 0.0;
            acc = acc + (l - d) * a.v[a.nctok[j]];
        }
        trades = any;
    } else {
        double2 d, l;
        read_trade(a.Delta, a.Lambda, a.Over, a.compact, i, d, l);
        const int2 t = select_tokens(a, i);
        trades = d.x != 0.0 || d.y != 0.0 || l.x != 0.0 || l.y != 0.0;
        acc = acc + (l.x - d.x) * a.v[t.x];
        acc = acc + (l.y - d.y) * a.v[t.y];
    }
    value = acc;
}

template <bool RAGGED>
__global__ __launch_bounds__(kSelBlock) void select_flag(SelectArgs a)
{
    __shared__ int wave_count[kSelBlock / 64];
    const long long i = (long long)blockIdx.x * kSelBlock + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    bool pred = false;
    if (i < a.m) {
        bool trades;
        double value;
        select_eval<RAGGED>(a, i, trades, value);
        pred = trades && !(value < a.min_value);   // a NaN value is never hidden
    }
    const unsigned long long word = __ballot(pred);
    if ((threadIdx.x & 63) == 0) {
        a.mask[(long long)blockIdx.x * (kSelBlock / 64) + wave] = word;
        wave_count[wave] = __popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < kSelBlock / 64; ++w) n += wave_count[w];
        a.counts[blockIdx.x] = n;
    }
}

// base[b] = Σ counts[0 .. b), *total = Σ counts[0 .. blocks): one block, chunk after chunk; within a chunk a wavefront scans
// its 64 counts with shuffles and the wavefronts' totals are combined through LDS
__global__ __launch_bounds__(kSelScanChunk) void select_scan(const int* __restrict__ counts, long long* __restrict__ base,
                                                             long long blocks, long long* __restrict__ total_host)
{
    __shared__ long long wave_total[kSelScanChunk / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long long first = 0; first < blocks; first += kSelScanChunk) {
        const long long b = first + threadIdx.x;
        const long long own = b < blocks ? (long long)counts[b] : 0;
        long long incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            const long long up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        long long before = 0, chunk = 0;
        for (int w = 0; w < kSelScanChunk / 64; ++w) {
            const long long t = wave_total[w];
            before += w < wave ? t : 0;
            chunk += t;
        }
        if (b < blocks) base[b] = carry + before + (incl - own);
        carry += chunk;
        __syncthreads();   // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *total_host = carry;
}

template <bool RAGGED>
__global__ __launch_bounds__(kSelBlock) void select_emit(SelectArgs a)
{
    const long long block_base = a.base[blockIdx.x];
    if (block_base >= a.capacity) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* words = a.mask + (long long)blockIdx.x * (kSelBlock / 64);
    const unsigned long long word = words[wave];
    if (!((word >> lane) & 1ull)) return;
    int earlier = 0;
    for (int w = 0; w < wave; ++w) earlier += __popcll(words[w]);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
    const long long slot = block_base + earlier + below;
    if (slot >= a.capacity) return;
    const long long i = (long long)blockIdx.x * kSelBlock + threadIdx.x;   // (< m: the bit is set)
    if (a.out_idx) a.out_idx[slot] = i;
    if (RAGGED) {
        double acc = 0.0;
        for (int k = 0; k < a.n_coins; ++k) {
            const long long j = (long long)k * a.m + i;
            const double d = a.ncD[j], l = a.ncL[j];
            if (a.out_D) a.out_D[slot * a.n_coins + k] = d;
            if (a.out_L) a.out_L[slot * a.n_coins + k] = l;
            acc = acc + (l - d) * a.v[a.nctok[j]];
        }
        if (a.out_value) a.out_value[slot] = acc;
    } else {
        double2 d, l;
        read_trade(a.Delta, a.Lambda, a.Over, a.compact, i, d, l);
        if (a.out_D) reinterpret_cast<double2*>(a.out_D)[slot] = d;
        if (a.out_L) reinterpret_cast<double2*>(a.out_L)[slot] = l;
        if (a.out_value) {
            const int2 t = select_tokens(a, i);
            double acc = 0.0;
            acc = acc + (l.x - d.x) * a.v[t.x];
            acc = acc + (l.y - d.y) * a.v[t.y];
            a.out_value[slot] = acc;
        }
    }
}

} // namespace cfmm
