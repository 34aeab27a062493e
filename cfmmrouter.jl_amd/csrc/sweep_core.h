// sweep_core.h -- the fused two-coin sweep: trade and row stores, the LDS layout, price staging, one pool's solve and
// epilogue (process_pool: finish_pool, and process_pool_lean for the lean two-coin kernels), the tile loops, the block epilogue and the kernels sweep_kernel (one segment) / sweep_multi (several).
#pragma once

#include "granule.h"
#include "ops_two_coin.h"
#include "ops_univ3.h"

#include <type_traits>

namespace cfmm {

// ---------------------------------------------------------------------------------------------
// The sweep: src/router.jl:38-42 fused with :79-83 and :98-100
// ---------------------------------------------------------------------------------------------
// Trade stores (Δ, Λ: 16 B per lane, written once, never re-read by the sweep) are write-through (`sc1`): the bytes
// leave during the sweep instead of in a serial flush of dirty L2 lines at its end (MI355X_MICROARCH.md, boundary row:
// + B / 6 TB/s for B dirty bytes; measured against plain and non-temporal stores in rounds 1 and 2: -1..-2 us per
// 1M-pool sweep).
// The s_nop is part of the store: a VMEM store of more than 8 bytes reads its upper data registers one cycle after
// issue, and the VALU must not overwrite them in that cycle (gfx9 hazard "VMEM store > 8 bytes followed by a write of
// the VGPRs holding the write data: 1 wait state").  The compiler inserts that wait state for its own stores; it
// cannot see through inline asm -- and the values stored here are selects computed right before the next store, so the
// next v_cndmask may land in the registers of this one (found as 9 % wrong rows in the two-row trade layout).
typedef double d2v __attribute__((ext_vector_type(2)));
// nt (SweepArgs::nt_stores, launch-uniform): non-temporal instead of write-through -- for markets whose pool state comes from
// HBM on every sweep (too large for the Infinity Cache, or a caller that rotates over many markets): the trade lines then
// bypass the cache hierarchy instead of displacing pool state that is about to be read.
__device__ __forceinline__ void store_pair(double2* dst, double x, double y, int nt)
{
    d2v val = {x, y};
    if (nt) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(dst), "v"(val) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(dst), "v"(val) : "memory");
}
// The lean kernels' form of the same write-through store: record i of the segment's trade rows as the rows' base (a launch
// constant, in SGPRs) plus a 32-bit per-lane byte offset -- the offset the lane's reserve load already uses, so a tile's
// store costs no address arithmetic.  The leading s_nop: the compiler may have parked the base in a VGPR lane, and a VMEM
// instruction must not read an SGPR in the 5 wait states after a v_readlane wrote it (it pads its own instructions, not
// the inside of an asm statement).
__device__ __forceinline__ void store_pair_at(double2* base, uint32_t i, double x, double y)
{
    d2v val = {x, y};
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" : : "v"(i * 16u), "v"(val), "s"(base) : "memory");
}

// Partial rows are written through as well: no dirty line is left for the end-of-kernel release in front of the fold
// launch (A/B: -0.3..-0.45 us per step on single-family launches, +-0.1 on config3; profiles/r03_ab_row_write_through.txt).
__device__ __forceinline__ void store_row(double* dst, double x)
{
    asm volatile("global_store_dwordx2 %0, %1, off sc1" : : "v"(dst), "v"(x) : "memory");
}

// One block's share of a segment: the tiles its block record names (sweep.h BlockRec); its
// partial row goes to partials[row].
// GBINS = true is the large-market mode (n_tokens > kMaxLdsTokens, v and the bins no longer fit
// LDS): v is gathered straight from global memory (it stays L2-resident) and every pool's two
// flows Λ−Δ are written to a flow array; Ψ is then PULLED per token over a token -> (pool, side)
// incidence list built at upload (gather_chunks / token_fold below) -- no float atomics, fixed
// summation order.  The partial rows carry only the dual scalar.
// LDS of a sweeping block: the prices {v, rcp_refined(v)} per token, the launch's fee table {γ, rcp_refined(γ)},
// log v (launches with a log-space GeometricMean segment), the netflow bins (one copy per wavefront, or one
// shared copy) and one slot per wavefront for the dual-scalar fold.
struct SweepLds {
    double2* vy;       // [n_pad] {v, rcp_refined(v)}  (a.v_shift == 3: [n_pad] doubles, the prices alone)
    double2* gtab;     // [gtab_n] {γ, rcp_refined(γ)}
    double* lv;        // [n_pad] log v (only when a.need_logv)
    double* bins;      // [copies][n_pad]
    double* wsum;      // [kWaves] dual-scalar fold
    double* flags;     // [kWaves + 1] stage_prices: per-wavefront "prices in the fast window", then "launch is live"
    double* my_bins;   // this wavefront's copy
};

template <int BLOCK, bool GBINS>
__device__ __forceinline__ SweepLds carve_lds(const SweepArgs& a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    SweepLds L;
    if constexpr (GBINS) {
        L.vy = nullptr;
        L.gtab = nullptr;
        L.lv = L.bins = L.my_bins = L.flags = nullptr;
        L.wsum = lds;
        return L;
    }
    L.vy = reinterpret_cast<double2*>(lds);
    L.gtab = reinterpret_cast<double2*>(lds + ((size_t)a.n_pad << (a.v_shift - 3)));
    L.lv = reinterpret_cast<double*>(L.gtab + a.gtab_n);
    L.bins = L.lv + (a.need_logv ? a.n_pad : 0);
    L.wsum = L.bins + (size_t)a.copies * a.n_pad;
    L.flags = L.wsum + BLOCK / 64;
    L.my_bins = L.bins + (size_t)(a.copies == 1 ? 0 : (threadIdx.x >> 6)) * a.n_pad;
    return L;
}

// Pre-armed launch: one lane waits for the host's word (see SweepArgs::arm_word).  1 = v is in place, 0 = the launch is
// cancelled -- this sequence number with the cancel bit, or ANY later sequence number: the host has moved on (it
// overwrites the one word while blocks of an abandoned launch may still be starting) --, -1 = gave up waiting.
__device__ __forceinline__ int wait_armed(const SweepArgs& a)
{
    const long long t0 = (long long)wall_clock64();
    for (;;) {
        const unsigned long long w = __hip_atomic_load(a.arm_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (w == a.arm_seq) return 1;
        if ((w & ~kArmCancel) > a.arm_seq || w == (a.arm_seq | kArmCancel)) return 0;
        if ((long long)wall_clock64() - t0 > a.arm_timeout) return -1;
        __builtin_amdgcn_s_sleep(1);
    }
}

// A block reports WHY it poisons its row (NaN in every column): one sticky word in mapped host memory, read by the
// host when it meets a non-finite result (abi_handover.cpp).  Rare paths only.
__device__ __forceinline__ void report(const SweepArgs& a, unsigned long long bit)
{
    if (a.flags && threadIdx.x == 0) __hip_atomic_fetch_or(a.flags, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// bins <- 0, fee table and prices -> LDS, barrier.  Whole block.  Result (block-uniform): kStageLive unless this is a
// pre-armed launch that was cancelled or gave up waiting for its prices (then also kStageGaveUp); kStageFast when every
// staged price lies in the window of the fast arithmetic.
constexpr int kStageLive = 1, kStageFast = 2, kStageGaveUp = 4;
// Prices first (sweep_kernel / sweep_multi): a lane's first kPricePre prices, v[tid], v[tid + BLOCK], requested at the
// kernel's FIRST instruction from the preloaded v and n, before the block's record is read -- behind them come a reciprocal
// and a binary64 logarithm per token and the barrier every wavefront waits at before its first pool, and the first tile's
// pool data is there when that barrier is passed (profiles/sweep_entry_preload.txt).  The indices are clamped to n - 1, so
// every lane loads a valid price and there is no branch in front of the loads; a lane uses only those with an index < n.
// A pre-armed launch requests them too and does not use them: its v is written after the kernel may have started.  Its
// own loads behind wait_armed are system-scope (sc0 sc1) loads of fine-grained memory, which are served by the memory
// itself and not by a line an earlier plain load -- these requests, or the previous evaluation's staging -- left in a cache:
// the assumption every pre-armed evaluation after the first has always made (the buffer is reused), not a new one.
constexpr int kPricePre = 2;
struct PricePre {
    double p[kPricePre];
};
template <int BLOCK>
__device__ __forceinline__ PricePre request_prices(const double* v, int n)
{
    PricePre r;
#pragma unroll
    for (int k = 0; k < kPricePre; ++k) {
        const int j = (int)threadIdx.x + k * BLOCK;
        r.p[k] = v[j < n ? j : n - 1];
    }
    return r;
}
template <int BLOCK, bool GBINS, bool PRE = false, bool LEAN = false>
__device__ __forceinline__ int stage_prices(const SweepArgs& a, const SweepLds& L, const PricePre& pre = PricePre{})
{
    if constexpr (GBINS) {
        __syncthreads();
        return kStageLive;
    }
    const int tid = threadIdx.x;
    const int n_zero = a.copies * a.n_pad;                // LDS bins to clear
    const bool logs = a.need_logv != 0;
    const bool armed = a.arm_word != nullptr;             // kernel argument: block-uniform
    bool live = true, gave_up = false;
    if (armed) {
        // pre-armed launch: everything that does not need the prices first, then the wait
        for (int j = tid; j < n_zero; j += BLOCK) L.bins[j] = 0.0;
        for (int j = tid; j < a.gtab_n; j += BLOCK) {
            const double g = a.gtab[j];
            L.gtab[j] = make_double2(g, rcp_refined(g));
        }
        if (tid == 0) L.flags[BLOCK / 64] = (double)wait_armed(a);
        __syncthreads();
        live = L.flags[BLOCK / 64] > 0.0;
        gave_up = L.flags[BLOCK / 64] < 0.0;
    }
    bool in_window = true;
    for (int j = tid, k = 0; j < a.n; j += BLOCK, ++k) {
        // armed: the host wrote v through the PCIe BAR after this kernel may have started -- system-scope loads
        double vj;
        if (armed) vj = __hip_atomic_load(a.v + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (PRE && k < kPricePre) vj = k == 0 ? pre.p[0] : pre.p[1];   // requested at the kernel's first instruction
        else vj = a.v[j];
        if (a.v_shift == 4) L.vy[j] = make_double2(vj, rcp_refined(vj));
        else reinterpret_cast<double*>(L.vy)[j] = vj;
        in_window = in_window && in_fast_window(vj);
        if (logs) L.lv[j] = log(vj);     // once per token per block: the only logarithm of a GeometricMean sweep
    }
    if (!armed) {
        // the price loads are in flight while the bins are cleared
        for (int j = tid; j < n_zero; j += BLOCK) L.bins[j] = 0.0;
        for (int j = tid; j < a.gtab_n; j += BLOCK) {
            const double g = a.gtab[j];
            L.gtab[j] = make_double2(g, rcp_refined(g));
        }
    }
    // block-wide AND of in_window through LDS (the library's __syncthreads_and would add 256 bytes of STATIC LDS to
    // every kernel, which the 160 KiB dynamic ceiling of hipFuncSetAttribute then no longer leaves room for)
    const bool wave_in = __all(in_window ? 1 : 0) != 0;
    if ((tid & 63) == 0) L.flags[tid >> 6] = wave_in ? 1.0 : 0.0;
    __syncthreads();
    bool all_in = true;
    if constexpr (LEAN) {
        // the lean kernels: the flags as 16-byte reads (carve_lds: 16-byte aligned there), one wait, and an AND of their high
        // words (1.0 / +0.0) instead of a short-circuit chain of one branch per wavefront
        static_assert((BLOCK / 64) % 2 == 0, "flags are read in pairs");
        const double2* pairs = reinterpret_cast<const double2*>(L.flags);
        int bits = -1;
#pragma unroll
        for (int w = 0; w < BLOCK / 128; ++w) {
            const double2 f = pairs[w];
            bits &= __double2hiint(f.x) & __double2hiint(f.y);
        }
        all_in = bits != 0;
    } else {
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) all_in = all_in && L.flags[w] != 0.0;
    }
    return (live ? kStageLive : 0) | (all_in ? kStageFast : 0) | (gave_up ? kStageGaveUp : 0);
}

// One pool behind its prices: closed form, trade record, dual scalar, netflow bins.
// LEAN (sweep_body): a.compact, a.nt_stores, a.v_shift, a.need_logv and a.copies are compile-time constants here, the fee
// comes from the LDS table and the trade record leaves through store_pair_at; the code is this one.
template <class Ops, bool MAT, bool GBINS, bool FAST, bool LEAN, class Idx>
__device__ __forceinline__ void finish_pool(const Ops& ops, const SweepArgs& a, const SweepLds& L, const typename Ops::Raw& raw,
                                            const Px& px, int2 tok, Idx i, double& acc)
{
    // a compact trade record {x, y} of pool i
    const auto put_record = [&](double x, double y) {
        if constexpr (LEAN) store_pair_at(a.Delta, i, x, y);
        else store_pair(a.Delta + i, x, y, a.nt_stores);
    };
    Trade t;
    double d, l;
    int dir;
    dir = ops.template solve_dir<FAST>(raw, px, d, l, t);
    const double v1 = px.v1, v2 = px.v2;
    // One direction (the common case): the tendered token's bin gets −d, the received token's +l, the dual scalar
    // l·v_out − d·v_in -- the reference's expressions (src/router.jl:82, :99) with their zero terms dropped: same bits.
    // A compact trade record needs two values with a clear sign bit; the tiny negative / −0.0 amounts the reference's
    // tick arithmetic leaves on degenerate UniV3 boundaries (and anything kDirBoth) take the general path below.
    const bool one = dir == kDir1 || dir == kDir2;
    const bool plain = one && (!MAT || !a.compact || (__double2hiint(d) | __double2hiint(l)) >= 0);
    if (plain) {
        const bool d1 = dir == kDir1;
        if (MAT) {
            if (a.compact) {
                put_record(d1 ? d : -d, l);   // {+Δ₁, Λ₂} or {−Δ₂, Λ₁}: the sign bit carries the direction
            } else {
                store_pair(a.Delta + i, d1 ? d : 0.0, d1 ? 0.0 : d, a.nt_stores);
                store_pair(a.Lambda + i, d1 ? 0.0 : l, d1 ? l : 0.0, a.nt_stores);
            }
        }
        acc += l * (d1 ? v2 : v1) - d * (d1 ? v1 : v2);
        if constexpr (GBINS) {
            a.gflow[i] = d1 ? make_double2(0.0 - d, l) : make_double2(l, 0.0 - d);
        } else {
            const double f_in = 0.0 - d;                       // Λ − Δ of the tendered token
            if (f_in != 0.0) atomicAdd(&L.my_bins[d1 ? tok.x : tok.y], f_in);   // ds_add_f64
            if (l != 0.0) atomicAdd(&L.my_bins[d1 ? tok.y : tok.x], l);
        }
        return;
    }
    if (dir == kDirNone) {
        if (MAT) {
            if (a.compact) {
                put_record(0.0, 0.0);
            } else {
                store_pair(a.Delta + i, 0.0, 0.0, a.nt_stores);
                store_pair(a.Lambda + i, 0.0, 0.0, a.nt_stores);
            }
        }
        if constexpr (GBINS) a.gflow[i] = make_double2(0.0, 0.0);
        return;
    }
    expand_dir(dir, d, l, t);
    if (MAT) {
        if (a.compact) {   // one 16-byte record per pool (see SweepArgs)
            // a record can carry one direction whose two values have a clear sign bit (NaN payloads survive the
            // sign flip) while the other direction is exactly +0; everything else -- both directions trading and
            // the tiny negative / -0.0 values the reference's tick arithmetic produces on degenerate UniV3
            // boundaries -- takes the overflow rows, so the encoding is lossless bit for bit
            const int d1h = __double2hiint(t.d1), d2h = __double2hiint(t.d2), l1h = __double2hiint(t.l1), l2h = __double2hiint(t.l2);
            const int z1 = d2h | __double2loint(t.d2) | l1h | __double2loint(t.l1);   // 0 <=> Δ₂ and Λ₁ are +0.0
            const int z2 = d1h | __double2loint(t.d1) | l2h | __double2loint(t.l2);   // 0 <=> Δ₁ and Λ₂ are +0.0
            const bool dir1 = (z1 == 0) & ((d1h | l2h) >= 0);
            const bool dir2 = (z2 == 0) & ((d2h | l1h) >= 0);
            double ra = t.d1, rb = t.l2;
            if (!dir1) {
                if (dir2) {
                    ra = -t.d2;          // sign bit set (−0.0 included): direction 2
                    rb = t.l1;
                } else {
                    a.Lambda[i] = make_double2(t.d1, t.d2);
                    a.Over[i] = make_double2(t.l1, t.l2);
                    ra = 0.0;
                    rb = -1.0;
                }
            }
            put_record(ra, rb);
        } else {
            store_pair(a.Delta + i, t.d1, t.d2, a.nt_stores);
            store_pair(a.Lambda + i, t.l1, t.l2, a.nt_stores);
        }
    }
    // src/router.jl:82  dot(Λ, v[Ai]) - dot(Δ, v[Ai])
    acc += (t.l1 * v1 + t.l2 * v2) - (t.d1 * v1 + t.d2 * v2);
    // src/router.jl:99 / :115  G[Ai] .+= Λ .- Δ
    const double f1 = t.l1 - t.d1, f2 = t.l2 - t.d2;
    if constexpr (GBINS) {
        a.gflow[i] = make_double2(f1, f2);
    } else {
        if (f1 != 0.0) atomicAdd(&L.my_bins[tok.x], f1);   // ds_add_f64
        if (f2 != 0.0) atomicAdd(&L.my_bins[tok.y], f2);
    }
}

// The families whose lean kernels run process_pool_lean (Ops::lean_solve): the two of the fused default launch
template <class Ops> struct HasLeanSolve : std::false_type {};
template <> struct HasLeanSolve<ProductOps> : std::true_type {};
template <> struct HasLeanSolve<GeoMeanLogOps> : std::true_type {};

// One pool of a lean kernel, ProductTwoCoin or log-space GeometricMean: a straight line for the pool every tile of a real
// market is made of -- one direction or none, finite prices, amounts with a clear sign bit.
//  * Every LDS read of the tile -- the fee pair, both {v, rcp v} pairs, both log v -- is issued from the packed record at
//    once and waited for ONCE: the asm statement below names all of them, so none can be deferred into a region behind a
//    wait of its own (what pinned() did for the fee alone, with a wait in front of the price reads).
//  * lean_solve hands back {d, l}, the direction and the lane predicates trades / rare; the common epilogue is the general
//    one's `plain` branch without its decoding: the record {dir1 ? d : -d, l} (a pool that does not trade: dir1, so
//    {+0.0, +0.0}), acc += l·v_out − d·v_in under `trades`, the two LDS adds under their != 0 tests.
//  * Rare lanes -- both directions live, a NaN price, ProductTwoCoin's predicate overlap, a set sign bit in a compact
//    record's amounts -- are found by ONE wave-uniform test, and a wavefront that has one takes finish_pool, the general
//    kernel's own solve and epilogue, with ALL its lanes and from the prices already read.  All of them, not the rare ones
//    alone: a wavefront's lanes share one bin copy, two lanes' adds to the same bin round differently in a different order,
//    and the order in which the general kernel issues the adds of its common and its rare lanes is the one its compiled
//    epilogue has.  (Rare lanes alone behind the branch, the others on the straight line: Ψ of an 8-token market differed
//    from the general kernel's in the last bit.)  A wavefront without a rare lane issues its two adds in the general order.
// Same operations on the same operands in the same order as process_pool: same bits (tests/test_gpu_lean_common_path.py).
template <class Ops, bool MAT, bool FAST, class Idx>
__device__ __forceinline__ void process_pool_lean(const Ops& ops, const SweepArgs& a, const SweepLds& L,
                                                  const typename Ops::Raw& raw_in, Idx i, double& acc)
{
    typename Ops::Raw raw = raw_in;
    const unsigned packed = (unsigned)raw.ai.x;
    const int2 tok = make_int2((int)(packed & 0xffffu), (int)(packed >> 16));
    const double2 gy = L.gtab[ops.p.gbase + raw.ai.y];
    const double2 a1 = L.vy[tok.x], a2 = L.vy[tok.y];
    double g = gy.x, yg = gy.y, v1 = a1.x, y1 = a1.y, v2 = a2.x, y2 = a2.y, lv1 = 0.0, lv2 = 0.0;
    if constexpr (Ops::kNeedsLogPrices) {
        lv1 = L.lv[tok.x];
        lv2 = L.lv[tok.y];
        asm volatile("" : "+v"(g), "+v"(yg), "+v"(v1), "+v"(y1), "+v"(v2), "+v"(y2), "+v"(lv1), "+v"(lv2));
    } else {
        asm volatile("" : "+v"(g), "+v"(yg), "+v"(v1), "+v"(y1), "+v"(v2), "+v"(y2));
    }
    raw.ai = tok;
    raw.g = g;
    raw.yg = yg;
    const Px px{v1, v2, y1, y2, yg, lv2 - lv1};
    double d, l;
    bool dir1, trades, rare;
    ops.template lean_solve<FAST>(raw, px, d, l, dir1, trades, rare);
    if (MAT) rare = rare | ((__double2hiint(d) | __double2hiint(l)) < 0);   // a compact record carries two clear sign bits
    if (__builtin_expect(__any(rare ? 1 : 0) != 0, 0)) {
        finish_pool<Ops, MAT, false, FAST, true>(ops, a, L, raw, px, tok, i, acc);
        return;
    }
    if (MAT) store_pair_at(a.Delta, i, dir1 ? d : -d, l);   // {+Δ₁, Λ₂} or {−Δ₂, Λ₁}: the sign bit carries the direction
    const double worth = l * (dir1 ? v2 : v1) - d * (dir1 ? v1 : v2);
    acc = trades ? acc + worth : acc;
    const double f_in = 0.0 - d;                            // Λ − Δ of the tendered token
    if (f_in != 0.0) atomicAdd(&L.my_bins[dir1 ? tok.x : tok.y], f_in);   // ds_add_f64
    if (l != 0.0) atomicAdd(&L.my_bins[dir1 ? tok.y : tok.x], l);
}

// One pool: prices from LDS, then finish_pool.
template <class Ops, bool MAT, bool GBINS, bool FAST, bool LEAN, class Idx>
__device__ __forceinline__ void process_pool(const Ops& ops, const SweepArgs& a, const SweepLds& L,
                                             const typename Ops::Raw& raw_in, Idx i, double& acc)
{
    if constexpr (LEAN && HasLeanSolve<Ops>::value) {
        process_pool_lean<Ops, MAT, FAST>(ops, a, L, raw_in, i, acc);
        return;
    }
    typename Ops::Raw raw = raw_in;
    ops.template resolve<GBINS, FAST, LEAN>(raw, L.gtab);   // packed records: {tokens, fee-table index} -> tokens, fee
    const int2 tok = ops.tokens(raw);
    Px px;                                            // v[r.cfmms[i].Ai]
    px.yg = raw.yg;
    if constexpr (GBINS) {
        px.v1 = a.v[tok.x];
        px.v2 = a.v[tok.y];
        px.y1 = px.y2 = 0.0;
        px.dlv = Ops::kNeedsLogPrices ? log(px.v2 / px.v1) : 0.0;   // large markets: v is not staged, one logarithm per pool
    } else {
        if constexpr (FAST) {   // {v, rcp_refined(v)} pairs (FAST implies a.stage_y)
            const double2 a1 = L.vy[tok.x], a2 = L.vy[tok.y];
            px.v1 = a1.x; px.y1 = a1.y;
            px.v2 = a2.x; px.y2 = a2.y;
        } else {                // pairs, or -- markets too wide for them -- the prices alone (a.v_shift = 4 / 3)
            const char* base = reinterpret_cast<const char*>(L.vy);
            px.v1 = *reinterpret_cast<const double*>(base + ((size_t)tok.x << a.v_shift));
            px.v2 = *reinterpret_cast<const double*>(base + ((size_t)tok.y << a.v_shift));
            px.y1 = px.y2 = 0.0;
        }
        px.dlv = 0.0;
        if constexpr (Ops::kNeedsLogPrices)   // log v staged per token, or -- markets too wide for that row -- one logarithm per pool
            px.dlv = a.need_logv ? L.lv[tok.y] - L.lv[tok.x] : log(px.v2 / px.v1);
    }
    finish_pool<Ops, MAT, GBINS, FAST, LEAN>(ops, a, L, raw, px, tok, i, acc);
}

// The tile loop of one pool family over a block's share of a segment: lane tid takes pools
// i + k·step, k = 0, 1, ... left - 1.  Returns this lane's dual-scalar part.
// The first tile's pool state is requested BEFORE v and the bins are staged in LDS, so that HBM round trip is not
// exposed behind the staging barrier.  Tile order alternates between consecutive sweeps (a.reverse): block-strided
// "phases" are walked first-to-last by one sweep and last-to-first by the next, so each sweep begins on the pool data
// the previous one touched last -- the part that is still in the XCD's 4 MB L2 (a forward-only walk over a
// 5.5 MB-per-XCD working set is the LRU worst case: 0 % hits; measured on a plain read stream of the
// same 44 MB: 9.6 -> 6.9 us, profiles/r02_launch_floor.txt).
// Requesting tile k+1 before tile k is solved (Ops::kPrefetch, single-family launches): +-0.1 us cache-warm, -4..-6 %
// HBM-resident on the two-coin families at +6..8 VGPRs (round 3 measured the same and dropped it for the registers; since round 4's per-kernel
// arithmetic they are free: profiles/r04_ab_prefetch_stores.txt); +4 % on the multi-tick UniV3 walk, which keeps the plain loop.
template <class Ops, bool MAT, int BLOCK, bool GBINS, bool FAST, bool PREFETCH, bool LEAN, class Idx>
__device__ __forceinline__ void tile_loop(const Ops& ops, const SweepArgs& a, const SweepLds& L, typename Ops::Raw cur,
                                          Idx i, Idx step, Idx left, double& acc)
{
    if constexpr (PREFETCH) {
        // tile k+1's pool state is requested before tile k is solved: two tiles' loads in flight per lane
        bool ok = left > 0;
        while (ok) {
            const bool more = left > 1;
            typename Ops::Raw nxt = cur;
            if (more) nxt = ops.template load<GBINS, LEAN>((Idx)(i + step));
            process_pool<Ops, MAT, GBINS, FAST, LEAN>(ops, a, L, cur, i, acc);
            i += step;
            --left;
            ok = more;
            cur = nxt;
        }
    } else {
        bool ok = left > 0;
        while (ok) {
            process_pool<Ops, MAT, GBINS, FAST, LEAN>(ops, a, L, cur, i, acc);
            i += step;
            ok = --left > 0;
            if (ok) cur = ops.template load<GBINS, LEAN>(i);
        }
    }
}

// FASTK selects the arithmetic of the WHOLE kernel (round 4).  Rounds 1-3 compiled both tile loops into every kernel and
// chose per block; the two copies cost 12-36 VGPRs over the larger of the two alone (ProductTwoCoin 70 vs 56 / 58,
// UniV3 84 vs 63 / 63, the fused materialising launch 116 vs 80 / 97: profiles/r04_kernel_resources.txt), i.e. one to
// three wavefronts per SIMD.  Now the HOST picks the kernel wherever it can:
//   kArithFull  the compiler's full-range sequences (fast_math = 0, pool constants or prices outside the window);
//   kArithFast  the fast arithmetic: every pool constant of the launch is inside the window (Segment::fast_ok, checked at
//               upload) and so are the prices -- which the host KNOWS (host-pointer sweeps, cfmm_route).  Every block still
//               checks the prices it stages; outside the window it does NOT compute: it poisons its row (NaN in every column
//               -- an error, never a wrong number) and reports kFlagWindow (reachable only through a pre-armed launch whose
//               host-side check raced; abi_handover.cpp cancels such launches before they run);
//   kArithAuto  round 5, device-pointer sweeps (cfmm_sweep_dev): the library cannot see these prices, so the kernel carries
//               BOTH tile loops and every block chooses from the prices it staged (block-uniform, and the same choice in every
//               block: all stage the same vector) -- prices outside the window, NaN included, take the full-range loop and
//               behave like the reference's arithmetic, instead of round 4's "refuse, report on a later call" protocol
//               (ADVICE r4, medium).  Costs the registers of rounds 1-3 again, which the default geometry (4 wavefronts per
//               SIMD) never needed.
constexpr int kArithFull = 0, kArithFast = 1, kArithAuto = 2;
template <class Ops, bool MAT, int BLOCK, bool GBINS, int FASTK, bool MULTI, bool LEAN, class Idx>
__device__ __forceinline__ double sweep_tiles(const Ops& ops, const SweepArgs& a, const SweepLds& L, const typename Ops::Raw& cur,
                                              Idx i, Idx step, Idx left, bool& poison, bool& live, const PricePre& pre)
{
    static_assert(!(GBINS && FASTK != kArithFull), "large-market mode runs on the compiler's sequences");
    double acc = 0.0;
    const int staged = stage_prices<BLOCK, GBINS, !GBINS, LEAN>(a, L, pre);
    poison = (staged & kStageLive) == 0;              // a pre-armed launch that is not needed (or gave up)
    live = !poison || (staged & kStageGaveUp) != 0;   // false: CANCELLED by the host (a launch that gave up waiting still reports NaN)
    if (staged & kStageGaveUp) report(a, kFlagGaveUp);
    if (FASTK == kArithFast && !poison && (staged & kStageFast) == 0) {
        poison = true;                                // prices outside the window of this kernel's arithmetic
        report(a, kFlagWindow);
    }
    if (poison) left = 0;
    // next-tile prefetch: single-family launches of the two-coin families (HBM-resident -4..-6 %, cache-warm +-0.1 us); the
    // fused multi-family launch keeps the plain loop (same-box A/B on config3: -2 % HBM-resident but +1.5 % on the warm step;
    // again in the lean fused kernel, which has the registers for it: 11.92-12.38 us per step with it against 11.93-12.09
    // without, 8 rounds -- no gain, profiles/lean_common_path.txt)
    constexpr bool kPre = Ops::kPrefetch && !MULTI;
    if constexpr (FASTK == kArithAuto) {
        if (staged & kStageFast) tile_loop<Ops, MAT, BLOCK, GBINS, true, kPre, LEAN>(ops, a, L, cur, i, step, left, acc);
        else tile_loop<Ops, MAT, BLOCK, GBINS, false, kPre, LEAN>(ops, a, L, cur, i, step, left, acc);
    } else {
        tile_loop<Ops, MAT, BLOCK, GBINS, FASTK == kArithFast, kPre, LEAN>(ops, a, L, cur, i, step, left, acc);
    }
    return acc;
}

// Block epilogue: fold the dual scalar (lanes by wave shuffles, waves through LDS, fixed order), fold
// the bin copies in a fixed order and write the block's partial row.
// Column j of a single-block launch's result, straight to its consumer (SweepArgs::direct): a plain store for device
// consumers, or the column's two self-validating granules {tag, 32 bits} as ONE 16-byte system-scope store -- adjacent lanes
// write adjacent columns, so a wavefront's store covers full 64-byte lines on the PCIe side (see fold_finish).
typedef unsigned long long u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void publish_column(const SweepArgs& a, int j, double val)
{
    if (a.direct_host.gran) {
        u2v g = {granule(a.direct_host.tag, val, 0), granule(a.direct_host.tag, val, 1)};
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(a.direct_host.gran + 2 * (size_t)j), "v"(g) : "memory");
    } else {
        a.direct_out[j] = val;
    }
}

template <int BLOCK, bool GBINS>
__device__ __forceinline__ void finish_row(const SweepArgs& a, const SweepLds& L, double acc, int row_id, bool poison, bool publish)
{
    const double nan = __builtin_nan("");
    if (poison) acc = nan;                               // every column of a poisoned row is NaN: whoever folds it sees an error
    constexpr int kWaves = BLOCK / 64;
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) L.wsum[wave] = acc;
    __syncthreads();

    const int n_cols = GBINS ? 0 : a.n;                  // Ψ columns of the partial row
    if (!GBINS && a.direct) {
        // the only block of its launch: the row is the result.  A cancelled pre-armed launch publishes nothing (the fold of
        // such an evaluation returns without output as well: the host has moved on and may reuse the sequence tag)
        if (!publish) return;
        for (int j = tid; j < n_cols; j += BLOCK) {
            double s = L.bins[j];
            for (int c = 1; c < a.copies; ++c) s += L.bins[(size_t)c * a.n_pad + j];
            publish_column(a, j, poison ? nan : s);
        }
        if (tid == 0) {
            double s = L.wsum[0];
            for (int w = 1; w < kWaves; ++w) s += L.wsum[w];
            publish_column(a, n_cols, poison ? nan : s);
        }
        return;
    }
    double* row = a.partials + (size_t)row_id * a.row_pitch;   // 128-byte aligned rows (SweepArgs::row_pitch)
    for (int j = tid; j < n_cols; j += BLOCK) {
        double s = L.bins[j];
        for (int c = 1; c < a.copies; ++c) s += L.bins[(size_t)c * a.n_pad + j];
        store_row(row + j, poison ? nan : s);
    }
    if (tid == 0) {
        double s = L.wsum[0];
        for (int w = 1; w < kWaves; ++w) s += L.wsum[w];
        store_row(row + n_cols, poison ? nan : s);
    }
}

// The kernels' entry.  The launch's leading arguments (the descriptor, v, the direction, n: sweep.h SweepLaunch) are kernel
// parameters of their own and arrive in SGPRs (kernarg preload; a firmware that does not preload runs the compatibility
// prologue, which loads them from the kernarg segment -- the only memory of the entry that is new, cache-cold, for every
// launch).  With them a lane requests its first prices at once (request_prices), and a block its record -- and, in
// sweep_kernel, segment 0's pool streams in the same batch; sweep_multi reads its segment's behind the record -- from the
// launch's descriptor in device memory (sweep.h SweepDesc), which nothing rewrites between launches.  The descriptor is read
// through the CONSTANT address space: it does not change while a kernel runs, so every one of its fields is a scalar load
// that the compiler may place where the field is first used.
// (A table with one 128-byte line of pool streams per block, which took sweep_multi's second dependent read away, was built
// and measured: the step was 0.1 us SLOWER with it on the benchmark's fused market, in two sessions -- a block's own line is a
// cold miss per block where the segment records are lines its neighbours have just fetched.  profiles/sweep_entry_preload.txt.)
#define CFMM_CONST_AS __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const CFMM_CONST_AS T* const_as(const T* p)
{
    return (const CFMM_CONST_AS T*)(reinterpret_cast<uintptr_t>(p));
}
// The preloaded arguments of a launch, as the kernels pass them on
struct LaunchHead {
    const SweepDesc* desc;
    const double* v;
    int reverse;
    int n;
};
// The tail of the arguments, read where it lies: in the kernarg segment, through the constant address space.  (A by-value
// kernel parameter is copied out of the segment at the kernel's FIRST instruction, and the words only the epilogue needs
// -- arm_*, direct_* -- then sit in SGPRs, or spilled to VGPR lanes, in front of the first pool load.)
// The same goes for v and n once the first prices are requested: what is used after that (v: prices beyond the requested
// ones, pre-armed and large-market launches; n: staging and the row) is read again -- v from the segment, n from the
// descriptor -- so the preloaded copies do not stay in SGPRs across the tile loop.
// The kernels' parameter list (desc, v, reverse, n, SweepTail) IS a SweepLaunch field by field: the kernarg segment
// lays parameters out by size and alignment as a struct lays out its members, and the launchers pass the fields' addresses.
static_assert(offsetof(SweepLaunch, desc) == 0 && offsetof(SweepLaunch, v) == 8 && offsetof(SweepLaunch, reverse) == 16 &&
                  offsetof(SweepLaunch, n) == 20 && offsetof(SweepLaunch, tail) == 24 && alignof(SweepTail) == 8,
              "sweep_kernel / sweep_multi (pointer, pointer, int, int, SweepTail) read the segment as a SweepLaunch");
typedef const CFMM_CONST_AS SweepLaunch& LaunchRef;
__device__ __forceinline__ LaunchRef launch_args()
{
    return *(const CFMM_CONST_AS SweepLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
}
__device__ __forceinline__ BlockRec block_rec(const SweepDesc* desc)
{
    const CFMM_CONST_AS BlockRec* recs =
        (const CFMM_CONST_AS BlockRec*)(reinterpret_cast<uintptr_t>(desc) + kSweepDescHead);
    const CFMM_CONST_AS BlockRec& r = recs[blockIdx.x];
    return BlockRec{r.first, r.stride, r.full, r.tail, r.row, r.seg, r.kind};
}
// The SweepArgs of this block: the launch's own fields, the descriptor's, its segment's
__device__ __forceinline__ SweepArgs block_args(const LaunchHead& h, LaunchRef la, const CFMM_CONST_AS SweepDesc& d,
                                                const CFMM_CONST_AS SegRec& sg)
{
    const CFMM_CONST_AS SweepTail& t = la.tail;
    SweepArgs a;
    a.v = la.v;
    a.n = d.n;
    a.n_pad = d.n_pad;
    a.v_shift = d.v_shift;
    a.need_logv = d.need_logv;
    a.gtab = d.gtab;
    a.gtab_n = d.gtab_n;
    a.copies = d.copies;
    a.flags = d.flags;
    a.m = sg.m;
    a.Delta = sg.Delta;
    a.Lambda = sg.Lambda;
    a.Over = sg.Over;
    a.compact = d.compact;
    a.partials = d.partials;
    a.row_pitch = d.row_pitch;
    a.gflow = sg.gflow;
    a.reverse = h.reverse;
    a.arm_word = t.arm_word;
    a.arm_seq = t.arm_seq;
    a.arm_timeout = t.arm_timeout;
    a.nt_stores = d.nt_stores;
    a.direct = d.direct;
    a.direct_out = t.direct_out;
    a.direct_host = HostOut{t.direct_host.gran, t.direct_host.tag};
    return a;
}
// a family's view of a segment record's pools
__device__ __forceinline__ ProductPools pools_of(const CFMM_CONST_AS AnyPools& u, const ProductPools*)
{
    return ProductPools{u.p.R, u.p.gamma, u.p.Ai, u.p.pk, u.p.gbase};
}
__device__ __forceinline__ GeoMeanPools pools_of(const CFMM_CONST_AS AnyPools& u, const GeoMeanPools*)
{
    return GeoMeanPools{u.g.R, u.g.w, u.g.gamma, u.g.Ai, u.g.eta, u.g.Q, u.g.reference_order, u.g.pk, u.g.gbase};
}
__device__ __forceinline__ UniV3Pools pools_of(const CFMM_CONST_AS AnyPools& u, const UniV3Pools*)
{
    return UniV3Pools{u.u.pg, u.u.Ai, u.u.cur_a, u.u.cur_b, u.u.cur_c, u.u.curR, u.u.walk, u.u.ticks, u.u.thr, u.u.head,
                      u.u.has_walk, u.u.cp, u.u.pk, u.u.gbase};
}
// One block's share of ONE segment (its BlockRec); its partial row goes to partials[br.row].
// The order is the point: the first tile's pool state is requested from the block record, the segment's pool streams and
// the launch's direction ALONE -- lane t takes pools first + t + k·stride, k < full + (t < tail): the host did the division
// -- and only then is everything else read (block_args: the LDS geometry, the trade and row buffers, the fee table), while
// those loads are in flight.
// LEAN: the same body for the one configuration every default launch has (launch_plan.h lean_launch, checked on the host:
// compact write-through trade records, prices staged as pairs, a fee table, one bin copy per wavefront, not direct, every
// pool stream shorter than 2 GiB).  What the general kernel asks per pool of every tile is a constant here, the pool index is
// 32 bits wide (stream_at, store_pair_at), and in a fused launch only the blocks of a family that reads log v stage it (the
// LDS layout is the launch's: carve_lds comes first).  Same grid, same tiles per lane in the same order, same operations
// on the same operands: every output bit is the general kernel's.
template <class Ops, bool MAT, int BLOCK, bool GBINS, int FASTK, bool MULTI, bool LEAN>
__device__ __forceinline__ void sweep_body(const LaunchHead& h, const CFMM_CONST_AS SweepDesc& d, const CFMM_CONST_AS SegRec& sg,
                                           const BlockRec& br, const PricePre& pre)
{
    static_assert(!(LEAN && (GBINS || FASTK == kArithFull)), "the lean kernels: LDS bins, prices staged as pairs");
    using Idx = typename std::conditional<LEAN, uint32_t, int64_t>::type;   // (LEAN: steps and indices wrap modulo 2^32, counts < 2^31)
    const Ops ops{pools_of(sg.pools, (const decltype(Ops::p)*)nullptr)};
    const int64_t stride = br.stride;
    const int64_t i0 = br.first + threadIdx.x;
    const int64_t left = br.full + ((int)threadIdx.x < br.tail ? 1 : 0);      // tiles of this lane
    const bool reverse = h.reverse != 0;
    const int64_t step = reverse ? -stride : stride;
    const int64_t i = reverse ? i0 + (left - 1) * stride : i0;
    typename Ops::Raw cur = {};
    if (left > 0) cur = ops.template load<GBINS, LEAN>((Idx)i);
    SweepArgs a = block_args(h, launch_args(), d, sg);
    if constexpr (LEAN) {
        a.compact = 1;
        a.nt_stores = 0;
        a.v_shift = 4;
        a.copies = BLOCK / 64;
        a.direct = 0;
    }
    const SweepLds L = carve_lds<BLOCK, GBINS>(a);
    if constexpr (LEAN) a.need_logv = Ops::kNeedsLogPrices ? 1 : 0;   // (a launch with such a family has the row: lean_launch)
    bool poison, live;
    const double acc = sweep_tiles<Ops, MAT, BLOCK, GBINS, FASTK, MULTI, LEAN>(ops, a, L, cur, (Idx)i, (Idx)step, (Idx)left, poison, live, pre);
    finish_row<BLOCK, GBINS>(a, L, acc, br.row, poison, live);
}

// One segment's own launch: segment 0 of the descriptor, whose pool streams are requested together with the block's record
template <class Ops, bool MAT, int BLOCK, bool GBINS, int FASTK, bool LEAN = false>
__global__ __launch_bounds__(BLOCK) void sweep_kernel(const SweepDesc* desc, const double* v, int reverse, int n, SweepTail)
{
    const LaunchHead h{desc, v, reverse, n};
    PricePre pre = {};
    if constexpr (!GBINS) pre = request_prices<BLOCK>(v, n);
    const BlockRec br = block_rec(desc);
    const CFMM_CONST_AS SweepDesc& d = *const_as(desc);
    sweep_body<Ops, MAT, BLOCK, GBINS, FASTK, false, LEAN>(h, d, d.seg[0], br, pre);
}

// Several segments (pool families) in ONE launch, so HBM-bound ProductTwoCoin blocks and ALU-bound GeometricMean /
// UniV3 blocks are co-resident on every CU and overlap, and the sweep pays one launch + one kernel boundary instead of nseg.
// The block -> segment map is the descriptor's block table.  With a grid that is a multiple of 256 blocks it is XCD-aware
// and cost-weighted (launch_plan.cpp plan_xcd_map, build_sweep_desc): blocks are dealt round-robin to the 8 XCDs (block b
// runs on XCD b % 8), so "segment = b % nseg" would put ALL blocks of one pool family on the same XCDs (nseg = 2:
// ProductTwoCoin on XCDs 0,2,4,6, GeometricMean on 1,3,5,7 -- half the chip does all the arithmetic).  There the 8 blocks
// of one deal (one per XCD) share a segment, consecutive deals walk through a 32-entry pattern in which segment s appears
// seg_w[s] times (its share of the launch's work: pools x cost per pool, so that all blocks finish together), and the
// pattern is rotated by one every 32 deals (one pass over an XCD's 32 CUs), so every XCD -- and, as the dispatcher fills
// CUs in order, every CU -- hosts all families.  Placement is only a performance assumption: any placement computes the
// same result.  Small grids: block b -> segment b % nseg.
template <bool MAT, int BLOCK, bool GBINS, int FASTK, bool LEAN = false>
__global__ __launch_bounds__(BLOCK) void sweep_multi(const SweepDesc* desc, const double* v, int reverse, int n, SweepTail)
{
    const LaunchHead h{desc, v, reverse, n};
    PricePre pre = {};
    if constexpr (!GBINS) pre = request_prices<BLOCK>(v, n);
    const BlockRec br = block_rec(desc);
    const CFMM_CONST_AS SweepDesc& d = *const_as(desc);
    const CFMM_CONST_AS SegRec& sg = d.seg[br.seg];
    switch (br.kind) {
    case 0: sweep_body<ProductOps, MAT, BLOCK, GBINS, FASTK, true, LEAN>(h, d, sg, br, pre); break;
    case 1: // log-space forms only; geomean_exact routers are swept by per-segment launches
        sweep_body<GeoMeanLogOps, MAT, BLOCK, GBINS, FASTK, true, LEAN>(h, d, sg, br, pre);
        break;
    default: sweep_body<UniV3Ops, MAT, BLOCK, GBINS, FASTK, true, LEAN>(h, d, sg, br, pre); break;
    }
}
#undef CFMM_CONST_AS

} // namespace cfmm
