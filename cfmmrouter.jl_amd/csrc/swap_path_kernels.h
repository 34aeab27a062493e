// swap_path_kernels.h -- cfmm_swap_path / cfmm_swap_path_out: swap paths that MOVE their pools, all or nothing, ONE LANE PER
// PATH of one wave, grid-stride over the wave.  The paths of a wave share no pool and a path names a pool at most once (the
// host has checked both: swap_path_waves.h, swap_path_checks.h), so no two lanes touch one pool and the hops of one path do
// not see each other's moves: the lane can quote the whole path first and apply it afterwards.  Plain vector loads and
// stores, no LDS, no atomics.
//   Pass 1 walks the hops as the quote_path kernels do -- hop_try: read_hop's rule, the kind's quote through path_hop, so the
//          amounts carry cfmm_quote_path's / cfmm_quote_path_out's bits -- and per hop tests the state the swap would leave
//          with swap_move (swap_pool.h), i.e. the refusal conditions of cfmm_swap; UniV3: the landing price
//          (swap_univ3_price), which goes to the price scratch as it is found.  It writes the hop amounts and stops at the
//          first hop that refuses (NaN from that hop on) or, exact output, cannot give that much (+inf from that hop on).
//   Pass 2 runs only for a path that no hop refuses and whose result clears its limit: hop by hop (apply_hop) it reads the
//          amounts back and stores the state swap_move computes again (untested: swap_move<KIND, false>), with swap_store.  A hop that moves nothing (amount 0)
//          leaves every bit of its pool.  UniV3 pools are moved by the host from the landing prices.
// Both loops stay rolled and carry one amount: no per-hop state is kept in registers, pass 2 reads the hop's 20 bytes and the
// pool again.  Lanes whose hops land in different kinds serialise, as in quote_path_kernel.
// The two kernels keep a pass 1 loop each: they differ in direction, in which slots they fill behind a stop and in their
// status codes, and share everything per hop (hop_try).
#pragma once

#include "quote_path_kernels.h"
#include "swap_pool.h"

namespace cfmm {

// Pass 1 of one hop: r = the quote of `given` (OUT false: entering the hop, r leaves it; OUT true: wanted from the hop, r
// is to be tendered) and whether the hop is in range and the state it would be left in is one a pool can take.  A hop that
// moves nothing has nothing to refuse; neither has one that cannot give that much (r == +inf, exact output only).
template <bool OUT>
__device__ __forceinline__ bool hop_try(const SwapPathArgs& a, int64_t at, double given, double& r)
{
    const auto h = read_hop(a, at, given);
    const PathSeg& s = h.seg.s;
    const bool moves = h.amt != 0.0;
    bool ok = h.ok, valid = true;
    with_kind(h.kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        r = path_hop<KIND, OUT>(s, h.m, h.row, h.ci, h.co, h.amt);
        const double in = OUT ? r : h.amt, out = OUT ? h.amt : r;
        if constexpr (KIND == CFMM_KIND_UNIV3) {
            if (!OUT || r != __builtin_inf()) {
                const double2 pg = s.pg[h.row];
                const double P = swap_univ3_price(pg.x, s.cur_a[h.row], s.cur_b[h.row], s.cur_c[h.row], s.walk[h.row], s.ticks, pg.y, h.ci, in);
                a.price[at] = P;
                valid = swap_finite_pos(P);
            }
        } else {
            if (moves && (!OUT || r != __builtin_inf())) valid = swap_move<KIND>(swap_view(h.seg), h.m, h.row, h.ci, h.co, in, out).valid;
        }
    }, [&] { r = 0.0; ok = false; });   // (a segment without pools)
    return ok && valid;
}

// Pass 2 of one hop that takes `in` and gives `out` != 0: every hop passed pass 1's range tests on these very words, so
// nothing is clamped again
__device__ __forceinline__ void apply_hop(const SwapPathArgs& a, int64_t at, double in, double out)
{
    const SwapPathSeg& t = a.segs[a.hop_seg[at]];
    const long long row = a.hop_row[at];
    const int ci = a.hop_coin_in[at], co = a.hop_coin_out[at];
    const int64_t m = t.s.m;
    with_kind(t.s.kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        if constexpr (KIND != CFMM_KIND_UNIV3) {   // (UniV3: the host moves the pool from a.price)
            const SwapView v = swap_view(t);
            swap_store<KIND>(v, m, row, ci, co, swap_move<KIND, false>(v, m, row, ci, co, in, out));   // (tested in pass 1)
        }
    }, [] {});
}

// exact input: x_{k+1} = quote(hop k, x_k); a.hops[k] = the amount LEAVING hop k; statuses kPath*.
// (The block size is a template argument for quote_path_kernel's reason: the kernel is emitted behind every kernel the
// translation unit had before.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void swap_path_kernel(SwapPathArgs a)
{
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.count; p += step) {
        int nh = a.n_hops[p];
        const double given = a.amount_in[p];
        double x = given;
        int status = kPathApplied;
        if (nh < 1 || nh > a.max_hops) {   // (the host has refused such a call; nothing is evaluated)
            nh = 0;
            x = nan;
            status = kPathRefused;
        }
        int k = 0;
        for (; k < nh && status == kPathApplied; ++k) {
            const int64_t at = (int64_t)k * a.stride + p;
            double r;
            if (hop_try<false>(a, at, x, r)) {
                x = r;
            } else {
                x = nan;
                status = kPathRefused;
            }
            a.hops[at] = x;
        }
        for (; k < a.max_hops; ++k) a.hops[(int64_t)k * a.stride + p] = nan;   // behind a refusing hop, and the unused slots
        if (status == kPathApplied && a.min_out && !(x >= a.min_out[p])) status = kPathBelowLimit;
        a.amount_out[p] = x;
        a.status[p] = status;
        if (status != kPathApplied) continue;
        double amt = given;
        for (k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * a.stride + p;
            const double out = a.hops[at];
            if (amt != 0.0) apply_hop(a, at, amt, out);
            amt = out;
        }
    }
}

// exact OUTPUT, on the same arguments with the roles of the amounts exchanged (sweep.h): a.amount_in is the amount wanted
// from the last hop, a.min_out the limit on the input, a.amount_out the input to tender to hop 0, a.hops[k] the amount TO
// TENDER to hop k; statuses kSwap*.  Both passes run from the last hop to the first, y_H = the wanted amount,
// y_k = quote_out(hop k, y_{k+1}), so that one amount is carried.  A hop that answers +inf makes that hop, every earlier hop
// and the answer +inf (kSwapUnobtainable, cfmm_quote_path_out's rule); a refusing hop writes NaN from itself towards hop 0
// (kSwapRefused).  A hop with y_{k+1} == 0 has y_k == +0.0 and moves nothing.  Last, !(y_0 <= limit) is kSwapOverLimit.  Each
// pool ends exactly where swap_out_kernel of (that hop, y_{k+1}) leaves it: R_in + γ·y_k, R_out − y_{k+1}.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void swap_path_out_kernel(SwapPathArgs a)
{
    const double nan = __builtin_nan("");
    const int64_t step = (int64_t)gridDim.x * BLOCK;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.count; p += step) {
        int nh = a.n_hops[p];
        const double want = a.amount_in[p];
        double y = want;
        int status = kSwapApplied;
        if (nh < 1 || nh > a.max_hops) {   // (the host has refused such a call; nothing is evaluated)
            nh = 0;
            y = nan;
            status = kSwapRefused;
        }
        for (int k = nh; k < a.max_hops; ++k) a.hops[(int64_t)k * a.stride + p] = nan;   // the unused slots
        int k = nh - 1;
        for (; k >= 0 && status == kSwapApplied; --k) {
            const int64_t at = (int64_t)k * a.stride + p;
            double r;
            if (!hop_try<true>(a, at, y, r)) {
                y = nan;
                status = kSwapRefused;
            } else {
                y = r;
                if (r == __builtin_inf()) status = kSwapUnobtainable;
            }
            a.hops[at] = y;
        }
        for (; k >= 0; --k) a.hops[(int64_t)k * a.stride + p] = y;   // towards hop 0 of a hop that refused (NaN) or cannot give (+inf)
        if (status == kSwapApplied && a.min_out && !(y <= a.min_out[p])) status = kSwapOverLimit;
        a.amount_out[p] = y;
        a.status[p] = status;
        if (status != kSwapApplied) continue;
        double out = want;
        for (k = nh - 1; k >= 0; --k) {
            const int64_t at = (int64_t)k * a.stride + p;
            const double in = a.hops[at];
            if (out != 0.0) apply_hop(a, at, in, out);
            out = in;
        }
    }
}

} // namespace cfmm
