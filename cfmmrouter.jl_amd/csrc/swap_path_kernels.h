// swap_path_kernels.h -- cfmm_swap_path: exact-input swap paths that MOVE their pools, all or nothing, ONE LANE PER PATH of
// one wave, grid-stride over the wave.  The paths of a wave share no pool and a path names a pool at most once (the host
// has checked both: swap_path_waves.h, swap_path_checks.h), so no two lanes touch one pool and the hops of one path do not
// see each other's moves: the lane can quote the whole path first and apply it afterwards.  Plain vector loads and stores,
// no LDS, no atomics.
//   Pass 1 walks the hops as quote_path_kernel does -- the same clamp-then-poison rule, the same quote_one<KIND> picked by
//          the segment's kind (path_hop, quote_path_kernels.h), so the amounts carry cfmm_quote_path's bits -- and per hop
//          tests the state the swap would leave with swap_pool.h's tests, i.e. cfmm_swap's refusal conditions; UniV3: the
//          landing price (swap_univ3_price), which goes to the price scratch as it is found.  It writes the hop amounts
//          and stops at the first refusing hop: NaN from that hop on, status kPathRefused.
//   Pass 2 runs only for a path that no hop refuses and whose result clears its limit (status kPathApplied): hop by hop
//          it reads the amounts back and writes the new reserves and refreshed constants with swap_kernel's own
//          expressions (swap_pool.h).  A hop entered with amount 0 leaves every bit of its pool.  UniV3 pools are moved by
//          the host from the landing prices.
// Both loops stay rolled and carry one amount: no per-hop state is kept in registers, pass 2 reads the hop's 20 bytes and the
// pool again.  Lanes whose hops land in different kinds serialise, as in quote_path_kernel.
#pragma once

#include "quote_path_kernels.h"
#include "swap_pool.h"

namespace cfmm {

// The state hop (row, ci, co) of a reserve-kind segment is left in by a swap of amt > 0 for out.  APPLY false: whether
// cfmm_pools_set_* accepts it (swap_kernel's tests); APPLY true: store it (swap_kernel's stores) -- the caller has seen the
// test pass on the same values.
template <int KIND, bool APPLY>
__device__ __forceinline__ bool swap_path_state(const SwapPathSeg& t, int64_t m, int64_t row, int ci, int co, double amt, double out)
{
    if constexpr (KIND == CFMM_KIND_PRODUCT || KIND == CFMM_KIND_SOLIDLY || KIND == CFMM_KIND_GEOMEAN) {
        const double2 R = t.s.R[row];
        const double g = t.s.gamma[row];
        const double2 rn = swap_reserves(ci == 0 ? R.x : R.y, co == 0 ? R.x : R.y, g, amt, out);
        if constexpr (!APPLY) {
            return swap_reserves_valid(rn, KIND == CFMM_KIND_SOLIDLY);
        } else {
            const double2 Rn = ci == 0 ? rn : make_double2(rn.y, rn.x);
            t.R[row] = Rn;
            if (t.left_window && !(swap_in_window(Rn.x) && swap_in_window(Rn.y))) *t.left_window = 1;
            if constexpr (KIND == CFMM_KIND_GEOMEAN) t.Q[row] = swap_geomean_q(g, t.eta[row], Rn.x, Rn.y);
            return true;
        }
    } else {
        static_assert(KIND == CFMM_KIND_WEIGHTED || KIND == CFMM_KIND_CURVE, "UniV3 has no state the kernel writes");
        const int64_t ji = (int64_t)ci * m + row, jo = (int64_t)co * m + row;
        const double2 rn = swap_reserves(t.s.nR[ji], t.s.nR[jo], t.s.nglg[row].x, amt, out);
        bool valid = swap_reserves_valid(rn, false);
        double qi, qo;
        if constexpr (KIND == CFMM_KIND_WEIGHTED) {
            qi = swap_weighted_q(rn.x, t.s.npar[ji]);
            qo = swap_weighted_q(rn.y, t.s.npar[jo]);
        } else {
            qi = swap_curve_q(rn.x);
            qo = swap_curve_q(rn.y);
            if constexpr (!APPLY) {
                const double2 ab = reinterpret_cast<const double2*>(t.s.npar)[row];   // {α, log β}
                if (valid && ab.x > 0.0) valid = swap_curve_in_range(ab.y, t.s.nq + row, m, t.s.n_coins, ci, qi, co, qo);
            }
        }
        if constexpr (APPLY) {
            t.nR[ji] = rn.x;
            t.nR[jo] = rn.y;
            t.nq[ji] = qi;
            t.nq[jo] = qo;
        }
        return valid;
    }
}

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
        // ---- pass 1: the amounts, and whether every hop's new state is one a pool can take
        int k = 0;
        for (; k < nh && status == kPathApplied; ++k) {
            const int64_t at = (int64_t)k * a.stride + p;
            int seg = a.hop_seg[at];
            long long row = a.hop_row[at];
            int ci = a.hop_coin_in[at];
            int co = a.hop_coin_out[at];
            bool ok = seg >= 0 && seg < a.nseg;
            seg = seg < 0 ? 0 : (seg >= a.nseg ? a.nseg - 1 : seg);
            const SwapPathSeg& t = a.segs[seg];
            const int kind = t.s.kind;
            const int nc = t.s.n_coins;
            const int64_t m = t.s.m;
            ok = ok && row >= 0 && row < m && ci >= 0 && ci < nc && co >= 0 && co < nc && ci != co && x >= 0.0 && x < __builtin_inf();
            row = row < 0 ? 0 : (row >= m ? m - 1 : row);
            ci = ci < 0 ? 0 : (ci >= nc ? nc - 1 : ci);
            co = co < 0 ? 0 : (co >= nc ? nc - 1 : co);
            const double amt = ok ? x : 0.0;
            const bool moves = amt != 0.0;   // (amt == 0: nothing moves, nothing to refuse)
            double r;
            bool valid = true;
            switch (kind) {
            case CFMM_KIND_PRODUCT:
                r = path_hop<CFMM_KIND_PRODUCT, false>(t.s, m, row, ci, co, amt);
                if (moves) valid = swap_path_state<CFMM_KIND_PRODUCT, false>(t, m, row, ci, co, amt, r);
                break;
            case CFMM_KIND_GEOMEAN:
                r = path_hop<CFMM_KIND_GEOMEAN, false>(t.s, m, row, ci, co, amt);
                if (moves) valid = swap_path_state<CFMM_KIND_GEOMEAN, false>(t, m, row, ci, co, amt, r);
                break;
            case CFMM_KIND_UNIV3: {
                r = path_hop<CFMM_KIND_UNIV3, false>(t.s, m, row, ci, co, amt);
                const double2 pg = t.s.pg[row];
                const double P = swap_univ3_price(pg.x, t.s.cur_a[row], t.s.cur_b[row], t.s.cur_c[row], t.s.walk[row], t.s.ticks, pg.y, ci, amt);
                a.price[at] = P;
                valid = swap_finite_pos(P);
                break;
            }
            case CFMM_KIND_WEIGHTED:
                r = path_hop<CFMM_KIND_WEIGHTED, false>(t.s, m, row, ci, co, amt);
                if (moves) valid = swap_path_state<CFMM_KIND_WEIGHTED, false>(t, m, row, ci, co, amt, r);
                break;
            case CFMM_KIND_CURVE:
                r = path_hop<CFMM_KIND_CURVE, false>(t.s, m, row, ci, co, amt);
                if (moves) valid = swap_path_state<CFMM_KIND_CURVE, false>(t, m, row, ci, co, amt, r);
                break;
            case CFMM_KIND_SOLIDLY:
                r = path_hop<CFMM_KIND_SOLIDLY, false>(t.s, m, row, ci, co, amt);
                if (moves) valid = swap_path_state<CFMM_KIND_SOLIDLY, false>(t, m, row, ci, co, amt, r);
                break;
            default: r = 0.0; ok = false; break;   // (a segment without pools)
            }
            if (ok && valid) {
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
        // ---- pass 2: every hop passed pass 1's range tests on these very words, so nothing is clamped again
        double amt = given;
        for (k = 0; k < nh; ++k) {
            const int64_t at = (int64_t)k * a.stride + p;
            const SwapPathSeg& t = a.segs[a.hop_seg[at]];
            const long long row = a.hop_row[at];
            const int ci = a.hop_coin_in[at], co = a.hop_coin_out[at];
            const int64_t m = t.s.m;
            const double out = a.hops[at];
            if (amt != 0.0) {
                switch (t.s.kind) {
                case CFMM_KIND_PRODUCT: swap_path_state<CFMM_KIND_PRODUCT, true>(t, m, row, ci, co, amt, out); break;
                case CFMM_KIND_GEOMEAN: swap_path_state<CFMM_KIND_GEOMEAN, true>(t, m, row, ci, co, amt, out); break;
                case CFMM_KIND_WEIGHTED: swap_path_state<CFMM_KIND_WEIGHTED, true>(t, m, row, ci, co, amt, out); break;
                case CFMM_KIND_CURVE: swap_path_state<CFMM_KIND_CURVE, true>(t, m, row, ci, co, amt, out); break;
                case CFMM_KIND_SOLIDLY: swap_path_state<CFMM_KIND_SOLIDLY, true>(t, m, row, ci, co, amt, out); break;
                default: break;   // UniV3: the host moves the pool from a.price
                }
            }
            amt = out;
        }
    }
}

// cfmm_swap_path_out: exact-OUTPUT paths, all or nothing.  The same two rolled passes with pass 1 reversed, on the same
// arguments with the roles of the amounts exchanged (sweep.h): a.amount_in is the amount wanted from the last hop,
// a.min_out the limit on the input, a.amount_out the input to tender to hop 0, a.hops[k] the amount TO TENDER to hop k.
//   Pass 1 walks from the last hop to the first as quote_path_out_kernel does: y_H = the wanted amount,
//          y_k = quote_out_one<KIND>(hop k, y_{k+1}) (path_hop<KIND, true>), so the amounts carry cfmm_quote_path_out's bits.
//          A hop that answers +inf makes that hop, every earlier hop and the answer +inf (kSwapUnobtainable, cfmm_quote_path_out's
//          rule).  Otherwise the state R_in + γ·y_k, R_out − y_{k+1} is tested with swap_pool.h's tests -- swap_path_state's
//          arguments are (amount entering, amount leaving) -- and on UniV3 the landing price swap_univ3_price(.., y_k), which
//          goes to the price scratch; a refusing hop writes NaN from itself towards hop 0 (kSwapRefused).  A hop with
//          y_{k+1} == 0 has y_k == +0.0 and moves nothing.  Last, !(y_0 <= limit) is kSwapOverLimit.
//   Pass 2 runs for kSwapApplied only, again from the last hop to the first so that one amount is carried: hop k takes
//          hops[k] in and gives the amount carried, with swap_path_state<KIND, true>'s stores -- each pool ends exactly where
//          swap_out_kernel of (that hop, y_{k+1}) leaves it.  UniV3 pools are moved by the host from the landing prices.
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
        // ---- pass 1, last hop first: the amounts, and whether every hop's new state is one a pool can take
        int k = nh - 1;
        for (; k >= 0 && status == kSwapApplied; --k) {
            const int64_t at = (int64_t)k * a.stride + p;
            int seg = a.hop_seg[at];
            long long row = a.hop_row[at];
            int ci = a.hop_coin_in[at];
            int co = a.hop_coin_out[at];
            bool ok = seg >= 0 && seg < a.nseg;
            seg = seg < 0 ? 0 : (seg >= a.nseg ? a.nseg - 1 : seg);
            const SwapPathSeg& t = a.segs[seg];
            const int kind = t.s.kind;
            const int nc = t.s.n_coins;
            const int64_t m = t.s.m;
            ok = ok && row >= 0 && row < m && ci >= 0 && ci < nc && co >= 0 && co < nc && ci != co && y >= 0.0 && y < __builtin_inf();
            row = row < 0 ? 0 : (row >= m ? m - 1 : row);
            ci = ci < 0 ? 0 : (ci >= nc ? nc - 1 : ci);
            co = co < 0 ? 0 : (co >= nc ? nc - 1 : co);
            const double out = ok ? y : 0.0;
            const bool moves = out != 0.0;   // (out == 0: the hop takes +0.0, nothing moves, nothing to refuse)
            const double inf = __builtin_inf();
            double r;
            bool valid = true;
            switch (kind) {
            case CFMM_KIND_PRODUCT:
                r = path_hop<CFMM_KIND_PRODUCT, true>(t.s, m, row, ci, co, out);
                if (moves && r != inf) valid = swap_path_state<CFMM_KIND_PRODUCT, false>(t, m, row, ci, co, r, out);
                break;
            case CFMM_KIND_GEOMEAN:
                r = path_hop<CFMM_KIND_GEOMEAN, true>(t.s, m, row, ci, co, out);
                if (moves && r != inf) valid = swap_path_state<CFMM_KIND_GEOMEAN, false>(t, m, row, ci, co, r, out);
                break;
            case CFMM_KIND_UNIV3: {
                r = path_hop<CFMM_KIND_UNIV3, true>(t.s, m, row, ci, co, out);
                if (r != inf) {
                    const double2 pg = t.s.pg[row];
                    const double P = swap_univ3_price(pg.x, t.s.cur_a[row], t.s.cur_b[row], t.s.cur_c[row], t.s.walk[row], t.s.ticks, pg.y, ci, r);
                    a.price[at] = P;
                    valid = swap_finite_pos(P);
                }
                break;
            }
            case CFMM_KIND_WEIGHTED:
                r = path_hop<CFMM_KIND_WEIGHTED, true>(t.s, m, row, ci, co, out);
                if (moves && r != inf) valid = swap_path_state<CFMM_KIND_WEIGHTED, false>(t, m, row, ci, co, r, out);
                break;
            case CFMM_KIND_CURVE:
                r = path_hop<CFMM_KIND_CURVE, true>(t.s, m, row, ci, co, out);
                if (moves && r != inf) valid = swap_path_state<CFMM_KIND_CURVE, false>(t, m, row, ci, co, r, out);
                break;
            case CFMM_KIND_SOLIDLY:
                r = path_hop<CFMM_KIND_SOLIDLY, true>(t.s, m, row, ci, co, out);
                if (moves && r != inf) valid = swap_path_state<CFMM_KIND_SOLIDLY, false>(t, m, row, ci, co, r, out);
                break;
            default: r = 0.0; ok = false; break;   // (a segment without pools)
            }
            if (!(ok && valid)) {
                y = nan;
                status = kSwapRefused;
            } else {
                y = r;
                if (r == inf) status = kSwapUnobtainable;
            }
            a.hops[at] = y;
        }
        for (; k >= 0; --k) a.hops[(int64_t)k * a.stride + p] = y;   // towards hop 0 of a hop that refused (NaN) or cannot give (+inf)
        if (status == kSwapApplied && a.min_out && !(y <= a.min_out[p])) status = kSwapOverLimit;
        a.amount_out[p] = y;
        a.status[p] = status;
        if (status != kSwapApplied) continue;
        // ---- pass 2: every hop passed pass 1's range tests on these very words, so nothing is clamped again
        double out = want;
        for (k = nh - 1; k >= 0; --k) {
            const int64_t at = (int64_t)k * a.stride + p;
            const SwapPathSeg& t = a.segs[a.hop_seg[at]];
            const long long row = a.hop_row[at];
            const int ci = a.hop_coin_in[at], co = a.hop_coin_out[at];
            const int64_t m = t.s.m;
            const double in = a.hops[at];
            if (out != 0.0) {
                switch (t.s.kind) {
                case CFMM_KIND_PRODUCT: swap_path_state<CFMM_KIND_PRODUCT, true>(t, m, row, ci, co, in, out); break;
                case CFMM_KIND_GEOMEAN: swap_path_state<CFMM_KIND_GEOMEAN, true>(t, m, row, ci, co, in, out); break;
                case CFMM_KIND_WEIGHTED: swap_path_state<CFMM_KIND_WEIGHTED, true>(t, m, row, ci, co, in, out); break;
                case CFMM_KIND_CURVE: swap_path_state<CFMM_KIND_CURVE, true>(t, m, row, ci, co, in, out); break;
                case CFMM_KIND_SOLIDLY: swap_path_state<CFMM_KIND_SOLIDLY, true>(t, m, row, ci, co, in, out); break;
                default: break;   // UniV3: the host moves the pool from a.price
                }
            }
            out = in;
        }
    }
}

} // namespace cfmm
