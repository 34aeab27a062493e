// ops_univ3.h -- UniV3 / BoundedProduct: lane per pool, the tick walk over the lists univ3_pool.h prepares at upload.
#pragma once

#include "ops_two_coin.h"

namespace cfmm {

// ---------------------------------------------------------------------------------------------
// UniV3 / BoundedProduct -- src/cfmms.jl:294-395 (lane per pool, serial tick walk)
// ---------------------------------------------------------------------------------------------
// Everything compute_at_tick (:294-313) derives is independent of v, so it is evaluated ONCE at
// upload (abi_upload.cpp, same IEEE operations, hence the same bits) into the constants
// find_arb_pos (:321-337) actually uses:
//   * the CURRENT tick, visited first by both walks, as one record per pool
//       cur_a = {k, sA = R₁+α}   cur_b = {sB = R₂+β, δmax↑ = k/β − sA}   cur_c = δmax↓ = k/α − sB
//     (the flipped pool of :289 swaps sA/sB), plus curR = {R₁, R₂}, read only when the tick drains;
//   * the ticks beyond it as per-direction walk lists of the NON-EMPTY ticks only, one 64-byte record per tick
//       ks = {k, s_in}   dt = {δmax, s_out}   rout = R_out   psum = sums of the drained ticks before it
//     ("in"/"out" already flipped), and the ticks' drain thresholds as a contiguous array (solve_dir).
// A sweep then costs one division and one or two square roots for the current tick and for the one tick the walk ends
// in, whatever the number of ticks in between, empty ticks cost nothing, and a pool that trades inside its
// current tick (the common case; every BoundedProduct pool) touches only coalesced per-pool
// streams.  `initial` (:352,:374) can only be true on the current tick, and only if it is non-empty.
// HEADS: the walk consults the per-pool threshold heads (UniV3Pools::head) -- segments with walk lists.  The lean
// instantiation (BoundedProduct segments: no list anywhere, config 5) carries neither the loads nor the registers
// (same-box A/B: 21.2 vs 21.5 us HBM-resident on config5 with the head code compiled in).
template <bool HEADS>
struct UniV3OpsT {
    static constexpr bool kNeedsLogPrices = false;
    static constexpr bool kPrefetch = false;     // (measured +4 % on the multi-tick walk, +-0 on BoundedProduct segments)
    struct Raw {
        double2 pg, ca, cb;   // pg = {current_price, γ}
        double cc;
        int2 ai;              // packed: {tok, gidx} until resolve()
        int4 walk;
        uint4 hu, hd;         // threshold heads of the two walk lists (UniV3Pools::head; zeros without one)
        int64_t i;
        double yg;
    };
    UniV3Pools p;
    template <bool GBINS, bool LEAN = false, class I>
    __device__ __forceinline__ Raw load(I i) const
    {
        Raw r;
        r.ca = stream_at<LEAN>(p.cur_a, i);
        r.cb = stream_at<LEAN>(p.cur_b, i);
        r.cc = stream_at<LEAN>(p.cur_c, i);
        r.walk = p.has_walk ? stream_at<LEAN>(p.walk, i) : make_int4(0, 0, 0, 0);
        r.hu = r.hd = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (HEADS) {
            if (p.head) {                                 // (kernel argument: uniform) 32 contiguous bytes per lane
                r.hu = stream_at<LEAN>(p.head, 2 * i);
                r.hd = stream_at<LEAN>(p.head, 2 * i + 1);
            }
        }
        r.i = i;
        r.yg = 0.0;
        if constexpr (GBINS) {
            r.pg = p.pg[i];
            r.ai = p.Ai[i];
        } else {   // packed record: price alone + {tokens, fee-table index} (+ the fee itself without a table)
            r.ai = load_packed<LEAN>(p.pk, i);
            r.pg = make_double2(stream_at<LEAN>(p.cp, i), LEAN ? 0.0 : load_packed_fee(p.gbase, &p.pg[i].y));
        }
        return r;
    }
    template <bool GBINS, bool FAST, bool LEAN = false>
    __device__ __forceinline__ void resolve(Raw& r, const double2* gtab_lds) const
    {
        if constexpr (!GBINS) resolve_packed<FAST, LEAN>(p.gbase, gtab_lds, r.ai, r.pg.y, r.yg);
    }
    __device__ __forceinline__ int2 tokens(const Raw& r) const { return r.ai; }

    // find_arb_pos (:321-337) on one prepared walk-list entry; yp = rcp_refined(price) (FAST)
    template <bool FAST>
    __device__ __forceinline__ void list_tick(const TickRec& rec, double price, double yp, double& d, double& l) const
    {
        const double2 ks = rec.ks, dt = rec.dt;                    // one 64-byte line per visited tick, requested at once
        const double rout = rec.rout;
        const double dd = (FAST ? fast_sqrt(div_by(ks.x, price, yp)) : sqrt(ks.x / price)) - ks.y;   // :323
        d = 0.0;
        l = 0.0;                                                   // :325-327
        if (dd > 0) {
            if (dd >= dt.x) {                                      // :330-332
                d = dt.x;
                l = rout;
            } else {
                l = dt.y - (FAST ? fast_sqrt(price * ks.x) : sqrt(price * ks.x));   // :334
                d = dd;
            }
        }
    }

    // The part of find_arb! before the walk lists (:340-361 / :381 and the current tick): block-uniformly FAST or not.
    // Returns false when the pool does not trade (or the price is NaN: t is then all-NaN).  cur: what the current tick
    // did -- kCurEmpty (no liquidity: contributes nothing, the walk goes on, :355-358), kCurPartial ({sd, sl} set: the
    // walk ends in this tick), kCurDrained (contributes {δmax, R_out}: not loaded here, see solve_dir).
    static constexpr int kCurEmpty = 0, kCurPartial = 1, kCurDrained = 2;
    template <bool FAST>
    __device__ __forceinline__ bool head(const Raw& r, const Px& px, Trade& t, bool& up, double& g, double& yg, double& price,
                                         double& yp, double& sd, double& sl, int& cur, bool& inside) const
    {
        inside = false;
        const double cp = r.pg.x;
        g = r.pg.y;
        yg = r.yg;
        const double pr = FAST ? div_by(px.v1, px.v2, px.y2) : px.v1 / px.v2;   // :340
        t.d1 = t.d2 = t.l1 = t.l2 = 0.0;
        sd = sl = 0.0;
        up = false;
        price = 1.0;
        yp = 1.0;
        cur = kCurEmpty;
        if (pr != pr) { t.d1 = t.d2 = t.l1 = t.l2 = pr; return false; }   // NaN prices propagate instead of "no trade"
        if (g * cp <= pr && pr <= (FAST ? div_by(cp, g, yg) : cp / g)) return false;   // :347-349
        up = pr < g * cp;                                                  // :351
        if constexpr (FAST) price = up ? div_by(pr, g, yg) : fast_div(1.0, g * pr);
        else price = up ? pr / g : 1.0 / (g * pr);                         // :361 / :381
        if constexpr (FAST) yp = rcp_refined(price);
        // current tick: `initial` is true here unless the tick is empty (:355-358), so no break test
        const double k0 = r.ca.x;
        if (k0 != 0) {
            const double s_in = up ? r.ca.y : r.cb.x, s_out = up ? r.cb.x : r.ca.y;
            const double dmax = up ? r.cb.y : r.cc;
            const double dd = (FAST ? fast_sqrt(div_by(k0, price, yp)) : sqrt(k0 / price)) - s_in;   // :323
            cur = kCurPartial;
            if (dd > 0) {                                                  // :325-327
                if (dd >= dmax) {                                          // :330-332
                    cur = kCurDrained;
                } else {
                    sl = s_out - (FAST ? fast_sqrt(price * k0) : sqrt(price * k0));   // :334
                    sd = dd;
                    // the target price lies INSIDE this tick by more than a relative 2^-29: sqrt(k/price) is below its
                    // value at the tick's far boundary, s_in + δmax, by more than 2^-30 of it -- no later tick can be
                    // entered (its s_in is the square root at a boundary price beyond this one's; rounding is monotone)
                    if (p.has_walk) inside = dd < dmax - 0x1p-30 * (s_in + dmax);   // (BoundedProduct segments have no lists: nothing to skip)
                }
            }
        }
        return true;
    }

    // The walk (:353-365 / :375-385).  The reference visits tick after tick; every tick it DRAINS contributes the
    // v-independent pair {δmax, R_out}, and whether it drains one is a monotone test on the price: sqrt(k/price) − s_in
    // > 0 and >= δmax holds for every price up to a threshold T and for none above it (division, square root and
    // subtraction are correctly rounded, hence monotone).  So the upload stores, per walk list in walk order,
    //   * the thresholds T_j CONTIGUOUSLY (p.thr: 8 ticks per 64-byte line; found by bisection on the reference's own
    //     floating-point test, so `price <= T_j` IS that test), a 0 closing every list, and
    //   * in tick j's record the sums {Σδ, Σλ} of everything BEFORE it -- current tick and ticks 0..j−1 all drained --
    //     accumulated in the walk's order with the walk's operations (same bits as walking), plus a closing record
    //     per list that carries the sums of the whole list.
    // A pool whose current tick drains (or is empty) then costs one scan of its thresholds and ONE record, however deep
    // it walks, instead of one scattered 64-byte line per visited tick; from the first tick that is not drained the
    // reference's tick-by-tick evaluation takes over (one partially filled tick, normally), and it goes on to the
    // following tick only inside a 2^-40 band around that tick's threshold -- outside it the next tick cannot be
    // entered: its s_in is sqrt(k/p⁺) with p⁺ <= this tick's far boundary < price, and rounding is monotone.  A pool
    // that ends inside its current tick (kCurPartial) reads no list at all (round 4; `inside` in head()) unless its
    // target price is within 2^-29 of the tick's far boundary, where the plain walk decides (it stops at the first list tick).
    template <bool FAST>
    __device__ __forceinline__ int solve_dir(const Raw& r, const Px& px, double& d, double& l, Trade& t) const
    {
        bool up, inside;
        int cur;
        double g, yg, price, yp, sd, sl;
        d = l = 0.0;
        if (!head<FAST>(r, px, t, up, g, yg, price, yp, sd, sl, cur, inside)) return t.d1 != t.d1 ? kDirBoth : kDirNone;   // (NaN price: t is all-NaN)
        const int begin = up ? r.walk.x : r.walk.z;
        // a pool that ends well inside its current tick (the common case) touches no list at all; the reference's next
        // find_arb_pos would return zeros and break (:363-365).  Within 2^-29 of the far boundary the plain walk decides.
        const int count = inside ? 0 : (up ? r.walk.y : r.walk.w);
        int j = 0;
        const bool jump = cur != kCurPartial && count > 0;
        TickRec rec;
        double thr_j = 0.0;                                                // T[j] of the tick the scan stopped at (TickRec::thr)
        bool have = false;
        if (jump) {
            // ticks 0..j−1 drain.  Round 5: the first four list ticks are decided from the pool's threshold head -- binary32
            // values rounded DOWN at upload, so with lo = the float and hi = the next float up (lo <= T <= hi):
            // price <= lo PROVES the tick drains, price > hi PROVES it does not; a price in between (a relative 2^-23 band
            // around a threshold), a threshold outside the float range (NaN pattern) or a walk deeper than four ticks falls
            // back to the exact array below.  Same decisions as the exact scan, without touching thr[] for ~4 of 5 walkers.
            bool exact = true;                                             // the exact scan (still) has to run, from tick j
            // T[j] of the tick the scan stops at, for the band test below -- from the scan's own registers, NOT from the record
            // (measured: taking it from rec.thr makes the walk wait for the record earlier, 44.4 -> 49.2 us with the heads off).
            // The head path knows only hi >= T[j]: good enough, the test "price > T[j](1 + 2^-40)" is then merely conservative
            // (a price inside (T[j], hi](1 + 2^-40) visits one more tick, which returns zeros and ends the walk the same way).
            double thr_t = 0.0;
            if (HEADS && p.head) {
                const uint4 h = up ? r.hu : r.hd;
                const unsigned hb[4] = {h.x, h.y, h.z, h.w};
                int adv = 0;
                bool stop = false, amb = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double lo = (double)__uint_as_float(hb[k]), hi = (double)__uint_as_float(hb[k] + 1u);
                    const bool go = !stop && !amb;
                    const bool drains = price <= lo, not_drains = hb[k] == 0u || price > hi;   // (0 = never; NaN: neither)
                    adv += (go && drains) ? 1 : 0;
                    thr_t = (go && !drains && not_drains) ? (hb[k] == 0u ? 0.0 : hi) : thr_t;
                    stop = stop || (go && !drains && not_drains);
                    amb = amb || (go && !drains && !not_drains);
                }
                if (!amb) {
                    j = adv;
                    exact = !stop && j < count;        // all four drain and the list goes on: the exact scan continues at tick 4
                }
            }
            if (exact) {
                // Four thresholds per round trip (the dependent chain of a walking pool is
                // walk span -> thresholds -> one record); every list ends in a 0 and the array is padded, so reading past
                // a short list is harmless and the first failing test ends the scan exactly like one-by-one.
                const double* T = p.thr + begin;
                for (;;) {
                    const double t0 = T[j], t1 = T[j + 1], t2 = T[j + 2], t3 = T[j + 3];
                    const int adv = !(price <= t0) ? 0 : !(price <= t1) ? 1 : !(price <= t2) ? 2 : !(price <= t3) ? 3 : 4;
                    thr_t = adv == 0 ? t0 : adv == 1 ? t1 : adv == 2 ? t2 : t3;
                    j += adv;
                    if (adv < 4 || j >= count) break;
                }
            }
            // (prices <= 0 from a caller's device vector pass every test, the closing 0 included: the closing record, whose
            //  threshold is 0 whichever path found it -- ADVICE r5)
            thr_t = j < count ? thr_t : 0.0;
            j = j < count ? j : count;
            rec = p.ticks[begin + j];                                      // (j == count: the list's closing record)
            thr_j = thr_t;                                                 // T[j] (or the float just above it) of the tick the scan stopped at
            have = true;
            sd = rec.psum.x;
            sl = rec.psum.y;
        } else if (cur == kCurDrained) {
            const double2 R = p.curR[r.i];                                 // no list in this direction: the current tick alone
            sd = up ? r.cb.y : r.cc;
            sl = up ? R.y : R.x;
        }
        for (; j < count; ++j) {                                           // :353 / :375, empty ticks elided
            double dj, lj;
            if (!have) {
                rec = p.ticks[begin + j];
                thr_j = rec.thr;
            }
            have = false;
            list_tick<FAST>(rec, price, yp, dj, lj);
            if (dj == 0 || lj == 0) break;                                 // :363-365 (initial is false here)
            sd += dj;
            sl += lj;
            if (jump && price > thr_j * (1.0 + 0x1p-40)) break;            // the next tick cannot be entered (see above)
            // (a safety net, never seen to trigger: on every fixture and parity row, targets 0..3 ulps beside a boundary included,
            //  the reference itself enters no tick after a partial one, so a band of 0 gives the same bits --
            //  tests/test_cp_precise_cpu.py::test_no_tick_is_entered_after_a_partial_one; the band is NOT covered by a failing mutant)
        }
        d = FAST ? div_by_signed_zero(sd, g, yg) : sd / g;                 // :366-372 / :386-391
        l = sl;
        return up ? kDir1 : kDir2;
    }
};

using UniV3Ops = UniV3OpsT<true>;
using UniV3OpsLean = UniV3OpsT<false>;

} // namespace cfmm
