// univ3_pool.h -- internal, host only: one UniV3 pool's find_arb_pos constants (sweep.h UniV3Pools), prepared with the IEEE
// operations the reference applies per sweep (src/cfmms.jl:226-245, :294-337).  The upload (abi_upload.cpp univ3_build) and
// the sparse price update (abi_update.cpp cfmm_pools_set_prices) both prepare a pool HERE, so a pool moved to a price and a
// pool uploaded at that price carry the same bits.  No HIP call, no context: tests/native/univ3_prepare_host.cpp builds it
// for the CPU.
#pragma once

#include "sweep.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

namespace cfmm {

inline bool finite_pos(double x) { return std::isfinite(x) && x > 0.0; }

// |x| in [2^-kFastExp, 2^kFastExp]: the operand window of the sweep's fast division / square root (sweep.h)
inline bool in_fast_window(double x)
{
    uint64_t bits;
    std::memcpy(&bits, &x, sizeof bits);
    const int e = (int)((bits >> 52) & 0x7ff);
    return e >= 1023 - kFastExp && e <= 1023 + kFastExp;
}

// Largest price P for which find_arb_pos (src/cfmms.jl:321-337) DRAINS a tick with the prepared constants k, s_in = R_in + α,
// δmax: dd = sqrt(k/P) − s_in is > 0 and >= δmax.  The test is monotone in P (IEEE division, square root and subtraction are
// correctly rounded, hence monotone), so there is exactly one such double; it is found on the test ITSELF -- gallop from the
// algebraic boundary k/(s_in + δmax)², then bisect on the bit patterns -- so that `price <= T` on the device is the
// reference's floating-point decision, not an approximation of it.  0: the tick never drains for a positive price.
inline double drain_threshold(double k, double s_in, double dmax)
{
    auto drains = [&](double P) {
        const double dd = std::sqrt(k / P) - s_in;
        return dd > 0 && dd >= dmax;
    };
    auto bits = [](double x) { int64_t b; std::memcpy(&b, &x, sizeof b); return b; };
    auto from = [](int64_t b) { double x; std::memcpy(&x, &b, sizeof x); return x; };
    const int64_t lo_lim = bits(0x1p-1000), hi_lim = bits(0x1p1000);
    double c0 = k / ((s_in + dmax) * (s_in + dmax));
    if (!(c0 > 0x1p-1000)) c0 = 0x1p-1000;     // (also catches NaN)
    if (!(c0 < 0x1p1000)) c0 = 0x1p1000;
    int64_t lo, hi;                            // drains(lo), !drains(hi)
    const int64_t cb = bits(c0);
    if (drains(c0)) {
        lo = cb;
        for (int64_t step = 1;; step *= 2) {
            const int64_t nb = lo + step;
            if (nb >= hi_lim) {
                if (drains(from(hi_lim))) return from(hi_lim);
                hi = hi_lim;
                break;
            }
            if (!drains(from(nb))) { hi = nb; break; }
            lo = nb;
        }
    } else {
        hi = cb;
        for (int64_t step = 1;; step *= 2) {
            const int64_t nb = hi - step;
            if (nb <= lo_lim) {
                if (!drains(from(lo_lim))) return 0.0;
                lo = lo_lim;
                break;
            }
            if (drains(from(nb))) { lo = nb; break; }
            hi = nb;
        }
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (drains(from(mid))) lo = mid;
        else hi = mid;
    }
    return from(lo);
}

// src/cfmms.jl:235: searchsortedlast(lower_ticks, current_price, rev=true), 1-based; 0: the price lies above the first tick
inline int64_t univ3_current_tick(const double* lt, int64_t nt, double cp)
{
    int64_t lo = 0, hi = nt + 1;
    while (lo < hi - 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (lt[mid - 1] < cp) hi = mid;
        else lo = mid;
    }
    return lo;
}

// The per-pool columns of UniV3Pools; `walk` holds the pool's list offsets in the record array the lists were appended to
struct UniV3PoolRec {
    double2 pg, cur_a, cur_b, curR;
    double cur_c;
    int4 walk;
};

// One pool at current tick ct (univ3_current_tick, >= 1) of its nt ticks lt / lq: the current tick's constants and both walk
// lists, APPENDED to `ticks` (closing records included).  Thresholds are not set yet (univ3_all_thresholds): until then
// TickRec::thr is 0, and 1 on a closing record.
inline void univ3_prepare_pool(double cp, double gamma, int64_t ct, int64_t nt, const double* lt, const double* lq,
                               UniV3PoolRec& out, std::vector<TickRec>& ticks)
{
    // compute_at_tick(cfmm, idx), src/cfmms.jl:294-313 (idx 1-based)
    auto at_tick = [&](int64_t idx, double& k, double& al, double& be, double& R1, double& R2) {
        k = lq[idx - 1];
        const double pplus = lt[idx - 1];                 // :251
        const double pminus = idx < nt ? lt[idx] : 0.0;   // :254-259
        al = std::sqrt(k / pplus);
        be = std::sqrt(k * pminus);
        const double p = idx > ct ? pplus : (idx < ct ? pminus : cp);
        R1 = std::sqrt(k / p) - al;
        R2 = std::sqrt(k * p) - be;
    };
    {   // the current tick, shared by both walks
        double k, al, be, R1, R2;
        at_tick(ct, k, al, be, R1, R2);
        const double sA = R1 + al, sB = R2 + be;
        out.cur_a = make_double2(k, sA);
        out.cur_b = make_double2(sB, k / be - sA);   // :329
        out.cur_c = k / al - sB;                     // :329 on the flipped pool (:289)
        out.curR = make_double2(R1, R2);
        if (k == 0) { out.cur_b.y = 0.0; out.cur_c = 0.0; } // 0/0: never read (k == 0 is skipped)
    }
    // Walk lists (UniV3Ops::solve_dir): the non-empty ticks beyond the current one, in walk order; every record also
    // carries the sums of the drained ticks BEFORE it, starting from what the current tick contributes when it drains
    // ({δmax, R_out}; nothing if it is empty) and accumulated with the walk's own additions; one closing record per
    // list carries the sums of the whole list.
    double kc, alc, bec, R1c, R2c;
    at_tick(ct, kc, alc, bec, R1c, R2c);
    int4 w;
    w.x = (int)ticks.size();
    int cnt = 0;
    double2 run = kc != 0 ? make_double2(out.cur_b.y, R2c) : make_double2(0.0, 0.0);   // price falling: δmax↑, R₂ out
    for (int64_t idx = ct + 1; idx <= nt; ++idx) {        // get_upper_pools beyond the current tick, :316
        double k, al, be, R1, R2;
        at_tick(idx, k, al, be, R1, R2);
        if (k == 0) continue;                             // is_empty_pool, :288
        const double s_in = R1 + al, dmax = k / be - s_in;
        ticks.push_back(TickRec{make_double2(k, s_in), make_double2(dmax, R2 + be), R2, 0.0, run});   // :329, :334
        run.x += dmax;
        run.y += R2;
        ++cnt;
    }
    ticks.push_back(TickRec{make_double2(0.0, 0.0), make_double2(0.0, 0.0), 0.0, 1.0, run});           // closing record (pad = 1 marks it)
    w.y = cnt;
    w.z = (int)ticks.size();
    cnt = 0;
    run = kc != 0 ? make_double2(out.cur_c, R1c) : make_double2(0.0, 0.0);                             // price rising (flipped pool, :289)
    for (int64_t idx = ct - 1; idx >= 1; --idx) {         // flip_sides.(get_lower_pools), :317,:289
        double k, al, be, R1, R2;
        at_tick(idx, k, al, be, R1, R2);
        if (k == 0) continue;
        const double s_in = R2 + be, dmax = k / al - s_in;
        ticks.push_back(TickRec{make_double2(k, s_in), make_double2(dmax, R1 + al), R1, 0.0, run});
        run.x += dmax;
        run.y += R1;
        ++cnt;
    }
    ticks.push_back(TickRec{make_double2(0.0, 0.0), make_double2(0.0, 0.0), 0.0, 1.0, run});
    w.w = cnt;
    out.walk = w;
    out.pg = make_double2(cp, gamma);
}

// Drain thresholds of all records (the closing records and ticks that end the walk when reached -- δmax = 0 or R_out = 0,
// :363-365 -- get 0 = "never"), a few bisection steps each: spread over the host's cores.  thr[e] for record e, and every
// record carries its own threshold too (closing records: 0; until here TickRec::thr == 1 marks them).
inline void univ3_all_thresholds(std::vector<TickRec>& ticks, std::vector<double>& thr)
{
    thr.assign(ticks.size(), 0.0);
    const size_t nrec = ticks.size();
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const unsigned nthr = nrec > 65536 ? hw : 1;
    auto work = [&](size_t lo, size_t hi) {
        for (size_t e = lo; e < hi; ++e) {
            const TickRec& r = ticks[e];
            if (r.thr != 0.0 || r.dt.x == 0.0 || r.rout == 0.0) continue;
            thr[e] = drain_threshold(r.ks.x, r.ks.y, r.dt.x);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(work, nrec * t / nthr, nrec * (t + 1) / nthr);
    work(0, nrec / nthr);
    for (auto& th : pool) th.join();
    for (size_t e = 0; e < nrec; ++e) ticks[e].thr = thr[e];
}

// Threshold heads (sweep.h UniV3Pools::head) of one pool: the first four thresholds of both lists as floats rounded DOWN;
// thr is indexed by the offsets in w
inline void univ3_heads(const int4& w, const double* thr, uint4* out)
{
    const auto enc = [](double T) -> unsigned {
        if (T == 0.0) return 0u;                                   // never drains (also: closing record, past the list)
        if (!(T >= 0x1p-120 && T <= 0x1p120)) return 0x7fc00000u;   // outside the comfortable binary32 range: NaN = "ask thr[]"
        float f = (float)T;
        if ((double)f > T) f = std::nextafterf(f, 0.0f);           // round toward zero = down (T > 0)
        unsigned b;
        std::memcpy(&b, &f, sizeof b);
        return b;
    };
    unsigned h[8];
    for (int k = 0; k < 4; ++k) {
        h[k] = k < w.y ? enc(thr[(size_t)w.x + k]) : 0u;           // beyond the list: the closing record's "never"
        h[4 + k] = k < w.w ? enc(thr[(size_t)w.z + k]) : 0u;
    }
    out[0] = make_uint4(h[0], h[1], h[2], h[3]);
    out[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

} // namespace cfmm
