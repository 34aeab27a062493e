// ops_two_coin.h -- the two-coin closed forms of the sweep: what process_pool (sweep_core.h) asks of a pool family (Raw,
// load, resolve, tokens, solve_dir; lean_solve for the families of process_pool_lean), the packed {tokens, fee index}
// record's two helpers, and the Ops structs of ProductTwoCoin, GeometricMeanTwoCoin (reference order and log space) and
// the Solidly-style stable pair.
#pragma once

#include "fast_arith.h"

#include <type_traits>

namespace cfmm {

struct Trade {
    double d1, d2, l1, l2;
};

// Prices of a pool's two tokens as the sweep hands them to solve(): the values, their refined reciprocals (FAST only;
// staged per token in LDS), the fee's refined reciprocal (FAST only: from the LDS fee table, or computed per pool) and
// log v2 − log v1 (log-space GeometricMean only).
struct Px {
    double v1, v2, y1, y2, yg, dlv;
};

// What Ops::solve_dir returns: a two-coin pool trades in at most one direction (the reference's four outputs are
// (Δ₁, 0), (0, Λ₂) or (0, Δ₂), (Λ₁, 0)), so the common case travels as {d, l} + a direction and the epilogue of a pool
// (trade record, dual scalar, netflow bins) works on two values instead of four.  kDirBoth: all four values in a Trade
// (γ > 1 pools trading both ways, the overlap of ProductTwoCoin's predicates, NaN prices).
constexpr int kDirNone = 0, kDir1 = 1, kDir2 = 2, kDirBoth = 3;
__device__ __forceinline__ void expand_dir(int dir, double d, double l, Trade& t)
{
    if (dir == kDirBoth) return;
    t.d1 = dir == kDir1 ? d : 0.0;
    t.d2 = dir == kDir2 ? d : 0.0;
    t.l1 = dir == kDir2 ? l : 0.0;
    t.l2 = dir == kDir1 ? l : 0.0;
}

// Element i of a pool stream.  LEAN (the lean kernels, sweep_core.h; i is then 32 bits wide and the host has checked that
// every stream of the launch is shorter than 2 GiB): the stream's base -- a launch constant, in SGPRs -- plus a 32-bit
// per-lane BYTE offset, the `global_load v, v_off, s[base]` form: the index of the next tile is one 32-bit add and one
// shift per record width instead of a 64-bit vector add per stream.
// The record is loaded as ONE register value of its width (8 or 16 bytes) and copied into T from there: copied as a struct
// from the computed address, the compiler turned the tile loop's `cur = nxt` into a choice between two ADDRESSES and loaded
// the record's fields where they are used -- in the next tile, behind its solve, with the first tile parked in scratch.
typedef unsigned int stream_u2 __attribute__((ext_vector_type(2), may_alias));
typedef unsigned int stream_u4 __attribute__((ext_vector_type(4), may_alias));
template <bool LEAN, class T, class I>
__device__ __forceinline__ T stream_at(const T* base, I i)
{
    if constexpr (LEAN) {
        static_assert(sizeof(T) == 8 || sizeof(T) == 16, "pool streams are 8- or 16-byte records");
        using Bits = typename std::conditional<sizeof(T) == 8, stream_u2, stream_u4>::type;
        const Bits bits = *reinterpret_cast<const Bits*>(reinterpret_cast<const char*>(base) + (size_t)((uint32_t)i * (uint32_t)sizeof(T)));
        T out;
        __builtin_memcpy(&out, &bits, sizeof(T));
        return out;
    } else {
        return base[i];
    }
}

// ---------------------------------------------------------------------------------------------
// The packed {tokens, fee index} record (sweep.h PackedFeeTok) of ProductTwoCoin, GeometricMeanTwoCoin and UniV3 segments
// ---------------------------------------------------------------------------------------------
// Every Ops::load() only ISSUES loads (no arithmetic on what it loaded): the compiler then keeps all of a tile's loads
// in flight together.  (Round 2 unpacked the {tokens, fee index} record inside load(); the compiler answered with
// s_waitcnt vmcnt(0) BEFORE it issued the reserve load -- two dependent memory round trips per tile.)  The record is
// taken apart in resolve(), after the tile's data has arrived.
// Outside GBINS (n_tokens > 8192: the plain gamma / Ai arrays) a load() ALWAYS reads the packed record --
// one load, no choice between two pointers for the compiler to merge and sink to the use (round 3: with a
// `pk ? pk[i] : Ai[i]` in here the record's load ended up at the TOP of the next tile, its latency exposed again) --
// plus the fee itself (*fee: the pool's entry of the gamma array) when the launch has no fee table (gbase < 0: too many
// fee tiers); with a table the fee is 0.0 until resolve_packed() reads it.  Two calls, so that a family can keep the
// order in which it issues its loads (UniV3 requests its price between the two: any other order changes its schedule).
template <bool LEAN = false, class I>
__device__ __forceinline__ int2 load_packed(const PackedFeeTok* pk, I i)
{
    const PackedFeeTok k = stream_at<LEAN>(pk, i);
    return make_int2((int)k.tok, (int)k.gidx);
}
__device__ __forceinline__ double load_packed_fee(int gbase, const double* fee) { return gbase < 0 ? *fee : 0.0; }
// after stage_prices(): take the packed record apart; the fee from the LDS table {γ, rcp_refined(γ)}, or -- no table --
// its reciprocal refined here (FAST only)
// LEAN: the launch has a fee table (launch_plan.h lean_launch), so there is nothing to decide
template <bool FAST, bool LEAN = false>
__device__ __forceinline__ void resolve_packed(int gbase, const double2* gtab_lds, int2& ai, double& g, double& yg)
{
    const unsigned tok = (unsigned)ai.x;
    if (LEAN || gbase >= 0) {
        const double2 gy = gtab_lds[gbase + ai.y];
        g = gy.x;
        yg = pinned(gy.y);
    } else if constexpr (FAST) {
        yg = rcp_refined(g);
    }
    ai = make_int2((int)(tok & 0xffffu), (int)(tok >> 16));
}

// ---------------------------------------------------------------------------------------------
// ProductTwoCoin -- src/cfmms.jl:125-140
// ---------------------------------------------------------------------------------------------
struct ProductOps {
    static constexpr bool kNeedsLogPrices = false;
    static constexpr bool kPrefetch = true;      // tile_loop: request the next tile's pool state before solving this one
    struct Raw {
        double2 R;
        double g;
        int2 ai;      // packed: {tok, gidx} until resolve()
        double yg;    // refined reciprocal of the fee (FAST with a fee table)
    };
    ProductPools p;
    // GBINS (n_tokens > 8192): the plain gamma / Ai arrays; otherwise the packed record (load_packed)
    template <bool GBINS, bool LEAN = false, class I>
    __device__ __forceinline__ Raw load(I i) const
    {
        Raw r;
        r.R = stream_at<LEAN>(p.R, i);
        r.yg = 0.0;
        if constexpr (GBINS) {
            r.g = p.gamma[i];
            r.ai = p.Ai[i];
        } else {
            r.ai = load_packed<LEAN>(p.pk, i);
            r.g = LEAN ? 0.0 : load_packed_fee(p.gbase, p.gamma + i);
        }
        return r;
    }
    template <bool GBINS, bool FAST, bool LEAN = false>
    __device__ __forceinline__ void resolve(Raw& r, const double2* gtab_lds) const
    {
        if constexpr (!GBINS) resolve_packed<FAST, LEAN>(p.gbase, gtab_lds, r.ai, r.g, r.yg);
    }
    __device__ __forceinline__ int2 tokens(const Raw& r) const { return r.ai; }
    // All four closed forms exactly as written in the reference (:134-138).
    __device__ __forceinline__ void solve_full(double R1, double R2, double g, double v1, double v2, Trade& t) const
    {
        const double k = R1 * R2;          // :132
        const double m12 = v2 / v1;        // m of :134/:138
        const double m21 = v1 / v2;        // m of :135/:137
        const double gm12 = g * m12;       // γ*m (== m*γ bitwise)
        const double gm21 = g * m21;
        t.d1 = max0(sqrt(gm12 * k) - R1) / g;   // :125,:134
        t.d2 = max0(sqrt(gm21 * k) - R2) / g;   // :125,:135
        t.l1 = max0(R1 - sqrt(k / gm21));       // :126,:137
        t.l2 = max0(R2 - sqrt(k / gm12));       // :126,:138
    }

    // At most one direction trades (Δ₁,Λ₂ > 0 ⇔ γ·v₂R₂ > v₁R₁;  Δ₂,Λ₁ > 0 ⇔ γ·v₁R₁ > v₂R₂), so only
    // that direction's two closed forms are evaluated -- with the reference's own expressions on
    // the selected operands, hence bit-identical values.  The predicates carry a 1e-12 relative
    // margin (>> the 1e-16 rounding of the forms), so a direction is only skipped where the
    // reference's max(·, 0) provably clamps to 0; the (measure-zero) overlap runs the full forms.
    // Returns the direction of the trade: kDirNone, kDir1 (Δ₁ = d, Λ₂ = l), kDir2 (Δ₂ = d, Λ₁ = l) or kDirBoth
    // (the four values in t: the overlap of the two predicates, or NaN inputs).
    template <bool FAST>
    __device__ __forceinline__ int solve_dir(const Raw& r, const Px& px, double& d, double& l, Trade& t) const
    {
        const double R1 = r.R.x, R2 = r.R.y, g = r.g, v1 = px.v1, v2 = px.v2;
        constexpr double kMargin = 1.0 + 1e-12;
        const double a = v1 * R1, b = v2 * R2;
        const bool p1 = (g * b) * kMargin >= a;    // direction 1 possibly active
        const bool p2 = (g * a) * kMargin >= b;    // direction 2 possibly active
        d = l = 0.0;
        if (p1 != p2) {
            const double k = R1 * R2;                          // :132
            const double r_in = p1 ? R1 : R2, r_out = p1 ? R2 : R1;
            if constexpr (FAST) {
                // m = v_out / v_in through the divisor's staged reciprocal; operands inside the window: same bits
                const double gm = g * div_by(p1 ? v2 : v1, p1 ? v1 : v2, p1 ? px.y1 : px.y2);
                d = div_by(__builtin_fmax(fast_sqrt(gm * k) - r_in, 0.0), g, px.yg);   // :125 (finite: max0 == fmax)
                l = __builtin_fmax(r_out - fast_sqrt(fast_div(k, gm)), 0.0);           // :126
            } else {
                const double gm = g * ((p1 ? v2 : v1) / (p1 ? v1 : v2));   // γ*m, m = v_out / v_in
                d = max0(sqrt(gm * k) - r_in) / g;             // :125
                l = max0(r_out - sqrt(k / gm));                // :126
            }
            return p1 ? kDir1 : kDir2;
        }
        if (p1 || a != a || b != b) {
            // both directions within the margin (γ ≈ 1 at the no-arbitrage price), or a NaN among the inputs
            // (both predicates are false on NaN): the reference's four forms, which propagate it
            solve_full(R1, R2, g, v1, v2, t);
            return kDirBoth;
        }
        return kDirNone;
    }
    // The lean kernels' solve (sweep_core.h process_pool_lean): the same predicates and the same forms on the same operands,
    // returned as what the epilogue of a pool uses instead of a code it has to decode -- the two amounts (+0.0 for a pool that
    // does not trade), the direction and two lane predicates.  rare: the overlap of the two predicates or a NaN among the
    // inputs; a wavefront with such a lane goes through solve_dir and the general epilogue, whatever d and l say here.
    // dir1 is true for a pool that does not trade, so that its record is {+0.0, +0.0} and never {-(+0.0), +0.0}.
    template <bool FAST>
    __device__ __forceinline__ void lean_solve(const Raw& r, const Px& px, double& d, double& l, bool& dir1, bool& trades, bool& rare) const
    {
        const double R1 = r.R.x, R2 = r.R.y, g = r.g, v1 = px.v1, v2 = px.v2;
        constexpr double kMargin = 1.0 + 1e-12;
        const double a = v1 * R1, b = v2 * R2;
        const bool p1 = (g * b) * kMargin >= a;
        const bool p2 = (g * a) * kMargin >= b;
        trades = p1 != p2;
        dir1 = !p2;
        rare = (p1 == p2) & (p1 | (a != a) | (b != b));
        d = l = 0.0;
        if (trades) {
            const double k = R1 * R2;                          // :132
            const double r_in = p1 ? R1 : R2, r_out = p1 ? R2 : R1;
            const double v_in = p1 ? v1 : v2, v_out = p1 ? v2 : v1;
            if constexpr (FAST) {
                const double gm = g * div_by(v_out, v_in, p1 ? px.y1 : px.y2);
                d = div_by(__builtin_fmax(fast_sqrt(gm * k) - r_in, 0.0), g, px.yg);   // :125
                l = __builtin_fmax(r_out - fast_sqrt(fast_div(k, gm)), 0.0);           // :126
            } else {
                const double gm = g * (v_out / v_in);          // γ*m, m = v_out / v_in
                d = max0(sqrt(gm * k) - r_in) / g;             // :125
                l = max0(r_out - sqrt(k / gm));                // :126
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------
// GeometricMeanTwoCoin -- src/cfmms.jl:180-196
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double geom_arb_delta(double m, double r1, double r2, double eta, double g)
{
    const double inner = (((g * m) * eta) * r1) * pow(r2, eta);    // :180
    return max0(pow(inner, 1.0 / (eta + 1.0)) - r2) / g;
}
__device__ __forceinline__ double geom_arb_lambda(double m, double r1, double r2, double eta, double g)
{
    const double base = (r2 * pow(r1, 1.0 / eta)) / ((eta * g) * m); // :181
    return max0(r1 - pow(base, eta / (1.0 + eta)));
}

struct GeoMeanOps {
    static constexpr bool kNeedsLogPrices = false;
    static constexpr bool kPrefetch = true;
    struct Raw {
        double2 R, w;
        double g;
        int2 ai;
        double yg;    // unused (interface of process_pool)
    };
    GeoMeanPools p;
    template <bool GBINS, bool LEAN = false, class I>
    __device__ __forceinline__ Raw load(I i) const { return Raw{p.R[i], p.w[i], p.gamma[i], p.Ai[i], 0.0}; }
    template <bool GBINS, bool FAST, bool LEAN = false>
    __device__ __forceinline__ void resolve(Raw&, const double2*) const {}
    __device__ __forceinline__ int2 tokens(const Raw& r) const { return r.ai; }
    // Same idea as ProductOps::solve: Δ₁,Λ₂ > 0 ⇔ γ·m₁₂·η·R₂ > R₁ and Δ₂,Λ₁ > 0 ⇔ γ·m₂₁·R₁/η > R₂
    // (the bases of :180 exceed r2^(η+1)); only the live direction's two forms (4 pow instead of
    // 8) are evaluated, with the reference's expressions on the selected operands.
    template <bool FAST>   // (no fast variant: pow dominates and the forms keep the reference's operation order)
    __device__ __forceinline__ int solve_dir(const Raw& r, const Px& px, double& d, double& l, Trade& t) const
    {
        d = l = 0.0;      // every trade travels in t (kDirBoth)
        const double v1 = px.v1, v2 = px.v2;
        const double R1 = r.R.x, R2 = r.R.y, g = r.g;
        const double eta = r.w.x / r.w.y;        // :188
        const double ieta = 1.0 / eta;
        const double m12 = v2 / v1, m21 = v1 / v2;
        constexpr double kMargin = 1.0 + 1e-11;  // pow is good to ~1 ulp; keep a wide margin
        const bool p1 = (((g * m12) * eta) * R2) * kMargin >= R1;
        const bool p2 = (((g * m21) * ieta) * R1) * kMargin >= R2;
        t.d1 = t.d2 = t.l1 = t.l2 = 0.0;
        if (p1 != p2) {
            const double m = p1 ? m12 : m21, e = p1 ? eta : ieta;
            const double ra = p1 ? R2 : R1, rb = p1 ? R1 : R2;
            const double dx = geom_arb_delta(m, ra, rb, e, g);    // :190 / :191
            const double lx = geom_arb_lambda(m, ra, rb, e, g);   // :194 / :193
            t.d1 = p1 ? dx : 0.0;
            t.d2 = p1 ? 0.0 : dx;
            t.l1 = p1 ? 0.0 : lx;
            t.l2 = p1 ? lx : 0.0;
        } else if (p1) {
            t.d1 = geom_arb_delta(m12, R2, R1, eta, g);   // :190
            t.d2 = geom_arb_delta(m21, R1, R2, ieta, g);  // :191
            t.l1 = geom_arb_lambda(m21, R1, R2, ieta, g); // :193
            t.l2 = geom_arb_lambda(m12, R2, R1, eta, g);  // :194
        }
        return kDirBoth;
    }
};

// Log-space evaluation of the same two closed forms (default for GeometricMeanTwoCoin).
// With c = γ·m·e·r_a (the pow-free factor of :180), l_x = log x:
//     X = (c·r_b^e)^(1/(e+1))                    = exp((l_c + e·l_b) / (e+1))      the tendered side's new reserve
//     Y = ((r_b·r_a^(1/e)) / (e·γ·m))^(e/(1+e))  = X·r_a/c                          the received side's new reserve
// (the second identity: at the optimum the pool's marginal price equals the fee-adjusted market
// price, which fixes the RATIO of the two new reserves).  Nothing per-pool is left inside a
// logarithm: l_c = log γ + log e + log r_a + (log v_out − log v_in), so with log v staged per TOKEN
// in LDS once per block (stage_prices) and the v-independent sums prepared per POOL at upload
//     direction 1 (e = η):    exponent = (Q1 + Δ) / (η+1),       Q1 = log γ + log η + log R2 + η·log R1
//     direction 2 (e = 1/η):  exponent = (Q2 − η·Δ) / (η+1),     Q2 = η·(log γ + log R1 − log η) + log R2
// with Δ = log v2 − log v1.  Per trading pool that leaves 1 exp + 3 divisions (the exponent, Y and
// the final /γ) instead of 4 pow + 6 divisions; pools inside the
// no-arbitrage band cost four multiplies and two compares.  The exponent carries an absolute rounding
// error of about u·(|log γ| + |log η| + |log v1| + |log v2| + |log r_a| + e·|log r_b|)/(e+1), u = 2^-53, so with
// κ = 1 + that sum / (e+1) the trades are within K·u·(κ·X* + r_b)/γ (Δ) and K·u·(κ·Y* + r_a) (Λ) of the exact
// ones: measured K <= 2.8 on every path (fast and full arithmetic, device-pointer sweeps, direct path), asserted at
// K = 4..8 against a 60-digit truth in tests/test_gpu_precise.py.  Unlike r2^η in the reference, nothing here can
// overflow.
struct GeoMeanLogOps {
    static constexpr bool kNeedsLogPrices = true;
    static constexpr bool kPrefetch = true;
    struct Raw {
        double2 R, Q;
        double eta, g;
        int2 ai;      // packed: {tok, gidx} until resolve()
        double yg;
    };
    GeoMeanPools p;
    template <bool GBINS, bool LEAN = false, class I>
    __device__ __forceinline__ Raw load(I i) const
    {
        Raw r;
        r.R = stream_at<LEAN>(p.R, i);
        r.Q = stream_at<LEAN>(p.Q, i);
        r.eta = stream_at<LEAN>(p.eta, i);
        r.yg = 0.0;
        if constexpr (GBINS) {
            r.g = p.gamma[i];
            r.ai = p.Ai[i];
        } else {
            r.ai = load_packed<LEAN>(p.pk, i);
            r.g = LEAN ? 0.0 : load_packed_fee(p.gbase, p.gamma + i);
        }
        return r;
    }
    template <bool GBINS, bool FAST, bool LEAN = false>
    __device__ __forceinline__ void resolve(Raw& r, const double2* gtab_lds) const
    {
        if constexpr (!GBINS) resolve_packed<FAST, LEAN>(p.gbase, gtab_lds, r.ai, r.g, r.yg);
    }
    __device__ __forceinline__ int2 tokens(const Raw& r) const { return r.ai; }
    // one direction of the log-space forms: {d, l} for direction 1 (dir1) or 2
    template <bool FAST>
    __device__ __forceinline__ void one_direction(const Raw& r, const Px& px, bool dir1, double n, double dd, double& d, double& l) const
    {
        const double R1 = r.R.x, R2 = r.R.y, g = r.g, eta = r.eta;
        const double ra = dir1 ? R2 : R1, rb = dir1 ? R1 : R2;
        const double A = dir1 ? (r.Q.x + px.dlv) : (r.Q.y - eta * px.dlv);
        double X, Y;
        if constexpr (FAST) {   // same correctly rounded quotients for operands inside the window (checked at upload / staging)
            X = fast_exp(fast_div(A, eta + 1.0));
            Y = fast_div((X * ra) * dd, n);
            d = div_by(max0(X - rb), g, px.yg);
        } else {
            X = exp(A / (eta + 1.0));     // the tendered side's reserve after the trade
            Y = ((X * ra) * dd) / n;      // X·r_a/c, c = n/d
            d = max0(X - rb) / g;
        }
        l = max0(ra - Y);
    }
    template <bool FAST>
    __device__ __forceinline__ int solve_dir(const Raw& r, const Px& px, double& d, double& l, Trade& t) const
    {
        const double v1 = px.v1, v2 = px.v2;                 // px.dlv = log v2 − log v1
        const double R1 = r.R.x, R2 = r.R.y, g = r.g;
        const double eta = r.eta;                     // η = w₁/w₂, prepared at upload
        const double n1 = ((g * v2) * eta) * R2, d1 = v1;   // c₁ = n1/d1: direction 1 trades iff c₁ > R₁
        const double n2 = (g * v1) * R1, d2 = v2 * eta;     // c₂ = n2/d2: direction 2 trades iff c₂ > R₂
        const bool p1 = n1 > R1 * d1, p2 = n2 > R2 * d2;
        d = l = 0.0;
        if (v1 != v1 || v2 != v2) { t.d1 = t.d2 = t.l1 = t.l2 = v1 + v2; return kDirBoth; }   // NaN prices propagate (reference: pow of NaN)
        if (!(p1 || p2)) return kDirNone;
        // the (normally only) live direction
        one_direction<FAST>(r, px, p1, p1 ? n1 : n2, p1 ? d1 : d2, d, l);
        if (!(p1 && p2)) return p1 ? kDir1 : kDir2;
        // BOTH directions live (needs γ > 1): direction 2 as a second trip through the same code
        t.d1 = d;
        t.l2 = l;
        one_direction<FAST>(r, px, false, n2, d2, t.d2, t.l1);
        return kDirBoth;
    }
    // The lean kernels' solve (see ProductOps::lean_solve).  rare: a NaN price, or both directions live (needs γ > 1);
    // a wavefront with such a lane goes through solve_dir and the general epilogue.  The live direction's operands are
    // SELECTED: both exponents' numerators are formed (an add, and a multiply and a subtract) and one is taken, instead of
    // a region per side.  The arithmetic is one_direction's.
    template <bool FAST>
    __device__ __forceinline__ void lean_solve(const Raw& r, const Px& px, double& d, double& l, bool& dir1, bool& trades, bool& rare) const
    {
        const double v1 = px.v1, v2 = px.v2;
        const double R1 = r.R.x, R2 = r.R.y, g = r.g, eta = r.eta;
        const double n1 = ((g * v2) * eta) * R2, d1 = v1;
        const double n2 = (g * v1) * R1, d2 = v2 * eta;
        const bool p1 = n1 > R1 * d1, p2 = n2 > R2 * d2;
        trades = p1 | p2;                                    // (a NaN price: both false)
        dir1 = !p2;
        rare = (p1 & p2) | (v1 != v1) | (v2 != v2);
        d = l = 0.0;
        if (trades) {
            const double A1 = r.Q.x + px.dlv, A2 = r.Q.y - eta * px.dlv;
            const double A = p1 ? A1 : A2;
            const double ra = p1 ? R2 : R1, rb = p1 ? R1 : R2;
            const double n = p1 ? n1 : n2, dd = p1 ? d1 : d2;
            double X, Y;
            if constexpr (FAST) {
                X = fast_exp(fast_div(A, eta + 1.0));
                Y = fast_div((X * ra) * dd, n);
                d = div_by(max0(X - rb), g, px.yg);
            } else {
                X = exp(A / (eta + 1.0));
                Y = ((X * ra) * dd) / n;
                d = max0(X - rb) / g;
            }
            l = max0(ra - Y);
        }
    }
};

// ---------------------------------------------------------------------------------------------
// Solidly-style stable pair, φ(x, y) = x³y + xy³.  The reference declares no such pool; the arbitrage
// problem is find_arb!'s (src/cfmms.jl:21-33) and has a closed form.
// ---------------------------------------------------------------------------------------------
// φ is homogeneous, so the marginal price of coin 1 in coin 2 depends on t = y/x only: p(t) = t(3 + t²)/(1 + 3t²), and
// with a = t + 1, b = t − 1 it is (a³ + b³)/(a³ − b³), hence p(t) = π ⇔ (t − 1)/(t + 1) = c, c = cbrt((π − 1)/(π + 1)).
// Written for the TENDERED coin a and the received coin b (φ is symmetric, so direction 2 is direction 1 with the coins
// swapped): the pool trades iff γ·p(r_b/r_a) > v_a/v_b, and the optimum has π = v_a/(γ·v_b), i.e.
//     c³ = (v_a − γ·v_b)/(v_a + γ·v_b)             the numerator with ONE rounding (fma): it cancels near the band
//     t  = (1 + c)/(1 − c) = π·(1 + c + c²)/(1 − c + c²)    (1 ± c = (1 ± c³)/(1 ∓ c + c²), and (1 + c³)/(1 − c³) = π: no
//                                                            cancellation for any π; both quadratics lie in [3/4, 3])
// for the ratio r_b′/r_a′ of the new reserves; φ(r′) = φ(r) then gives r_a′ = r_a·(t₀(1 + t₀²)/(t(1 + t²)))^¼ with
// t₀ = r_b/r_a (two square roots; k = φ(R) itself is never formed: it overflows at R ≈ 1e77) and r_b′ = t·r_a′.
// With γ <= 1 (checked at upload) the two directions exclude each other, in floating point too: the two tests share
// their products A, B, and g·A > B implies A >= fl(g·A) > B >= fl(g·B).  One arithmetic (the compiler's full-range
// division, square root and cbrt): upload range R ∈ [2^-150, 2^150] keeps t₀³ finite.
struct SolidlyOps : ProductOps {     // ProductTwoCoin's pool layout, Raw, load, resolve and tokens: only the solve differs
    template <bool FAST>   // (no fast variant)
    __device__ __forceinline__ int solve_dir(const Raw& r, const Px& px, double& d, double& l, Trade& t) const
    {
        const double R1 = r.R.x, R2 = r.R.y, g = r.g, v1 = px.v1, v2 = px.v2;
        d = l = 0.0;
        if (v1 != v1 || v2 != v2) { t.d1 = t.d2 = t.l1 = t.l2 = v1 + v2; return kDirBoth; }   // NaN prices propagate
        // direction without a division: γ·v₂·φₓ(R) > v₁·φ_y(R) (1), v₂·φₓ(R) < γ·v₁·φ_y(R) (2); inside the band neither
        const double s1 = R1 * R1, s2 = R2 * R2;
        const double A = v2 * (R2 * __builtin_fma(3.0, s1, s2));
        const double B = v1 * (R1 * __builtin_fma(3.0, s2, s1));
        const bool p1 = g * A > B, p2 = A < g * B;
        if (!(p1 || p2)) return kDirNone;
        const double va = p1 ? v1 : v2, vb = p1 ? v2 : v1;     // prices of the tendered / received coin
        const double ra = p1 ? R1 : R2, rb = p1 ? R2 : R1;
        const double num = __builtin_fma(-g, vb, va), den = __builtin_fma(g, vb, va);
        const double c = cbrt(num / den);
        const double c2 = c * c;
        const double tt = (va * ((1.0 + c) + c2)) / ((g * vb) * ((1.0 - c) + c2));   // r_b′/r_a′
        const double t0 = rb / ra;
        const double rho = (t0 * __builtin_fma(t0, t0, 1.0)) / (tt * __builtin_fma(tt, tt, 1.0));
        const double xa = ra * sqrt(sqrt(rho));                // the tendered coin's new reserve
        d = max0(xa - ra) / g;
        l = max0(rb - tt * xa);
        return p1 ? kDir1 : kDir2;
    }
};

} // namespace cfmm
