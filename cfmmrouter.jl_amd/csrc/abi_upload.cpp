// abi_upload.cpp -- pool validation and upload (include/cfmm_amd.h): what the reference's constructors validate
// (src/cfmms.jl:76-90) plus what its kernels silently assume (src/cfmms.jl:129 "Assumes that v > 0 and γ > 0"),
// the packed fee + token records, and the v-independent constants of the GeometricMean / UniV3 closed forms,
// prepared once on the host with the same IEEE operations the reference applies per sweep.
#include "ctx.h"
#include "pool_checks.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace {

// Packed fee + token record of a segment (sweep.h PackedFeeTok): {i1 | i2 << 16, index of the pool's fee among the
// segment's distinct fees}.  Built for every segment outside large-market mode (token ids fit 16 bits there); a segment
// with more than kMaxFeeTable distinct fees keeps the records for the tokens only (gvals empty: its launches read the
// fee from the gamma array).
int build_packed(cfmm_ctx* c, Segment& s, int64_t m, const double* gamma, const int32_t* Ai)
{
    s.pk.reset();
    s.gvals.clear();
    if (global_bins(c) || m == 0) return CFMM_OK;
    std::vector<PackedFeeTok> pk((size_t)m);
    std::vector<double> vals;
    uint64_t last_bits = 0;
    uint32_t last_idx = 0;
    bool have_last = false, table = true;
    for (int64_t i = 0; i < m; ++i) {
        uint32_t idx = 0;
        if (table) {
            uint64_t bits;
            std::memcpy(&bits, &gamma[i], sizeof bits);
            if (have_last && bits == last_bits) {
                idx = last_idx;
            } else {
                idx = (uint32_t)vals.size();
                for (uint32_t k = 0; k < (uint32_t)vals.size(); ++k) {   // <= 256 entries: a linear scan beats a hash map
                    uint64_t vb;
                    std::memcpy(&vb, &vals[k], sizeof vb);
                    if (vb == bits) { idx = k; break; }
                }
                if (idx == (uint32_t)vals.size()) {
                    if ((int)vals.size() == kMaxFeeTable) { table = false; idx = 0; }   // too many fee tiers: no table
                    else vals.push_back(gamma[i]);
                }
                last_bits = bits; last_idx = idx; have_last = true;
            }
        }
        pk[(size_t)i].tok = (uint32_t)Ai[2 * i] | ((uint32_t)Ai[2 * i + 1] << 16);
        pk[(size_t)i].gidx = idx;
    }
    int rc = s.pk.upload(c, pk.data(), (size_t)m);
    if (rc != CFMM_OK) return rc;
    if (table) s.gvals.swap(vals);
    return CFMM_OK;
}

// What two_coin_check_cast (src/cfmms.jl:76-90) enforces structurally is implied by the [m][2]
// layout; here we check the values the closed forms assume.
int check_two_coin(cfmm_ctx* c, int64_t m, const double* R, const double* gamma, const int32_t* Ai)
{
    if (m < 0) return fail(c, CFMM_ERR_INVALID_ARG, "negative pool count");
    if (m > 0 && (!R || !gamma || !Ai)) return fail(c, CFMM_ERR_INVALID_ARG, "null pool array");
    for (int64_t i = 0; i < m; ++i) {
        const int rc = check_reserves(c, i, R + 2 * i, 2);
        if (rc != CFMM_OK) return rc;
        if (!finite_pos(gamma[i]))
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: fee gamma must be finite and > 0", (long long)i);
        const int32_t a = Ai[2 * i], b = Ai[2 * i + 1];
        if (a < 0 || a >= c->n || b < 0 || b >= c->n)
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: token index out of range [0, %d)", (long long)i, c->n);
        if (a == b)
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: the two token indices must differ", (long long)i);
    }
    return CFMM_OK;
}

int add_segment_common(cfmm_ctx* c, Segment&& s, const int32_t* Ai)
{
    if (s.m == 0) return CFMM_OK;   // an empty batch contributes no pools, no trades and no partial rows: not stored
    if (global_bins(c) && s.m > 0) s.h_ai.assign(Ai, Ai + 2 * s.m);
    c->segs.push_back(std::move(s));
    c->geometry_dirty = c->desc_dirty = true;
    c->have_out = false;
    c->have_trades = false;
    return CFMM_OK;
}

// The checks cfmm_pools_add_weighted and cfmm_pools_add_curve share, in this order: the arguments (arrays: no pool array is
// null), then pool by pool each coin's reserve, the family's own check of that coin (coin_ok(i, j), j = i·n_coins + k),
// its token index (range, distinct within the pool), then the family's own checks of the pool (pool_ok(i)) and its fee.
// coin_ok / pool_ok return CFMM_OK or fail(...).
template <class CoinOk, class PoolOk>
int ncoin_check(cfmm_ctx* c, int kind, int64_t m, int32_t n_coins, const double* R, const double* gamma, const int32_t* Ai,
                bool arrays, CoinOk coin_ok, PoolOk pool_ok)
{
    const char* fam = kind_info(kind).name;
    if (m < 0) return fail(c, CFMM_ERR_INVALID_ARG, "negative pool count");
    if (n_coins < 2 || n_coins > kMaxCoins)
        return fail(c, CFMM_ERR_INVALID_ARG, "n_coins = %d: %s pools have 2 .. %d coins", (int)n_coins, fam, kMaxCoins);
    if (c->n > kMaxLdsTokens)
        return fail(c, CFMM_ERR_UNSUPPORTED, "%s pools need n_tokens <= %d (large-market mode sweeps two-coin pools only)", fam,
                    kMaxLdsTokens);
    if (m > 0 && !arrays) return fail(c, CFMM_ERR_INVALID_ARG, "null pool array");
    const int nc = n_coins;
    int rc;
    for (int64_t i = 0; i < m; ++i) {
        for (int k = 0; k < nc; ++k) {
            const size_t j = (size_t)(i * nc + k);
            if ((rc = check_reserves(c, i, R + j, 1)) != CFMM_OK) return rc;
            if ((rc = coin_ok(i, j)) != CFMM_OK) return rc;
            const int32_t a = Ai[j];
            if (a < 0 || a >= c->n)
                return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: token index out of range [0, %d)", (long long)i, c->n);
            for (int k2 = 0; k2 < k; ++k2)
                if (Ai[(size_t)(i * nc + k2)] == a)
                    return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: the token indices must be distinct", (long long)i);
        }
        if ((rc = pool_ok(i)) != CFMM_OK) return rc;
        if (!finite_pos(gamma[i])) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: fee gamma must be finite and > 0", (long long)i);
        if (gamma[i] > 1.0)
            return fail(c, CFMM_ERR_INVALID_ARG,
                        "pool %lld: fee gamma must be <= 1 (gamma > 1 pays for round trips: the arbitrage problem is unbounded)",
                        (long long)i);
    }
    return CFMM_OK;
}

// The upload of m checked N-coin pools: coin-major columns (sweep.h NCoinPools) of R, tokens, the family's per-coin constant
// q and its own column par, filled pool by pool by fill(i, q, par) (q[0 .. n_coins), par[0 .. par_per_pool)), {γ, log γ},
// the segment's trade arrays, and the segment itself
template <class Fill>
int ncoin_add(cfmm_ctx* c, int kind, int64_t m, int nc, const double* R, const double* gamma, const int32_t* Ai, Fill fill)
{
    const KindInfo& fam = kind_info(kind);
    const size_t cells = (size_t)m * (size_t)nc, np = (size_t)fam.par_per_pool(nc);
    std::vector<double> cR(cells), cq(cells), cpar((size_t)m * np);
    std::vector<int32_t> ct(cells);
    std::vector<double2> glg((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        double q[kMaxCoins], par[kMaxCoins];
        fill(i, q, par);
        for (int k = 0; k < nc; ++k) {
            const size_t src = (size_t)(i * nc + k), dst = (size_t)k * (size_t)m + (size_t)i;
            cR[dst] = R[src];
            cq[dst] = q[k];
            ct[dst] = Ai[src];
        }
        for (size_t k = 0; k < np; ++k) cpar[fam.par_coin_major ? k * (size_t)m + (size_t)i : (size_t)i * np + k] = par[k];
        glg[(size_t)i] = make_double2(gamma[i], std::log(gamma[i]));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    Segment s;
    s.kind = kind;
    s.m = m;
    s.n_coins = nc;
    s.fast_ok = 0;   // one arithmetic only (the compiler's)
    if (kind == CFMM_KIND_WEIGHTED) s.h_par = cpar;   // the normalised weights q is prepared from (cfmm_pools_set_reserves)
    int rc;
    if ((rc = s.nc.R.upload(c, cR.data(), cells)) || (rc = s.nc.q.upload(c, cq.data(), cells)) ||
        (rc = s.nc.tok.upload(c, ct.data(), cells)) || (rc = s.nc.par.upload(c, cpar.data(), cpar.size())) ||
        (rc = s.nc.glg.upload(c, glg.data(), (size_t)m)))
        return rc;
    if (s.nc.D.alloc(c, cells) != CFMM_OK || s.nc.L.alloc(c, cells) != CFMM_OK)
        return fail(c, CFMM_ERR_HIP, "trade buffers of a %s segment: allocation failed", fam.name);
    return add_segment_common(c, std::move(s), Ai);
}

} // namespace

namespace cfmm {

// Validates m UniV3 pools and prepares + uploads the find_arb_pos constants (see UniV3Ops) into `u`; fast_ok: Segment::fast_ok
// of these constants.  What does not depend on the prices (Ai, the packed records) is the caller's.
int univ3_build(cfmm_ctx* c, UniV3State& u, int& fast_ok, int64_t m, const double* current_price, const double* gamma, const int32_t* Ai,
                const int64_t* tick_off, const double* lower_ticks, const double* liquidity)
{
    const int64_t T = m > 0 ? tick_off[m] : 0;
    if (T < 0 || 2 * (T + 2 * m) > (int64_t)0x3fffffff) return fail(c, CFMM_ERR_UNSUPPORTED, "too many ticks in one segment");
    std::vector<double2> pg((size_t)m), cur_a((size_t)m), cur_b((size_t)m), curR((size_t)m);
    std::vector<double> cur_c((size_t)m);
    std::vector<TickRec> ticks;
    std::vector<int4> walk((size_t)m);
    int longest = 0;
    bool fast = true;   // every operand of the sweep's divisions / square roots inside the fast window (sweep.h)
    ticks.reserve((size_t)T + 2 * (size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t o = tick_off[i], nt = tick_off[i + 1] - o;
        if (nt < 1) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: needs at least one tick", (long long)i);
        int rc = check_univ3_price(c, i, current_price[i]);
        if (rc != CFMM_OK) return rc;
        if (!finite_pos(gamma[i]))
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: fee gamma must be finite and > 0", (long long)i);
        const int32_t a = Ai[2 * i], b = Ai[2 * i + 1];
        if (a < 0 || a >= c->n || b < 0 || b >= c->n)
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: token index out of range [0, %d)", (long long)i, c->n);
        if (a == b) return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: the two token indices must differ", (long long)i);
        const double* lt = lower_ticks + o;
        const double* lq = liquidity + o;
        if ((rc = check_univ3_ladder(c, i, lt, lq, nt)) != CFMM_OK) return rc;
        const double cp = current_price[i];
        fast = fast && in_fast_window(cp) && in_fast_window(gamma[i]) && univ3_liquidity_in_window(lq, nt);
        int64_t ct;
        if ((rc = check_univ3_tick(c, i, lt, nt, cp, ct)) != CFMM_OK) return rc;
        UniV3PoolRec rec;
        univ3_prepare_pool(cp, gamma[i], ct, nt, lt, lq, rec, ticks);   // (univ3_pool.h: both lists appended to `ticks`)
        cur_a[(size_t)i] = rec.cur_a;
        cur_b[(size_t)i] = rec.cur_b;
        cur_c[(size_t)i] = rec.cur_c;
        curR[(size_t)i] = rec.curR;
        longest = std::max(longest, std::max(rec.walk.y, rec.walk.w));
        walk[(size_t)i] = rec.walk;
        pg[(size_t)i] = rec.pg;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // drain thresholds of all records; every record also carries its own (univ3_pool.h)
    std::vector<double> thr;
    univ3_all_thresholds(ticks, thr);
    thr.resize(ticks.size() + 4, 0.0);   // the scan reads four thresholds at a time
    u.has_walk = longest > 0 ? 1 : 0;
    // threshold heads (sweep.h UniV3Pools::head): the first four thresholds of both lists of every pool as floats rounded DOWN
    std::vector<uint4> head;
    if (u.has_walk) {
        head.resize(2 * (size_t)m);
        for (int64_t i = 0; i < m; ++i) univ3_heads(walk[(size_t)i], thr.data(), &head[2 * (size_t)i]);
    }
    fast_ok = fast ? 1 : 0;
    u.tick_used = u.tick_cap = (int64_t)ticks.size();   // no spare records: the first price update that needs some regrows (abi_update.cpp)
    u.h_walk = walk;
    int rc;
    if ((rc = u.pg.upload(c, pg.data(), (size_t)m)) ||
        (rc = u.cur_a.upload(c, cur_a.data(), (size_t)m)) || (rc = u.cur_b.upload(c, cur_b.data(), (size_t)m)) ||
        (rc = u.cur_c.upload(c, cur_c.data(), (size_t)m)) || (rc = u.curR.upload(c, curR.data(), (size_t)m)) ||
        (rc = u.walk.upload(c, walk.data(), (size_t)m)) || (rc = u.ticks.upload(c, ticks.data(), ticks.size())) ||
        (rc = u.thr.upload(c, thr.data(), thr.size())) || (rc = u.head.upload(c, head.data(), head.size())) ||
        (rc = u.cp.upload(c, current_price, (size_t)m)))
        return rc;
    return CFMM_OK;
}

} // namespace cfmm

extern "C" {

int cfmm_pools_add_product(cfmm_ctx* c, int64_t m, const double* R, const double* gamma, const int32_t* Ai)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_two_coin(c, m, R, gamma, Ai);
    if (rc != CFMM_OK) return rc;
    if (!c->shards.empty())
        return multi_add(c, CFMM_KIND_PRODUCT, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            return cfmm_pools_add_product(child, hi - lo, R + 2 * lo, gamma + lo, Ai + 2 * lo);
        });
    HIP_TRY(c, hipSetDevice(c->device));
    Segment s;
    s.kind = CFMM_KIND_PRODUCT;
    s.m = m;
    s.fast_ok = 1;
    for (int64_t i = 0; i < m && s.fast_ok; ++i)
        s.fast_ok = in_fast_window(R[2 * i]) && in_fast_window(R[2 * i + 1]) && in_fast_window(gamma[i]);
    if ((rc = s.R.upload(c, R, (size_t)m)) || (rc = s.gamma.upload(c, gamma, (size_t)m)) ||
        (rc = s.Ai.upload(c, Ai, (size_t)m)) || (rc = build_packed(c, s, m, gamma, Ai)))
        return rc;
    return add_segment_common(c, std::move(s), Ai);
}

int cfmm_pools_add_solidly(cfmm_ctx* c, int64_t m, const double* R, const double* gamma, const int32_t* Ai)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_two_coin(c, m, R, gamma, Ai);
    if (rc != CFMM_OK) return rc;
    for (int64_t i = 0; i < m; ++i) {
        if (gamma[i] > 1.0)
            return fail(c, CFMM_ERR_INVALID_ARG,
                        "pool %lld: fee gamma must be <= 1 (gamma > 1 pays for round trips: the arbitrage problem is unbounded)",
                        (long long)i);
        if ((rc = check_solidly_range(c, i, R + 2 * i)) != CFMM_OK) return rc;
    }
    if (!c->shards.empty())
        return multi_add(c, CFMM_KIND_SOLIDLY, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            return cfmm_pools_add_solidly(child, hi - lo, R + 2 * lo, gamma + lo, Ai + 2 * lo);
        });
    HIP_TRY(c, hipSetDevice(c->device));
    Segment s;
    s.kind = CFMM_KIND_SOLIDLY;
    s.m = m;
    s.fast_ok = 0;   // one arithmetic only (the compiler's)
    if ((rc = s.R.upload(c, R, (size_t)m)) || (rc = s.gamma.upload(c, gamma, (size_t)m)) ||
        (rc = s.Ai.upload(c, Ai, (size_t)m)) || (rc = build_packed(c, s, m, gamma, Ai)))
        return rc;
    return add_segment_common(c, std::move(s), Ai);
}

int cfmm_pools_add_geomean(cfmm_ctx* c, int64_t m, const double* R, const double* w, const double* gamma,
                           const int32_t* Ai)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = check_two_coin(c, m, R, gamma, Ai);
    if (rc != CFMM_OK) return rc;
    if (m > 0 && !w) return fail(c, CFMM_ERR_INVALID_ARG, "null weight array");
    for (int64_t i = 0; i < m; ++i)
        if (!finite_pos(w[2 * i]) || !finite_pos(w[2 * i + 1]))
            return fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: weights must be finite and > 0", (long long)i);
    if (!c->shards.empty())
        return multi_add(c, CFMM_KIND_GEOMEAN, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            return cfmm_pools_add_geomean(child, hi - lo, R + 2 * lo, w + 2 * lo, gamma + lo, Ai + 2 * lo);
        });
    // v-independent pieces of the log-space closed forms (ops_two_coin.h, GeoMeanLogOps)
    std::vector<double2> lR((size_t)m);
    std::vector<double> etas((size_t)m);
    bool fast = true;
    for (int64_t i = 0; i < m; ++i) {
        const double e = w[2 * i] / w[2 * i + 1]; // src/cfmms.jl:188
        fast = fast && in_fast_window(R[2 * i]) && in_fast_window(R[2 * i + 1]) && in_fast_window(gamma[i]) && in_fast_window(e);
        etas[(size_t)i] = e;
        lR[(size_t)i] = geomean_q(gamma[i], e, R[2 * i], R[2 * i + 1]);   // {Q1, Q2}
    }
    HIP_TRY(c, hipSetDevice(c->device));
    Segment s;
    s.kind = CFMM_KIND_GEOMEAN;
    s.m = m;
    s.fast_ok = fast ? 1 : 0;
    s.h_gamma.assign(gamma, gamma + m);   // host copies of what {Q1, Q2} are prepared from besides R (cfmm_pools_set_reserves)
    s.h_eta = etas;
    if ((rc = s.eta.upload(c, etas.data(), (size_t)m)) || (rc = s.lR.upload(c, lR.data(), (size_t)m)) ||
        (rc = s.R.upload(c, R, (size_t)m)) || (rc = s.w.upload(c, w, (size_t)m)) ||
        (rc = s.gamma.upload(c, gamma, (size_t)m)) || (rc = s.Ai.upload(c, Ai, (size_t)m)) ||
        (rc = build_packed(c, s, m, gamma, Ai)))
        return rc;
    return add_segment_common(c, std::move(s), Ai);
}

int cfmm_pools_add_univ3(cfmm_ctx* c, int64_t m, const double* current_price, const double* gamma,
                         const int32_t* Ai, const int64_t* tick_off, const double* lower_ticks,
                         const double* liquidity)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (m < 0) return fail(c, CFMM_ERR_INVALID_ARG, "negative pool count");
    if (m > 0 && (!current_price || !gamma || !Ai || !tick_off || !lower_ticks || !liquidity))
        return fail(c, CFMM_ERR_INVALID_ARG, "null pool array");
    if (m > 0 && tick_off[0] != 0) return fail(c, CFMM_ERR_INVALID_ARG, "tick_off[0] must be 0");
    if (!c->shards.empty()) {
        for (int64_t i = 0; i < m; ++i)
            if (tick_off[i + 1] < tick_off[i]) return fail(c, CFMM_ERR_INVALID_ARG, "tick_off must be non-decreasing");
        return multi_add(c, CFMM_KIND_UNIV3, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            std::vector<int64_t> off((size_t)(hi - lo + 1));
            for (int64_t i = lo; i <= hi; ++i) off[(size_t)(i - lo)] = tick_off[i] - tick_off[lo];   // CSR rebased to the block
            return cfmm_pools_add_univ3(child, hi - lo, current_price + lo, gamma + lo, Ai + 2 * lo, off.data(),
                                        lower_ticks + tick_off[lo], liquidity + tick_off[lo]);
        });
    }
    Segment s;
    s.kind = CFMM_KIND_UNIV3;
    s.m = m;
    s.n_ticks_total = m > 0 ? tick_off[m] : 0;
    int rc = univ3_build(c, s.u, s.fast_ok, m, current_price, gamma, Ai, tick_off, lower_ticks, liquidity);
    if (rc != CFMM_OK || (rc = s.Ai.upload(c, Ai, (size_t)m)) || (rc = build_packed(c, s, m, gamma, Ai))) return rc;
    // host copy of the pool definitions: update_reserves! re-derives the tick constants from them
    s.h_cp.assign(current_price, current_price + m);
    s.h_gamma.assign(gamma, gamma + m);
    s.h_ai.assign(Ai, Ai + 2 * m);
    s.lad.assign(m, tick_off, lower_ticks, liquidity);
    return add_segment_common(c, std::move(s), Ai);
}

int cfmm_pools_add_weighted(cfmm_ctx* c, int64_t m, int32_t n_coins, const double* R, const double* w, const double* gamma,
                            const int32_t* Ai)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const auto weight_ok = [&](int64_t i, size_t j) {
        return finite_pos(w[j]) ? CFMM_OK : fail(c, CFMM_ERR_INVALID_ARG, "pool %lld: weights must be finite and > 0", (long long)i);
    };
    int rc = ncoin_check(c, CFMM_KIND_WEIGHTED, m, n_coins, R, gamma, Ai, R && w && gamma && Ai, weight_ok,
                         [](int64_t) { return CFMM_OK; });
    if (rc != CFMM_OK) return rc;
    const int nc = n_coins;
    if (!c->shards.empty())
        return multi_add(c, CFMM_KIND_WEIGHTED, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            return cfmm_pools_add_weighted(child, hi - lo, n_coins, R + nc * lo, w + nc * lo, gamma + lo, Ai + nc * lo);
        }, nc);
    // weights normalised to sum to 1, q = log(R / w)
    return ncoin_add(c, CFMM_KIND_WEIGHTED, m, nc, R, gamma, Ai, [&](int64_t i, double* q, double* wn) {
        double ws = 0.0;
        for (int k = 0; k < nc; ++k) ws += w[(size_t)(i * nc + k)];
        for (int k = 0; k < nc; ++k) {
            const size_t src = (size_t)(i * nc + k);
            wn[k] = w[src] / ws;
            q[k] = weighted_q(R[src], wn[k]);
        }
    });
}

int cfmm_pools_add_curve(cfmm_ctx* c, int64_t m, int32_t n_coins, const double* R, const double* gamma, const int32_t* Ai,
                         const double* alpha, const double* beta)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    const auto ab_ok = [&](int64_t i) { return check_curve_params(c, i, alpha[i], beta[i], R + i * n_coins, n_coins); };
    int rc = ncoin_check(c, CFMM_KIND_CURVE, m, n_coins, R, gamma, Ai, R && gamma && Ai && alpha && beta,
                         [](int64_t, size_t) { return CFMM_OK; }, ab_ok);
    if (rc != CFMM_OK) return rc;
    const int nc = n_coins;
    if (!c->shards.empty())
        return multi_add(c, CFMM_KIND_CURVE, m, [&](cfmm_ctx* child, int64_t lo, int64_t hi) -> int {
            return cfmm_pools_add_curve(child, hi - lo, n_coins, R + nc * lo, gamma + lo, Ai + nc * lo, alpha + lo, beta + lo);
        }, nc);
    // q = log R; per pool {α, log β} (curve_solve_lbeta: at α = 0, one that keeps P₀/R_k inside the solve's range)
    return ncoin_add(c, CFMM_KIND_CURVE, m, nc, R, gamma, Ai, [&](int64_t i, double* q, double* ab) {
        curve_fill(R + i * nc, alpha[i], beta[i], nc, q, ab);
    });
}

int cfmm_pools_clear(cfmm_ctx* c)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    if (!c->shards.empty()) {
        for (cfmm_ctx* child : c->shards) cfmm_pools_clear(child);
        c->psegs.clear();
        c->m_total = 0;
        c->flat_total = 0;
        c->any_ragged = false;
        c->have_out = c->have_trades = false;
        return CFMM_OK;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->segs.clear();
    c->m_total = 0;
    c->flat_total = 0;
    c->any_ragged = false;
    c->rows_total = 0;
    c->geometry_dirty = c->desc_dirty = true;
    c->have_out = c->have_trades = false;
    return CFMM_OK;
}

} // extern "C"
