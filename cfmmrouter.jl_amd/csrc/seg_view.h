// seg_view.h -- internal: a segment as the query entries (abi_quote.cpp, abi_swap.cpp, abi_quote_path.cpp, abi_swap_path.cpp,
// abi_find_path.cpp) hand it to their kernels and to their checks.  Host-side only, on top of ctx.h.
// path_seg is the ONE place that reads the addresses of a segment's pool arrays for a quote; every other view is derived from
// its result or sits beside it.  A view holds the addresses the segment holds NOW -- cfmm_update_reserves, cfmm_pools_set_ticks
// and tick compaction swap UniV3 arrays -- so it is taken per launch (the tables: per call, and again behind a wave that moved
// UniV3 pools) and never kept.  A new per-segment array or pool family is added here and nowhere else.
#pragma once

#include "ctx.h"
#include "path_checks.h"

#include <algorithm>
#include <cstring>

namespace cfmm {

// the entry's name, its _dev form's and the given amount's, as the messages spell them (each file keeps its two constants)
struct Dir {
    bool exact_out;
    const char *who, *dev, *given;
    bool rated = false;   // cfmm_swap_limit: an exact-input swap behind a limit on the marginal rate, with the amount used beside its answer
};

// {kind, m, coins per pool} of segment `seg` as the checks see it, on a single context or a parent (its own list); the
// number of segments; all of them
template <class Seg>
PathSegInfo seg_info(const Seg& s) { return {s.kind, s.m, ragged_kind(s.kind) ? s.n_coins : 2}; }
inline PathSegInfo seg_info(const cfmm_ctx* c, int32_t seg) { return c->shards.empty() ? seg_info(c->segs[(size_t)seg]) : seg_info(c->psegs[(size_t)seg]); }
inline int64_t seg_count(const cfmm_ctx* c) { return (int64_t)(c->shards.empty() ? c->segs.size() : c->psegs.size()); }
inline std::vector<PathSegInfo> seg_infos(const cfmm_ctx* c)
{
    std::vector<PathSegInfo> v;
    for (int64_t i = 0; i < seg_count(c); ++i) v.push_back(seg_info(c, (int32_t)i));
    return v;
}

// The quotes' view of a segment: kind -1 when it has no pools (no hop is valid on it), 2 coins unless ragged, and the
// members of the segment's OWN kind -- the rest stays null
inline PathSeg path_seg(const Segment& s)
{
    PathSeg r;
    std::memset(&r, 0, sizeof r);
    r.kind = s.m > 0 ? s.kind : -1;
    r.n_coins = ragged_kind(s.kind) ? s.n_coins : 2;
    r.m = s.m;
    if (s.kind == CFMM_KIND_UNIV3) {
        r.pg = s.u.pg.get();
        r.cur_a = s.u.cur_a.get();
        r.cur_b = s.u.cur_b.get();
        r.cur_c = s.u.cur_c.get();
        r.curR = s.u.curR.get();
        r.walk = s.u.walk.get();
        r.ticks = s.u.ticks.get();
    } else if (ragged_kind(s.kind)) {
        r.nR = s.nc.R.get();
        r.nq = s.nc.q.get();
        r.nglg = s.nc.glg.get();
        r.npar = s.nc.par.get();
    } else {
        r.R = s.R.get();
        r.w = s.w.get();
        r.gamma = s.gamma.get();
    }
    return r;
}

// ... as the single-segment kernels take it: QuoteArgs' segment members and the two pool structs, whose other members these
// kernels do not read (the members of a kind the segment is not are null in `p`, so they are here)
inline UniV3Pools univ3_view(const PathSeg& p)   // (Ai, thr, head, has_walk, cp, pk, gbase: the sweep's)
{
    return UniV3Pools{p.pg, nullptr, p.cur_a, p.cur_b, p.cur_c, p.curR, p.walk, p.ticks, nullptr, nullptr, 0, nullptr, nullptr, 0};
}
inline NCoinPools ncoin_view(const PathSeg& p)   // (tok, Delta, Lambda: the sweep's)
{
    return NCoinPools{p.nR, p.nq, nullptr, p.nglg, p.npar, p.nR ? p.n_coins : 0, nullptr, nullptr};
}
inline void quote_view(const PathSeg& p, QuoteArgs& a)
{
    a.m = p.m;
    a.n_coins = p.n_coins;
    a.R = p.R;
    a.w = p.w;
    a.gamma = p.gamma;
}

// The swaps' view: the quotes', the segment's arrays again as WRITABLE pointers, what swap_kernel takes besides them and the
// window flag `left` of the kinds with a fast arithmetic whose state is their reserves
inline SwapPathSeg swap_path_seg(const Segment& s, int* left)
{
    SwapPathSeg r;
    std::memset(&r, 0, sizeof r);
    r.s = path_seg(s);
    if (ragged_kind(s.kind)) {
        r.nR = s.nc.R.get();
        r.nq = s.nc.q.get();
    } else if (s.kind != CFMM_KIND_UNIV3) {
        r.R = s.R.get();
        r.Q = s.lR.get();
        r.eta = s.eta.get();
        if (kind_info(s.kind).has_fast) r.left_window = left;
    }
    return r;
}
inline void swap_view(const SwapPathSeg& p, SwapArgs& a)
{
    quote_view(p.s, a.q);
    a.R = p.R;
    a.Q = p.Q;
    a.eta = p.eta;
    a.ncR = p.nR;
    a.ncq = p.nq;
    a.left_window = p.left_window;
}

// The search's view: the quotes', the segment's token arrays and where it starts in the numberings of blocks and of pools
inline FindSeg find_seg(const Segment& s, int64_t first_tile, int64_t first_pool)
{
    FindSeg f;
    std::memset(&f, 0, sizeof f);
    f.s = path_seg(s);
    if (ragged_kind(s.kind)) {
        f.tok = s.nc.tok.get();
    } else {
        f.pk = s.pk.get();
        f.Ai = s.Ai.get();
    }
    f.first_tile = first_tile;
    f.first_pool = first_pool;
    return f;
}

// The tables of the path kernels: one record per segment from make(segment, its number), and AT LEAST ONE record, so that the
// kernel's clamp of a segment number always lands on one -- a context without pools: a record of kind -1
inline size_t table_records(const cfmm_ctx* c) { return std::max<size_t>(1, c->segs.size()); }
inline PathSeg& quote_part(PathSeg& r) { return r; }
template <class Rec>
PathSeg& quote_part(Rec& r) { return r.s; }
template <class Rec, class Make>
void build_table(const cfmm_ctx* c, Rec* t, Make make)
{
    std::memset(t, 0, sizeof(Rec));
    quote_part(t[0]).kind = -1;
    quote_part(t[0]).n_coins = 2;
    for (size_t i = 0; i < c->segs.size(); ++i) t[i] = make(c->segs[i], i);
}

} // namespace cfmm
