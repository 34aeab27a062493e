// find_path_kernels.h -- cfmm_find_path and cfmm_find_path_out: the best swap WALK of at most max_hops hops between two tokens,
// found on the device by ONE layered search run in either direction (FindDir<OUT> below holds what differs).
//   forwards   best[0][token_in] = amount_in, and best[h][t] is the LARGEST quote_one<KIND>(pool, ci -> co, best[h-1][tok(ci)])
//              over every pool of every segment and every ordered coin pair whose tok(co) is t and whose source is reached;
//   backwards  need[0][token_out] = amount_out, and need[h][t] is the SMALLEST quote_out_one<KIND>(pool, ci -> co,
//              need[h-1][tok(co)]) over every pair whose tok(ci) is t and whose destination is reached.  FindArgs serves with the
//              amounts' roles exchanged, as PathArgs serves both quote directions: a.amount_in carries the wanted amount_out,
//              a.amount_out receives the amount to tender, a.best holds need.
// Every hop is quoted against the pool AS IT STANDS (cfmm_quote_path's rule); a walk may visit a pool twice.
//   init     one lane per query: layer 0 of the start token <- the amount given (the scratch was set by a memset)
//   relax    THE HOT PATH, one launch per layer, ONE LANE PER POOL of every segment (a block finds its
//            segment in the table by its tile number).  A lane reads its pool's token ids (8 bytes; 4 per coin of a ragged pool),
//            then the layer-before words of those tokens for the queries of its group, and leaves when none is reached -- a
//            wavefront without any reached lane leaves on one ballot, before any pool state is read.  For every reached (query,
//            near coin) and every other coin it evaluates path_hop<KIND, OUT> (quote_path_kernels.h: the single-pool kernels'
//            body, so the bits are cfmm_quote's / cfmm_quote_out's) and folds the answer into the far coin's word with a 64-BIT
//            UNSIGNED INTEGER atomic on the double's bits: positive finite doubles order as their bit patterns and an integer
//            max / min does not depend on the order of arrival -- there is no float atomic.  Where a group of queries' layer
//            rows fit the LDS, a block first folds several tiles into its own copy.
//   select   one lane per query: the best layer entry of the end token over h >= 1, the FEWEST hops that attain it
//   claim    the walk, one launch per layer from h* down: one lane per pool again, but only a lane whose pool holds the CURRENT
//            TARGET token of some query evaluates anything -- the quotes that reach that token, compared bit for bit with the
//            layer's word; among the edges that attain it the smallest (segment, row, coin_in, coin_out) wins by an integer
//            atomic min on the packed edge (pool number << 6 | coin_in << 3 | coin_out), stored in path order
//   advance  one lane per query: the claimed edge's near token becomes the target of the layer before
//   finish   one lane per query: n_hops, the four hop-major hop arrays, the amount, the status; the pool-repeat check
// Nothing is trusted from device memory that the host did not validate, and what it validated is clamped before it indexes.
#pragma once

#include "../../include/cfmm_amd.h"
#include "quote_path_kernels.h"

namespace cfmm {

static_assert(sizeof(FindSeg) == 192 && kMaxCoins <= 8, "the find table: a PathSeg and half a line; a coin fits 3 bits of an edge");

constexpr unsigned long long kFindNoEdge = ~0ull;

__device__ __forceinline__ int find_clamp_token(int t, int n) { return t < 0 ? 0 : (t >= n ? n - 1 : t); }

// the segment whose tiles (TILE) or pools (!TILE) hold number x: the last record whose first number is <= x
template <bool TILE>
__device__ __forceinline__ int find_segment(const FindSeg* segs, int nseg, long long x)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((TILE ? segs[mid].first_tile : segs[mid].first_pool) <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the token ids of pool `row` (< m) of a segment, the way select_kernels.h reads them; clamped into the token range
__device__ __forceinline__ void find_tokens(const FindSeg& f, int nc, long long m, long long row, int n_tokens, int (&tok)[kMaxCoins])
{
    if (f.tok) {
        for (int k = 0; k < kMaxCoins; ++k) tok[k] = k < nc ? find_clamp_token(f.tok[(long long)k * m + row], n_tokens) : 0;
    } else {
        int2 t;
        if (f.pk) {
            const unsigned w = f.pk[row].tok;
            t = make_int2((int)(w & 0xffffu), (int)(w >> 16));
        } else {
            t = f.Ai[row];
        }
        tok[0] = find_clamp_token(t.x, n_tokens);
        tok[1] = find_clamp_token(t.y, n_tokens);
        for (int k = 2; k < kMaxCoins; ++k) tok[k] = 0;
    }
}

// a quote enters the layers only as a positive finite amount (NaN fails the first comparison)
__device__ __forceinline__ bool find_enters(double r) { return r > 0.0 && r < __builtin_inf(); }

// ---- one search, two directions ----
// OUT false, cfmm_find_path: the layers hold the LARGEST amount that reaches each token from token_in, a hop is quoted with
// quote_one and extends a walk at its END.  OUT true, cfmm_find_path_out: the layers hold the SMALLEST amount that buys the
// wanted output from each token, a hop is quoted with quote_out_one and extends a walk at its START.  FindDir<OUT> is
// everything that differs; the kernels (find_dir_kernels.h) are written once over it.  In every hop `near` is the coin whose token the layer
// before knows (coin_in going forward, coin_out going backward) and `far` the coin the hop reaches.
template <bool OUT>
struct FindDir {
    // the word of a token no walk has reached; the scratch is set to it by a memset (0x00 / 0xff)
    static constexpr unsigned long long kUnreached = OUT ? ~0ull : 0ull;
    // whether a layer word holds an amount.  (Backwards, all-ones is a NaN and only positive finite words are ever written:
    // the scratch is not trusted to say so.)
    static __device__ __forceinline__ bool reached(unsigned long long w)
    {
        if (!OUT) return w != 0;
        return w != kUnreached && find_enters(__longlong_as_double((long long)w));
    }
    // several words of one pool into one that is kUnreached iff all of them are
    static __device__ __forceinline__ unsigned long long gather(unsigned long long acc, unsigned long long w) { return OUT ? acc & w : acc | w; }
    // strictly better: the fold of a layer, and select's "fewest hops among those that attain it"
    static __device__ __forceinline__ bool better(unsigned long long w, unsigned long long than) { return OUT ? w < than : w > than; }
    // One candidate folded into a layer word by a 64-BIT UNSIGNED INTEGER atomic (max forwards, min backwards): positive finite
    // doubles order as their bit patterns and the result does not depend on the order of arrival -- no float atomic.  LDS: the
    // block's own copy (ds_max_u64 / ds_min_u64).  Global: behind a plain look at the word -- the words only improve, so a value
    // that does not beat what is already there (even a stale copy of it) cannot change it, and once a layer has met its good
    // values most candidates stop here (the atomic is what a layer with few tokens is bound by: a million lanes on 256 addresses).
    template <bool LDS>
    static __device__ __forceinline__ void fold(unsigned long long* word, unsigned long long bits)
    {
        if (LDS || better(bits, __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            if (OUT) atomicMin(word, bits);
            else atomicMax(word, bits);
        }
    }
    static __device__ __forceinline__ const int32_t* start_token(const FindArgs& a) { return OUT ? a.token_out : a.token_in; }
    static __device__ __forceinline__ const int32_t* end_token(const FindArgs& a) { return OUT ? a.token_in : a.token_out; }
    // where the hop that joins layer - 1 and layer stands in the path of h_star hops
    static __device__ __forceinline__ int slot(int layer, int h_star) { return OUT ? h_star - layer : layer - 1; }
    // the answer without a path: nothing comes out; nothing need be paid for nothing, else no amount buys it
    static __device__ __forceinline__ double none(double given) { return !OUT ? 0.0 : (given == 0.0 ? 0.0 : __builtin_inf()); }
};

// one hop of the search from its near coin to its far coin (row and coins are in range by construction, amt > 0 and finite);
// a segment of no kind reaches nothing
template <bool OUT>
__device__ __forceinline__ double find_quote(const PathSeg& s, int kind, long long m, long long row, int near, int far, double amt)
{
    const int ci = OUT ? far : near, co = OUT ? near : far;
    double r;
    with_kind(kind, [&](auto K) { r = path_hop<decltype(K)::value, OUT>(s, m, row, ci, co, amt); }, [&] { r = OUT ? __builtin_inf() : 0.0; });
    return r;
}

__device__ __forceinline__ unsigned long long find_pack(long long pool, int near, int far, bool out)
{
    return ((unsigned long long)pool << 6) | ((unsigned long long)(out ? far : near) << 3) | (unsigned long long)(out ? near : far);
}

// a claimed edge as (segment, row, coin_in, coin_out); false: no edge, or one that is no pool of the table
__device__ __forceinline__ bool find_decode(const FindArgs& a, unsigned long long e, int& sg, long long& row, int& ci, int& co)
{
    if (e == kFindNoEdge) return false;
    const long long pool = (long long)(e >> 6);
    ci = (int)((e >> 3) & 7);
    co = (int)(e & 7);
    sg = find_segment<false>(a.segs, a.nseg, pool);
    row = pool - a.segs[sg].first_pool;
    return a.segs[sg].s.kind >= 0 && row >= 0 && row < a.segs[sg].s.m && ci < a.segs[sg].s.n_coins && co < a.segs[sg].s.n_coins;
}

// The 14 entries launch_find names (the relax kernels twice each, with and without the LDS copy), in the order the translation
// unit has always emitted them: find_dir_kernels.h, once per direction.
#define CFMM_FIND_OUT false
#define CFMM_FIND(role) find_##role
#include "find_dir_kernels.h"
#undef CFMM_FIND_OUT
#undef CFMM_FIND
#define CFMM_FIND_OUT true
#define CFMM_FIND(role) find_out_##role
#include "find_dir_kernels.h"
#undef CFMM_FIND_OUT
#undef CFMM_FIND

} // namespace cfmm

// The header that comes LAST in sweep_kernels.hip stays this one (tests/test_find_path_cpu.py pins that, so that new templates are
// emitted behind every kernel the translation unit had); what came after it is included from here, behind everything above.
#include "size_path_kernels.h"
