// find_path_kernels.h -- cfmm_find_path: the best swap WALK of at most max_hops hops between two tokens, found on the device.
// The layered form of the search: best[0][token_in] = amount_in, and best[h][t] is the largest quote_one<KIND>(pool, ci -> co,
// best[h-1][tok(ci)]) over every pool of every segment and every ordered coin pair whose tok(co) is t and whose source is
// reached.  Every hop is quoted against the pool AS IT STANDS (cfmm_quote_path's rule); a walk may visit a pool twice.
//   find_init     one lane per query: best[0][q][token_in] <- amount_in (the scratch was cleared by a memset)
//   find_relax    THE HOT PATH, one launch per layer, ONE LANE PER POOL of every segment (a block finds its segment in the
//                 table by its tile number).  A lane reads its pool's token ids (8 bytes; 4 per coin of a ragged pool), then the
//                 best[h-1] words of those tokens for the queries of its group, and leaves when none is reached -- a wavefront
//                 without any reached lane leaves on one ballot, before any pool state is read.  For every reached (query, ci)
//                 and every co != ci it evaluates path_hop<KIND> (quote_path_kernels.h: quote_one<KIND>'s body, so the bits are
//                 cfmm_quote's) and folds the answer into best[h][q][tok(co)] with a 64-BIT UNSIGNED INTEGER atomic max on the
//                 double's bits: non-negative finite doubles order as their bit patterns, 0 bits = unreached, and an integer
//                 max does not depend on the order of arrival -- there is still no global float atomic.  Where a group of
//                 queries' layer rows fit the LDS, a block first folds several tiles into its own copy (ds_max_u64).
//   find_select   one lane per query: amount_out = max over h >= 1 of best[h][q][token_out], the FEWEST hops that attain it
//   find_claim    walking back, one launch per layer from the last: one lane per pool again, but only a lane whose pool holds
//                 the CURRENT TARGET token of some query evaluates anything -- the quotes INTO that token, compared bit for bit
//                 with best[h][target]; among the edges that attain it the smallest (segment, row, coin_in, coin_out) wins by
//                 an integer atomic min on the packed edge (pool number << 6 | coin_in << 3 | coin_out)
//   find_advance  one lane per query: the claimed edge's coin_in token becomes the target of the layer before
//   find_finish   one lane per query: n_hops, the four hop-major hop arrays, amount_out, the status; the pool-repeat check
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

// one hop of the search: path_step's switch on the kind (row and coins are in range by construction, amt > 0 and finite)
__device__ __forceinline__ double find_quote(const PathSeg& s, int kind, long long m, long long row, int ci, int co, double amt)
{
    switch (kind) {
    case CFMM_KIND_PRODUCT: return path_hop<CFMM_KIND_PRODUCT, false>(s, m, row, ci, co, amt);
    case CFMM_KIND_GEOMEAN: return path_hop<CFMM_KIND_GEOMEAN, false>(s, m, row, ci, co, amt);
    case CFMM_KIND_UNIV3: return path_hop<CFMM_KIND_UNIV3, false>(s, m, row, ci, co, amt);
    case CFMM_KIND_WEIGHTED: return path_hop<CFMM_KIND_WEIGHTED, false>(s, m, row, ci, co, amt);
    case CFMM_KIND_CURVE: return path_hop<CFMM_KIND_CURVE, false>(s, m, row, ci, co, amt);
    case CFMM_KIND_SOLIDLY: return path_hop<CFMM_KIND_SOLIDLY, false>(s, m, row, ci, co, amt);
    default: return 0.0;
    }
}

// a quote enters the layers only as a positive finite amount (NaN fails the first comparison)
__device__ __forceinline__ bool find_enters(double r) { return r > 0.0 && r < __builtin_inf(); }

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_init(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const double x = a.amount_in[q];
    const int t = a.token_in[q];
    if (find_enters(x) && t >= 0 && t < a.n_tokens) a.best[q * a.n_tokens + t] = (unsigned long long)__double_as_longlong(x);
}

// One candidate folded into a layer word.  LDS: the block's own copy (ds_max_u64).  Global: an integer atomic max behind a
// plain look at the word -- the words only grow, so a value that does not beat what is already there (even a stale copy of it)
// cannot change it, and once a layer has met its large values most candidates stop here (the atomic is what a layer with few
// tokens is bound by: a million lanes on 256 addresses).
template <bool LDS>
__device__ __forceinline__ void find_fold(unsigned long long* word, unsigned long long bits)
{
    if (LDS) atomicMax(word, bits);
    else if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
}

// layer a.layer (1 .. max_hops) from the layer before.
//   LDS = false: grid = (tiles of every segment, query groups of kFindLaneQueries); every candidate goes to the layer in
//                global memory.
//   LDS = true (n_tokens x a.group words fit the block's LDS): grid = (tiles / a.tiles_per_block, query groups of a.group); the
//                block folds the candidates of its tiles into its own copy of the group's layer rows and then folds the
//                copy's reached words into global memory -- tiles_per_block x BLOCK x coin pairs candidates become at most
//                n_tokens atomics per query.  The same integer maxima either way: the result cannot differ.
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void find_relax(FindArgs a)
{
    extern __shared__ unsigned long long find_rows[];   // [group][n_tokens], LDS only
    const int group = LDS ? a.group : kFindLaneQueries;
    const long long q0 = (long long)blockIdx.y * group;
    const int nq = (int)(a.count - q0 < group ? a.count - q0 : group);
    const long long layer_words = a.count * (long long)a.n_tokens;
    const unsigned long long* prev = a.best + (long long)(a.layer - 1) * layer_words + q0 * a.n_tokens;
    unsigned long long* cur = a.best + (long long)a.layer * layer_words + q0 * a.n_tokens;
    unsigned long long* into = LDS ? find_rows : cur;
    const int words = nq * a.n_tokens;
    if (LDS) {
        for (int i = threadIdx.x; i < words; i += BLOCK) find_rows[i] = 0;
        __syncthreads();
    }
    const long long per_block = LDS ? a.tiles_per_block : 1;
    const long long tile0 = (long long)blockIdx.x * per_block;
    const long long tile1 = tile0 + per_block < a.tiles ? tile0 + per_block : a.tiles;
    for (long long tile = tile0; tile < tile1; ++tile) {
        const int sg = find_segment<true>(a.segs, a.nseg, tile);
        const FindSeg& f = a.segs[sg];
        const int kind = f.s.kind;
        const int nc = f.s.n_coins < 2 ? 2 : (f.s.n_coins > kMaxCoins ? kMaxCoins : f.s.n_coins);
        const long long m = f.s.m;
        const long long row = (tile - f.first_tile) * BLOCK + threadIdx.x;
        int tok[kMaxCoins];
        unsigned long long reached = 0;   // bit j: some coin of this pool is reached in query q0 + j
        const bool live = kind >= 0 && row >= 0 && row < m;
        if (live) {
            find_tokens(f, nc, m, row, a.n_tokens, tok);
            for (int j = 0; j < nq; ++j) {
                unsigned long long any = 0;
                for (int k = 0; k < nc; ++k) any |= prev[(long long)j * a.n_tokens + tok[k]];
                reached |= (unsigned long long)(any != 0) << j;
            }
        }
        if (__ballot(reached != 0) == 0) continue;   // the whole wavefront: no pool state was touched
        while (reached) {
            const int j = __builtin_ctzll(reached);
            reached &= reached - 1;
            const unsigned long long* pj = prev + (long long)j * a.n_tokens;
            unsigned long long* cj = into + (long long)j * a.n_tokens;
            for (int ci = 0; ci < nc; ++ci) {
                const unsigned long long bits = pj[tok[ci]];
                if (!bits) continue;
                const double amt = __longlong_as_double((long long)bits);
                for (int co = 0; co < nc; ++co) {
                    if (co == ci) continue;
                    const double r = find_quote(f.s, kind, m, row, ci, co, amt);
                    if (find_enters(r)) find_fold<LDS>(cj + tok[co], (unsigned long long)__double_as_longlong(r));
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += BLOCK) {
            const unsigned long long bits = find_rows[i];
            if (bits) find_fold<false>(cur + i, bits);
        }
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_select(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const int t = a.token_out[q];
    const long long layer_words = a.count * (long long)a.n_tokens;
    unsigned long long top = 0;
    int h_star = 0;
    if (t >= 0 && t < a.n_tokens)
        for (int h = 1; h <= a.max_hops; ++h) {
            const unsigned long long b = a.best[(long long)h * layer_words + q * a.n_tokens + t];
            if (b > top) {   // strictly: the fewest hops among those that attain the maximum
                top = b;
                h_star = h;
            }
        }
    a.h_star[q] = h_star;
    a.target[q] = h_star ? t : -1;
}

// the hop that ends layer a.layer: grid as find_relax.  Only a lane whose pool holds a query's target evaluates anything.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_claim(FindArgs a)
{
    const int sg = find_segment<true>(a.segs, a.nseg, blockIdx.x);
    const FindSeg& f = a.segs[sg];
    const int kind = f.s.kind;
    const int nc = f.s.n_coins < 2 ? 2 : (f.s.n_coins > kMaxCoins ? kMaxCoins : f.s.n_coins);
    const long long m = f.s.m;
    const long long row = ((long long)blockIdx.x - f.first_tile) * BLOCK + threadIdx.x;
    if (kind < 0 || row < 0 || row >= m) return;
    const long long q0 = (long long)blockIdx.y * kFindLaneQueries;
    const int nq = (int)(a.count - q0 < kFindLaneQueries ? a.count - q0 : kFindLaneQueries);
    const long long layer_words = a.count * (long long)a.n_tokens;
    int tok[kMaxCoins];
    find_tokens(f, nc, m, row, a.n_tokens, tok);
    for (int j = 0; j < nq; ++j) {
        const long long q = q0 + j;
        if (a.h_star[q] < a.layer) continue;
        const int t = a.target[q];
        if (t < 0 || t >= a.n_tokens) continue;
        const unsigned long long* pj = a.best + (long long)(a.layer - 1) * layer_words + q * a.n_tokens;
        unsigned long long want = 0;
        bool have = false;
        for (int co = 0; co < nc; ++co) {
            if (tok[co] != t) continue;
            if (!have) {
                want = a.best[(long long)a.layer * layer_words + q * a.n_tokens + t];
                have = true;
            }
            for (int ci = 0; ci < nc; ++ci) {
                if (ci == co) continue;
                const unsigned long long bits = pj[tok[ci]];
                if (!bits) continue;
                const double r = find_quote(f.s, kind, m, row, ci, co, __longlong_as_double((long long)bits));
                if (find_enters(r) && (unsigned long long)__double_as_longlong(r) == want)
                    atomicMin(a.edge + (long long)(a.layer - 1) * a.count + q,
                              ((unsigned long long)(f.first_pool + row) << 6) | ((unsigned long long)ci << 3) | (unsigned long long)co);
            }
        }
    }
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

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_advance(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count || a.h_star[q] < a.layer) return;
    int sg, ci, co;
    long long row;
    int t = -1;
    if (find_decode(a, a.edge[(long long)(a.layer - 1) * a.count + q], sg, row, ci, co)) {
        const FindSeg& f = a.segs[sg];
        int tok[kMaxCoins];
        find_tokens(f, f.s.n_coins, f.s.m, row, a.n_tokens, tok);
        t = tok[ci];
    }
    a.target[q] = t;   // -1: nothing claims from here on, and find_finish answers that no path was found
}

// outputs of query q at q (per query) and k*stride + q (hop k): the pointers already stand at the chunk's first query
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_finish(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    int h = a.h_star[q];
    h = h < 0 ? 0 : (h > a.max_hops ? a.max_hops : h);
    int sg[CFMM_MAX_PATH_HOPS], ci[CFMM_MAX_PATH_HOPS], co[CFMM_MAX_PATH_HOPS];
    long long row[CFMM_MAX_PATH_HOPS];
    bool whole = h > 0;
    for (int k = 0; k < CFMM_MAX_PATH_HOPS; ++k) {
        sg[k] = ci[k] = co[k] = -1;
        row[k] = -1;
        if (k < h && whole) whole = find_decode(a, a.edge[(long long)k * a.count + q], sg[k], row[k], ci[k], co[k]);
    }
    if (!whole) h = 0;
    bool repeats = false;
    for (int k = 1; k < CFMM_MAX_PATH_HOPS; ++k)
        for (int i = 0; i < k; ++i) repeats = repeats || (k < h && sg[i] == sg[k] && row[i] == row[k]);
    for (int k = 0; k < a.max_hops; ++k) {
        const long long at = (long long)k * a.stride + q;
        const bool used = k < h;
        a.hop_seg[at] = used ? sg[k] : -1;
        a.hop_row[at] = used ? row[k] : -1;
        a.hop_coin_in[at] = used ? ci[k] : -1;
        a.hop_coin_out[at] = used ? co[k] : -1;
    }
    const long long layer_words = a.count * (long long)a.n_tokens;
    const int t = find_clamp_token(a.token_out[q], a.n_tokens);
    a.n_hops[q] = h;
    a.amount_out[q] = h ? __longlong_as_double((long long)a.best[(long long)h * layer_words + q * a.n_tokens + t]) : 0.0;
    a.status[q] = !h ? CFMM_FOUND_NONE : (repeats ? CFMM_FOUND_REPEATS : CFMM_FOUND);
}

// ---- cfmm_find_path_out: the cheapest walk that BUYS an exact amount, the same search run backwards from the wanted output ----
// need[0][token_out] = amount_out, and need[h][t] is the SMALLEST quote_out_one<KIND>(pool, ci -> co, need[h-1][tok(co)]) over
// every pool of every segment and every ordered coin pair whose tok(ci) is t and whose destination is reached.  FindArgs serves
// with the amounts' roles exchanged, as PathArgs serves both quote directions: a.amount_in carries the wanted amount_out,
// a.amount_out receives the amount to tender, a.best holds need -- a positive finite double's bits, ALL ONES = unreached (the
// scratch is set by a memset of 0xff), so that the fold is a 64-BIT UNSIGNED INTEGER atomic min: still no float atomic.
//   find_out_init     one lane per query: need[0][q][token_out] <- amount_out
//   find_out_relax    THE HOT PATH: find_relax's grid, tiles and ballot early-out (a wavefront none of whose pools holds a reached
//                     DESTINATION leaves before any pool state is read).  For every reached (query, co) and every ci != co it
//                     evaluates path_hop<KIND, true> (quote_out_one<KIND>'s body, so the bits are cfmm_quote_out's) and folds the
//                     answer into need[h][q][tok(ci)]; +inf ("that pool cannot give that much") enters nothing.  The LDS copy
//                     (ds_min_u64) starts at all ones, under find_relax's group and tiles_per_block rule.
//   find_out_select   one lane per query: amount_in = min over h >= 1 of need[h][q][token_in], the FEWEST hops that attain it
//   find_out_claim    walking FORWARD from (h*, token_in), one launch per layer from h* down: one lane per pool, but only a lane
//                     whose pool holds the CURRENT token of some query evaluates anything -- the quotes OUT OF that token, compared
//                     bit for bit with need[h][current]; the smallest (segment, row, coin_in, coin_out) wins by an integer atomic
//                     min on the packed edge, which lands in the hop's slot in PATH ORDER (hop k = h* - layer)
//   find_out_advance  one lane per query: the claimed edge's coin_out token becomes the current token of the layer below
//   find_out_finish   one lane per query: as find_finish; no path: amount_in +0.0 where amount_out is 0 (nothing to buy), else +inf
constexpr unsigned long long kFindUnreached = ~0ull;

__device__ __forceinline__ double find_quote_out(const PathSeg& s, int kind, long long m, long long row, int ci, int co, double amt)
{
    switch (kind) {
    case CFMM_KIND_PRODUCT: return path_hop<CFMM_KIND_PRODUCT, true>(s, m, row, ci, co, amt);
    case CFMM_KIND_GEOMEAN: return path_hop<CFMM_KIND_GEOMEAN, true>(s, m, row, ci, co, amt);
    case CFMM_KIND_UNIV3: return path_hop<CFMM_KIND_UNIV3, true>(s, m, row, ci, co, amt);
    case CFMM_KIND_WEIGHTED: return path_hop<CFMM_KIND_WEIGHTED, true>(s, m, row, ci, co, amt);
    case CFMM_KIND_CURVE: return path_hop<CFMM_KIND_CURVE, true>(s, m, row, ci, co, amt);
    case CFMM_KIND_SOLIDLY: return path_hop<CFMM_KIND_SOLIDLY, true>(s, m, row, ci, co, amt);
    default: return __builtin_inf();
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_out_init(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const double y = a.amount_in[q];   // (the wanted amount_out)
    const int t = a.token_out[q];
    if (find_enters(y) && t >= 0 && t < a.n_tokens) a.best[q * a.n_tokens + t] = (unsigned long long)__double_as_longlong(y);
}

// find_fold's mirror: the words only shrink, so a value that does not undercut what is already there cannot change it
template <bool LDS>
__device__ __forceinline__ void find_fold_min(unsigned long long* word, unsigned long long bits)
{
    if (LDS) atomicMin(word, bits);
    else if (bits < __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(word, bits);
}

// layer a.layer (1 .. max_hops) from the layer before; the two grids are find_relax's
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void find_out_relax(FindArgs a)
{
    extern __shared__ unsigned long long find_rows[];   // [group][n_tokens], LDS only
    const int group = LDS ? a.group : kFindLaneQueries;
    const long long q0 = (long long)blockIdx.y * group;
    const int nq = (int)(a.count - q0 < group ? a.count - q0 : group);
    const long long layer_words = a.count * (long long)a.n_tokens;
    const unsigned long long* prev = a.best + (long long)(a.layer - 1) * layer_words + q0 * a.n_tokens;
    unsigned long long* cur = a.best + (long long)a.layer * layer_words + q0 * a.n_tokens;
    unsigned long long* into = LDS ? find_rows : cur;
    const int words = nq * a.n_tokens;
    if (LDS) {
        for (int i = threadIdx.x; i < words; i += BLOCK) find_rows[i] = kFindUnreached;
        __syncthreads();
    }
    const long long per_block = LDS ? a.tiles_per_block : 1;
    const long long tile0 = (long long)blockIdx.x * per_block;
    const long long tile1 = tile0 + per_block < a.tiles ? tile0 + per_block : a.tiles;
    for (long long tile = tile0; tile < tile1; ++tile) {
        const int sg = find_segment<true>(a.segs, a.nseg, tile);
        const FindSeg& f = a.segs[sg];
        const int kind = f.s.kind;
        const int nc = f.s.n_coins < 2 ? 2 : (f.s.n_coins > kMaxCoins ? kMaxCoins : f.s.n_coins);
        const long long m = f.s.m;
        const long long row = (tile - f.first_tile) * BLOCK + threadIdx.x;
        int tok[kMaxCoins];
        unsigned long long reached = 0;   // bit j: some coin of this pool is a reached destination in query q0 + j
        const bool live = kind >= 0 && row >= 0 && row < m;
        if (live) {
            find_tokens(f, nc, m, row, a.n_tokens, tok);
            for (int j = 0; j < nq; ++j) {
                unsigned long long all = kFindUnreached;
                for (int k = 0; k < nc; ++k) all &= prev[(long long)j * a.n_tokens + tok[k]];
                reached |= (unsigned long long)(all != kFindUnreached) << j;
            }
        }
        if (__ballot(reached != 0) == 0) continue;   // the whole wavefront: no pool state was touched
        while (reached) {
            const int j = __builtin_ctzll(reached);
            reached &= reached - 1;
            const unsigned long long* pj = prev + (long long)j * a.n_tokens;
            unsigned long long* cj = into + (long long)j * a.n_tokens;
            for (int co = 0; co < nc; ++co) {
                const unsigned long long bits = pj[tok[co]];
                if (bits == kFindUnreached) continue;
                const double amt = __longlong_as_double((long long)bits);
                if (!find_enters(amt)) continue;   // (only such words are ever written; the scratch is not trusted to say so)
                for (int ci = 0; ci < nc; ++ci) {
                    if (ci == co) continue;
                    const double r = find_quote_out(f.s, kind, m, row, ci, co, amt);
                    if (find_enters(r)) find_fold_min<LDS>(cj + tok[ci], (unsigned long long)__double_as_longlong(r));
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += BLOCK) {
            const unsigned long long bits = find_rows[i];
            if (bits != kFindUnreached) find_fold_min<false>(cur + i, bits);
        }
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_out_select(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const int t = a.token_in[q];
    const long long layer_words = a.count * (long long)a.n_tokens;
    unsigned long long low = kFindUnreached;
    int h_star = 0;
    if (t >= 0 && t < a.n_tokens)
        for (int h = 1; h <= a.max_hops; ++h) {
            const unsigned long long b = a.best[(long long)h * layer_words + q * a.n_tokens + t];
            if (b < low) {   // strictly: the fewest hops among those that attain the minimum
                low = b;
                h_star = h;
            }
        }
    a.h_star[q] = h_star;
    a.target[q] = h_star ? t : -1;
}

// the hop that LEAVES layer a.layer: grid as find_out_relax without the LDS copy.  Only a lane whose pool holds a query's
// current token evaluates anything.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_out_claim(FindArgs a)
{
    const int sg = find_segment<true>(a.segs, a.nseg, blockIdx.x);
    const FindSeg& f = a.segs[sg];
    const int kind = f.s.kind;
    const int nc = f.s.n_coins < 2 ? 2 : (f.s.n_coins > kMaxCoins ? kMaxCoins : f.s.n_coins);
    const long long m = f.s.m;
    const long long row = ((long long)blockIdx.x - f.first_tile) * BLOCK + threadIdx.x;
    if (kind < 0 || row < 0 || row >= m) return;
    const long long q0 = (long long)blockIdx.y * kFindLaneQueries;
    const int nq = (int)(a.count - q0 < kFindLaneQueries ? a.count - q0 : kFindLaneQueries);
    const long long layer_words = a.count * (long long)a.n_tokens;
    int tok[kMaxCoins];
    find_tokens(f, nc, m, row, a.n_tokens, tok);
    for (int j = 0; j < nq; ++j) {
        const long long q = q0 + j;
        const int hs = a.h_star[q];
        if (hs < a.layer || hs > a.max_hops) continue;
        const int t = a.target[q];
        if (t < 0 || t >= a.n_tokens) continue;
        const unsigned long long* pj = a.best + (long long)(a.layer - 1) * layer_words + q * a.n_tokens;
        unsigned long long want = 0;
        bool have = false;
        for (int ci = 0; ci < nc; ++ci) {
            if (tok[ci] != t) continue;
            if (!have) {
                want = a.best[(long long)a.layer * layer_words + q * a.n_tokens + t];
                have = true;
            }
            for (int co = 0; co < nc; ++co) {
                if (co == ci) continue;
                const unsigned long long bits = pj[tok[co]];
                if (bits == kFindUnreached) continue;
                const double amt = __longlong_as_double((long long)bits);
                if (!find_enters(amt)) continue;
                const double r = find_quote_out(f.s, kind, m, row, ci, co, amt);
                if (find_enters(r) && (unsigned long long)__double_as_longlong(r) == want)
                    atomicMin(a.edge + (long long)(hs - a.layer) * a.count + q,
                              ((unsigned long long)(f.first_pool + row) << 6) | ((unsigned long long)ci << 3) | (unsigned long long)co);
            }
        }
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_out_advance(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const int hs = a.h_star[q];
    if (hs < a.layer || hs > a.max_hops) return;
    int sg, ci, co;
    long long row;
    int t = -1;
    if (find_decode(a, a.edge[(long long)(hs - a.layer) * a.count + q], sg, row, ci, co)) {
        const FindSeg& f = a.segs[sg];
        int tok[kMaxCoins];
        find_tokens(f, f.s.n_coins, f.s.m, row, a.n_tokens, tok);
        t = tok[co];
    }
    a.target[q] = t;   // -1: nothing claims from here on, and find_out_finish answers that no path was found
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void find_out_finish(FindArgs a)
{
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    int h = a.h_star[q];
    h = h < 0 ? 0 : (h > a.max_hops ? a.max_hops : h);
    int sg[CFMM_MAX_PATH_HOPS], ci[CFMM_MAX_PATH_HOPS], co[CFMM_MAX_PATH_HOPS];
    long long row[CFMM_MAX_PATH_HOPS];
    bool whole = h > 0;
    for (int k = 0; k < CFMM_MAX_PATH_HOPS; ++k) {
        sg[k] = ci[k] = co[k] = -1;
        row[k] = -1;
        if (k < h && whole) whole = find_decode(a, a.edge[(long long)k * a.count + q], sg[k], row[k], ci[k], co[k]);
    }
    if (!whole) h = 0;
    bool repeats = false;
    for (int k = 1; k < CFMM_MAX_PATH_HOPS; ++k)
        for (int i = 0; i < k; ++i) repeats = repeats || (k < h && sg[i] == sg[k] && row[i] == row[k]);
    for (int k = 0; k < a.max_hops; ++k) {
        const long long at = (long long)k * a.stride + q;
        const bool used = k < h;
        a.hop_seg[at] = used ? sg[k] : -1;
        a.hop_row[at] = used ? row[k] : -1;
        a.hop_coin_in[at] = used ? ci[k] : -1;
        a.hop_coin_out[at] = used ? co[k] : -1;
    }
    const long long layer_words = a.count * (long long)a.n_tokens;
    const int t = find_clamp_token(a.token_in[q], a.n_tokens);
    a.n_hops[q] = h;
    a.amount_out[q] = h ? __longlong_as_double((long long)a.best[(long long)h * layer_words + q * a.n_tokens + t])
                        : (a.amount_in[q] == 0.0 ? 0.0 : __builtin_inf());   // (the amount to tender)
    a.status[q] = !h ? CFMM_FOUND_NONE : (repeats ? CFMM_FOUND_REPEATS : CFMM_FOUND);
}

} // namespace cfmm

// The header that comes LAST in sweep_kernels.hip stays this one (tests/test_find_path_cpu.py pins that, so that new templates are
// emitted behind every kernel the translation unit had); what came after it is included from here, behind everything above.
#include "size_path_kernels.h"
