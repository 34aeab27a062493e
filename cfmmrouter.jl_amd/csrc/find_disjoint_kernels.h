// find_disjoint_kernels.h -- cfmm_find_disjoint_paths: up to 8 paths per query that share no pool, by SUCCESSIVE runs of
// cfmm_find_path's layered search (find_path_kernels.h; cfmm_find_disjoint_paths_out: of cfmm_find_path_out's) in which every pool of the query's earlier paths is
// ABSENT.  The ban is a bitmap in device memory: one row of ban_words 64-bit words per query of the chunk, bit p & 63 of word
// p >> 6 for pool number p = first_pool + row -- the number find_pack packs into an edge.  Round r is
//   find_ban_init     find_init, but a query that has ENDED (an earlier round found nothing for it) puts nothing into layer 0:
//                     its layers stay unreached, every lane of every later launch leaves on the ballot or on h_star == 0, and
//                     the query costs no quote
//   find_ban_relax    find_relax with one addition: for a query whose bit is set in the lane's `reached` mask the lane looks at
//                     its pool's ban bit BEFORE it quotes anything for that query.  It stands behind the wave-wide ballot, so a
//                     wavefront that reaches nothing still leaves before it touches anything; the 64 pools of a wavefront read
//                     one or two words of a query's row.  Round 0 has nothing banned and does not look.
//   find_select       unchanged
//   find_ban_claim    find_claim with the same test before a pool may attain a layer word: a banned pool whose quote ties the
//                     word bit for bit is not claimed
//   find_advance      unchanged
//   find_ban_finish   find_finish into slot r of the outputs (the host hands it FindArgs whose output pointers stand at the
//                     slot), and: the path's pools are ORed into the query's ban row, the query is marked ended when nothing
//                     was found, n_paths is written (round 0) or incremented.  ONE LANE OWNS ITS QUERY'S ROW, so plain loads
//                     and vector stores do: no atomics.
// cfmm_find_disjoint_paths_out is the same with the direction turned (find_out_ban_init .. find_out_ban_finish; select and advance
// are find_out_select and find_out_advance, unchanged): the text of the four kernels stands ONCE, in the second half of THIS
// file, which includes itself once per direction as find_path_kernels.h includes find_dir_kernels.h: with CFMM_FIND_BAN
// defined an inclusion yields the kernels' text alone, CFMM_FIND_OUT the direction and CFMM_FIND_BAN(role) the kernel's name
// (find_ban_init .. find_ban_finish, find_out_ban_init .. find_out_ban_finish).  Everything that differs between the directions
// is FindDir<OUT> (find_path_kernels.h), used exactly as find_dir_kernels.h uses it.  With OUT false every line is the forward
// kernel's as it was: the four forward kernels compile to the instructions they had.  The existing fourteen search kernels
// are not touched: FindArgs is theirs, what the ban needs travels in FindBanArgs.
#if !defined(CFMM_FIND_BAN)   /* ---- the header proper, once ---- */
#ifndef CFMM_FIND_DISJOINT_KERNELS_H
#define CFMM_FIND_DISJOINT_KERNELS_H

#include "find_path_kernels.h"

namespace cfmm {

__device__ __forceinline__ bool find_banned(const FindBanArgs& b, long long q, long long pool)
{
    return (b.ban[q * b.ban_words + (pool >> 6)] >> (pool & 63)) & 1ull;
}

#define CFMM_FIND_OUT false
#define CFMM_FIND_BAN(role) find_ban_##role
#include "find_disjoint_kernels.h"
#undef CFMM_FIND_OUT
#undef CFMM_FIND_BAN
#define CFMM_FIND_OUT true
#define CFMM_FIND_BAN(role) find_out_ban_##role
#include "find_disjoint_kernels.h"
#undef CFMM_FIND_OUT
#undef CFMM_FIND_BAN

} // namespace cfmm

// (what came after this header is included from here, behind everything above: find_path_kernels.h's rule)
#include "split_paths_out_kernels.h"

#endif
#else   /* ---- the four kernels' text, once per direction (inside namespace cfmm) ---- */

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND_BAN(init)(FindArgs a, FindBanArgs b)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    if (b.round > 0 && b.ended[q]) return;
    const double x = a.amount_in[q];   // (backwards: the wanted amount_out)
    const int t = D::start_token(a)[q];
    if (find_enters(x) && t >= 0 && t < a.n_tokens) a.best[q * a.n_tokens + t] = (unsigned long long)__double_as_longlong(x);
}

// find_relax's grids and LDS copy (find_dir_kernels.h); a pool's number is < the table's pools, so its word is < ban_words
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND_BAN(relax)(FindArgs a, FindBanArgs b)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
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
        for (int i = threadIdx.x; i < words; i += BLOCK) find_rows[i] = D::kUnreached;
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
                unsigned long long any = D::kUnreached;
                for (int k = 0; k < nc; ++k) any = D::gather(any, prev[(long long)j * a.n_tokens + tok[k]]);
                reached |= (unsigned long long)(any != D::kUnreached) << j;
            }
        }
        if (__ballot(reached != 0) == 0) continue;   // the whole wavefront: neither pool state nor a ban word was touched
        while (reached) {
            const int j = __builtin_ctzll(reached);
            reached &= reached - 1;
            if (b.round > 0 && find_banned(b, q0 + j, f.first_pool + row)) continue;   // absent for this query
            const unsigned long long* pj = prev + (long long)j * a.n_tokens;
            unsigned long long* cj = into + (long long)j * a.n_tokens;
            for (int near = 0; near < nc; ++near) {
                const unsigned long long bits = pj[tok[near]];
                if (!D::reached(bits)) continue;
                const double amt = __longlong_as_double((long long)bits);
                for (int far = 0; far < nc; ++far) {
                    if (far == near) continue;
                    const double r = find_quote<OUT>(f.s, kind, m, row, near, far, amt);
                    if (find_enters(r)) D::template fold<LDS>(cj + tok[far], (unsigned long long)__double_as_longlong(r));
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += BLOCK) {
            const unsigned long long bits = find_rows[i];
            if (bits != D::kUnreached) D::template fold<false>(cur + i, bits);
        }
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND_BAN(claim)(FindArgs a, FindBanArgs b)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
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
        if (hs < a.layer || (OUT && hs > a.max_hops)) continue;
        const int t = a.target[q];
        if (t < 0 || t >= a.n_tokens) continue;
        const unsigned long long* pj = a.best + (long long)(a.layer - 1) * layer_words + q * a.n_tokens;
        unsigned long long want = 0;
        bool have = false;
        for (int far = 0; far < nc; ++far) {
            if (tok[far] != t) continue;
            if (!have) {
                if (b.round > 0 && find_banned(b, q, f.first_pool + row)) break;   // absent for this query: it attains nothing
                want = a.best[(long long)a.layer * layer_words + q * a.n_tokens + t];
                have = true;
            }
            for (int near = 0; near < nc; ++near) {
                if (near == far) continue;
                const unsigned long long bits = pj[tok[near]];
                if (!D::reached(bits)) continue;
                const double r = find_quote<OUT>(f.s, kind, m, row, near, far, __longlong_as_double((long long)bits));
                if (find_enters(r) && (unsigned long long)__double_as_longlong(r) == want)
                    atomicMin(a.edge + (long long)D::slot(a.layer, hs) * a.count + q, find_pack(f.first_pool + row, near, far, OUT));
            }
        }
    }
}

// find_finish (the outputs of query q at q and k*stride + q of pointers that stand at slot r and the chunk's first query), then
// the ban row, the ended mark and n_paths
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND_BAN(finish)(FindArgs a, FindBanArgs b)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
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
    const int t = find_clamp_token(D::end_token(a)[q], a.n_tokens);
    a.n_hops[q] = h;
    a.amount_out[q] = h ? __longlong_as_double((long long)a.best[(long long)h * layer_words + q * a.n_tokens + t]) : D::none(a.amount_in[q]);
    a.status[q] = !h ? CFMM_FOUND_NONE : (repeats ? CFMM_FOUND_REPEATS : CFMM_FOUND);
    // the path's pools leave the market of this query's later rounds (find_decode accepted each: the number is a pool's)
    for (int k = 0; k < CFMM_MAX_PATH_HOPS; ++k)
        if (k < h) {
            const long long pool = a.segs[sg[k]].first_pool + row[k];
            b.ban[q * b.ban_words + (pool >> 6)] |= 1ull << (pool & 63);
        }
    b.ended[q] = h == 0;
    b.n_paths[q] = (b.round > 0 ? b.n_paths[q] : 0) + (h != 0);
}

#endif
