// find_dir_kernels.h -- the six kernels of the path search, ONE text, included once per direction by find_path_kernels.h with
// CFMM_FIND_OUT the direction (false: cfmm_find_path, true: cfmm_find_path_out) and CFMM_FIND(role) the kernel's name
// (find_init .. find_finish, find_out_init .. find_out_finish).  Everything that differs between the directions is
// FindDir<OUT> (find_path_kernels.h).  The text stands in the __global__ functions themselves and not in bodies behind one-line
// wrappers, because a wrapper costs these kernels their loads' address spaces: inlined into a wrapper, the layer kernels with
// the LDS copy and the claim kernel read pool streams and token words with flat loads instead of global loads (the pointers a
// kernel loads from the segment table are no longer proved to be global), the finish kernel is unrolled differently, and the
// layer and walk launches ran 0.1 .. 0.4 % slower than the parent's (profiles/query_kernels_refactor.txt).
// No include guard: the second inclusion is the point.

// one lane per query: layer 0 of the start token <- the amount given
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(init)(FindArgs a)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const double x = a.amount_in[q];   // (backwards: the wanted amount_out)
    const int t = D::start_token(a)[q];
    if (find_enters(x) && t >= 0 && t < a.n_tokens) a.best[q * a.n_tokens + t] = (unsigned long long)__double_as_longlong(x);
}

// layer a.layer (1 .. max_hops) from the layer before.
//   LDS = false: grid = (tiles of every segment, query groups of kFindLaneQueries); every candidate goes to the layer in
//                global memory.
//   LDS = true (n_tokens x a.group words fit the block's LDS): grid = (tiles / a.tiles_per_block, query groups of a.group); the
//                block folds the candidates of its tiles into its own copy of the group's layer rows and then folds the
//                copy's reached words into global memory -- tiles_per_block x BLOCK x coin pairs candidates become at most
//                n_tokens atomics per query.  The same integer extrema either way: the result cannot differ.
template <int BLOCK, bool LDS>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(relax)(FindArgs a)
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
        if (__ballot(reached != 0) == 0) continue;   // the whole wavefront: no pool state was touched
        while (reached) {
            const int j = __builtin_ctzll(reached);
            reached &= reached - 1;
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

// one lane per query: the best layer entry of the end token, the FEWEST hops that attain it
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(select)(FindArgs a)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const int t = D::end_token(a)[q];
    const long long layer_words = a.count * (long long)a.n_tokens;
    unsigned long long top = D::kUnreached;
    int h_star = 0;
    if (t >= 0 && t < a.n_tokens)
        for (int h = 1; h <= a.max_hops; ++h) {
            const unsigned long long b = a.best[(long long)h * layer_words + q * a.n_tokens + t];
            if (D::better(b, top)) {   // strictly: the fewest hops
                top = b;
                h_star = h;
            }
        }
    a.h_star[q] = h_star;
    a.target[q] = h_star ? t : -1;
}

// the hop between layer a.layer - 1 and a.layer of every query's answer: find_relax's grid without the LDS copy.  Only a lane
// whose pool holds a query's CURRENT TARGET token evaluates anything -- the quotes that reach that token, compared bit for
// bit with the layer's word; among the edges that attain it the smallest (segment, row, coin_in, coin_out) wins by an
// integer atomic min on the packed edge (pool number << 6 | coin_in << 3 | coin_out), which lands in the hop's slot in
// PATH ORDER.  (h_star indexes that slot: it is not trusted beyond max_hops.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(claim)(FindArgs a)
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

// one lane per query: the claimed edge's near token becomes the target of the layer before
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(advance)(FindArgs a)
{
    constexpr bool OUT = CFMM_FIND_OUT;
    using D = FindDir<OUT>;
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= a.count) return;
    const int hs = a.h_star[q];
    if (hs < a.layer || (OUT && hs > a.max_hops)) return;
    int sg, ci, co;
    long long row;
    int t = -1;
    if (find_decode(a, a.edge[(long long)D::slot(a.layer, hs) * a.count + q], sg, row, ci, co)) {
        const FindSeg& f = a.segs[sg];
        int tok[kMaxCoins];
        find_tokens(f, f.s.n_coins, f.s.m, row, a.n_tokens, tok);
        t = tok[OUT ? co : ci];
    }
    a.target[q] = t;   // -1: nothing claims from here on, and find_finish answers that no path was found
}

// one lane per query: n_hops, the four hop-major hop arrays, the amount, the status; the pool-repeat check.
// Outputs of query q at q (per query) and k*stride + q (hop k): the pointers already stand at the chunk's first query.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void CFMM_FIND(finish)(FindArgs a)
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
}
