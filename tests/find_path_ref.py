"""The layered path search of cfmm_find_path on the host, with the contract's tie-breaks (include/cfmm_amd.h): the reference
the device is pinned to.  It knows nothing of pools: it takes the market as one [m, coins] table of 0-based token ids per
segment and a callable quote(seg, amounts, coin_in, coin_out, rows) -> amounts out (Context.quote's argument order), and
evaluates a whole layer's edges with one call per segment (per block of QUERY_BLOCK queries, which bounds its memory).

    best[0][token_in] = amount_in; best[h][t] = max of quote(pool, ci -> co, best[h-1][tok(ci)]) over every pool and ordered
    coin pair with tok(co) == t whose source is reached; a quote that is NaN, not finite or <= 0 enters nothing.
    amount_out = max over h >= 1 of best[h][token_out]; the fewest hops that attain it; walked back through the smallest
    (segment, row, coin_in, coin_out) that attains each layer entry bit for bit.
"""
import numpy as np

FOUND, FOUND_NONE, FOUND_REPEATS = 0, 1, 2
QUERY_BLOCK = 128


def _pairs(nc):
    p = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
    return p[:, 0], p[:, 1]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def layers(tok, quote, n_tokens, token_in, amount_in, max_hops):
    """best [max_hops + 1, count, n_tokens]; 0.0 = unreached"""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    amount_in = np.asarray(amount_in, dtype=np.float64).reshape(-1)
    Q = token_in.size
    best = np.zeros((max_hops + 1, Q, n_tokens))
    best[0, np.arange(Q), token_in] = np.where(amount_in > 0, amount_in, 0.0)
    for h in range(1, max_hops + 1):
        for q0 in range(0, Q, QUERY_BLOCK):
            prev = best[h - 1, q0:q0 + QUERY_BLOCK]
            cur = best[h, q0:q0 + QUERY_BLOCK].reshape(-1)               # (a view: the block's rows are contiguous)
            for s, T in enumerate(tok):
                pci, pco = _pairs(T.shape[1])
                src = prev[:, T[:, pci]]                                  # [queries, m, pairs]
                q, row, p = np.nonzero(src > 0)
                if q.size == 0:
                    continue
                out = np.asarray(quote(s, src[q, row, p], pci[p], pco[p], row))
                ok = np.isfinite(out) & (out > 0)
                np.maximum.at(cur, (q * n_tokens + T[row, pco[p]])[ok], out[ok])
    return best


def find_path_ref(tok, quote, n_tokens, token_in, token_out, amount_in, max_hops, best=None):
    """-> (amount_out, n_hops, seg, row, coin_in, coin_out, status), the hop arrays [count, max_hops] with -1 in the unused
    slots.  best: layers(...) of the same queries with at least max_hops layers, computed before (layer h does not depend on
    the layers behind it, so one computation serves every smaller max_hops)."""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    Q, H = token_in.size, int(max_hops)
    if best is None:
        best = layers(tok, quote, n_tokens, token_in, amount_in, H)
    every = np.arange(Q)
    col = best[1:H + 1, every, token_out]                                 # [H, count]
    amount = col.max(axis=0)
    h_star = np.where(amount > 0, np.argmax(col, axis=0) + 1, 0)          # argmax: the FIRST layer that attains the maximum
    seg, ci, co = (np.full((Q, H), -1, dtype=np.int32) for _ in range(3))
    rows = np.full((Q, H), -1, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum([T.shape[0] for T in tok])]).astype(np.int64)
    target = token_out.copy()
    for h in range(H, 0, -1):
        act = np.flatnonzero(h_star >= h)
        if act.size == 0:
            continue
        want = _bits(best[h, act, target[act]])
        edge = np.full(act.size, np.iinfo(np.int64).max, dtype=np.int64)
        for s, T in enumerate(tok):
            pci, pco = _pairs(T.shape[1])
            src = best[h - 1, act][:, T[:, pci]]
            into = T[:, pco][None, :, :] == target[act][:, None, None]
            q, row, p = np.nonzero((src > 0) & into)
            if q.size == 0:
                continue
            out = np.asarray(quote(s, src[q, row, p], pci[p], pco[p], row))
            hit = np.isfinite(out) & (out > 0) & (_bits(out) == want[q])
            key = ((first[s] + row[hit]) << 6) | (pci[p[hit]].astype(np.int64) << 3) | pco[p[hit]].astype(np.int64)
            np.minimum.at(edge, q[hit], key)                              # (pools in segment order: the order of (segment, row))
        assert np.all(edge != np.iinfo(np.int64).max), "a layer entry that no edge attains"
        pool = edge >> 6
        s_of = np.searchsorted(first, pool, side="right") - 1
        seg[act, h - 1], rows[act, h - 1] = s_of, pool - first[s_of]
        ci[act, h - 1], co[act, h - 1] = (edge >> 3) & 7, edge & 7
        target[act] = [tok[s][r, c] for s, r, c in zip(s_of, rows[act, h - 1], ci[act, h - 1])]
    status = np.where(h_star > 0, FOUND, FOUND_NONE).astype(np.int32)
    for q in np.flatnonzero(h_star > 1):
        visited = list(zip(seg[q, :h_star[q]].tolist(), rows[q, :h_star[q]].tolist()))
        if len(set(visited)) < len(visited):
            status[q] = FOUND_REPEATS
    return amount, h_star.astype(np.int32), seg, rows, ci, co, status


def brute_force_walks(tok, token_in, token_out, max_hops):
    """every walk of 1 .. max_hops hops from token_in to token_out, as a list of hop lists [(seg, row, ci, co), ...]"""
    edges = {}
    for s, T in enumerate(tok):
        for row in range(T.shape[0]):
            for i in range(T.shape[1]):
                for j in range(T.shape[1]):
                    if i != j:
                        edges.setdefault(int(T[row, i]), []).append((s, row, i, j, int(T[row, j])))
    walks, frontier = [], [((), int(token_in))]
    for _ in range(max_hops):
        nxt = []
        for path, t in frontier:
            for s, row, i, j, to in edges.get(t, ()):
                step = path + ((s, row, i, j),)
                nxt.append((step, to))
                if to == int(token_out):
                    walks.append(list(step))
        frontier = nxt
    return walks
