"""The successive layered search of cfmm_find_disjoint_paths on the host (include/cfmm_amd_find_disjoint.h): the reference the
device is pinned to.  It is find_path_ref.py's layered search and walk with a per-query boolean mask of pools applied to the
SOURCES before anything is quoted -- a banned pool reaches nothing and attains nothing -- run for max_paths rounds, the pools
of every found path joining the query's mask.  Like find_path_ref.py it knows nothing of pools: the market is one [m, coins]
table of 0-based token ids per segment and a callable quote(seg, amounts, coin_in, coin_out, rows) -> amounts out.
"""
import numpy as np

from find_path_ref import FOUND, FOUND_NONE, FOUND_REPEATS, QUERY_BLOCK, _bits, _pairs


def first_pools(tok):
    """the pool number of every segment's row 0 (and the market's pools, last): the number the tie-break orders by"""
    return np.concatenate([[0], np.cumsum([T.shape[0] for T in tok])]).astype(np.int64)


def masked_layers(tok, quote, n_tokens, token_in, amount_in, max_hops, ban):
    """find_path_ref.layers with ban [count, pools] (True: the pool is absent for that query)"""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    amount_in = np.asarray(amount_in, dtype=np.float64).reshape(-1)
    Q = token_in.size
    first = first_pools(tok)
    best = np.zeros((max_hops + 1, Q, n_tokens))
    best[0, np.arange(Q), token_in] = np.where(amount_in > 0, amount_in, 0.0)
    for h in range(1, max_hops + 1):
        for q0 in range(0, Q, QUERY_BLOCK):
            prev = best[h - 1, q0:q0 + QUERY_BLOCK]
            cur = best[h, q0:q0 + QUERY_BLOCK].reshape(-1)
            for s, T in enumerate(tok):
                pci, pco = _pairs(T.shape[1])
                src = np.where(ban[q0:q0 + QUERY_BLOCK, first[s]:first[s + 1], None], 0.0, prev[:, T[:, pci]])   # [queries, m, pairs]
                q, row, p = np.nonzero(src > 0)
                if q.size == 0:
                    continue
                out = np.asarray(quote(s, src[q, row, p], pci[p], pco[p], row))
                ok = np.isfinite(out) & (out > 0)
                np.maximum.at(cur, (q * n_tokens + T[row, pco[p]])[ok], out[ok])
    return best


def masked_find(tok, quote, n_tokens, token_in, token_out, amount_in, max_hops, ban):
    """find_path_ref.find_path_ref on the market without the pools of ban [count, pools]:
    -> (amount_out, n_hops, seg, row, coin_in, coin_out, status)"""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    Q, H = token_in.size, int(max_hops)
    best = masked_layers(tok, quote, n_tokens, token_in, amount_in, H, ban)
    every = np.arange(Q)
    col = best[1:H + 1, every, token_out]
    amount = col.max(axis=0)
    h_star = np.where(amount > 0, np.argmax(col, axis=0) + 1, 0)
    seg, ci, co = (np.full((Q, H), -1, dtype=np.int32) for _ in range(3))
    rows = np.full((Q, H), -1, dtype=np.int64)
    first = first_pools(tok)
    target = token_out.copy()
    for h in range(H, 0, -1):
        act = np.flatnonzero(h_star >= h)
        if act.size == 0:
            continue
        want = _bits(best[h, act, target[act]])
        edge = np.full(act.size, np.iinfo(np.int64).max, dtype=np.int64)
        for s, T in enumerate(tok):
            pci, pco = _pairs(T.shape[1])
            src = np.where(ban[act, first[s]:first[s + 1], None], 0.0, best[h - 1, act][:, T[:, pci]])
            into = T[:, pco][None, :, :] == target[act][:, None, None]
            q, row, p = np.nonzero((src > 0) & into)
            if q.size == 0:
                continue
            out = np.asarray(quote(s, src[q, row, p], pci[p], pco[p], row))
            hit = np.isfinite(out) & (out > 0) & (_bits(out) == want[q])
            key = ((first[s] + row[hit]) << 6) | (pci[p[hit]].astype(np.int64) << 3) | pco[p[hit]].astype(np.int64)
            np.minimum.at(edge, q[hit], key)
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


def find_disjoint_ref(tok, quote, n_tokens, token_in, token_out, amount_in, max_paths, max_hops):
    """-> (n_paths [count], amount_out [count, K], n_hops [count, K], seg, row, coin_in, coin_out [count, K, max_hops],
    status [count, K]), K = max_paths: Context.find_disjoint_paths' shapes.  Round r sees the market without the pools of the
    query's paths 0 .. r-1; a query for which a round found nothing is probed with 0.0 from then on (it reaches nothing)."""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    amount_in = np.array(amount_in, dtype=np.float64).reshape(-1)
    Q, K, H = token_in.size, int(max_paths), int(max_hops)
    first = first_pools(tok)
    ban = np.zeros((Q, int(first[-1])), dtype=bool)
    out = np.zeros((Q, K))
    n_hops, status = np.zeros((Q, K), dtype=np.int32), np.full((Q, K), FOUND_NONE, dtype=np.int32)
    seg, ci, co = (np.full((Q, K, H), -1, dtype=np.int32) for _ in range(3))
    row = np.full((Q, K, H), -1, dtype=np.int64)
    for r in range(K):
        out[:, r], n_hops[:, r], seg[:, r], row[:, r], ci[:, r], co[:, r], status[:, r] = masked_find(
            tok, quote, n_tokens, token_in, token_out, amount_in, H, ban)
        for q in range(Q):
            used = slice(0, n_hops[q, r])
            ban[q, first[seg[q, r, used]] + row[q, r, used]] = True
        amount_in[status[:, r] == FOUND_NONE] = 0.0
    return np.sum(status != FOUND_NONE, axis=1).astype(np.int32), out, n_hops, seg, row, ci, co, status
