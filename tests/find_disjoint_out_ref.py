"""The successive layered search of cfmm_find_disjoint_paths_out on the host (include/cfmm_amd_find_disjoint_out.h): the reference
the device is pinned to.  It is find_path_out_ref.py's layered search and forward walk with a per-query boolean mask of pools
applied to the DESTINATIONS before anything is quoted -- a banned pool reaches nothing and attains nothing -- run for max_paths
rounds, the pools of every found path joining the query's mask.  Like find_path_out_ref.py it knows nothing of pools: the market
is one [m, coins] table of 0-based token ids per segment and a callable quote_out(seg, amounts_out, coin_in, coin_out, rows) ->
amounts in.
"""
import numpy as np

from find_disjoint_ref import first_pools
from find_path_out_ref import UNREACHED
from find_path_ref import FOUND, FOUND_NONE, FOUND_REPEATS, QUERY_BLOCK, _bits, _pairs


def masked_layers_out(tok, quote_out, n_tokens, token_out, amount_out, max_hops, ban):
    """find_path_out_ref.layers_out with ban [count, pools] (True: the pool is absent for that query)"""
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    amount_out = np.asarray(amount_out, dtype=np.float64).reshape(-1)
    Q = token_out.size
    first = first_pools(tok)
    need = np.full((max_hops + 1, Q, n_tokens), UNREACHED)
    need[0, np.arange(Q), token_out] = np.where(amount_out > 0, amount_out, UNREACHED)
    for h in range(1, max_hops + 1):
        for q0 in range(0, Q, QUERY_BLOCK):
            prev = need[h - 1, q0:q0 + QUERY_BLOCK]
            if not np.any(np.isfinite(prev)):
                continue
            cur = need[h, q0:q0 + QUERY_BLOCK].reshape(-1)               # (a view: the block's rows are contiguous)
            for s, T in enumerate(tok):
                pci, pco = _pairs(T.shape[1])
                dst = np.where(ban[q0:q0 + QUERY_BLOCK, first[s]:first[s + 1], None], UNREACHED, prev[:, T[:, pco]])   # [queries, m, pairs]
                q, row, p = np.nonzero(np.isfinite(dst))
                if q.size == 0:
                    continue
                cost = np.asarray(quote_out(s, dst[q, row, p], pci[p], pco[p], row))
                ok = np.isfinite(cost) & (cost > 0)
                np.minimum.at(cur, (q * n_tokens + T[row, pci[p]])[ok], cost[ok])
    return need


def masked_find_out(tok, quote_out, n_tokens, token_in, token_out, amount_out, max_hops, ban):
    """find_path_out_ref.find_path_out_ref on the market without the pools of ban [count, pools]:
    -> (amount_in, n_hops, seg, row, coin_in, coin_out, status); amount_in of a query without a path is +inf here (the caller
    knows the amount the call was made with and puts the none value)"""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    Q, H = token_in.size, int(max_hops)
    need = masked_layers_out(tok, quote_out, n_tokens, token_out, amount_out, H, ban)
    every = np.arange(Q)
    col = need[1:H + 1, every, token_in]
    amount = col.min(axis=0)
    h_star = np.where(np.isfinite(amount), np.argmin(col, axis=0) + 1, 0)  # argmin: the FIRST layer that attains the minimum
    seg, ci, co = (np.full((Q, H), -1, dtype=np.int32) for _ in range(3))
    rows = np.full((Q, H), -1, dtype=np.int64)
    first = first_pools(tok)
    current = token_in.copy()
    for h in range(H, 0, -1):
        act = np.flatnonzero(h_star >= h)
        if act.size == 0:
            continue
        k = h_star[act] - h                                               # the hop, in path order
        want = _bits(need[h, act, current[act]])
        edge = np.full(act.size, np.iinfo(np.int64).max, dtype=np.int64)
        for s, T in enumerate(tok):
            pci, pco = _pairs(T.shape[1])
            dst = np.where(ban[act, first[s]:first[s + 1], None], UNREACHED, need[h - 1, act][:, T[:, pco]])
            out_of = T[:, pci][None, :, :] == current[act][:, None, None]
            q, row, p = np.nonzero(np.isfinite(dst) & out_of)
            if q.size == 0:
                continue
            cost = np.asarray(quote_out(s, dst[q, row, p], pci[p], pco[p], row))
            hit = np.isfinite(cost) & (cost > 0) & (_bits(cost) == want[q])
            key = ((first[s] + row[hit]) << 6) | (pci[p[hit]].astype(np.int64) << 3) | pco[p[hit]].astype(np.int64)
            np.minimum.at(edge, q[hit], key)
        assert np.all(edge != np.iinfo(np.int64).max), "a layer entry that no edge attains"
        pool = edge >> 6
        s_of = np.searchsorted(first, pool, side="right") - 1
        seg[act, k], rows[act, k] = s_of, pool - first[s_of]
        ci[act, k], co[act, k] = (edge >> 3) & 7, edge & 7
        current[act] = [tok[s][r, c] for s, r, c in zip(s_of, rows[act, k], co[act, k])]
    assert np.all(current[h_star > 0] == token_out[h_star > 0]), "a walk that does not end at token_out"
    status = np.where(h_star > 0, FOUND, FOUND_NONE).astype(np.int32)
    for q in np.flatnonzero(h_star > 1):
        visited = list(zip(seg[q, :h_star[q]].tolist(), rows[q, :h_star[q]].tolist()))
        if len(set(visited)) < len(visited):
            status[q] = FOUND_REPEATS
    return amount, h_star.astype(np.int32), seg, rows, ci, co, status


def find_disjoint_out_ref(tok, quote_out, n_tokens, token_in, token_out, amount_out, max_paths, max_hops):
    """-> (n_paths [count], amount_in [count, K], n_hops [count, K], seg, row, coin_in, coin_out [count, K, max_hops],
    status [count, K]), K = max_paths: Context.find_disjoint_paths_out's shapes.  Round r sees the market without the pools of the
    query's paths 0 .. r-1; a query for which a round found nothing is probed with 0.0 from then on (it reaches nothing).  An
    empty slot carries find_path_out's none value for the amount the CALL was made with: +inf, or +0.0 where it is 0."""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    given = np.array(amount_out, dtype=np.float64).reshape(-1)
    probe = given.copy()
    Q, K, H = token_in.size, int(max_paths), int(max_hops)
    first = first_pools(tok)
    ban = np.zeros((Q, int(first[-1])), dtype=bool)
    cost = np.zeros((Q, K))
    n_hops, status = np.zeros((Q, K), dtype=np.int32), np.full((Q, K), FOUND_NONE, dtype=np.int32)
    seg, ci, co = (np.full((Q, K, H), -1, dtype=np.int32) for _ in range(3))
    row = np.full((Q, K, H), -1, dtype=np.int64)
    none = np.where(given == 0, 0.0, np.inf)
    for r in range(K):
        cost[:, r], n_hops[:, r], seg[:, r], row[:, r], ci[:, r], co[:, r], status[:, r] = masked_find_out(
            tok, quote_out, n_tokens, token_in, token_out, probe, H, ban)
        missing = status[:, r] == FOUND_NONE
        cost[missing, r] = none[missing]
        for q in range(Q):
            used = slice(0, n_hops[q, r])
            ban[q, first[seg[q, r, used]] + row[q, r, used]] = True
        probe[missing] = 0.0
    return np.sum(status != FOUND_NONE, axis=1).astype(np.int32), cost, n_hops, seg, row, ci, co, status
