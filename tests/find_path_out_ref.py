"""The layered path search of cfmm_find_path_out on the host, with the contract's tie-breaks (include/cfmm_amd_find_out.h): the
reference the device is pinned to.  Like tests/find_path_ref.py it knows nothing of pools: it takes the market as one [m, coins]
table of 0-based token ids per segment and a callable quote_out(seg, amounts_out, coin_in, coin_out, rows) -> amounts in
(Context.quote_out's argument order), and evaluates a whole layer's edges with one call per segment (per block of QUERY_BLOCK
queries, which bounds its memory).

    need[0][token_out] = amount_out; need[h][t] = min of quote_out(pool, ci -> co, need[h-1][tok(co)]) over every pool and
    ordered coin pair with tok(ci) == t whose destination is reached; a quote that is NaN, +inf or <= 0 enters nothing.
    amount_in = min over h >= 1 of need[h][token_in]; the fewest hops h* that attain it; walked FORWARD from (h*, token_in)
    through the smallest (segment, row, coin_in, coin_out) that attains each layer entry bit for bit.
    No path: amount_in +inf, or +0.0 where amount_out is 0.
"""
import numpy as np

from find_path_ref import FOUND, FOUND_NONE, FOUND_REPEATS, QUERY_BLOCK, _bits, _pairs

UNREACHED = np.inf


def layers_out(tok, quote_out, n_tokens, token_out, amount_out, max_hops):
    """need [max_hops + 1, count, n_tokens]; +inf = unreached"""
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    amount_out = np.asarray(amount_out, dtype=np.float64).reshape(-1)
    Q = token_out.size
    need = np.full((max_hops + 1, Q, n_tokens), UNREACHED)
    need[0, np.arange(Q), token_out] = np.where(amount_out > 0, amount_out, UNREACHED)
    for h in range(1, max_hops + 1):
        for q0 in range(0, Q, QUERY_BLOCK):
            prev = need[h - 1, q0:q0 + QUERY_BLOCK]
            cur = need[h, q0:q0 + QUERY_BLOCK].reshape(-1)               # (a view: the block's rows are contiguous)
            for s, T in enumerate(tok):
                pci, pco = _pairs(T.shape[1])
                dst = prev[:, T[:, pco]]                                  # [queries, m, pairs]
                q, row, p = np.nonzero(np.isfinite(dst))
                if q.size == 0:
                    continue
                cost = np.asarray(quote_out(s, dst[q, row, p], pci[p], pco[p], row))
                ok = np.isfinite(cost) & (cost > 0)
                np.minimum.at(cur, (q * n_tokens + T[row, pci[p]])[ok], cost[ok])
    return need


def find_path_out_ref(tok, quote_out, n_tokens, token_in, token_out, amount_out, max_hops, need=None):
    """-> (amount_in, n_hops, seg, row, coin_in, coin_out, status), the hop arrays [count, max_hops] in path order with -1 in the
    unused slots.  need: layers_out(...) of the same queries with at least max_hops layers, computed before (layer h does not
    depend on the layers behind it, so one computation serves every smaller max_hops)."""
    token_in = np.asarray(token_in, dtype=np.int64).reshape(-1)
    token_out = np.asarray(token_out, dtype=np.int64).reshape(-1)
    amount_out = np.asarray(amount_out, dtype=np.float64).reshape(-1)
    Q, H = token_in.size, int(max_hops)
    if need is None:
        need = layers_out(tok, quote_out, n_tokens, token_out, amount_out, H)
    every = np.arange(Q)
    col = need[1:H + 1, every, token_in]                                  # [H, count]
    amount = col.min(axis=0)
    h_star = np.where(np.isfinite(amount), np.argmin(col, axis=0) + 1, 0)  # argmin: the FIRST layer that attains the minimum
    amount = np.where(h_star > 0, amount, np.where(amount_out == 0, 0.0, np.inf))
    seg, ci, co = (np.full((Q, H), -1, dtype=np.int32) for _ in range(3))
    rows = np.full((Q, H), -1, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum([T.shape[0] for T in tok])]).astype(np.int64)
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
            dst = need[h - 1, act][:, T[:, pco]]
            out_of = T[:, pci][None, :, :] == current[act][:, None, None]
            q, row, p = np.nonzero(np.isfinite(dst) & out_of)
            if q.size == 0:
                continue
            cost = np.asarray(quote_out(s, dst[q, row, p], pci[p], pco[p], row))
            hit = np.isfinite(cost) & (cost > 0) & (_bits(cost) == want[q])
            key = ((first[s] + row[hit]) << 6) | (pci[p[hit]].astype(np.int64) << 3) | pco[p[hit]].astype(np.int64)
            np.minimum.at(edge, q[hit], key)                              # (pools in segment order: the order of (segment, row))
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
