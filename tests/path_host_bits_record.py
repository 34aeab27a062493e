"""Every answer of the order-level path entries tests/query_bits_record.py predates -- split_paths, split_paths_out and their
_dev forms, swap_order and swap_order_out, and the read-only path entries on a two-shard parent -- on one small market, as a dict
of arrays: what tests/golden/make_path_host_bits_golden.py stores from one build and tests/test_gpu_path_host_bits.py replays on
another, bit for bit.  Public API only, so the same file runs unchanged on the recorded commit and on every later tree.

Market: 64 tokens, one segment per kind in the order of the kind numbers, 512 pools each.
Splits: 48 orders of K = 1 .. 8 paths cycling (216 paths) of 1 .. 3 hops, 5 rounds; order 5 has amount 0 (SPLIT_NONE), order 13
wants a billion times its scale (exact output: SPLIT_UNOBTAINABLE); the _dev forms run on the same arrays.
Executions: 48 orders of K = 1 .. 4 paths cycling (120 paths) of 1 .. 3 hops whose hops fall on 48 rows per segment, so orders
share pools and the plan has several waves (restated and asserted below: at least 3, and at least two of them with UniV3 hops
on more than one hop level, so the move between waves and the table's second upload run).  Order 7 cannot meet its limit;
order 11's first path holds a refusing hop -- exact input: it tenders 2^80 reserves to a ProductTwoCoin pool, x / (R + x) rounds
to 1 and nothing would be left; exact output: it asks the one doctored pool (market) for all but 2^-152 of a coin, which Solidly's
window refuses --; exact output: order 13's first path wants twice the reserve (unobtainable).  The pool state of every segment and the
trades of one sweep on it are recorded afterwards.
Parent: quote_path and size_path on 100 paths, split_paths and split_paths_out on 24 orders (108 paths), on a single context and
on a two-shard parent on the same device, with the parent's "size_launches" / "split_launches"."""
import numpy as np

import query_bits_record as rec

N = 64
M = 512
SEED = 23
ROUNDS = 5
H = 3
SPLIT_ORDERS, SPLIT_KS = 48, 8
EXEC_ORDERS, EXEC_KS, EXEC_ROWS = 48, 4, 48
PARENT_PATHS, PARENT_ORDERS = 100, 24
LIMIT_ORDER, REFUSING_ORDER, UNOBTAINABLE_ORDER, NONE_ORDER = 7, 11, 13, 5
THIN = 500                          # the doctored Solidly row


def market(cr, synth):
    """synth's generators with a fixed seed; ONE pool is doctored, Solidly row THIN, which no path but the exact-output refusing
    one names: it holds {1, 2^-120}, so that giving all but 2^-152 of its second coin -- a finite quote -- would leave that coin
    positive but outside Solidly's window [2^-150, 2^150] (the state is refused, tests/test_gpu_swap_path_out.py's case)"""
    b = [synth.product_pools(M, N, seed=SEED), synth.geomean_pools(M, N, seed=SEED + 1),
         synth.univ3_ragged_pools(M, N, min_ticks=3, max_ticks=8, seed=SEED + 2), synth.weighted_pools(M, N, 3, seed=SEED + 3),
         synth.curve_pools(M, N, 4, seed=SEED + 4), synth.solidly_pools(M, N, seed=SEED + 5, wide=True)]
    assert [len(x) for x in b] == [M] * 6
    R = b[5].R.copy()
    R[THIN] = [1.0, 2.0 ** -120]
    b[5] = cr.PoolBatch(b[5].kind, R=R, γ=b[5].γ.copy(), Ai=b[5].Ai.copy())
    return b


def order_first_of(count, kmax):
    return np.concatenate(([0], np.cumsum([1 + g % kmax for g in range(count)]))).astype(np.int64)


def paths(synth, batches, n, rows, stream):
    """n paths of 1 + p % 3 hops: hop k of path p in segment (p + k) % 6 on row (7p + 11k) % rows -- no pool twice among paths
    fewer than 6 apart, so none twice in an order --, coins cycling through every ordered pair; -> the five path columns, and
    per path the scale of the coin it tenders and of the coin it yields"""
    p, k = np.meshgrid(np.arange(n), np.arange(H), indexing="ij")
    n_hops = (1 + np.arange(n) % H).astype(np.int32)
    seg = ((p + k) % 6).astype(np.int32)
    row = ((7 * p + 11 * k) % rows).astype(np.int64)
    ci, co = np.zeros((n, H), dtype=np.int32), np.zeros((n, H), dtype=np.int32)
    for s, b in enumerate(batches):
        nc = b.Ai.shape[1]
        pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
        at = seg == s
        pick = (p[at] + 2 * k[at]) % len(pairs)
        ci[at], co[at] = pairs[pick, 0], pairs[pick, 1]
    lead = np.array([rec.scale(batches[seg[i, 0]])[row[i, 0], ci[i, 0]] for i in range(n)])
    last = np.array([rec.scale(batches[seg[i, n_hops[i] - 1]])[row[i, n_hops[i] - 1], co[i, n_hops[i] - 1]] for i in range(n)])
    return (n_hops, seg, row, ci, co), lead, last


def order_waves(first, cols):
    """the planner's rule restated -> per order its wave"""
    n_hops, seg, row = cols[:3]
    free, wave = {}, []
    for g in range(len(first) - 1):
        named = [(int(seg[q, k]), int(row[q, k])) for q in range(first[g], first[g + 1]) for k in range(n_hops[q])]
        assert len(set(named)) == len(named), g
        w = max(free.get(x, 0) for x in named)
        for x in named:
            free[x] = w + 1
        wave.append(w)
    return np.array(wave)


def split_case(synth, batches, orders=SPLIT_ORDERS):
    first = order_first_of(orders, SPLIT_KS)
    n = int(first[-1])
    cols, lead, last = paths(synth, batches, n, M, 3)
    u = 10.0 ** (-4.0 + 3.0 * synth.uniform(SEED + 10, 1, orders))
    amount_in = np.array([lead[first[g]] for g in range(orders)]) * u
    amount_out = np.array([last[first[g]] for g in range(orders)]) * u * 1e-2
    amount_in[NONE_ORDER] = amount_out[NONE_ORDER] = 0.0
    amount_out[UNOBTAINABLE_ORDER] *= 1e11
    return first, cols, amount_in, amount_out


def exec_case(synth, batches, out):
    first = order_first_of(EXEC_ORDERS, EXEC_KS)
    n = int(first[-1])
    cols, lead, last = paths(synth, batches, n, EXEC_ROWS, 4)
    n_hops, seg, row, ci, co = cols
    amount = (last * 1e-2 if out else lead) * 10.0 ** (-5.0 + 2.0 * synth.uniform(SEED + 11, 2 + out, n))
    R = batches[0].R
    q = int(first[REFUSING_ORDER])                      # one hop on a pool no other path names
    if out:                                             # Solidly row THIN: would be left with 2^-152 (market's docstring)
        n_hops[q], seg[q, 0], row[q, 0], ci[q, 0], co[q, 0] = 1, 5, THIN, 0, 1
        amount[q] = 2.0 ** -120 * (1.0 - 2.0 ** -32)
    else:                                               # ProductTwoCoin row 500: x / (R + x) rounds to 1, nothing would be left
        n_hops[q], seg[q, 0], row[q, 0], ci[q, 0], co[q, 0] = 1, 0, 500, 0, 1
        amount[q] = R[500, 0] * 2.0 ** 80
    if out:
        q = int(first[UNOBTAINABLE_ORDER])
        n_hops[q], seg[q, 0], row[q, 0], ci[q, 0], co[q, 0] = 1, 0, 501, 0, 1
        amount[q] = 2.0 * R[501, 1]
    for q in range(first[LIMIT_ORDER], first[LIMIT_ORDER + 1]):     # one small hop per path: nothing but the limit can stop it
        n_hops[q] = 1
        amount[q] = rec.scale(batches[seg[q, 0]])[row[q, 0], co[q, 0] if out else ci[q, 0]] * 1e-6
    limit = np.full(EXEC_ORDERS, 1e300 if out else 0.0)
    limit[LIMIT_ORDER] = 0.0 if out else 1e300
    wave = order_waves(first, cols)
    univ3_levels = [{k for g in np.flatnonzero(wave == w) for q in range(first[g], first[g + 1]) for k in range(n_hops[q]) if seg[q, k] == 2}
                    for w in range(wave.max() + 1)]
    assert wave.max() + 1 >= 3 and sum(len(s) >= 2 for s in univ3_levels) >= 2, (wave.max() + 1, univ3_levels)
    return first, cols, amount, limit, int(wave.max()) + 1


def states(ctx, batches, res, name, synth):
    for s, b in enumerate(batches):
        res[f"{name}.state{s}"] = ctx.prices(s, len(b)) if hasattr(b, "tick_off") else ctx.reserves(s, len(b), b.Ai.shape[1])
    ctx.find_arb(synth.sweep_prices(N, seed=SEED + 60, spread=0.3))
    res[f"{name}.sweep_delta"], res[f"{name}.sweep_lambda"] = ctx.trades()


def record_all(cr, synth):
    from cfmmrouter_amd._lib import ORDER_REFUSED, PATH_REFUSED, SWAP_REFUSED
    batches = market(cr, synth)
    res = {}
    T = lambda a: np.ascontiguousarray(a.T)
    fresh = lambda device=0: cr.DeviceBackend(N, batches, device=device)
    parts = ("x", "y", "total", "status")

    # ---- the splits, host and device pointers, one context
    first, cols, amount_in, amount_out = split_case(synth, batches)
    n = int(first[-1])
    be = fresh()
    try:
        ctx = be.ctx
        for name, host, dev, amount in (("split_paths", ctx.split_paths, ctx.split_paths_dev, amount_in),
                                        ("split_paths_out", ctx.split_paths_out, ctx.split_paths_out_dev, amount_out)):
            for part, a in zip(parts, host(first, amount, *cols, rounds=ROUNDS)):
                res[f"{name}.{part}"] = a
            arrays = [first, amount, cols[0]] + [T(a) for a in cols[1:]]
            got = rec.on_device(ctx, arrays, [(n, "f"), (n, "f"), (SPLIT_ORDERS, "f"), (SPLIT_ORDERS, "i")],
                                lambda i, o: dev(SPLIT_ORDERS, i[0], i[1], n, H, *i[2:], ROUNDS, *o))
            for part, a in zip(parts, got):
                res[f"{name}_dev.{part}"] = a
    finally:
        be.close()

    # ---- the executions, a fresh context each
    for out, name in ((0, "swap_order"), (1, "swap_order_out")):
        efirst, ecols, amount, limit, waves = exec_case(synth, batches, out)
        be = fresh()
        try:
            ctx = be.ctx
            res[f"{name}.price_before"] = ctx.prices(2, M)
            if out:
                got = ctx.swap_order_out(efirst, *ecols, amount, max_total_in=limit, hops=True)
            else:
                got = ctx.swap_order(efirst, *ecols, amount, min_total_out=limit, hops=True)
            for part, a in zip(("path", "total", "status", "path_status", "hops"), got):
                res[f"{name}.{part}"] = a
            assert got[2][REFUSING_ORDER] == ORDER_REFUSED and got[3][efirst[REFUSING_ORDER]] == (SWAP_REFUSED if out else PATH_REFUSED), name
            res[f"{name}.launches"] = np.array([ctx.get_option("swap_launches"), waves, ctx.get_option("swap_refused")], dtype=np.int64)
            states(ctx, batches, res, name, synth)
        finally:
            be.close()

    # ---- the read-only path entries on a single context and on a two-shard parent on the same device
    pfirst, pcols, p_in, p_out = split_case(synth, batches, PARENT_ORDERS)
    few = tuple(a[:PARENT_PATHS] for a in pcols)
    x = np.array([rec.scale(batches[few[1][i, 0]])[few[2][i, 0], few[3][i, 0]] for i in range(PARENT_PATHS)]) * 1e-3
    for who, device in (("single", 0), ("parent", [0, 0])):
        be = fresh(device)
        try:
            ctx = be.ctx
            res[f"{who}.quote_path"], res[f"{who}.quote_path.hops"] = ctx.quote_path(*few, x, hops=True)
            for part, a in zip(("amount_in", "amount_out", "gain", "status"), ctx.size_path(*few, 64.0 * x, None, None, ROUNDS)):
                res[f"{who}.size_path.{part}"] = a
            launches = [ctx.get_option("size_launches")]
            for name, host, amount in (("split_paths", ctx.split_paths, p_in), ("split_paths_out", ctx.split_paths_out, p_out)):
                for part, a in zip(parts, host(pfirst, amount, *pcols, rounds=ROUNDS)):
                    res[f"{who}.{name}.{part}"] = a
                launches.append(ctx.get_option("split_launches"))
            res[f"{who}.launches"] = np.array(launches, dtype=np.int64)     # size, split, split_out
        finally:
            be.close()
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


as_words = rec.as_words
