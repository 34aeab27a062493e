"""Every answer of every query entry on one small market, as a dict of arrays: what tests/golden/make_query_bits_golden.py
stores from one build and tests/test_gpu_query_bits.py replays on another, bit for bit.  Public API only, so the same file
runs unchanged on the recorded commit and on every later tree.

Market: 12 tokens, one segment per kind in the order of the kind numbers -- ProductTwoCoin 300 pools (two 256-pool find tiles,
the second partial), GeometricMeanTwoCoin 70 (one wavefront and a partial one), UniV3 70 (3 .. 8 ticks), weighted 70 (3 coins),
Curve 70 (4 coins, a fifth with alpha = 0), Solidly 70.  600 single-pool queries and 600 paths (a partial third block), 70 find
queries (more than the 64 a lane group holds) and 70 sized paths.  The moving entries run on a fresh context each and the
pool state they leave is recorded.  The device-pointer entries get the inputs no host entry lets through: rows, coins and
segments out of range on both sides, coin_in == coin_out, negative / NaN / +inf amounts, n_hops 0 and max_hops + 1."""
import numpy as np

N = 12
SIZES = (300, 70, 70, 70, 70, 70)
Q = 600
H = 8
FIND = 70
SIZED = 70
SEED = 11


def market(cr, synth):
    from cfmmrouter_amd._lib import KIND_CURVE, KIND_GEOMEAN, KIND_PRODUCT, KIND_SOLIDLY, KIND_UNIV3, KIND_WEIGHTED
    b = [synth.product_pools(SIZES[0], N, seed=SEED), synth.geomean_pools(SIZES[1], N, seed=SEED + 1),
         synth.univ3_ragged_pools(SIZES[2], N, min_ticks=3, max_ticks=8, seed=SEED + 2), synth.weighted_pools(SIZES[3], N, 3, seed=SEED + 3),
         synth.curve_pools(SIZES[4], N, 4, seed=SEED + 4), synth.solidly_pools(SIZES[5], N, seed=SEED + 5, wide=True)]
    assert [x.kind for x in b] == [KIND_PRODUCT, KIND_GEOMEAN, KIND_UNIV3, KIND_WEIGHTED, KIND_CURVE, KIND_SOLIDLY]
    assert np.all(np.diff(b[2].tick_off) >= 3) and 0 < np.sum(b[4].α == 0.0) < SIZES[4]
    return b


def scale(b):
    """[m, coins] the size an amount of each coin is measured in (UniV3: the pool's sqrt-liquidity scale)"""
    if hasattr(b, "tick_off"):
        return np.repeat(np.sqrt(b.liquidity[b.tick_off[:-1]] + 1.0)[:, None], 2, axis=1)
    return b.R


def pool_queries(synth, b, s, out):
    """600 queries of segment s: rows with repeats, every ordered coin pair, amounts 10^U[-6, 0.5) of the coin's scale (of the
    coin wanted when out), every 50th 0 and every 50th a million times the scale (unobtainable, or a state a pool refuses)"""
    m, nc = len(b), b.Ai.shape[1]
    q = np.arange(Q)
    idx = np.minimum((synth.uniform(SEED + 20 + s, 1, Q) * m).astype(np.int64), m - 1)
    pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
    ci, co = pairs[q % len(pairs), 0].copy(), pairs[q % len(pairs), 1].copy()
    amt = scale(b)[idx, co if out else ci] * 10.0 ** (-6.0 + 6.5 * synth.uniform(SEED + 30 + s, 2 + out, Q))
    amt[q % 50 == 7] = 0.0
    amt[q % 50 == 23] *= 1e6
    return idx, ci, co, amt


def paths(synth, batches, count, distinct):
    """n_hops = 1 + p % 8, hop k in segment (p + k) % 6, coins cycling through every ordered pair, rows pseudo-random (distinct:
    7p + 11k mod m, so that a path names no pool twice); the first amount 10^U[-5, -1) of the coin's scale, every 40th 0 and every 40th a million scales"""
    p, k = np.meshgrid(np.arange(count), np.arange(H), indexing="ij")
    n_hops = (1 + np.arange(count) % H).astype(np.int32)
    seg = ((p + k) % 6).astype(np.int32)
    m = np.array(SIZES)[seg]
    row = ((7 * p + 11 * k) % m if distinct else np.minimum((synth.uniform(SEED + 40, 3, count * H).reshape(count, H) * m).astype(np.int64), m - 1)).astype(np.int64)
    ci, co = np.zeros((count, H), dtype=np.int32), np.zeros((count, H), dtype=np.int32)
    for s, b in enumerate(batches):
        nc = b.Ai.shape[1]
        pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
        at = seg == s
        pick = (p[at] + 2 * k[at]) % len(pairs)
        ci[at], co[at] = pairs[pick, 0], pairs[pick, 1]
    first = np.array([scale(batches[seg[i, 0]])[row[i, 0], ci[i, 0]] for i in range(count)])
    last = np.array([scale(batches[seg[i, n_hops[i] - 1]])[row[i, n_hops[i] - 1], co[i, n_hops[i] - 1]] for i in range(count)])
    u = 10.0 ** (-5.0 + 4.0 * synth.uniform(SEED + 41, 4, count))
    zero = np.arange(count) % 40 == 9
    u = np.where(np.arange(count) % 40 == 29, 1e6, u)                  # a hop on the way cannot give that much, or refuses its new state
    return (n_hops, seg, row, ci, co), np.where(zero, 0.0, first * u), np.where(zero, 0.0, last * u)


def states(ctx, batches, res, name, synth):
    """what a moving entry leaves: the reserves / prices the context hands back, and -- the prepared constants it refreshed
    (GeometricMean's {Q1, Q2}, the weighted and Curve log columns) cannot be downloaded -- the trades of one sweep, which is
    computed from them"""
    for s, b in enumerate(batches):
        res[f"{name}.state{s}"] = ctx.prices(s, len(b)) if hasattr(b, "tick_off") else ctx.reserves(s, len(b), b.Ai.shape[1])
    ctx.find_arb(synth.sweep_prices(N, seed=SEED + 60, spread=0.3))
    res[f"{name}.sweep_delta"], res[f"{name}.sweep_lambda"] = ctx.trades()


def on_device(ctx, arrays, outs, call):
    """arrays up, call(input pointers, output pointers) on the current stream, outputs down"""
    import torch
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    o = [torch.full((n,), 7, dtype=torch.float64 if dt == "f" else torch.int32, device=dev) for n, dt in outs]
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        call([x.data_ptr() for x in t], [x.data_ptr() for x in o])
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    return [x.cpu().numpy() for x in o]


def spoil_pool_queries(idx, ci, co, amt, m, nc):
    idx, ci, co, amt = idx.copy(), ci.copy(), co.copy(), amt.copy()
    idx[3], idx[4], idx[5] = m, -5, 2 ** 40
    ci[10], ci[11], co[12], co[13] = nc, -1, nc + 7, -2
    co[14] = ci[14]
    amt[20], amt[21], amt[22], amt[23] = -1.0, np.nan, np.inf, -np.inf
    return idx, ci, co, amt


def spoil_paths(cols, amt):
    n_hops, seg, row, ci, co = (a.copy() for a in cols)
    amt = amt.copy()
    n_hops[40], n_hops[41], n_hops[42] = 0, H + 1, -3
    seg[50, 0], seg[51, 1], seg[52, 0] = 6, -1, 2 ** 30          # paths 50 .. 59 have 3 .. 8 hops, or 1 .. 4: hop 0 is always used
    row[59, 0], row[60, 0], row[61, 0] = 300, -1, 2 ** 40
    ci[70, 0], ci[71, 0], co[72, 0], co[73, 0] = 8, -1, 4, -1
    co[74, 0] = ci[74, 0]
    amt[80], amt[81], amt[82] = -1.0, np.nan, np.inf
    return (n_hops, seg, row, ci, co), amt


def record_all(cr, synth):
    batches = market(cr, synth)
    res = {}
    fresh = lambda: cr.DeviceBackend(N, batches)
    T = lambda a: np.ascontiguousarray(a.T)

    # ---- the read-only entries, one context
    be = fresh()
    try:
        ctx = be.ctx
        for s, b in enumerate(batches):
            m, nc = len(b), b.Ai.shape[1]
            for out, name, host, dev in ((0, "quote", ctx.quote, ctx.quote_dev), (1, "quote_out", ctx.quote_out, ctx.quote_out_dev)):
                idx, ci, co, amt = pool_queries(synth, b, s, out)
                res[f"{name}{s}"] = host(s, amt, ci, co, idx)
                res[f"{name}{s}.dense"] = host(s, amt[:70], ci[:70], None if nc == 2 else co[:70])   # rows 0 .. 69; two coins: coin_out = 1 - coin_in
                bad = spoil_pool_queries(idx, ci, co, amt, m, nc)
                res[f"{name}_dev{s}"], = on_device(ctx, bad, [(Q, "f")], lambda i, o: dev(s, Q, i[3], i[1], o[0], i[2], i[0]))
        (cols, x0, y0) = paths(synth, batches, Q, distinct=False)
        res["quote_path"], res["quote_path.hops"] = ctx.quote_path(*cols, x0, hops=True)
        res["quote_path_out"], res["quote_path_out.hops"] = ctx.quote_path_out(*cols, y0, hops=True)
        for name, dev, given in (("quote_path_dev", ctx.quote_path_dev, x0), ("quote_path_out_dev", ctx.quote_path_out_dev, y0)):
            bad, amt = spoil_paths(cols, given)
            arrays = [bad[0]] + [T(a) for a in bad[1:]] + [amt]
            res[name], res[name + ".hops"] = on_device(ctx, arrays, [(Q, "f"), (Q * H, "f")], lambda i, o: dev(Q, H, *i, o[0], o[1]))
        # the searches, with and without the LDS copy of the layers
        q = np.arange(FIND)
        tin, tout = (q % N).astype(np.int32), ((5 * q + 1 + q // N) % N).astype(np.int32)
        unit = np.median(batches[0].R)
        amt_in = unit * 10.0 ** (-5.0 + 5.0 * synth.uniform(SEED + 50, 5, FIND))
        amt_out = unit * 10.0 ** (-6.0 + 4.0 * synth.uniform(SEED + 51, 6, FIND))
        amt_in[17] = amt_out[17] = 0.0
        amt_out[33] *= 1e9                                              # nobody can give that much
        for lds in (1, 0):
            ctx.set_option("find_lds", lds)
            try:
                for name, fn, amt in (("find_path", ctx.find_path, amt_in), ("find_path_out", ctx.find_path_out, amt_out)):
                    for part, a in zip(("amount", "n_hops", "seg", "row", "ci", "co", "status"), fn(tin, tout, amt, 3)):
                        res[f"{name}.lds{lds}.{part}"] = a
            finally:
                ctx.set_option("find_lds", 1)
        # sizing
        sized = tuple(a[:SIZED] for a in cols)
        x = x0[:SIZED] + (x0[:SIZED] == 0.0) * 1.0
        y = ctx.quote_path(*sized, x)
        vi = np.where(y > 0, 0.5 * y / x, 1.0)
        for part, a in zip(("amount_in", "amount_out", "gain", "status"), ctx.size_path(*sized, 64.0 * x, vi, None, 5)):
            res[f"size_path.{part}"] = a
        bad, lim = spoil_paths(tuple(a[:100] for a in cols), 64.0 * (x0[:100] + (x0[:100] == 0.0) * 1.0))
        arrays = [bad[0]] + [T(a) for a in bad[1:]] + [lim]
        got = on_device(ctx, arrays, [(100, "f"), (100, "f"), (100, "f"), (100, "i")], lambda i, o: ctx.size_path_dev(100, H, *i, 0, 0, 5, *o))
        for part, a in zip(("amount_in", "amount_out", "gain", "status"), got):
            res[f"size_path_dev.{part}"] = a
    finally:
        be.close()

    # ---- the moving entries, a fresh context each
    for out, name in ((0, "swap"), (1, "swap_out")):
        be = fresh()
        try:
            ctx = be.ctx
            for s, b in enumerate(batches):
                idx, ci, co, amt = pool_queries(synth, b, s, out)
                if out:
                    quoted = ctx.quote_out(s, amt, ci, co, idx)
                    lim = np.where(np.arange(Q) % 3 == 0, 0.5, 2.0) * np.where(np.isfinite(quoted), quoted, 1.0)     # a third bind
                    res[f"{name}{s}"], res[f"{name}{s}.status"] = ctx.swap_out(s, amt, ci, co, idx, max_in=lim, status=True)
                else:
                    res[f"{name}{s}"] = ctx.swap(s, amt, ci, co, idx)
            states(ctx, batches, res, name, synth)
        finally:
            be.close()
    (cols, x0, y0) = paths(synth, batches, Q, distinct=True)
    for out, name in ((0, "swap_path"), (1, "swap_path_out")):
        be = fresh()
        try:
            ctx = be.ctx
            if out:
                quoted = ctx.quote_path_out(*cols, y0)
                lim = np.where(np.arange(Q) % 3 == 0, 0.5, 2.0) * np.where(np.isfinite(quoted), quoted, 1.0)
                res[name], res[name + ".status"], res[name + ".hops"] = ctx.swap_path_out(*cols, y0, max_in=lim, hops=True)
            else:
                quoted = ctx.quote_path(*cols, x0)
                lim = np.where(np.arange(Q) % 3 == 0, 2.0, 0.5) * np.where(np.isfinite(quoted), quoted, 1.0)
                res[name], res[name + ".status"], res[name + ".hops"] = ctx.swap_path(*cols, x0, min_out=lim, hops=True)
            states(ctx, batches, res, name, synth)
        finally:
            be.close()
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


def as_words(a):
    """the array as unsigned integers of its own width: what is compared"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])
