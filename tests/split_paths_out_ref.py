"""The contract of cfmm_split_paths_out (include/cfmm_amd_split_out.h) on the host, in numpy: the greedy search with scaling over
the OUTPUT, operation by operation.  It knows nothing of pools: the market is a callable quote_path_out(path_index_array,
amounts) -> costs that answers what buying amounts[i] through path path_index_array[i] costs, +inf where the path cannot give
that much (ctx.quote_path_out on the device tests, a plain-numpy closed form on the CPU tests).  Every step is one rounded
binary64 operation, in the order the header states.  The grid points are split_paths_ref's; the orders are worked on side by
side ([orders, 8 paths, 64 points] arrays; the slots of paths an order does not have are never chosen)."""
import numpy as np

from split_paths_ref import MAX_PATHS, MAX_ROUNDS, POINTS, SPLIT_NAN, SPLIT_NONE, SPLIT_OK, grid_points

SPLIT_UNOBTAINABLE = 4
CLEAN, BAD_INF, BAD_NAN = 0, 1, 2      # what the first step with a taken increment that is not finite was


def best_path_out(d, active):
    """per row the smallest k among the active ones whose d is the SMALLEST, compared as numbers (+inf is one); a NaN loses to
    every number (no active d is a number: 0).  -> (k*, d[k*])"""
    nan = np.isnan(d) | ~active
    rows = np.arange(d.shape[0])
    some = ~nan.all(axis=1)
    k = np.argmin(np.where(nan, np.inf, d), axis=1)              # (the first of equals -- but a NaN in front of a true +inf ties it)
    fix = nan[rows, k] & some
    k[fix] = np.argmax(~nan[fix], axis=1)                        # every number there is +inf: the first of them
    k[~some] = 0
    return k, np.where(some, d[rows, k], np.nan)


def greedy_out(c, K, bad=None):
    """one round's 63 steps on c [G, 8, 64] -> (n [G, 8], bad [G]): bad carries CLEAN / BAD_INF / BAD_NAN through the rounds, set
    by the FIRST step whose taken increment is not finite and never again"""
    G = c.shape[0]
    rows = np.arange(G)
    active = np.arange(MAX_PATHS)[None, :] < K[:, None]
    n = np.zeros((G, MAX_PATHS), dtype=np.int64)
    bad = np.zeros(G, dtype=np.int64) if bad is None else bad.copy()
    paths = np.arange(MAX_PATHS)[None, :]
    for _ in range(POINTS - 1):
        at = np.minimum(n, POINTS - 2)                           # (a path that holds all 63 slices is asked for nothing more)
        with np.errstate(invalid="ignore"):
            d = c[rows[:, None], paths, at + 1] - c[rows[:, None], paths, at]
        k, dk = best_path_out(d, active)
        now = np.where(np.isfinite(dk), CLEAN, np.where(np.isnan(dk), BAD_NAN, BAD_INF))
        bad = np.where(bad == CLEAN, now, bad)
        n[rows, k] += 1
    return n, bad


def split_paths_out_ref(quote_path_out, order_first, amount_out, rounds=5, trace=None):
    """-> (path_amount_out [n_paths], path_amount_in [n_paths], total_in [orders], status [orders]).  An amount that is no valid
    number makes the order SPLIT_NAN, as the device-pointer entry does.  trace: a list that receives every round's
    (x [G, 8, 64], c [G, 8, 64], n [G, 8], rem [G], bad [G]); slots of paths an order does not have hold NaN."""
    assert 1 <= rounds <= MAX_ROUNDS
    first = np.ascontiguousarray(order_first, dtype=np.int64).reshape(-1)
    B0 = np.ascontiguousarray(amount_out, dtype=np.float64).reshape(-1)
    G = B0.size
    assert first.size == G + 1
    K = np.diff(first)
    assert np.all((K >= 1) & (K <= MAX_PATHS))
    n_paths = int(first[-1])
    valid = (B0 >= 0) & np.isfinite(B0)
    B = np.where(valid, B0, np.nan)
    active = np.arange(MAX_PATHS)[None, :] < K[:, None]                        # [G, 8]
    path_of = np.where(active, first[:-1, None] + np.arange(MAX_PATHS)[None, :], 0)
    base = np.zeros((G, MAX_PATHS))
    rem = B.copy()
    bad = np.zeros(G, dtype=np.int64)
    x = c = n = None
    for r in range(rounds):
        x = grid_points(base, np.broadcast_to(rem[:, None], base.shape))
        c = np.full(x.shape, np.nan)
        ask = active[:, :, None] & np.isfinite(x) & (x >= 0)               # (anything else is no amount: NaN, quote_path_out's rule)
        if ask.any():
            idx = np.broadcast_to(path_of[:, :, None], x.shape)
            c[ask] = quote_path_out(idx[ask], x[ask])
        n, bad = greedy_out(c, K, bad)
        if trace is not None:
            trace.append((np.where(active[:, :, None], x, np.nan), c, n.copy(), rem.copy(), bad.copy()))
        if r + 1 < rounds:
            m = np.maximum(n - 1, 0)
            base = np.take_along_axis(x, m[:, :, None], axis=2)[:, :, 0]
            total = base[:, 0].copy()
            for k in range(1, MAX_PATHS):
                total = np.where(k < K, total + base[:, k], total)
            with np.errstate(invalid="ignore"):
                rem = np.maximum(B - total, 0.0)
    xs = np.take_along_axis(x, n[:, :, None], axis=2)[:, :, 0]
    cs = np.take_along_axis(c, n[:, :, None], axis=2)[:, :, 0]
    total = cs[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, MAX_PATHS):
            total = np.where(k < K, total + cs[:, k], total)
    status = answer_status(bad, B, total)
    xs = written(xs, status[:, None], cost=False)
    cs = written(cs, status[:, None], cost=True)
    total = written(total, status, cost=True)
    share, cost = np.empty(n_paths), np.empty(n_paths)
    share[path_of[active]] = xs[active]
    cost[path_of[active]] = cs[active]
    return share, cost, total, status


def answer_status(bad, B, total):
    """the first bad step decides; then a total that is no number; then B == 0"""
    status = np.where(B == 0, SPLIT_NONE, SPLIT_OK).astype(np.int32)
    status[(bad == BAD_NAN) | np.isnan(total)] = SPLIT_NAN
    status[bad == BAD_INF] = SPLIT_UNOBTAINABLE
    return status


def written(v, st, cost):
    """what an order of status st has written: NaN; +0.0; +inf for the costs and +0.0 for the shares; the value"""
    out = np.where(st == SPLIT_OK, v, 0.0)
    out = np.where(st == SPLIT_NAN, np.nan, out)
    if cost:
        out = np.where(st == SPLIT_UNOBTAINABLE, np.inf, out)
    return out
