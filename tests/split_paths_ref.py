"""The contract of cfmm_split_paths (include/cfmm_amd_split.h) on the host, in numpy: the greedy search with scaling, operation
by operation.  It knows nothing of pools: the market is a callable quote_path(path_index_array, amounts) -> amounts that
answers what carrying amounts[i] through path path_index_array[i] gives (ctx.quote_path on the device tests, a plain-numpy
closed form on the CPU tests).  Every step is one rounded binary64 operation, in the order the header states.  The orders are
worked on side by side ([orders, 8 paths, 64 points] arrays; the slots of paths an order does not have are never chosen)."""
import numpy as np

POINTS = 64                # CFMM_SPLIT_POINTS
MAX_PATHS = 8              # CFMM_MAX_SPLIT_PATHS
MAX_ROUNDS = 16            # CFMM_MAX_SPLIT_ROUNDS
SPLIT_OK, SPLIT_NONE, SPLIT_NAN, SPLIT_SATURATED = 0, 1, 2, 3


def grid_points(base, rem):
    """[.., 64]: x_j = base + (rem / 63) * j for j <= 62 (the quotient, the product, the sum), x_63 = base + rem"""
    base, rem = np.asarray(base, dtype=np.float64), np.asarray(rem, dtype=np.float64)
    s = rem / np.float64(POINTS - 1)
    d = s[..., None] * np.arange(POINTS, dtype=np.float64)
    x = base[..., None] + d
    x[..., POINTS - 1] = base + rem
    return x


def best_path(d, active):
    """per row the smallest k among the active ones whose d is the largest, compared as numbers; a NaN loses to every number
    (no active d is a number: 0).  -> (k*, whether some active d is a number)"""
    nan = np.isnan(d) | ~active
    key = np.where(nan, -np.inf, d)
    k = np.argmax(key, axis=1)                                   # (the first of equals)
    rows = np.arange(d.shape[0])
    some = ~nan.all(axis=1)
    fix = (key[rows, k] == -np.inf) & some                       # a true -inf still beats a NaN in front of it
    k[fix] = np.argmax(~nan[fix], axis=1)
    k[~some] = 0
    return k, some


def greedy(y, K):
    """one round's 63 steps on y [G, 8, 64] -> (n [G, 8], a step had no increment that is a number [G], a step took an
    increment that is a number but not > 0 [G])"""
    G = y.shape[0]
    rows = np.arange(G)
    active = np.arange(MAX_PATHS)[None, :] < K[:, None]
    n = np.zeros((G, MAX_PATHS), dtype=np.int64)
    step_nan, step_flat = np.zeros(G, dtype=bool), np.zeros(G, dtype=bool)
    paths = np.arange(MAX_PATHS)[None, :]
    for _ in range(POINTS - 1):
        at = np.minimum(n, POINTS - 2)                           # (a path that holds all 63 slices is asked for nothing more)
        d = y[rows[:, None], paths, at + 1] - y[rows[:, None], paths, at]
        k, some = best_path(d, active)
        step_nan |= ~some
        step_flat |= some & ~(d[rows, k] > 0)
        n[rows, k] += 1
    return n, step_nan, step_flat


def split_paths_ref(quote_path, order_first, amount_in, rounds=5, trace=None):
    """-> (path_amount_in [n_paths], path_amount_out [n_paths], total_out [orders], status [orders]).  An amount that is no valid
    number makes the order SPLIT_NAN, as the device-pointer entry does.  trace: a list that receives every round's
    (x [G, 8, 64], y [G, 8, 64], n [G, 8], rem [G]); slots of paths an order does not have hold NaN."""
    assert 1 <= rounds <= MAX_ROUNDS
    first = np.ascontiguousarray(order_first, dtype=np.int64).reshape(-1)
    A0 = np.ascontiguousarray(amount_in, dtype=np.float64).reshape(-1)
    G = A0.size
    assert first.size == G + 1
    K = np.diff(first)
    assert np.all((K >= 1) & (K <= MAX_PATHS))
    n_paths = int(first[-1])
    valid = (A0 >= 0) & np.isfinite(A0)
    A = np.where(valid, A0, np.nan)
    rows = np.arange(G)
    active = np.arange(MAX_PATHS)[None, :] < K[:, None]                        # [G, 8]
    path_of = np.where(active, first[:-1, None] + np.arange(MAX_PATHS)[None, :], 0)
    base = np.zeros((G, MAX_PATHS))
    rem = A.copy()
    any_nan = np.zeros(G, dtype=bool)
    last_flat = np.zeros(G, dtype=bool)
    x = y = n = None
    for r in range(rounds):
        x = grid_points(base, np.broadcast_to(rem[:, None], base.shape))
        y = np.full(x.shape, np.nan)
        ask = active[:, :, None] & np.isfinite(x) & (x >= 0)               # (anything else is no amount: NaN, quote_path's rule)
        if ask.any():
            idx = np.broadcast_to(path_of[:, :, None], x.shape)
            y[ask] = quote_path(idx[ask], x[ask])
        n, step_nan, last_flat = greedy(y, K)
        any_nan |= step_nan
        if trace is not None:
            trace.append((np.where(active[:, :, None], x, np.nan), y, n.copy(), rem.copy()))
        if r + 1 < rounds:
            m = np.maximum(n - 1, 0)
            base = np.take_along_axis(x, m[:, :, None], axis=2)[:, :, 0]
            total = base[:, 0].copy()
            for k in range(1, MAX_PATHS):
                total = np.where(k < K, total + base[:, k], total)
            with np.errstate(invalid="ignore"):
                rem = np.maximum(A - total, 0.0)
    xs = np.take_along_axis(x, n[:, :, None], axis=2)[:, :, 0]
    ys = np.take_along_axis(y, n[:, :, None], axis=2)[:, :, 0]
    total = ys[:, 0].copy()
    for k in range(1, MAX_PATHS):
        total = np.where(k < K, total + ys[:, k], total)
    is_nan = any_nan | np.isnan(total)
    none = ~is_nan & ((A == 0) | ~(total > 0))
    status = np.where(last_flat, SPLIT_SATURATED, SPLIT_OK).astype(np.int32)
    status[none] = SPLIT_NONE
    status[is_nan] = SPLIT_NAN
    put = lambda v, per_order: np.where(is_nan[:, None] if not per_order else is_nan, np.nan, np.where(none[:, None] if not per_order else none, 0.0, v))
    xs, ys, total = put(xs, False), put(ys, False), put(total, True)
    path_in, path_out = np.empty(n_paths), np.empty(n_paths)
    path_in[path_of[active]] = xs[active]
    path_out[path_of[active]] = ys[active]
    return path_in, path_out, total, status
