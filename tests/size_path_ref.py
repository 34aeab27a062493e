"""The contract of cfmm_size_path (include/cfmm_amd_size_path.h) on the host, in numpy: the bracketing search, operation by
operation.  It knows nothing of pools: the market is a callable quote_path(path_index_array, amounts) -> amounts that answers
what carrying amounts[i] through path path_index_array[i] gives (ctx.quote_path on the device tests, a plain-numpy closed
form on the CPU tests).  Every step is one rounded binary64 operation, in the order the header states."""
import numpy as np

POINTS = 64                # CFMM_SIZE_POINTS
MAX_ROUNDS = 16            # CFMM_MAX_SIZE_ROUNDS
SIZED, SIZED_NONE, SIZED_AT_LIMIT, SIZED_NAN = 0, 1, 2, 3


def trial_sizes(lo, hi):
    """[n, 64]: x_0 = lo, x_63 = hi, otherwise min(lo + (hi - lo) * (j / 63.0), hi)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    t = np.arange(POINTS, dtype=np.float64) / np.float64(POINTS - 1)
    w = hi - lo
    d = w[:, None] * t[None, :]
    x = lo[:, None] + d
    x = np.minimum(x, hi[:, None])
    x[:, 0] = lo
    x[:, POINTS - 1] = hi
    return x


def gains(value_in, value_out, x, y):
    a = value_out[:, None] * y
    b = value_in[:, None] * x
    return a - b


def select(g):
    """per row the smallest j whose g is the largest, compared as numbers; a NaN loses to every number (all NaN: 0)"""
    nan = np.isnan(g)
    key = np.where(nan, -np.inf, g)
    j = np.argmax(key, axis=1)                                   # (the first of equals)
    rows = np.arange(g.shape[0])
    fix = (key[rows, j] == -np.inf) & ~nan.all(axis=1)            # a true -inf still beats a NaN in front of it
    j[fix] = np.argmax(~nan[fix], axis=1)
    return j


def size_path_ref(quote_path, max_in, value_in=None, value_out=None, rounds=5, trace=None):
    """-> (amount_in, amount_out, gain, status).  A max_in or value that is no valid number makes the path SIZED_NAN, as the
    device-pointer entry does.  trace: a list that receives every round's (x [n, 64], g [n, 64], j* [n])."""
    assert 1 <= rounds <= MAX_ROUNDS
    max_in = np.ascontiguousarray(max_in, dtype=np.float64).reshape(-1)
    n = max_in.size
    vi = np.ones(n) if value_in is None else np.broadcast_to(np.asarray(value_in, dtype=np.float64), (n,)).copy()
    vo = np.ones(n) if value_out is None else np.broadcast_to(np.asarray(value_out, dtype=np.float64), (n,)).copy()
    valid = (max_in >= 0) & np.isfinite(max_in) & (vi > 0) & np.isfinite(vi) & (vo > 0) & np.isfinite(vo)
    lo = np.where(valid, 0.0, np.nan)
    hi = np.where(valid, max_in, np.nan)
    rows = np.arange(n)
    idx = np.repeat(rows, POINTS)
    any_nan = np.zeros(n, dtype=bool)
    bx = by = bg = np.zeros(n)
    for _ in range(rounds):
        x = trial_sizes(lo, hi)
        y = np.full((n, POINTS), np.nan)
        ask = np.isfinite(x) & (x >= 0)                           # (anything else is no amount: NaN, quote_path's rule)
        if ask.any():
            y[ask] = quote_path(idx[ask.ravel()], x[ask])
        g = gains(vi, vo, x, y)
        j = select(g)
        if trace is not None:
            trace.append((x, g, j))
        bx, by, bg = x[rows, j], y[rows, j], g[rows, j]
        any_nan |= np.isnan(bg)
        lo, hi = x[rows, np.maximum(j - 1, 0)], x[rows, np.minimum(j + 1, POINTS - 1)]
    status = np.where(bx == max_in, SIZED_AT_LIMIT, SIZED).astype(np.int32)
    none = ~(bg > 0)
    status[none] = SIZED_NONE
    status[any_nan] = SIZED_NAN
    out = [np.where(none, 0.0, v) for v in (bx, by, bg)]
    out = [np.where(any_nan, np.nan, v) for v in out]
    return out[0], out[1], out[2], status
