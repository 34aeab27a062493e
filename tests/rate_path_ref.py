"""The path contract of cfmm_quote_path_rate (include/cfmm_amd_rate.h) on the host, in numpy, operation by operation:
    x_0 = amount_in,  x_{k+1} = quote(hop k, x_k),  r_k = rate(hop k, x_k)
    hop_out[k, p] = x_{k+1},  hop_rate[k, p] = r_k,  rate[p] = ((r_0·r_1)·r_2)..., each product rounded on its own
Every hop is evaluated against the pool as it stands.  A hop of rate 0 (an exhausted ladder) makes the path's rate 0 and the
hops behind it are still evaluated.  Slots at k >= n_hops[p] are NaN.  What is no amount (negative, not finite) entering a
hop poisons that hop's amount AND rate, and both travel on; an n_hops outside 1 .. max_hops makes the whole path NaN with no
hop evaluated.  No device, no library."""
import numpy as np


def fold_rates(n_hops, hop_rate):
    """rate [count] from hop_rate [max_hops, count]: the left fold over the path's first n_hops[p] rows, in binary64"""
    n_hops = np.asarray(n_hops)
    hop_rate = np.asarray(hop_rate, dtype=np.float64)
    H, n = hop_rate.shape
    rate = np.full(n, np.nan)
    for p in range(n):
        if not 1 <= n_hops[p] <= H:
            continue
        f = hop_rate[0, p]
        for k in range(1, int(n_hops[p])):
            f = np.float64(f) * np.float64(hop_rate[k, p])
        rate[p] = f
    return rate


def walk(n_hops, max_hops, amount_in, hop):
    """hop(p, k, x) -> (amount out, rate) of hop k of path p entered with x, or None for a hop that is refused (bad segment,
    row or coins).  Returns (amount_out, rate, hop_out, hop_rate)."""
    n = len(n_hops)
    out, rate = np.full(n, np.nan), np.full(n, np.nan)
    hop_out, hop_rate = np.full((max_hops, n), np.nan), np.full((max_hops, n), np.nan)
    for p in range(n):
        if not 1 <= n_hops[p] <= max_hops:
            continue
        x, f = np.float64(amount_in[p]), np.float64(np.nan)
        for k in range(int(n_hops[p])):
            ans = hop(p, k, x) if (x >= 0.0 and np.isfinite(x)) else None
            x, r = (np.float64(np.nan), np.float64(np.nan)) if ans is None else (np.float64(ans[0]), np.float64(ans[1]))
            with np.errstate(invalid="ignore"):
                f = r if k == 0 else f * r
            hop_out[k, p], hop_rate[k, p] = x, r
        out[p], rate[p] = x, f
    return out, rate, hop_out, hop_rate
