"""cfmm_swap_order against cfmm_swap_path on the same flat paths, and against the way the job was done before the call existed,
on the GPU.

    python scripts/swap_order_times.py [count ...]        -> stdout and profiles/swap_order.txt

Batches of count pool-disjoint orders of K = 4 three-hop ProductTwoCoin paths over a market of 3 x count x K pools (every path
its own three pools: one wave).  Per batch, three ways of executing it, each with a limit per order that every order clears:
  order      one call of Context.swap_order: the kernel's span ("swap_ns" under "time_kernels") and the wall time of the call;
  flat       one call of Context.swap_path on the same count x K paths (no order-level limit: what the kernel does per path
             without the group step): the same loads and stores, one lane per path;
  before     the parent commit's way of doing the whole job: Context.quote_path on the paths, the totals and the limit test on
             the host (numpy), then Context.swap_path on the paths of the orders that pass -- kernel = "quote_ns" + "swap_ns",
             wall = all three steps;
  1 path     one call of Context.swap_path on the batch's first path alone: the latency of ONE path's walk and launch, which a
             one-lane-per-order kernel would pay about K times over for a lone order.
The ways are timed in turn inside every repetition (order, flat, before, 1 path, order, ...), so that whatever else shares the host
falls on all of them alike.  Every call moves the market by about a millionth of its reserves, so all repetitions see the same
work.  Each figure is the median of REPS repetitions after a warm-up of each; the spread is min .. max of the same repetitions."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import KIND_PRODUCT, ORDER_APPLIED, PATH_APPLIED

OUT = os.path.join(ROOT, "profiles", "swap_order.txt")
K, REPS = 4, 9


def orders(count, seed=3):
    """count orders of K paths of three product pools each, a -> b -> c -> d; every path carries a millionth of its first reserve"""
    rng = np.random.default_rng(seed)
    P = count * K
    R = 10.0 ** rng.uniform(4, 8, (3 * P, 2))
    Ai = np.tile(np.array([[1, 2]], dtype=np.int64), (3 * P, 1))
    Ai[P:2 * P] = [2, 3]
    Ai[2 * P:] = [3, 4]
    batch = cr.PoolBatch(KIND_PRODUCT, R=R, γ=np.full(3 * P, 0.997), Ai=Ai)
    n_hops = np.full(P, 3, dtype=np.int32)
    seg = np.zeros((P, 3), dtype=np.int32)
    row = (np.arange(P)[:, None] + P * np.arange(3)[None, :]).astype(np.int64)
    ci, co = np.zeros((P, 3), dtype=np.int32), np.ones((P, 3), dtype=np.int32)
    first = np.arange(0, P + 1, K, dtype=np.int64)
    return batch, first, 1e-6 * R[:P, 0], (n_hops, seg, row, ci, co)


def main(counts):
    lines = [f"cfmm_swap_order on count pool-disjoint orders of K = {K} three-hop ProductTwoCoin paths (one wave), beside cfmm_swap_path on the same",
             "flat paths and beside quote_path + host decision + swap_path (the way before the call existed); the ways (and cfmm_swap_path on one path alone) alternate inside every repetition",
             f"median of {REPS} repetitions after a warm-up (min .. max of the same repetitions); kernel = device events, wall = host clock around the synchronous calls; microseconds",
             f"{'count':>8} {'way':>7} {'kernel us':>11} {'kernel spread':>22} {'wall us':>11} {'wall spread':>22}"]
    for count in counts:
        batch, first, amount, hops = orders(count)
        be = cr.DeviceBackend(4, [batch])
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        limit = np.zeros(count)
        try:
            def order():
                t0 = time.perf_counter()
                out, total, status, _ = ctx.swap_order(first, *hops, amount, min_total_out=limit)
                wall = (time.perf_counter() - t0) * 1e6
                assert np.all(status == ORDER_APPLIED) and ctx.get_option("swap_launches") == 1
                return ctx.get_option("swap_ns") * 1e-3, wall

            def flat():
                t0 = time.perf_counter()
                out, status = ctx.swap_path(*hops, amount)
                wall = (time.perf_counter() - t0) * 1e6
                assert np.all(status == PATH_APPLIED) and ctx.get_option("swap_launches") == 1
                return ctx.get_option("swap_ns") * 1e-3, wall

            def before():
                t0 = time.perf_counter()
                quoted = ctx.quote_path(*hops, amount)
                quote_ns = ctx.get_option("quote_ns")
                passes = np.repeat(np.add.reduceat(quoted, first[:-1]) >= limit, K)
                assert np.all(passes)
                out, status = ctx.swap_path(*(h[passes] for h in hops), amount[passes], min_out=quoted[passes])
                wall = (time.perf_counter() - t0) * 1e6
                assert np.all(status == PATH_APPLIED)
                return (quote_ns + ctx.get_option("swap_ns")) * 1e-3, wall
            def one_path():
                t0 = time.perf_counter()
                out, status = ctx.swap_path(*(h[:1] for h in hops), amount[:1])
                wall = (time.perf_counter() - t0) * 1e6
                assert np.all(status == PATH_APPLIED)
                return ctx.get_option("swap_ns") * 1e-3, wall
            ways = (("order", order), ("flat", flat), ("before", before), ("1 path", one_path))
            for _, fn in ways:
                fn()
            samples = {name: [] for name, _ in ways}
            for _ in range(REPS):
                for name, fn in ways:
                    samples[name].append(fn())
            for name, _ in ways:
                k, w = np.array(samples[name]).T
                lines.append(f"{count:>8} {name:>7} {np.median(k):>11.1f} {f'{k.min():.1f} .. {k.max():.1f}':>22} {np.median(w):>11.1f} {f'{w.min():.1f} .. {w.max():.1f}':>22}")
            ko, kf = np.array(samples["order"])[:, 0], np.array(samples["flat"])[:, 0]
            lines.append(f"{'':>8} order kernel - flat kernel: {np.median(ko) - np.median(kf):+.1f} us (flat's own spread {kf.max() - kf.min():.1f} us); "
                         f"order / flat {np.median(ko) / np.median(kf):.2f}")
        finally:
            be.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 64, 4096, 65536])
