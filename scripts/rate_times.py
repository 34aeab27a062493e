"""cfmm_quote_rate against cfmm_quote, and cfmm_quote_path_rate against cfmm_quote_path, on the same queries, on the GPU.

    python scripts/rate_times.py        -> stdout and profiles/rate.txt

The figure is the KERNEL's span as the command processor records it under "time_kernels" ("quote_ns" / "rate_ns"): the two
entries stage and copy the same columns, and differ in their kernels.  The baseline is cfmm_quote / cfmm_quote_path, the entries
that exist without this feature.  The two alternate inside every repetition (quote, rate, quote, rate, ...), so that clock
and cache state drift hits both alike; per case: the median of REPS repetitions after a warm-up pair, with min..max, and the
ratio of the medians.  Cases:
    dense Product at 1, 4 096 and 1 048 576 queries (idx == NULL: query q is row q)
    65 536 queries on UniV3 pools with 8 .. 64 ticks, amounts spread over the whole ladder (sparse idx)
    65 536 three-hop paths through Product pools, against cfmm_quote_path
What to expect from the code alone: the quote's loads, one more 8-byte store per query and a handful of FP64 operations."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

OUT = os.path.join(ROOT, "profiles", "rate.txt")
REPS = 9
N = 64


def alternate(ctx, quote, rate):
    """[REPS] kernel spans of each, the calls alternating; one warm-up pair first"""
    q_ns, r_ns = [], []
    for rep in range(REPS + 1):
        quote()
        a = ctx.get_option("quote_ns")
        rate()
        b = ctx.get_option("rate_ns")
        if rep:
            q_ns.append(a)
            r_ns.append(b)
    return np.array(q_ns), np.array(r_ns)


def line(name, q_ns, r_ns):
    mq, mr = float(np.median(q_ns)), float(np.median(r_ns))
    return (f"{name:<44s} quote {mq / 1e3:9.2f} us ({q_ns.min() / 1e3:.2f} .. {q_ns.max() / 1e3:.2f})   "
            f"rate {mr / 1e3:9.2f} us ({r_ns.min() / 1e3:.2f} .. {r_ns.max() / 1e3:.2f})   ratio {mr / mq:.3f}")


def main():
    lines = ["# cfmm_quote_rate vs cfmm_quote, cfmm_quote_path_rate vs cfmm_quote_path: kernel spans, medians of %d alternating "
             "repetitions after a warm-up (min .. max)" % REPS]
    # dense Product
    for count in (1, 4096, 1 << 20):
        b = synth.product_pools(count, N, seed=3)
        be = cr.DeviceBackend(N, [b])
        try:
            ctx = be.ctx
            ctx.set_option("time_kernels", 1)
            ci = (np.arange(count) % 2).astype(np.int32)
            a = 0.01 * b.R[np.arange(count), ci]
            ref = ctx.quote(0, a, ci)
            out, rate = ctx.quote_rate(0, a, ci)
            assert np.array_equal(out, ref) and np.all(rate > 0)
            q, r = alternate(ctx, lambda: ctx.quote(0, a, ci), lambda: ctx.quote_rate(0, a, ci))
            lines.append(line(f"Product, dense, {count} queries", q, r))
        finally:
            be.close()
    # multi-tick UniV3
    count, m = 65536, 4096
    b = synth.univ3_ragged_pools(m, N, min_ticks=8, max_ticks=64, seed=5)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        rng = np.random.default_rng(6)
        idx = rng.integers(0, m, count)
        ci = (np.arange(count) % 2).astype(np.int32)
        scale = np.sqrt(b.liquidity[b.tick_off[:-1]][idx] + 1.0)
        a = scale * 10.0 ** rng.uniform(-3, 1.5, count)
        ref = ctx.quote(0, a, ci, None, idx)
        out, rate = ctx.quote_rate(0, a, ci, None, idx)
        assert np.array_equal(out, ref) and np.all(rate >= 0)
        q, r = alternate(ctx, lambda: ctx.quote(0, a, ci, None, idx), lambda: ctx.quote_rate(0, a, ci, None, idx))
        lines.append(line(f"UniV3 8..64 ticks, sparse, {count} queries", q, r))
    finally:
        be.close()
    # three-hop paths
    count, m = 65536, 65536
    b = synth.product_pools(m, N, seed=7)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        rng = np.random.default_rng(8)
        n_hops = np.full(count, 3, dtype=np.int32)
        seg = np.zeros((count, 3), dtype=np.int32)
        row = rng.integers(0, m, (count, 3))
        ci = rng.integers(0, 2, (count, 3)).astype(np.int32)
        co = (1 - ci).astype(np.int32)
        a = 0.01 * b.R[row[:, 0], ci[:, 0]]
        ref = ctx.quote_path(n_hops, seg, row, ci, co, a)
        out, rate = ctx.quote_path_rate(n_hops, seg, row, ci, co, a)
        assert np.array_equal(out, ref) and np.all(rate > 0)
        q, r = alternate(ctx, lambda: ctx.quote_path(n_hops, seg, row, ci, co, a), lambda: ctx.quote_path_rate(n_hops, seg, row, ci, co, a))
        lines.append(line(f"three-hop Product paths, {count} paths", q, r))
    finally:
        be.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
