"""cfmm_quote_to_rate against cfmm_quote_rate, and cfmm_swap_limit against cfmm_swap, on the same queries, on the GPU.

    python scripts/to_rate_times.py        -> stdout and profiles/to_rate.txt

The figure is the KERNEL's span as the command processor records it under "time_kernels" ("limit_ns" / "rate_ns" / "swap_ns").
There is no earlier time for a capability that did not exist: the yardstick is cfmm_quote_rate, the forward function, on the
same pools and queries in the same session.  Per family 16 384 and 1 048 576 dense queries (query q is row q) on synthetic
pools of that family, limits at 0.5 .. 0.999 of each pool's spot rate; the two entries alternate inside every repetition, and
the figure is the median of 15 calls after 3 warm-ups with min .. max, and the ratio of the medians.  cfmm_swap_limit against
cfmm_swap: 16 384 swaps of distinct Product rows (one wave), every swap limited at 0.9 of the spot rate with an amount that
stays short of it -- so both entries apply the same swaps -- on two contexts that hold the same market.
What to expect from the code alone: the closed-form families add a spot rate, a square root or an exp/log pair to the rate
kernel's work; Curve iterates (a median of 7 evaluations of the rate per query on the precision fixture in the host build, up to 101).
The pools are synthetic, one family per run: config 3's market has no Curve, Solidly, N-coin or multi-tick UniV3 pools."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

OUT = os.path.join(ROOT, "profiles", "to_rate.txt")
REPS, WARM = 15, 3
N = 64


def alternate(ctx, first, first_key, second, second_key):
    a_ns, b_ns = [], []
    for rep in range(REPS + WARM):
        first()
        a = ctx.get_option(first_key)
        second()
        b = ctx.get_option(second_key)
        if rep >= WARM:
            a_ns.append(a)
            b_ns.append(b)
    return np.array(a_ns), np.array(b_ns)


def line(name, what_a, a_ns, what_b, b_ns):
    ma, mb = float(np.median(a_ns)), float(np.median(b_ns))
    return (f"{name:<40s} {what_a} {ma / 1e3:9.2f} us ({a_ns.min() / 1e3:.2f} .. {a_ns.max() / 1e3:.2f})   "
            f"{what_b} {mb / 1e3:9.2f} us ({b_ns.min() / 1e3:.2f} .. {b_ns.max() / 1e3:.2f})   ratio {mb / ma:.3f}")


def families(count):
    """(name, pools, coin_out or None: the other coin)"""
    yield "Product", synth.product_pools(count, N, seed=3), None
    yield "GeometricMean", synth.geomean_pools(count, N, seed=4), None
    yield "Solidly", synth.solidly_pools(count, N, seed=5), None
    yield "weighted (3 coins)", synth.weighted_pools(count, N, 3, seed=6), 1
    yield "Curve (3 coins)", synth.curve_pools(count, N, 3, seed=7), 1
    yield "UniV3 (8 ticks)", synth.univ3_pools(count, N, 8, seed=8), None


def main():
    lines = ["# cfmm_quote_to_rate vs cfmm_quote_rate (dense, per family), cfmm_swap_limit vs cfmm_swap: kernel spans, medians of "
             "%d alternating calls after %d warm-ups (min .. max)" % (REPS, WARM)]
    for count in (16384, 1 << 20):
        for name, b, co in families(count):
            be = cr.DeviceBackend(N, [b])
            try:
                ctx = be.ctx
                ctx.set_option("time_kernels", 1)
                ci = np.zeros(count, dtype=np.int32)
                cout = None if co is None else np.full(count, co, dtype=np.int32)
                spot = ctx.quote_rate(0, None, ci, cout, None, count=count, want_out=False)[1]
                ok = np.isfinite(spot) & (spot > 0)
                lim = np.where(ok, spot, 1.0) * np.resize([0.999, 0.9, 0.5, 0.99], count)
                amount, out = ctx.quote_to_rate(0, lim, ci, cout)
                assert np.all(amount[ok] >= 0)
                back = ctx.quote_rate(0, np.where(np.isfinite(amount), amount, 0.0), ci, cout)[1]
                amount = np.where(np.isfinite(amount), amount, 0.0)
                a, t = alternate(ctx, lambda: ctx.quote_rate(0, amount, ci, cout), "rate_ns", lambda: ctx.quote_to_rate(0, lim, ci, cout), "limit_ns")
                inner = ok & np.isfinite(amount) & (amount > 0) & (back > 0)
                off = float(np.max(np.abs(back[inner] / lim[inner] - 1.0))) if inner.any() else float("nan")
                # (UniV3: a limit in an empty tick's range or below the last tick lands at a boundary, where the rate jumps past it)
                trip = "" if name.startswith("UniV3") else f"   max |rate(a)/r - 1| {off:.1e}"
                lines.append(line(f"{name}, {count} queries", "quote_rate", a, "quote_to_rate", t) + trip)
            finally:
                be.close()
    count = 16384
    b = synth.product_pools(count, N, seed=3)
    one, two = cr.DeviceBackend(N, [b]), cr.DeviceBackend(N, [b])
    try:
        for be in (one, two):
            be.ctx.set_option("time_kernels", 1)
        ci = np.zeros(count, dtype=np.int32)
        s_ns, l_ns = [], []
        for rep in range(REPS + WARM):
            spot = one.ctx.quote_rate(0, None, ci, None, None, count=count, want_out=False)[1]
            amt = 1e-4 * b.R[:, 0]
            want = one.ctx.swap(0, amt, ci)
            s = one.ctx.get_option("swap_ns")
            used, got, status = two.ctx.swap_limit(0, amt, 0.9 * spot, ci)
            l = two.ctx.get_option("swap_ns")
            assert np.array_equal(got, want) and np.all(status == cr.LIMIT_FILLED)
            if rep >= WARM:
                s_ns.append(s)
                l_ns.append(l)
        lines.append(line(f"Product, {count} swaps, one wave", "swap", np.array(s_ns), "swap_limit", np.array(l_ns)))
    finally:
        one.close()
        two.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text)


if __name__ == "__main__":
    main()
