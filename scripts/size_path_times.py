"""cfmm_size_path against the same work done with cfmm_quote_path alone, on the GPU.

    python scripts/size_path_times.py [count ...]        -> stdout and profiles/size_path.txt

Three-hop ProductTwoCoin cycles over a market of 3 x `count` pools (every cycle its own three pools), rounds = 5.  Per count:
  size_path     one call of Context.size_path: the kernel's span ("size_ns" under "time_kernels") and the wall time of the call
                (staging, copies, launch, synchronise, read-back);
  quote ladder  what a caller could do before: five calls of Context.quote_path on 64 x count paths (the hop arrays repeated 64
                times), the trial sizes, gains, arg-max and next bracket in numpy between them -- the kernels' spans ("quote_ns",
                summed) and the wall time of the whole.
The ladder's 64 x copy of the hop arrays is made once and is not timed.  Both give the same answers (asserted, bit for bit).
Each figure is the median of REPS (the ladder: LADDER_REPS) calls after a warm-up call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import KIND_PRODUCT
from size_path_ref import size_path_ref

OUT = os.path.join(ROOT, "profiles", "size_path.txt")
ROUNDS, REPS, LADDER_REPS = 5, 7, 3


def cycles(count, seed=3):
    """count cycles of three product pools: a -> b -> c -> a with 0.5 .. 3 % round the cycle before fees"""
    rng = np.random.default_rng(seed)
    R = 10.0 ** rng.uniform(4, 8, (3 * count, 2))
    edge = 1.0 + rng.uniform(0.005, 0.03, count)
    R[2 * count:, 1] = R[2 * count:, 0] * (R[:count, 0] / R[:count, 1]) * (R[count:2 * count, 0] / R[count:2 * count, 1]) * edge
    gamma = np.full(3 * count, 0.9995)
    Ai = np.tile(np.array([[1, 2]], dtype=np.int64), (3 * count, 1))
    Ai[count:2 * count] = [2, 3]
    Ai[2 * count:] = [3, 1]
    batch = cr.PoolBatch(KIND_PRODUCT, R=R, γ=gamma, Ai=Ai)
    n_hops = np.full(count, 3, dtype=np.int32)
    seg = np.zeros((count, 3), dtype=np.int32)
    row = (np.arange(count)[:, None] + count * np.arange(3)[None, :]).astype(np.int64)
    ci = np.zeros((count, 3), dtype=np.int32)
    co = np.ones((count, 3), dtype=np.int32)
    return batch, (n_hops, seg, row, ci, co), 0.2 * R[:count, 0]


def median_of(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t.append(fn())
    return tuple(float(np.median([s[k] for s in t])) for k in range(len(t[0])))


def main(counts):
    lines = [f"cfmm_size_path vs {ROUNDS} x cfmm_quote_path on 64 x count paths + numpy selection; three-hop ProductTwoCoin cycles, rounds = {ROUNDS}",
             f"median of {REPS} calls (the ladder: {LADDER_REPS}) after a warm-up; kernel = device events (size_ns / summed quote_ns), wall = host clock around the synchronous calls",
             f"{'count':>8} {'size kernel us':>15} {'size wall us':>13} {'ladder kernels us':>18} {'ladder wall us':>15} {'wall ratio':>11}"]
    for count in counts:
        batch, hops, max_in = cycles(count)
        be = cr.DeviceBackend(3, [batch])
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        try:
            def sized():
                t0 = time.perf_counter()
                sized.out = ctx.size_path(*hops, max_in, None, None, ROUNDS)
                return (ctx.get_option("size_ns") * 1e-3, (time.perf_counter() - t0) * 1e6)

            def ladder():
                ns = [0]

                def quote(idx, x):                                   # (every trial size of these markets is an amount: idx is all of them)
                    y = ctx.quote_path(*repeated, x)
                    ns[0] += ctx.get_option("quote_ns")
                    return y
                t0 = time.perf_counter()
                ladder.out = size_path_ref(quote, max_in, None, None, ROUNDS)
                return (ns[0] * 1e-3, (time.perf_counter() - t0) * 1e6)
            repeated = tuple(np.repeat(a, 64, axis=0) for a in hops)   # the ladder's 64 x copy of the hop arrays, made once, untimed
            a, b = median_of(sized), median_of(ladder, LADDER_REPS)
            for u, v in zip(sized.out, ladder.out):
                assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)), "the two ways disagree"
            st = sized.out[3]
            lines.append(f"{count:>8} {a[0]:>15.1f} {a[1]:>13.1f} {b[0]:>18.1f} {b[1]:>15.1f} {b[1] / a[1]:>11.1f}")
            lines.append(f"{'':>8} statuses: sized {int(np.sum(st == 0))}, none {int(np.sum(st == 1))}, at limit {int(np.sum(st == 2))}, nan {int(np.sum(st == 3))}")
        finally:
            be.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 100_000])
