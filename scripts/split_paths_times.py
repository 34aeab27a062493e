"""cfmm_split_paths against cfmm_size_path on the same paths, on the GPU.

    python scripts/split_paths_times.py [count ...]        -> stdout and profiles/split_paths.txt

Orders of K = 2, 4, 8 three-hop ProductTwoCoin paths over a market of 3 x count x K pools (every path its own three pools),
rounds = 5.  Per (count, K):
  split_paths   one call of Context.split_paths on count orders: the kernel's span ("split_ns" under "time_kernels") and the
                wall time of the call (staging, copies, launch, synchronise, read-back);
  size_path     one call of Context.size_path on the same count x K paths and rounds, on the same library: the same number of
                path quotes (rounds x 64 per path), one wavefront per PATH and a six-step arg-max per round where split_paths
                has one wavefront per ORDER and 63 greedy steps per round.
The ratio of the two kernel spans is what the greedy steps and the K-fold narrower parallelism cost over the quotes alone.
Each figure is the median of REPS calls after a warm-up call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import KIND_PRODUCT

OUT = os.path.join(ROOT, "profiles", "split_paths.txt")
ROUNDS, REPS = 5, 7


def orders(count, K, seed=3):
    """count orders of K paths of three product pools each, a -> b -> c -> d; the amount is a fifth of the order's first reserves"""
    rng = np.random.default_rng(seed)
    P = count * K
    R = 10.0 ** rng.uniform(4, 8, (3 * P, 2))
    gamma = np.full(3 * P, 0.997)
    Ai = np.tile(np.array([[1, 2]], dtype=np.int64), (3 * P, 1))
    Ai[P:2 * P] = [2, 3]
    Ai[2 * P:] = [3, 4]
    batch = cr.PoolBatch(KIND_PRODUCT, R=R, γ=gamma, Ai=Ai)
    n_hops = np.full(P, 3, dtype=np.int32)
    seg = np.zeros((P, 3), dtype=np.int32)
    row = (np.arange(P)[:, None] + P * np.arange(3)[None, :]).astype(np.int64)
    ci = np.zeros((P, 3), dtype=np.int32)
    co = np.ones((P, 3), dtype=np.int32)
    first = np.arange(0, P + 1, K, dtype=np.int64)
    amount = 0.2 * np.add.reduceat(R[:P, 0], first[:-1])
    return batch, first, amount, (n_hops, seg, row, ci, co)


def median_of(fn, reps=REPS):
    fn()
    t = []
    for _ in range(reps):
        t.append(fn())
    return tuple(float(np.median([s[k] for s in t])) for k in range(len(t[0])))


def main(counts):
    lines = [f"cfmm_split_paths on count orders of K paths vs cfmm_size_path on the same count x K paths; three-hop ProductTwoCoin paths, rounds = {ROUNDS}",
             f"median of {REPS} calls after a warm-up; kernel = device events (split_ns / size_ns), wall = host clock around the synchronous calls",
             f"{'count':>8} {'K':>2} {'split kernel us':>16} {'split wall us':>14} {'size kernel us':>15} {'size wall us':>13} {'kernel ratio':>13}"]
    for count in counts:
        for K in (2, 4, 8):
            batch, first, amount, hops = orders(count, K)
            be = cr.DeviceBackend(4, [batch])
            ctx = be.ctx
            ctx.set_option("time_kernels", 1)
            try:
                def split():
                    t0 = time.perf_counter()
                    split.out = ctx.split_paths(first, amount, *hops, ROUNDS)
                    return (ctx.get_option("split_ns") * 1e-3, (time.perf_counter() - t0) * 1e6)

                def sized():
                    t0 = time.perf_counter()
                    ctx.size_path(*hops, np.repeat(amount, K), None, 1e-3, ROUNDS)
                    return (ctx.get_option("size_ns") * 1e-3, (time.perf_counter() - t0) * 1e6)
                a, b = median_of(split), median_of(sized)
                st = split.out[3]
                lines.append(f"{count:>8} {K:>2} {a[0]:>16.1f} {a[1]:>14.1f} {b[0]:>15.1f} {b[1]:>13.1f} {a[0] / b[0]:>13.2f}")
                lines.append(f"{'':>11} statuses: ok {int(np.sum(st == 0))}, none {int(np.sum(st == 1))}, nan {int(np.sum(st == 2))}, saturated {int(np.sum(st == 3))}")
            finally:
                be.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 64, 4096])
