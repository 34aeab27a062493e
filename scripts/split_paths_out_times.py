"""cfmm_split_paths_out against cfmm_split_paths on the same orders, on the GPU.

    python scripts/split_paths_out_times.py [count ...]        -> stdout and profiles/split_paths_out.txt

scripts/split_paths_times.py's orders: K = 2, 4, 8 three-hop ProductTwoCoin paths over a market of 3 x count x K pools (every
path its own three pools), rounds = 5.  Per (count, K):
  split_paths_out   one call of Context.split_paths_out on count orders that each buy a tenth of what their paths' last pools
                    hold together: the kernel's span ("split_ns" under "time_kernels") and the wall time of the call;
  split_paths       one call of Context.split_paths on the same orders and rounds, on the same library: the same number of
                    path quotes (rounds x 64 per path) and of greedy steps, exact-input forms in place of exact-output ones.
The ratio of the two kernel spans is what the exact-output forms and the per-lane skip of a path that has answered +inf cost.
Each figure is the median of REPS calls after a warm-up call."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np

import cfmmrouter_amd as cr
from split_paths_times import REPS, ROUNDS, median_of, orders

OUT = os.path.join(ROOT, "profiles", "split_paths_out.txt")


def main(counts):
    lines = [f"cfmm_split_paths_out vs cfmm_split_paths on the same count orders of K paths; three-hop ProductTwoCoin paths, rounds = {ROUNDS}",
             f"median of {REPS} calls after a warm-up; kernel = device events (split_ns), wall = host clock around the synchronous calls",
             f"{'count':>8} {'K':>2} {'out kernel us':>14} {'out wall us':>12} {'in kernel us':>13} {'in wall us':>11} {'kernel ratio':>13}"]
    for count in counts:
        for K in (2, 4, 8):
            batch, first, amount, hops = orders(count, K)
            P = count * K
            want = 0.1 * np.add.reduceat(batch.R[2 * P:, 1], first[:-1])     # a tenth of the last hops' output reserves
            be = cr.DeviceBackend(4, [batch])
            ctx = be.ctx
            ctx.set_option("time_kernels", 1)
            try:
                def split_out():
                    t0 = time.perf_counter()
                    split_out.out = ctx.split_paths_out(first, want, *hops, ROUNDS)
                    return (ctx.get_option("split_ns") * 1e-3, (time.perf_counter() - t0) * 1e6)

                def split_in():
                    t0 = time.perf_counter()
                    ctx.split_paths(first, amount, *hops, ROUNDS)
                    return (ctx.get_option("split_ns") * 1e-3, (time.perf_counter() - t0) * 1e6)
                a, b = median_of(split_out), median_of(split_in)
                st = split_out.out[3]
                lines.append(f"{count:>8} {K:>2} {a[0]:>14.1f} {a[1]:>12.1f} {b[0]:>13.1f} {b[1]:>11.1f} {a[0] / b[0]:>13.2f}")
                lines.append(f"{'':>11} statuses: ok {int(np.sum(st == 0))}, none {int(np.sum(st == 1))}, nan {int(np.sum(st == 2))}, "
                             f"unobtainable {int(np.sum(st == 4))}")
            finally:
                be.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1, 64, 4096])
