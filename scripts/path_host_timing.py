"""Host wall time per call of the path entries, by the protocol of profiles/query_host_timing.txt: the median of
time.perf_counter around one host-pointer call through the Python Context method, after untimed warm-up calls.  One run measures
the library CFMM_AMD_LIB names (default: this tree's); profiles/path_host_timing.txt holds parent1, result1, parent2, result2 of
one session and the table `--table` makes of them.

    python scripts/path_host_timing.py > run.txt                     # one run, on the MI355X
    python scripts/path_host_timing.py --table p1 r1 p2 r2           # the table of four runs

Market: that file's (500 000 ProductTwoCoin + 500 000 GeometricMeanTwoCoin pools, 256 tokens) plus one UniV3 segment of 65 536
pools (3 ticks).  Paths: two hops, row q of segment 0 then row q of segment 1 (distinct rows: one wave); amounts 1e-7 of the
tendered reserve (exact output: half of what that quotes), so the executions barely move the pools over the repetitions.  Orders:
8 paths each (8 192 orders at 65 536 paths; one order of one path at count 1).  `swap`: the UniV3 segment, rows 0 .. count - 1.
"single" = one context on device 0, "parent[0,0]" = a two-shard parent on the same device (the four read-only entries)."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, MU = 256, 500000, 65536
BIG = 65536
ROUNDS = 5


def median_ms(call, reps, warm=3):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(t)


def run():
    import cfmmrouter_amd as cr
    from cfmmrouter_amd import synth
    batches = [synth.product_pools(M, N, seed=1), synth.geomean_pools(M, N, seed=2), synth.univ3_pools(MU, N, 3, seed=3)]
    print(f"# library: {os.environ.get('CFMM_AMD_LIB', 'this tree')}", flush=True)
    for who, device in (("single", 0), ("parent[0,0]", [0, 0])):
        be = cr.DeviceBackend(N, batches, device=device)
        try:
            ctx = be.ctx
            for count in (1, BIG):
                reps = 200 if count == 1 else 20
                q = np.arange(count)
                n_hops = np.full(count, 2, dtype=np.int32)
                seg = np.tile(np.array([0, 1], dtype=np.int32), (count, 1))
                row = np.stack([q, q], axis=1).astype(np.int64)
                ci = np.tile(np.array([0, 1], dtype=np.int32), (count, 1))
                co = 1 - ci
                cols = (n_hops, seg, row, ci, co)
                x = 1e-7 * batches[0].R[q, 0]
                y = 0.5 * ctx.quote_path(*cols, x)
                K = 8 if count > 1 else 1
                first = np.arange(0, count + 1, K, dtype=np.int64)
                ax = x.reshape(-1, K).sum(axis=1)
                ay = y.reshape(-1, K).sum(axis=1)
                slow = 5 if (count > 1 and who != "single") else reps          # a parent's search: 5 rounds of 64 x count paths
                say = lambda name, ms: print(f"{name} {who} count={count}\t{ms:.4f}", flush=True)
                say("quote_path", median_ms(lambda: ctx.quote_path(*cols, x), reps))
                say("size_path", median_ms(lambda: ctx.size_path(*cols, 64.0 * x, None, None, ROUNDS), slow, warm=2))
                say("split_paths", median_ms(lambda: ctx.split_paths(first, ax, *cols, rounds=ROUNDS), slow, warm=2))
                say("split_paths_out", median_ms(lambda: ctx.split_paths_out(first, ay, *cols, rounds=ROUNDS), slow, warm=2))
                if who != "single":
                    continue
                u = batches[2]
                ua = 1e-7 * np.sqrt(u.liquidity[u.tick_off[:-1]][q] + 1.0)
                uc = (q % 2).astype(np.int32)
                say("swap(univ3)", median_ms(lambda: ctx.swap(2, ua, uc, None, q.astype(np.int64)), reps))
                say("swap_path", median_ms(lambda: ctx.swap_path(*cols, x), reps))
                say("swap_path_out", median_ms(lambda: ctx.swap_path_out(*cols, y), reps))
                say("swap_order", median_ms(lambda: ctx.swap_order(first, *cols, x), reps))
                say("swap_order_out", median_ms(lambda: ctx.swap_order_out(first, *cols, y), reps))
        finally:
            be.close()


def table(files):
    runs = []
    for f in files:
        d = {}
        for line in open(f):
            if "\t" in line and not line.startswith("#"):
                k, v = line.rstrip("\n").split("\t")
                d[k] = float(v)
        runs.append(d)
    p1, r1, p2, r2 = runs
    print(f"{'entry (wall ms per call, median)':<52}{'parent1':>10}{'parent2':>10}{'result1':>10}{'result2':>10}   verdicts")
    both = []
    for k in p1:
        lo, hi = min(p1[k], p2[k]), max(p1[k], p2[k])
        spread = hi - lo
        verdict = lambda v: "ABOVE" if v > hi + spread else ("below" if v < lo - spread else "ok")
        v1, v2 = verdict(r1[k]), verdict(r2[k])
        if v1 == v2 == "ABOVE":
            both.append(k)
        print(f"{k:<52}{p1[k]:>10.4f}{p2[k]:>10.4f}{r1[k]:>10.4f}{r2[k]:>10.4f}   {v1} {v2}")
    print(f"-> ABOVE in both result runs: {', '.join(both) if both else 'none'}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        table(sys.argv[2:6])
    else:
        run()
