"""What a sparse pool-state update costs next to the only path there was before it -- cfmm_pools_clear + re-adding every
segment -- on one MI355X: config3's market (1M mixed pools) and bench.py's 1M-pool multi-tick UniV3 market (univ3_ticks).
For K updated pools: the time of (update, cfmm_eval) and of (clear, re-add, cfmm_eval), their ratio, how the update's time
splits into the host call (checks, prepared constants, packing, launch) and the wait for the device, and the UniV3
compaction count.  A measurement, not a test.
usage: python scripts/pool_update_bench.py [--reps 5] > profiles/pool_update_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cfmmrouter_amd as cr
from benchlib.workloads import WORKLOADS, build_market, sweep_prices_for
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_UNIV3


def moved(b, rows, rep):
    """new state of pools `rows` of batch b: reserves scaled by up to ±5 %, prices moved by up to ±3 % (capped at the first tick)"""
    u = synth.uniform(900 + rep, 1, rows.size)
    if b.kind == KIND_UNIV3:
        top = b.lower_ticks[b.tick_off[rows]]
        return np.minimum(b.current_price[rows] * (0.97 + 0.06 * u), top)
    return b.R[rows] * (0.95 + 0.1 * u)[:, None]


def run(name, Ks, reps):
    n = WORKLOADS[name][1]
    batches = [b for b in build_market(name, 0, 1, "weak") if len(b)]
    v = sweep_prices_for(name, n)
    be = cr.DeviceBackend(n, batches)
    ctx = be.ctx
    ctx.eval(v)
    for s, b in enumerate(batches):                  # (see below: the first update after an upload)
        (ctx.set_prices(s, [0], b.current_price[:1]) if b.kind == KIND_UNIV3 else ctx.set_reserves(s, [0], b.R[:1]))
    sizes = np.array([len(b) for b in batches])
    print(f"\n## {name}: {sizes.sum()} pools in {len(batches)} segments, {n} tokens")
    print(f"{'K':>7} {'sparse+eval ms':>15} {'host call ms':>13} {'device wait ms':>15} {'reload+eval ms':>15} {'ratio':>8} {'first after upload ms':>22} {'regrows':>8}")
    for K in Ks:
        ts, th, tr, tf = [], [], [], []
        for rep in range(reps):
            picks = []
            for s, b in enumerate(batches):          # K pools spread over the segments in proportion to their sizes
                k = int(round(K * len(b) / sizes.sum()))
                rows = np.sort(np.argsort(synth.uniform(800 + rep, 10 + s, len(b)))[:k]).astype(np.int64)
                picks.append((rows, moved(b, rows, rep)))
            t0 = time.perf_counter()
            for s, (b, (rows, state)) in enumerate(zip(batches, picks)):
                (ctx.set_prices if b.kind == KIND_UNIV3 else ctx.set_reserves)(s, rows, state)
            t1 = time.perf_counter()
            ctx.eval(v)
            t2 = time.perf_counter()
            for b, (rows, state) in zip(batches, picks):   # the host mirror follows: the reload uploads the same market
                (b.current_price if b.kind == KIND_UNIV3 else b.R)[rows] = state
            ts.append(t2 - t0)
            th.append(t1 - t0)
            t0 = time.perf_counter()
            be.reload(batches)
            ctx.eval(v)
            tr.append(time.perf_counter() - t0)
            # An upload leaves a UniV3 segment no spare records: the FIRST update after it compacts and regrows (its time is
            # reported apart).  The timed updates above are the steady state a live user is in, so the regrow is taken here.
            t0 = time.perf_counter()
            for s, (b, (rows, state)) in enumerate(zip(batches, picks)):
                (ctx.set_prices if b.kind == KIND_UNIV3 else ctx.set_reserves)(s, rows, state)
            ctx.eval(v)
            tf.append(time.perf_counter() - t0)
        sp, ho, rl = 1e3 * np.median(ts), 1e3 * np.median(th), 1e3 * np.median(tr)
        print(f"{K:7d} {sp:15.3f} {ho:13.3f} {sp - ho:15.3f} {rl:15.3f} {rl / sp:8.1f} {1e3 * np.median(tf):22.3f} {ctx.get_option('pool_update_regrows'):8d}")
    be.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, nargs="*", default=[100, 1_000, 10_000, 100_000])
    a = ap.parse_args()
    print("# scripts/pool_update_bench.py: median of", a.reps, "repetitions; 'device wait' = the following cfmm_eval, which waits for the scatter")
    for name in ("config3", "univ3_ticks"):
        run(name, a.K, a.reps)
