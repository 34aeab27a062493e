"""cfmm_quote_dev against the fused sweep of the same segment IN THE SAME PROCESS: 1M pools per kind (UniV3: the ragged 2..64-tick
ladders of bench.py's univ3_ticks workload, 17.3M ticks), 256 tokens, a dense quote of a typical amount per pool (query q is row q), warm (one market quoted
again and again) and HBM-resident (a ring of market copies touching >= 2 x the 256 MiB Infinity Cache), plus one sparse case per
kind: 16k random rows of the 1M.  Kernel spans from the command processor's start / stop events (option "time_kernels":
"quote_ns", and the sweep's kernel_times).

    python scripts/quote_bench.py [m]

Bytes per query from the layout: the pool's record as the quote kernel reads it + 12 B of query (coin_in, amount; + 4 B coin_out
on the N-coin kinds, + 8 B idx when sparse) + 8 B written.  ratio = the quote's span over the fused sweep's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np
import torch

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

n = 256
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
SPARSE = 16384
dev = torch.device("cuda:0")


def market(kind):
    """-> (batch, pool bytes the quote reads per query, pool bytes the fused sweep reads per pool)"""
    if kind == "product":
        return synth.product_pools(m, n, seed=100), 16 + 8, 24
    if kind == "solidly":
        return synth.solidly_pools(m, n, seed=101), 16 + 8, 24
    if kind == "geomean":
        return synth.geomean_pools(m, n, seed=102), 16 + 16 + 8, 48
    if kind == "weighted3":
        return synth.weighted_pools(m, n, 3, seed=103), 2 * 8 + 2 * 8 + 16, 36 * 3 + 16
    if kind == "curve3":
        return synth.curve_pools(m, n, 3, seed=104), 2 * 8 + 3 * 8 + 16 + 16, 36 * 3 + 16
    b = synth.univ3_ragged_pools(m, n, seed=105)      # the generator's defaults: 2..64 ticks, 17.3M at 1M pools
    return b, 16 + 16 + 16 + 8 + 16 + 16, 104          # current-tick constants; + 64 B per record probed


def queries(b, rows):
    nc = b.Ai.shape[1]
    ci = (rows % nc).astype(np.int32)
    co = ((rows + 1) % nc).astype(np.int32)
    f = 0.002 + 0.05 * synth.uniform(9, 70, rows.size)
    if hasattr(b, "tick_off"):
        return ci, co, f * np.sqrt(b.liquidity[b.tick_off[:-1]][rows] + 1.0)
    return ci, co, f * b.R[rows, ci]


def run(kind):
    b, q_pool, s_pool = market(kind)
    ncoin = b.Ai.shape[1] > 2
    ticks = int(b.tick_off[-1]) if hasattr(b, "tick_off") else 0
    pool_bytes = s_pool * m + 64 * ticks
    v = synth.sweep_prices(n, seed=7, spread=0.5)
    for hbm in (False, True):
        copies = max(1, int(np.ceil(2 * (256 << 20) / pool_bytes))) if hbm else 1
        ring = [cr.DeviceBackend(n, [b]) for _ in range(copies)]
        try:
            for be in ring:
                be.ctx.set_option("time_kernels", 1)
            for sparse in (False, True):
                rows = np.sort(np.random.default_rng(3).choice(m, SPARSE, replace=False)) if sparse else np.arange(m)
                ci, co, a = queries(b, rows)
                t = [torch.from_numpy(x).to(dev) for x in (rows.astype(np.int64), ci, co, a)]
                out = torch.empty(rows.size, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                K = max(3 * copies, 20)
                spans = []
                for k in range(2 * copies + K):
                    ctx = ring[k % copies].ctx
                    ctx.quote_dev(0, rows.size, t[3].data_ptr(), t[1].data_ptr(), out.data_ptr(), t[2].data_ptr() if ncoin else 0,
                                  t[0].data_ptr() if sparse else 0)
                    ns = ctx.get_option("quote_ns")                      # waits for that kernel
                    if k >= 2 * copies:
                        spans.append(ns)
                us = np.median(spans) / 1e3
                per_q = q_pool + 12 + (4 if ncoin else 0) + (8 if sparse else 0) + 8
                # the yardstick: the fused sweep (cfmm_eval: no trade write-back) of the same segment, same ring
                for k in range(2 * copies):
                    ring[k % copies].eval(v)
                for be in ring:
                    be.ctx.kernel_times()
                for k in range(K):
                    ring[k % copies].eval(v)
                launches, ms = 0, 0.0
                for be in ring:
                    kt = be.ctx.kernel_times()
                    launches += kt["sweep_launches"]
                    ms += kt["sweep_ms"]
                sweep_us = 1e3 * ms / launches
                frac = per_q * rows.size / (us * 1e-6) / 8e12
                print(f"  {kind:9s}  {'sparse 16k' if sparse else 'dense':10s}  {'hbm' if hbm else 'warm':5s} {copies:4d}  {us:9.2f}  "
                      f"{rows.size / (us * 1e-6):11.3e}  {per_q:5d}  {frac:6.3f}  {sweep_us:9.2f}  {us / sweep_us:6.2f}"
                      + (f"   ({ticks} ticks)" if ticks else ""), flush=True)
        finally:
            for be in ring:
                be.close()


print(f"# cfmm_quote_dev vs the fused sweep (cfmm_eval) of the same segment, {m} pools per kind, {n} tokens; kernel spans from CP events,")
print("# quote: median of K launches, sweep: mean of K launches")
print("# kind       queries     res.  copies  quote us    queries/s   B/query  frac of 8 TB/s  sweep us  quote/sweep")
for kind in (sys.argv[2:] or ["product", "solidly", "geomean", "weighted3", "curve3", "univ3"]):
    run(kind)
