"""Solidly-style stable pairs (CFMM_KIND_SOLIDLY, sweep_kernel<SolidlyOps, ...>) against the roofline and against the
ProductTwoCoin single-family sweep IN THE SAME RUN: 1M pools, 256 tokens, prices at e^±0.5 and within 1e-3, fused
(cfmm_eval: no trade write-back) and materialising (cfmm_find_arb) sweeps, cache-warm (one market swept again and again) and
HBM-resident (a ring of market copies touching >= 2 x the 256 MiB Infinity Cache).  Kernel span from the command
processor's start / stop events (option "time_kernels").

    python scripts/solidly_bench.py [m]

Pools: synth.solidly_pools (t₀ within e^±0.05, fees 5 bp / none) and synth.product_pools.  Bytes of the layout, per pool,
for both families: 16 R + 8 packed {tokens, fee index}, plus one 16-byte trade record when materialising.
frac = those bytes / kernel span / 8 TB/s; ratio = the span over ProductTwoCoin's at the same variant and residency."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

n = 256
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000


def span(batch, v, mat, hbm, per_pool):
    copies = int(np.ceil(2 * (256 << 20) / (per_pool * m))) if hbm else 1
    ring = [cr.DeviceBackend(n, batch) for _ in range(copies)]
    try:
        for b in ring:
            b.ctx.set_option("time_kernels", 1)
        K = max(3 * copies, 30)
        for k in range(2 * copies):      # warm-up: every copy once (twice)
            (ring[k % copies].find_arb if mat else ring[k % copies].eval)(v)
        for b in ring:
            b.ctx.kernel_times()         # reset
        for k in range(K):
            (ring[k % copies].find_arb if mat else ring[k % copies].eval)(v)
        launches, ms = 0, 0.0
        for b in ring:
            t = b.ctx.kernel_times()
            launches += t["sweep_launches"]
            ms += t["sweep_ms"]
        return 1e3 * ms / launches, copies
    finally:
        for b in ring:
            b.close()


print(f"# Solidly stable pairs vs ProductTwoCoin, {m} pools, {n} tokens; kernel span per sweep launch (CP events), mean of K launches")
print("# prices   family    variant        residency  copies   sweep us   pool-evals/s   bytes/pool   frac of 8 TB/s   ratio to product")
families = (("product", [synth.product_pools(m, n, seed=100)]), ("solidly", [synth.solidly_pools(m, n, seed=101)]))
for pname, spread in (("e^±0.5", 0.5), ("1e-3", 1e-3)):
    v = synth.sweep_prices(n, seed=7, spread=spread)
    for mat in (False, True):
        per_pool = 24 + (16 if mat else 0)
        for hbm in (False, True):
            base = None
            for fam, batch in families:
                us, copies = span(batch, v, mat, hbm, per_pool)
                base = us if fam == "product" else base
                frac = per_pool * m / (us * 1e-6) / 8e12
                print(f"  {pname:7s}  {fam:8s}  {'materialising' if mat else 'fused':13s}  {'hbm' if hbm else 'warm':9s}  {copies:6d} "
                      f"{us:10.2f}   {m / (us * 1e-6):12.3e}   {per_pool:10d}   {frac:6.3f}   {us / base:16.2f}", flush=True)
