"""Curve (StableSwap) pools (CFMM_KIND_CURVE, sweep_ncoin<CurveFamily>) against the roofline: 1M pools at N = 2, 3, 4, 8 coins,
256 tokens, fused (cfmm_eval: no trade write-back) and materialising (cfmm_find_arb) sweeps, cache-warm (one market swept
again and again) and HBM-resident (a ring of market copies touching >= 2 x the 256 MiB Infinity Cache).  Kernel span from
the command processor's start / stop events (option "time_kernels").

    python scripts/curve_bench.py [m]

Pools: synth.curve_pools (60 % StableSwap with A in 1 .. 5000, 20 % small A, 20 % α = 0) at prices spread by e^±0.5.
Bytes of the layout, per pool: per coin 8 R + 8 log R + 4 token, plus 16 {α, log β} and 16 {γ, log γ}, plus 16 per coin
written when materialising.  frac = those bytes / kernel span / 8 TB/s."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

n = 256
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
v = synth.sweep_prices(n, seed=7, spread=0.5)
print(f"# Curve pools, {m} pools, {n} tokens; kernel span per sweep launch (CP events), mean of K launches")
print("# coins  variant        residency  copies   sweep us   pool-evals/s   bytes/pool   frac of 8 TB/s")
for nc in (2, 3, 4, 8):
    batch = [synth.curve_pools(m, n, nc, seed=100 + nc)]
    for mat in (False, True):
        per_pool = 20 * nc + 32 + (16 * nc if mat else 0)
        for hbm in (False, True):
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
                us = 1e3 * ms / launches
                frac = per_pool * m / (us * 1e-6) / 8e12
                print(f"  {nc:5d}  {'materialising' if mat else 'fused':13s}  {'hbm' if hbm else 'warm':9s}  {copies:6d} "
                      f"{us:10.2f}   {m / (us * 1e-6):12.3e}   {per_pool:10d}   {frac:6.3f}", flush=True)
            finally:
                for b in ring:
                    b.close()
