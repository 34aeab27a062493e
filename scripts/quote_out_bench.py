"""cfmm_quote_out_dev against cfmm_quote_dev of the same segment IN THE SAME PROCESS: 1M pools per kind (UniV3: the ragged
2..64-tick ladders of bench.py's univ3_ticks workload), 256 tokens.  Each pool is first asked the forward quote of a typical
amount; the inverse is then asked for exactly that output, so both kernels walk the same pool state to the same point.
Dense (query q is row q), warm (one market quoted again and again) and HBM-resident (a ring of market copies touching
>= 2 x the 256 MiB Infinity Cache), plus one sparse case per kind: 16k random rows of the 1M.  Kernel spans from the command
processor's start / stop events (option "time_kernels": "quote_ns", which reports the latest call of either direction),
median of >= 20 launches each.

    python scripts/quote_out_bench.py [m] [kind ...]        -> stdout and profiles/quote_out_bench.txt

Bytes per query are the forward quote's (scripts/quote_bench.py): the same record, the same query, the same 8 B written.
ratio = the inverse's span over the forward's."""
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
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quote_out_bench.txt")
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def market(kind):
    """-> (batch, pool bytes a quote reads per query, pool bytes of the segment per pool: what sizes the ring)"""
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
    b = synth.univ3_ragged_pools(m, n, seed=105)      # the generator's defaults: 2..64 ticks
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
                back = torch.empty(rows.size, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                K = max(3 * copies, 20)
                p_co, p_idx = (t[2].data_ptr() if ncoin else 0), (t[0].data_ptr() if sparse else 0)
                spans = {"fwd": [], "inv": []}
                for which in ("fwd", "inv"):      # the forward pass leaves in `out` the outputs the inverse is asked for
                    for k in range(2 * copies + K):
                        ctx = ring[k % copies].ctx
                        if which == "fwd":
                            ctx.quote_dev(0, rows.size, t[3].data_ptr(), t[1].data_ptr(), out.data_ptr(), p_co, p_idx)
                        else:
                            ctx.quote_out_dev(0, rows.size, out.data_ptr(), t[1].data_ptr(), back.data_ptr(), p_co, p_idx)
                        ns = ctx.get_option("quote_ns")                      # waits for that kernel
                        if k >= 2 * copies:
                            spans[which].append(ns)
                torch.cuda.synchronize()
                err = float(torch.nan_to_num(((back - t[3]).abs() / t[3]), nan=0.0, posinf=0.0).max())
                fwd_us, inv_us = np.median(spans["fwd"]) / 1e3, np.median(spans["inv"]) / 1e3
                per_q = q_pool + 12 + (4 if ncoin else 0) + (8 if sparse else 0) + 8
                frac = per_q * rows.size / (inv_us * 1e-6) / 8e12
                emit(f"  {kind:9s}  {'sparse 16k' if sparse else 'dense':10s}  {'hbm' if hbm else 'warm':5s} {copies:4d}  {inv_us:9.2f}  "
                      f"{rows.size / (inv_us * 1e-6):11.3e}  {per_q:5d}  {frac:6.3f}  {fwd_us:9.2f}  {inv_us / fwd_us:6.2f}  {err:9.2e}"
                     + (f"   ({ticks} ticks)" if ticks else ""))
        finally:
            for be in ring:
                be.close()


emit(f"# cfmm_quote_out_dev vs cfmm_quote_dev of the same segment, {m} pools per kind, {n} tokens; kernel spans from CP events, median of K launches each;")
emit("# the inverse is asked for the forward quote's output (round-trip error: max |quote_out(quote(a)) - a| / a over the finite rows)")
emit("# (UniV3: the round-trip column is 1 because some pools hold no liquidity in the asked direction: quote gives 0 and quote_out(0) = 0;")
emit("#  tests/test_gpu_quote_out.py checks the round trip row by row against its bound.)")
emit("# kind       queries     res.  copies  inverse us  queries/s   B/query  frac of 8 TB/s  forward us  inverse/forward  round trip")
for kind in (sys.argv[2:] or ["product", "solidly", "geomean", "weighted3", "curve3", "univ3"]):
    run(kind)
with open(OUT, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
