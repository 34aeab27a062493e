"""Where cfmm_find_path's time goes, launch by launch, on the config-3 market of benchlib/workloads.py (1M mixed ProductTwoCoin +
GeometricMeanTwoCoin pools, 256 tokens): the span of every relax layer (find_relax: one lane per pool, the pools' token ids
read once per layer) and of every walk-back step (find_claim + find_advance), for 1 and 64 queries at max_hops 3.

    python scripts/find_path_times.py [pools] [counts ...]        -> stdout and profiles/find_path_times.txt

Metric: kernel spans from the command processor's start / stop events (option "time_kernels"; read-only options
"find_relax_ns_<h>", "find_claim_ns_<h>", "find_advance_ns_<h>").  Yardstick, in the same session: one MATERIALISING sweep of the
same market (cfmm_kernel_times) -- a launch that reads every pool's state and tokens once and writes a trade per pool; a relax
layer reads the tokens of every pool and the state of the reached ones only.  Medians of K repetitions after 3 warm-up calls,
min and max beside them.  A/B in the same session: option "find_lds" = 1 (default: a block folds its candidates into an LDS copy
of the layer rows first) against 0 (every candidate goes to global memory).  Measured, not a gate.  The answers are checked against cfmm_quote_path before timing."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from benchlib import workloads
from cfmmrouter_amd import synth

NAME = "config3"
HOPS = 3
K = 15
scale = (int(sys.argv[1]) / 1_000_000) if len(sys.argv) > 1 else 1.0
COUNTS = [int(a) for a in sys.argv[2:]] or [1, 64]
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "find_path_times.txt")
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def med(xs):
    xs = np.asarray(xs, dtype=np.float64) / 1e3
    return f"{np.median(xs):8.1f} ({xs.min():.1f}-{xs.max():.1f})"


_, n, parts = workloads.WORKLOADS[NAME]
batches = [gen(max(1, int(m * scale)), n, seed=1234, first=0, **kw) for gen, m, kw in parts]
be = cr.DeviceBackend(n, batches)
ctx = be.ctx
ctx.set_option("time_kernels", 1)
m_total = sum(len(b) for b in batches)
emit(f"# cfmm_find_path on {NAME}: {m_total} pools ({' + '.join(str(len(b)) for b in batches)}), {n} tokens, max_hops {HOPS}; kernel spans in us from")
emit(f"# CP events, median (min-max) of {K} calls after 3 warm-up calls; one session")
try:
    v = workloads.sweep_prices_for(NAME, n)
    for _ in range(3):
        ctx.find_arb(v)
    ctx.kernel_times()
    sweeps = []
    for _ in range(K):
        ctx.find_arb(v)
        times = ctx.kernel_times()
        launches = times["sweep_launches"]
        sweeps.append(times["sweep_ms"] * 1e6)
    emit(f"yardstick: one materialising sweep of the same market ({launches} launch(es)): {med(sweeps)} us")
    R0 = np.median(batches[0].R[:, 0])
    for count in COUNTS:
        q = np.arange(count)
        tin = (q * 37 % n).astype(np.int32)
        tout = ((q * 37 + 1 + q % 7) % n).astype(np.int32)
        amt = R0 * 10.0 ** (-4.0 + 3.0 * synth.uniform(9, 1, count))
        out, n_hops, seg, row, ci, co, status = ctx.find_path(tin, tout, amt, HOPS)
        f = np.flatnonzero(status != cr.FOUND_NONE)
        again = ctx.quote_path(n_hops[f], seg[f], row[f], ci[f], co[f], amt[f])
        if not np.array_equal(again.view(np.uint64), out[f].view(np.uint64)):
            raise SystemExit("find_path and quote_path on its result disagree")
        for lds in (1, 0):
            ctx.set_option("find_lds", lds)
            if not all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ctx.find_path(tin, tout, amt, HOPS), (out, n_hops, seg, row, ci, co, status))):
                raise SystemExit("find_lds changes the answer")
            spans = {key: [] for key in [f"find_{k}_ns_{h}" for k in ("relax", "claim", "advance") for h in range(1, HOPS + 1)] + ["find_relax_ns", "find_walk_ns"]}
            wall = []
            for rep in range(3 + K):
                t0 = time.perf_counter()
                ctx.find_path(tin, tout, amt, HOPS)
                dt = time.perf_counter() - t0
                if rep >= 3:
                    wall.append(dt * 1e9)
                    for key in spans:
                        spans[key].append(ctx.get_option(key))
            emit(f"count {count}, {'LDS copy per block (default)' if lds else 'every candidate to global memory (find_lds = 0)'}: {f.size} found, "
                 f"hops histogram {np.bincount(n_hops, minlength=HOPS + 1).tolist()}, {ctx.get_option('find_launches')} launches per call, "
                 f"wall {med(wall)} us per call")
            for h in range(1, HOPS + 1):
                emit(f"  layer {h}:  find_relax {med(spans[f'find_relax_ns_{h}'])}   find_claim {med(spans[f'find_claim_ns_{h}'])}   "
                     f"find_advance {med(spans[f'find_advance_ns_{h}'])}")
            emit(f"  all layers: find_relax {med(spans['find_relax_ns'])}   walk back (claim + advance) {med(spans['find_walk_ns'])}")
        ctx.set_option("find_lds", 1)
finally:
    be.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w", encoding="utf-8") as fh:
    fh.write("\n".join(lines) + "\n")
