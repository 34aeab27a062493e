"""Where cfmm_find_path_out's time goes, launch by launch, on the config-3 market of benchlib/workloads.py (1M mixed
ProductTwoCoin + GeometricMeanTwoCoin pools, 256 tokens): the span of every min-relaxation layer (find_out_relax: one lane per
pool) and of every step of the forward walk (find_out_claim + find_out_advance), for 1 and 64 queries at max_hops 3 -- the
sibling of scripts/find_path_times.py, whose measurement of cfmm_find_path it repeats in the same session on the same queries.

    python scripts/find_path_out_times.py [--out FILE] [pools] [counts ...]   -> stdout and profiles/find_path_out_times.txt

Metric: kernel spans from the command processor's start / stop events (option "time_kernels"; read-only options
"find_relax_ns_<h>", "find_claim_ns_<h>", "find_advance_ns_<h>", which describe the latest call of either entry; h is the layer,
and the forward walk claims layer h* first).  Yardsticks, in the same session: one MATERIALISING sweep of the same market
(cfmm_kernel_times), and cfmm_find_path on the same token pairs (compare with profiles/find_path_times.txt: its kernels are the
ones that file measured).  Medians of K repetitions after 3 warm-up calls, min and max beside them.  A/B in the same session:
option "find_lds" = 1 (default) against 0.  Measured, not a gate.  The answers are checked against cfmm_quote_path_out /
cfmm_quote_path before timing."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from benchlib import workloads
from cfmmrouter_amd import synth

NAME = "config3"
HOPS = 3
K = 15
argv = sys.argv[1:]
OUT = os.path.join(ROOT, "profiles", "find_path_out_times.txt")
if argv[:1] == ["--out"]:
    OUT, argv = argv[1], argv[2:]
scale = (int(argv[0]) / 1_000_000) if argv else 1.0
COUNTS = [int(a) for a in argv[1:]] or [1, 64]
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def med(xs):
    xs = np.asarray(xs, dtype=np.float64) / 1e3
    return f"{np.median(xs):8.1f} ({xs.min():.1f}-{xs.max():.1f})"


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


def timed(ctx, call, count, what, lds, found, n_hops):
    keys = [f"find_{k}_ns_{h}" for k in ("relax", "claim", "advance") for h in range(1, HOPS + 1)] + ["find_relax_ns", "find_walk_ns"]
    spans = {key: [] for key in keys}
    wall = []
    for rep in range(3 + K):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if rep >= 3:
            wall.append(dt * 1e9)
            for key in spans:
                spans[key].append(ctx.get_option(key))
    emit(f"{what}, count {count}, {'LDS copy per block (default)' if lds else 'every candidate to global memory (find_lds = 0)'}: {found} found, "
         f"hops histogram {np.bincount(n_hops, minlength=HOPS + 1).tolist()}, {ctx.get_option('find_launches')} launches per call, "
         f"wall {med(wall)} us per call")
    for h in range(1, HOPS + 1):
        emit(f"  layer {h}:  relax {med(spans[f'find_relax_ns_{h}'])}   claim {med(spans[f'find_claim_ns_{h}'])}   "
             f"advance {med(spans[f'find_advance_ns_{h}'])}")
    emit(f"  all layers: relax {med(spans['find_relax_ns'])}   walk (claim + advance) {med(spans['find_walk_ns'])}")


_, n, parts = workloads.WORKLOADS[NAME]
batches = [gen(max(1, int(m * scale)), n, seed=1234, first=0, **kw) for gen, m, kw in parts]
be = cr.DeviceBackend(n, batches)
ctx = be.ctx
ctx.set_option("time_kernels", 1)
m_total = sum(len(b) for b in batches)
emit(f"# cfmm_find_path_out and cfmm_find_path on {NAME}: {m_total} pools ({' + '.join(str(len(b)) for b in batches)}), {n} tokens, max_hops {HOPS};")
emit(f"# kernel spans in us from CP events, median (min-max) of {K} calls after 3 warm-up calls; one session")
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
        amt = R0 * 10.0 ** (-4.0 + 3.0 * synth.uniform(9, 1, count))      # scripts/find_path_times.py's queries
        want = R0 * 10.0 ** (-5.0 + 3.0 * synth.uniform(9, 1, count))     # the wanted outputs: a tenth of those sizes
        ans_out = ctx.find_path_out(tin, tout, want, HOPS)
        f = np.flatnonzero(ans_out[6] != cr.FOUND_NONE)
        again = ctx.quote_path_out(ans_out[1][f], ans_out[2][f], ans_out[3][f], ans_out[4][f], ans_out[5][f], want[f])
        if not np.array_equal(again.view(np.uint64), ans_out[0][f].view(np.uint64)):
            raise SystemExit("find_path_out and quote_path_out on its result disagree")
        ans_in = ctx.find_path(tin, tout, amt, HOPS)
        g = np.flatnonzero(ans_in[6] != cr.FOUND_NONE)
        again = ctx.quote_path(ans_in[1][g], ans_in[2][g], ans_in[3][g], ans_in[4][g], ans_in[5][g], amt[g])
        if not np.array_equal(again.view(np.uint64), ans_in[0][g].view(np.uint64)):
            raise SystemExit("find_path and quote_path on its result disagree")
        for lds in (1, 0):
            ctx.set_option("find_lds", lds)
            if not same(ctx.find_path_out(tin, tout, want, HOPS), ans_out) or not same(ctx.find_path(tin, tout, amt, HOPS), ans_in):
                raise SystemExit("find_lds changes the answer")
            timed(ctx, lambda: ctx.find_path_out(tin, tout, want, HOPS), count, "find_path_out", lds, f.size, ans_out[1])
            timed(ctx, lambda: ctx.find_path(tin, tout, amt, HOPS), count, "find_path (yardstick)", lds, g.size, ans_in[1])
        ctx.set_option("find_lds", 1)
finally:
    be.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w", encoding="utf-8") as fh:
    fh.write("\n".join(lines) + "\n")
