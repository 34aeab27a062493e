"""cfmm_swap_out and cfmm_swap_path_out against what a caller does without them, IN THE SAME PROCESS.  Market: three segments of
`pools` pools each (ProductTwoCoin, GeometricMeanTwoCoin, Curve with 3 coins; synth.py), 256 tokens.

    python scripts/swap_out_bench.py [pools] [paths ...]        -> stdout and profiles/swap_out_bench.txt

1. Single pools, every row of a segment once (one wave): cfmm_swap_out's "swap_ns" against the two-call baseline it replaces --
   cfmm_quote_out ("quote_ns") and then cfmm_swap of the answer ("swap_ns") on the same queries -- and beside it cfmm_swap's own
   span, the kernel that does the same stores behind the other closed form.  Wanted amounts: 1e-4 of the reserve asked.
2. 3-hop paths over distinct pools (hop k in segment k; path p on row p of every segment, or on rows permuted per segment: a
   gather): cfmm_swap_path_out against cfmm_quote_path_out with hop_in and then one cfmm_swap_out per hop level (kernels:
   "quote_ns" + three "swap_ns").  Wanted amounts: half of what a tender of 1e-4 of the first reserve yields.
Baseline and new call alternate in one process; 7 repetitions, the first dropped; median (min-max); us = kernel spans under
"time_kernels" (the command processor's start / stop events), ms = wall-clock of the call sequences through the Python host.
The pools move by 1e-4 per repetition: every repetition meets a slightly different market, the same for both sides.
Measured, not a gate."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

n = 256
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
COUNTS = [int(a) for a in sys.argv[2:]] or [16_384, 1 << 20]
REPS = 7
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "swap_out_bench.txt")
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def stat(x, scale):
    x = np.asarray(x[1:], dtype=np.float64) * scale
    return f"{np.median(x):.4g} ({x.min():.4g}-{x.max():.4g})"


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def single(ctx, s, b, name):
    rows = np.arange(len(b))
    nc = b.Ai.shape[1]
    ci = (rows % nc).astype(np.int32)
    co = ((ci + 1) % nc).astype(np.int32)
    base_k, base_w, new_k, new_w, fwd_k = [], [], [], [], []
    for _ in range(REPS):
        want = 1e-4 * ctx.reserves(s, len(b), nc)[rows, co]
        (a, ns), w = timed(lambda: two_calls(ctx, s, want, ci, co))
        base_k.append(ns); base_w.append(w); fwd_k.append(ctx.get_option("swap_ns"))
        (_, st), w = timed(lambda: ctx.swap_out(s, want, ci, co, status=True))
        new_k.append(ctx.get_option("swap_ns")); new_w.append(w)
        assert np.all(st == 0) and np.all(np.isfinite(a))
    emit(f"{name} {len(b)} swaps: quote_out + swap: kernels {stat(base_k, 1e-3)} us (of them swap {stat(fwd_k, 1e-3)} us), wall {stat(base_w, 1e3)} ms"
         f" | swap_out: kernel {stat(new_k, 1e-3)} us, wall {stat(new_w, 1e3)} ms")


def two_calls(ctx, s, want, ci, co):
    a = ctx.quote_out(s, want, ci, co)
    ns = ctx.get_option("quote_ns")
    ctx.swap(s, a, ci, co)
    return a, ns + ctx.get_option("swap_ns")


def paths(batches, count, permuted):
    H = len(batches)
    seg = np.tile(np.arange(H, dtype=np.int32), (count, 1))
    if permuted:
        row = np.stack([np.argsort(synth.uniform(11 + s, 1, len(b)))[:count].astype(np.int64) for s, b in enumerate(batches)], axis=1)
    else:
        row = np.tile(np.arange(count, dtype=np.int64)[:, None], (1, H))
    ncoins = np.array([b.Ai.shape[1] for b in batches])
    p, k = np.meshgrid(np.arange(count), np.arange(H), indexing="ij")
    ci = ((p + k) % ncoins[seg]).astype(np.int32)
    co = ((ci + 1) % ncoins[seg]).astype(np.int32)
    return np.full(count, H, dtype=np.int32), seg, row, ci, co


def path_run(ctx, batches, count, permuted):
    P = paths(batches, count, permuted)
    n_hops, seg, row, ci, co = P
    H = len(batches)
    first = batches[0]

    def wanted():
        """half of what a tender of 1e-4 of the first reserve yields on the market as it stands: every hop can give its part"""
        return 0.5 * ctx.quote_path(*P, 1e-4 * ctx.reserves(0, len(first), 2)[row[:, 0], ci[:, 0]])
    base_k, base_w, new_k, new_w, not_applied = [], [], [], [], 0
    for _ in range(REPS):
        want = wanted()

        def baseline():
            a, hv = ctx.quote_path_out(*P, want, hops=True)
            ns = ctx.get_option("quote_ns")
            for k in reversed(range(H)):
                out = want if k == H - 1 else np.where(np.isfinite(hv[k + 1]), hv[k + 1], 0.0)   # (a path a pool cannot serve: nothing asked)
                ctx.swap_out(k, out, ci[:, k], co[:, k], row[:, k])
                ns += ctx.get_option("swap_ns")
            return ns
        ns, w = timed(baseline)
        base_k.append(ns); base_w.append(w)
        want = wanted()
        (_, st), w = timed(lambda: ctx.swap_path_out(*P, want))
        new_k.append(ctx.get_option("swap_ns")); new_w.append(w)
        not_applied = int(np.sum(st != 0))
    emit(f"{count} paths, rows {'permuted' if permuted else 'in order'}: quote_path_out + {H} swap_outs: kernels {stat(base_k, 1e-3)} us, wall {stat(base_w, 1e3)} ms"
         f" | swap_path_out: kernel {stat(new_k, 1e-3)} us, wall {stat(new_w, 1e3)} ms | not applied {not_applied}")


batches = [synth.product_pools(m, n, seed=100), synth.geomean_pools(m, n, seed=102), synth.curve_pools(m, n, 3, seed=103)]
be = cr.DeviceBackend(n, batches)
be.ctx.set_option("time_kernels", 1)
emit(f"# MI355X, {m} pools per segment (Product, GeometricMean, Curve 3 coins; synth.py); swaps want 1e-4 of the reserve asked, 3-hop paths half of what 1e-4 of the first reserve yields")
emit(f"# baseline and new call alternate in one process; {REPS} repetitions, the first dropped; median (min-max); us = kernel spans, ms = wall")
try:
    for s, (b, name) in enumerate(zip(batches, ("Product", "GeometricMean", "Curve3"))):
        single(be.ctx, s, b, name)
    for count in COUNTS:
        for permuted in (False, True):
            path_run(be.ctx, batches, min(count, m), permuted)
finally:
    be.close()
with open(OUT, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
