"""cfmm_quote_path against what a caller does without it, IN THE SAME PROCESS: pricing the same 3-hop paths by one cfmm_quote
call per hop level and segment.  Market: 1M pools, 256 tokens -- config 3's families (ProductTwoCoin, GeometricMeanTwoCoin)
plus one N-coin segment (3-coin weighted).  Workload: 1M paths and 16k paths of 3 hops, rows random, each once with the hops of
a wavefront in one kind (64 neighbouring paths share their segment at every hop) and once with the kinds interleaved lane by
lane (neighbouring paths sit in different segments at every hop: the lanes of a wavefront serialise over the kinds).

    python scripts/quote_path_bench.py [pools] [paths ...]        -> stdout and profiles/quote_path_bench.txt

Metric: the path kernel's span ("quote_ns" under "time_kernels": the command processor's start / stop events).  Yardstick: the
SUM of the "quote_ns" spans of the nine cfmm_quote calls (3 hop levels x 3 segments) that price the same paths.  Beside them
the wall-clock of the two whole call sequences through the Python host (host pointers: staging copies, launches,
synchronisations, and for the chain the gather / scatter of the intermediate amounts between the calls).  Medians of K
repetitions.  Measured, not a gate.  The two ways must agree bit for bit; the script checks that first."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

n = 256
m = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
COUNTS = [int(a) for a in sys.argv[2:]] or [1_000_000, 16_384]
HOPS = 3
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quote_path_bench.txt")
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def paths(batches, count, interleaved):
    p, k = np.meshgrid(np.arange(count), np.arange(HOPS), indexing="ij")
    nseg = len(batches)
    seg = ((p if interleaved else p // 64) + k) % nseg
    u = synth.uniform(7, 1, count * HOPS).reshape(count, HOPS)
    sizes = np.array([len(b) for b in batches])
    row = np.minimum((u * sizes[seg]).astype(np.int64), sizes[seg] - 1)
    ncoins = np.array([b.Ai.shape[1] for b in batches])
    ci = ((p + k) % ncoins[seg]).astype(np.int32)
    co = ((ci + 1) % ncoins[seg]).astype(np.int32)
    first = np.empty(count)
    for s, b in enumerate(batches):
        at = seg[:, 0] == s
        first[at] = b.R[row[at, 0], ci[at, 0]]
    amt = first * (0.002 + 0.05 * synth.uniform(7, 2, count))
    return np.full(count, HOPS, dtype=np.int32), seg.astype(np.int32), row, ci, co, amt


def chain(ctx, P, subsets):
    """one ctx.quote per hop level and segment -> (answers, sum of the kernel spans in ns)"""
    _, _, row, ci, co, amt = P
    x = amt.copy()
    ns = 0
    for k in range(HOPS):
        for s, q in subsets[k]:
            x[q] = ctx.quote(s, x[q], ci[q, k], co[q, k], row[q, k])
            ns += ctx.get_option("quote_ns")
    return x, ns


def run(ctx, batches, count, interleaved):
    P = paths(batches, count, interleaved)
    subsets = [[(s, np.flatnonzero(P[1][:, k] == s)) for s in range(len(batches))] for k in range(HOPS)]
    subsets = [[(s, q) for s, q in level if q.size] for level in subsets]
    want, _ = chain(ctx, P, subsets)
    got = ctx.quote_path(*P)
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        raise SystemExit("quote_path and the chain of quotes disagree")
    K = 7 if count > 100_000 else 25
    span, wall, c_span, c_wall = [], [], [], []
    for _ in range(2 + K):
        t0 = time.perf_counter()
        ctx.quote_path(*P)
        wall.append(time.perf_counter() - t0)
        span.append(ctx.get_option("quote_ns"))
        t0 = time.perf_counter()
        _, ns = chain(ctx, P, subsets)
        c_wall.append(time.perf_counter() - t0)
        c_span.append(ns)
    span_us, c_span_us = np.median(span[2:]) / 1e3, np.median(c_span[2:]) / 1e3
    wall_ms, c_wall_ms = np.median(wall[2:]) * 1e3, np.median(c_wall[2:]) * 1e3
    calls = sum(len(level) for level in subsets)
    emit(f"  {count:8d}  {'interleaved' if interleaved else 'uniform':11s}  {span_us:10.2f}  {c_span_us:12.2f}  {span_us / c_span_us:6.2f}  "
         f"{count * HOPS / (span_us * 1e-6):10.3e}  {wall_ms:9.2f}  {c_wall_ms:10.2f}  {calls:5d}")


batches = [synth.product_pools(int(0.45 * m), n, seed=100), synth.geomean_pools(int(0.45 * m), n, seed=102),
           synth.weighted_pools(m - 2 * int(0.45 * m), n, 3, seed=103)]
be = cr.DeviceBackend(n, batches)
be.ctx.set_option("time_kernels", 1)
emit(f"# cfmm_quote_path vs the chain of cfmm_quote calls that prices the same paths; {m} pools "
     f"({' + '.join(str(len(b)) for b in batches)}: ProductTwoCoin, GeometricMeanTwoCoin, weighted N = 3), {n} tokens, {HOPS} hops per path;")
emit("# kernel spans from CP events (path: one kernel; chain: the sum over its calls), wall-clock of the whole call sequences through the")
emit("# Python host (host pointers); medians.  Bit-equality of the two ways is checked before timing.")
emit("#    paths  wavefronts   path span us  chain spans us   ratio     hops/s  path wall ms  chain wall ms  chain calls")
try:
    for count in COUNTS:
        for interleaved in (False, True):
            run(be.ctx, batches, count, interleaved)
finally:
    be.close()
with open(OUT, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")
