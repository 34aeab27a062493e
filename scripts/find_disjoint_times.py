"""What a round of cfmm_find_disjoint_paths costs beside one cfmm_find_path search, on the config-3 market of
benchlib/workloads.py (1M mixed ProductTwoCoin + GeometricMeanTwoCoin pools, 256 tokens): 256 queries, max_hops 3,
max_paths 1, 4 and 8.

    python scripts/find_disjoint_times.py [pools]        -> stdout and profiles/find_disjoint.txt
    CFMM_YARDSTICK_TREE=<a checkout of the parent commit, built> python scripts/find_disjoint_times.py

Metric: kernel spans from the command processor's start / stop events (option "time_kernels"): per round the layer launches
("find_round_relax_ns_<r>") and the walk back ("find_round_walk_ns_<r>"), and per layer over all rounds ("find_relax_ns_<h>",
"find_claim_ns_<h>", "find_advance_ns_<h>").  Yardstick: cfmm_find_path on the same queries -- from this library, and, where
CFMM_YARDSTICK_TREE names a built checkout of the parent commit, from THAT library in a child process (the same script with
--yardstick).  Then the rounds of queries that have ended: the same call with half, and with all, of the amounts 0.0 (such a
query finds nothing in round 0 and is skipped from then on).  Medians of REPS calls after 3 warm-up calls, min and max beside
them; one session.  Measured, not a gate.  Slot 0 is checked against find_path, and quote_path against every slot, before timing."""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("CFMM_TREE", HERE)                    # the tree whose library is measured (--yardstick: the parent's)
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np

import cfmmrouter_amd as cr
from benchlib import workloads
from cfmmrouter_amd import synth

NAME, HOPS, COUNT, REPS = "config3", 3, 256, 9
YARDSTICK = "--yardstick" in sys.argv[1:]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
scale = (int(args[0]) / 1_000_000) if args else 1.0
OUT = os.path.join(HERE, "profiles", "find_disjoint.txt")
lines = []


def emit(line):
    print(line, flush=True)
    lines.append(line)


def med(xs):
    xs = np.asarray(xs, dtype=np.float64) / 1e3
    return f"{np.median(xs):8.1f} ({xs.min():.1f}-{xs.max():.1f})"


def timed(call, keys):
    spans, wall = {k: [] for k in keys}, []
    for rep in range(3 + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if rep >= 3:
            wall.append(dt * 1e9)
            for k in keys:
                spans[k].append(ctx.get_option(k))
    return spans, wall


_, n, parts = workloads.WORKLOADS[NAME]
batches = [gen(max(1, int(m * scale)), n, seed=1234, first=0, **kw) for gen, m, kw in parts]
be = cr.DeviceBackend(n, batches)
ctx = be.ctx
ctx.set_option("time_kernels", 1)
m_total = sum(len(b) for b in batches)
q = np.arange(COUNT)
tin = (q * 37 % n).astype(np.int32)
tout = ((q * 37 + 1 + q % 7) % n).astype(np.int32)
amt = np.median(batches[0].R[:, 0]) * 10.0 ** (-4.0 + 3.0 * synth.uniform(9, 1, COUNT))
LAYER_KEYS = [f"find_{k}_ns_{h}" for k in ("relax", "claim", "advance") for h in range(1, HOPS + 1)]
try:
    spans, wall = timed(lambda: ctx.find_path(tin, tout, amt, HOPS), ["find_relax_ns", "find_walk_ns"] + LAYER_KEYS)
    who = "the parent commit's library" if YARDSTICK else "this library"
    head = f"yardstick, cfmm_find_path from {who}: relax {med(spans['find_relax_ns'])}   walk back {med(spans['find_walk_ns'])}   wall {med(wall)} us"
    per_layer = "   ".join(f"layer {h}: relax {med(spans[f'find_relax_ns_{h}'])} claim {med(spans[f'find_claim_ns_{h}'])}" for h in range(1, HOPS + 1))
    if YARDSTICK:
        print(head + "\n  " + per_layer, flush=True)
        sys.exit(0)
    emit(f"# cfmm_find_disjoint_paths on {NAME}: {m_total} pools ({' + '.join(str(len(b)) for b in batches)}), {n} tokens, {COUNT} queries, max_hops {HOPS};")
    emit(f"# kernel spans in us from CP events, median (min-max) of {REPS} calls after 3 warm-up calls; one session")
    emit(head)
    emit("  " + per_layer)
    tree = os.environ.get("CFMM_YARDSTICK_TREE")
    if tree:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick"] + args, env=dict(os.environ, CFMM_TREE=tree),
                               capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            raise SystemExit("the yardstick run failed: " + child.stderr[-1500:])
        for line in child.stdout.rstrip().split("\n"):
            emit(line)
    one = ctx.find_path(tin, tout, amt, HOPS)
    for label, amounts in (("every query live", amt), ("every second query ended (amount 0.0)", np.where(q % 2, 0.0, amt)),
                           ("every query ended (amount 0.0)", np.zeros(COUNT))):
        for K in ((1, 4, 8) if amounts is amt else (4,)):
            n_paths, out, n_hops, seg, row, ci, co, status = ctx.find_disjoint_paths(tin, tout, amounts, K, HOPS)
            if amounts is amt:
                if not (np.array_equal(out[:, 0].view(np.uint64), one[0].view(np.uint64)) and np.array_equal(row[:, 0], one[3])):
                    raise SystemExit("slot 0 is not find_path's answer")
                f, r = np.nonzero(status == cr.FOUND)
                again = ctx.quote_path(n_hops[f, r], seg[f, r], row[f, r], ci[f, r], co[f, r], amounts[f])
                if not np.array_equal(again.view(np.uint64), out[f, r].view(np.uint64)):
                    raise SystemExit("find_disjoint_paths and quote_path on its result disagree")
            keys = [f"find_round_{k}_ns_{r}" for k in ("relax", "walk") for r in range(1, K + 1)] + ["find_relax_ns", "find_walk_ns"] + LAYER_KEYS
            spans, wall = timed(lambda: ctx.find_disjoint_paths(tin, tout, amounts, K, HOPS), keys)
            emit(f"max_paths {K}, {label}: n_paths histogram {np.bincount(n_paths, minlength=K + 1).tolist()}, "
                 f"{ctx.get_option('find_launches')} launches per call, wall {med(wall)} us per call")
            for r in range(1, K + 1):
                emit(f"  round {r}: relax {med(spans[f'find_round_relax_ns_{r}'])}   walk back {med(spans[f'find_round_walk_ns_{r}'])}")
            emit("  all rounds, " + "   ".join(f"layer {h}: relax {med(spans[f'find_relax_ns_{h}'])} claim {med(spans[f'find_claim_ns_{h}'])}"
                                               for h in range(1, HOPS + 1)))
finally:
    be.close()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w", encoding="utf-8") as fh:
    fh.write("\n".join(lines) + "\n")
