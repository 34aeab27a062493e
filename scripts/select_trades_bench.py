"""What the selection of the trades worth executing (cfmm_select_trades) costs next to the only read-back there was before it,
the full download (cfmm_get_trades), on one MI355X: config3's market (1M mixed pools) and bench.py's 1M-pool multi-tick
UniV3 market (univ3_ticks).  Two states per market, both calls in the same process on the same trades:
  chain step        route!, update_reserves!, K pools moved with cfmm_pools_set_*, cfmm_find_arb at the same prices:
                    almost every pool sits inside its fee band (min_value = 0)
  full selectivity  right after route!, min_value = -inf: every trading pool is selected
Reported: medians of `reps` calls after a warm-up call each, the selected count, and the spans of the three kernels from
events (option "time_kernels", a separate pass: summed over the segments).  A measurement, not a test.
usage: python scripts/select_trades_bench.py [--reps 3] [--K 1000] > profiles/select_trades_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cfmmrouter_amd as cr
from benchlib.workloads import WORKLOADS, build_market, objective_for
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_UNIV3


def median_ms(fn, reps):
    fn()                                             # warm-up: buffers grown, pages touched, clocks up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def measure(ctx, shapes, m_all, tau, reps, label):
    D, L = np.empty((m_all, 2)), np.empty((m_all, 2))
    got = {}

    def select():
        got["rows"] = [ctx.select_trades(s, tau, n_coins=c) for s, (m, c) in enumerate(shapes)]

    def count_only():
        got["count"] = sum(ctx.select_count(s, tau) for s in range(len(shapes)))

    t_dl = median_ms(lambda: ctx.trades(out=(D, L)), reps)
    t_sel = median_ms(select, reps)
    t_cnt = median_ms(count_only, reps)
    selected = sum(r[0].size for r in got["rows"])
    assert selected == got["count"]
    ctx.set_option("time_kernels", 1)
    spans = np.zeros(3)
    for s, (m, c) in enumerate(shapes):
        ctx.select_trades(s, tau, n_coins=c)
        spans += [ctx.get_option(k) for k in ("select_flag_ns", "select_scan_ns", "select_emit_ns")]
    ctx.set_option("time_kernels", 0)
    print(f"{label:>17} {selected:9d} {100.0 * selected / m_all:8.3f} {t_sel:10.3f} {t_cnt:13.3f} {t_dl:12.3f} {t_dl / t_sel:7.1f}"
          f" {spans[0] / 1e3:9.1f} {spans[1] / 1e3:9.1f} {spans[2] / 1e3:9.1f}")
    return selected, t_sel, t_dl


def run(name, K, reps):
    n = WORKLOADS[name][1]
    batches = [b for b in build_market(name, 0, 1, "weak") if len(b)]
    shapes = [(len(b), int(b.Ai.shape[1])) for b in batches]
    m_all = sum(m for m, _ in shapes)
    r = cr.Router(objective_for(name, n), batches, n)
    ctx = r._backend.ctx
    print(f"\n## {name}: {m_all} pools in {len(batches)} segments, {n} tokens")
    print(f"{'state':>17} {'selected':>9} {'%':>8} {'select ms':>10} {'count-only ms':>13} {'download ms':>12} {'ratio':>7}"
          f" {'flag us':>9} {'scan us':>9} {'emit us':>9}")
    cr.route_(r, solver="native")
    v = r.v.copy()
    measure(ctx, shapes, m_all, -np.inf, reps, "full selectivity")
    ctx.update_reserves()
    for s, b in enumerate(batches):                  # K pools spread over the segments in proportion to their sizes
        k = int(round(K * len(b) / m_all))
        rows = np.sort(np.argsort(synth.uniform(800, 10 + s, len(b)))[:k]).astype(np.int64)
        u = synth.uniform(900, 1 + s, rows.size)
        if b.kind == KIND_UNIV3:
            cp = ctx.prices(s, len(b))[rows]
            ctx.set_prices(s, rows, np.minimum(cp * (0.97 + 0.06 * u), b.lower_ticks[b.tick_off[rows]]))
        else:
            ctx.set_reserves(s, rows, ctx.reserves(s, len(b))[rows] * (0.95 + 0.1 * u)[:, None])
    ctx.find_arb(v)
    selected, t_sel, t_dl = measure(ctx, shapes, m_all, 0.0, reps, f"chain step K={K}")
    if selected <= 0.01 * m_all:
        print(f"# at most 1 % selected: selection {'FASTER' if t_sel < t_dl else 'NOT faster'} than the full download ({t_sel:.3f} vs {t_dl:.3f} ms)")
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--markets", nargs="*", default=["config3", "univ3_ticks"])
    a = ap.parse_args()
    print("# scripts/select_trades_bench.py: medians of", a.reps, "calls; select / count-only = cfmm_select_trades over all segments,",
          "download = cfmm_get_trades; kernel spans from events, summed over the segments")
    for name in a.markets:
        run(name, a.K, a.reps)
