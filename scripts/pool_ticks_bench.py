"""What a UniV3 mint / burn costs through cfmm_pools_set_ticks next to the only path there was before it -- cfmm_pools_clear +
re-adding the segment -- and what the compaction of the tick records costs, on one MI355X with bench.py's 1M-pool multi-tick
UniV3 market (univ3_ticks).  Medians of 3.  A measurement, not a test.
  (a) set_ticks of K ladders + cfmm_eval against clear + re-add + cfmm_eval, in the same process;
  (b) the first update after an upload, which compacts the tick records: the call's wall time and, from the command
      processor's events (option "time_kernels"), the span of compact_walks itself.  --prices-only measures (b) with
      cfmm_pools_set_prices alone, so that the same script runs on a commit without cfmm_pools_set_ticks.
usage: python scripts/pool_ticks_bench.py [--reps 3] [--K 1000] [--prices-only] > profiles/pool_ticks_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cfmmrouter_amd as cr
from benchlib.workloads import WORKLOADS, build_market, sweep_prices_for
from cfmmrouter_amd import synth


def minted(b, rows, rep):
    """-> (prices, tick_off, lower_ticks, liquidity): pools `rows` after a mint into two new ticks below the last one and a
    burn of a tenth of every tick's liquidity; the price stays (a pure mint / burn)"""
    lts, lqs = [], []
    for k, i in enumerate(rows):
        o, e = b.tick_off[i], b.tick_off[i + 1]
        lt, lq = b.lower_ticks[o:e], b.liquidity[o:e]
        if (k + rep) % 2 and lt.size > 2:                        # every other pool: a burn that removes the last tick instead
            lts.append(lt[:-1]), lqs.append(lq[:-1] * 0.9)
        else:
            lts.append(np.concatenate([lt, [lt[-1] * 0.97, lt[-1] * 0.94]])), lqs.append(np.concatenate([lq * 0.9, [2e5, 1e5]]))
    off = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum([a.size for a in lts], out=off[1:])
    return np.minimum(b.current_price[rows], [a[0] for a in lts]), off, np.concatenate(lts), np.concatenate(lqs)


def mirror(b, rows, state):
    """the batch with the rows' new ladders (host side)"""
    p, off, lt, lq = state
    m, old_len = len(b), np.diff(b.tick_off)
    new_len, keep = old_len.copy(), np.ones(m, dtype=bool)
    new_len[rows] = np.diff(off)
    keep[rows] = False
    new_off = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(new_len, out=new_off[1:])
    nlt, nlq = np.empty(new_off[-1]), np.empty(new_off[-1])
    src, dst = np.repeat(keep, old_len), np.repeat(keep, new_len)
    nlt[dst], nlq[dst] = b.lower_ticks[src], b.liquidity[src]
    for j, r in enumerate(rows):
        nlt[new_off[r]:new_off[r + 1]], nlq[new_off[r]:new_off[r + 1]] = lt[off[j]:off[j + 1]], lq[off[j]:off[j + 1]]
    cp = b.current_price.copy()
    cp[rows] = p
    return cr.PoolBatch(b.kind, current_price=cp, tick_off=new_off, lower_ticks=nlt, liquidity=nlq, γ=b.γ, Ai=b.Ai)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--prices-only", action="store_true")
    a = ap.parse_args()
    name = "univ3_ticks"
    n = WORKLOADS[name][1]
    batches = [b for b in build_market(name, 0, 1, "weak") if len(b)]
    assert len(batches) == 1
    b = batches[0]
    v = sweep_prices_for(name, n)
    be = cr.DeviceBackend(n, batches)
    ctx = be.ctx
    ctx.eval(v)
    print(f"# scripts/pool_ticks_bench.py: {name}, {len(b)} pools, {int(b.tick_off[-1])} ticks, {n} tokens; medians of {a.reps}")
    has_ticks = hasattr(ctx, "set_ticks") and not a.prices_only
    try:
        ctx.set_option("time_kernels", 1)
        ctx.get_option("compact_walks_ns")
        spans = True
    except Exception:
        spans = False                                            # (a commit whose compaction runs on the host)
    first, span, sparse, host, reload_ = [], [], [], [], []
    for rep in range(a.reps):
        rows = np.sort(np.argsort(synth.uniform(800 + rep, 10, len(b)))[:a.K]).astype(np.int64)
        # (b) the first update after an upload compacts (an upload allocates no spare records)
        r0 = ctx.get_option("pool_update_regrows")
        one = rows[:1]
        t0 = time.perf_counter()
        ctx.set_prices(0, one, b.current_price[one])
        ctx.eval(v)
        first.append(time.perf_counter() - t0)
        assert ctx.get_option("pool_update_regrows") == r0 + 1
        if spans:
            span.append(ctx.get_option("compact_walks_ns") * 1e-9)
        if has_ticks:                                            # (a) K mints / burns in the steady state, against the reload
            state = minted(b, rows, rep)
            t0 = time.perf_counter()
            ctx.set_ticks(0, rows, *state)
            t1 = time.perf_counter()
            ctx.eval(v)
            t2 = time.perf_counter()
            sparse.append(t2 - t0)
            host.append(t1 - t0)
            b = mirror(b, rows, state)
        t0 = time.perf_counter()
        be.reload([b])
        ctx.eval(v)
        reload_.append(time.perf_counter() - t0)
    ms = lambda x: 1e3 * float(np.median(x))
    if has_ticks:
        print("\n## (a) mint / burn against reload")
        print(f"{'K':>7} {'set_ticks+eval ms':>18} {'host call ms':>13} {'device wait ms':>15} {'reload+eval ms':>15} {'ratio':>8}")
        print(f"{a.K:7d} {ms(sparse):18.3f} {ms(host):13.3f} {ms(sparse) - ms(host):15.3f} {ms(reload_):15.3f} {ms(reload_) / ms(sparse):8.1f}")
    print("\n## (b) the first update after an upload (compaction of the tick records)")
    print(f"{'first update+eval ms':>21} {'compact_walks span ms':>22} {'reload+eval ms':>15} {'regrows':>8}")
    print(f"{ms(first):21.3f} {(f'{ms(span):.3f}' if spans else 'n/a (host compaction)'):>22} {ms(reload_):15.3f} {ctx.get_option('pool_update_regrows'):8d}")
    be.close()


if __name__ == "__main__":
    main()
