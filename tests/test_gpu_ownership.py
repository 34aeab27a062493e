"""No resource outlives its owner (csrc/devbuf.h, csrc/hostres.h).  libcfmm_amd_hooks.so counts, per family, what went through
the raw create functions and has not come back through the matching destroy: device arrays (read-only option
"debug_live_allocs", the fine-grained arm buffer included), pinned host buffers ("debug_live_pinned"), events
("debug_live_events") and streams ("debug_live_streams"), all process-wide.  The body below runs in a child process on that
build.  It checks the device-array count around every path that replaces or releases device arrays -- the UniV3 swap of
update_reserves!, the sparse updates with a regrow of the tick arrays, clear() and close() -- and all four counts over two
rounds of every call that creates a pinned buffer, an event or a stream on first use: nothing may grow per call, and after
close() everything is back where it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth

pytestmark = pytest.mark.gpu

N, M = 64, 300


def market():
    """one segment of each of the six kinds (weighted and Curve with 3 coins), UniV3 twice: multi-tick and single-tick pools"""
    return [synth.product_pools(M, N, seed=1), synth.geomean_pools(M, N, seed=2),
            synth.univ3_ragged_pools(M, N, min_ticks=2, max_ticks=12, seed=3), synth.univ3_pools(M, N, 1, seed=4),
            synth.weighted_pools(M, N, 3, seed=5), synth.curve_pools(M, N, 3, seed=6), synth.solidly_pools(M, N, seed=7)]


PRODUCT, MULTI_TICK, SINGLE_TICK, CURVE, BIG = 0, 2, 3, 5, 7
BIG_M = 131072          # 2 x TradeStaging::kChunkRows: the smallest download that takes the staged path (streams, pinned slots, events)
COUNTERS = ("debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams")


def ownership_body(device):
    from cfmmrouter_amd._lib import OBJ_LINEAR_NONNEGATIVE
    from test_gpu_pool_update import moved_prices, rows_of
    probe = cr.Context(4)                      # reads the process-wide counts while the context under test does not exist
    live_all = lambda: tuple(probe.get_option(k) for k in COUNTERS)
    live = lambda: live_all()[0]
    for key in COUNTERS:
        with pytest.raises(Exception, match="unknown option"):
            probe.set_option(key, 0)                                                  # read-only
    before = live_all()
    shards = len(device) if isinstance(device, list) else 1
    be = cr.DeviceBackend(N, [], device=device)
    try:
        created = live_all()
        baseline = created[0]
        assert baseline > before[0]
        assert created[1] >= before[1] + shards and created[3] == before[3] + shards   # per shard: the stage, the own stream
        batches = market() + [synth.product_pools(BIG_M, N, seed=11)]
        assert np.diff(batches[MULTI_TICK].tick_off).max() > 2 and np.diff(batches[SINGLE_TICK].tick_off).max() == 1
        be.reload(batches)
        pools_only = live()
        assert pools_only > baseline
        assert live_all()[1:] == created[1:]                                              # an upload creates no host resource
        v = synth.sweep_prices(N, seed=8, spread=0.3)
        compact = be.ctx.get_option("compact_trades") != 0
        u = batches[MULTI_TICK]
        steady, after = None, []
        for rnd in range(2):
            be.ctx.set_option("time_kernels", 1)
            be.find_arb(v)
            host = live_all()[1:]
            D, L = be.trades()                                                            # (allocates the expanded trade buffers)
            # the BIG segment's rows take the staged path on one device (a shard of [0, 0] holds half of them: plain copies),
            # whose set-up happens once: TradeStaging's kThreads = 4 streams, 4 x kSlots = 8 pinned slots and 8 events
            staged = (8, 8, 4) if rnd == 0 and shards == 1 else (0, 0, 0)
            assert tuple(a - b for a, b in zip(live_all()[1:], host)) == staged
            assert D.size == be.ctx.trades_len and np.isfinite(D).all() and np.isfinite(L).all()
            for seg in (PRODUCT, BIG):                                                    # (the selection scratch, its pinned word, six events)
                idx, sD, sL, val = be.ctx.select_trades(seg, 0.0)
                assert idx.size > 0 and be.ctx.get_option("select_flag_ns") > 0
            be.ctx.set_option("time_kernels", 0)
            if steady is None:
                steady = live()
            assert live() == steady
            rows = rows_of(M, 5, 9)
            be.ctx.set_reserves(PRODUCT, rows, batches[PRODUCT].R[rows] * 1.25)
            o = synth.curve_pools(M, N, 3, seed=10)
            be.ctx.set_curve(CURVE, rows, o.R[rows], o.α[rows], o.β[rows])
            assert live() == steady
            regrows = be.ctx.get_option("pool_update_regrows")
            for r in range(24):                                                           # ... and so does a regrow of the tick arrays
                if be.ctx.get_option("pool_update_regrows") > regrows:
                    break
                pick = rows_of(M, M // 2, 20 + r)
                be.ctx.set_prices(MULTI_TICK, pick, moved_prices(u, 30 + 24 * rnd + r)[pick])
                assert live() == steady
            assert be.ctx.get_option("pool_update_regrows") > regrows
            # cfmm_route: pre-armed evaluations where the box can arm (large BAR), launch-when-ready ones where it cannot
            vr, psi, info = be.ctx.route(OBJ_LINEAR_NONNEGATIVE, synth.linear_prices(N, seed=12), 0, v0=np.ones(N), maxfun=40)
            assert np.isfinite(psi).all()
            be.ctx.kernel_times()
            assert live() == steady
            be.ctx.update_reserves()                                                      # the UniV3 swap frees exactly what it replaces
            assert live() == steady
            after.append(live_all())
            print("round", rnd, dict(zip(COUNTERS, after[-1])), flush=True)
        assert all(b <= a for a, b in zip(*after)), after                                 # nothing grows per call
        be.find_arb(v)
        assert live() == steady
        be.ctx.clear()
        # what clear() keeps by design: the context-level buffers a sweep and a trade download have grown, per shard
        kept = {"d_gtab": True, "d_partials": True,                                      # (every launch has a fee-table slot and rows)
                "d_delta": True, "d_lambda": True, "d_over": True,                      # two-coin trade rows exist
                "d_xdelta": compact, "d_xlambda": compact,                              # expanded copies: compact records only
                "d_flow": False, "d_entries": False, "d_chunks": False, "d_tok_chunk_off": False, "d_chunk_sums": False}   # large-market mode only
        sel = 8                                                                           # the selection scratch (SelectScratch): all eight arrays were asked for
        assert live() == baseline + shards * (sum(kept.values()) + sel)
        assert steady - live() == pools_only - baseline                                   # the segments' arrays, no more and no less
        assert live_all()[1:] == after[-1][1:]                                            # clear() changes only the device-array count
    finally:
        be.close()
    assert live_all() == before
    probe.close()


def test_no_allocation_outlives_its_owner():
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_ownership as t\n"
            "t.ownership_body(0)\n"
            "t.ownership_body([0, 0])\n"
            "print('ownership-ok')\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "ownership-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])
