"""No device allocation outlives its owner (csrc/devbuf.h).  libcfmm_amd_hooks.so counts the allocations that went through
dev_alloc and have not come back through dev_free (read-only option "debug_live_allocs", process-wide); the body below runs
in a child process on that build and checks the count around every path that replaces or releases device arrays: the UniV3
swap of update_reserves!, the sparse updates with a regrow of the tick arrays, clear() and close()."""
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


PRODUCT, MULTI_TICK, SINGLE_TICK, CURVE = 0, 2, 3, 5


def ownership_body(device):
    from test_gpu_pool_update import moved_prices, rows_of
    probe = cr.Context(4)                      # reads the process-wide count while the context under test does not exist
    live = lambda: probe.get_option("debug_live_allocs")
    with pytest.raises(Exception, match="unknown option"):
        probe.set_option("debug_live_allocs", 0)                                      # read-only
    before = live()
    shards = len(device) if isinstance(device, list) else 1
    be = cr.DeviceBackend(N, [], device=device)
    try:
        baseline = live()
        assert baseline > before
        batches = market()
        assert np.diff(batches[MULTI_TICK].tick_off).max() > 2 and np.diff(batches[SINGLE_TICK].tick_off).max() == 1
        be.reload(batches)
        pools_only = live()
        assert pools_only > baseline
        v = synth.sweep_prices(N, seed=8, spread=0.3)
        compact = be.ctx.get_option("compact_trades") != 0
        be.find_arb(v)
        be.trades()                                                                       # (allocates the expanded trade buffers)
        steady = live()
        be.ctx.update_reserves()                                                          # the UniV3 swap frees exactly what it replaces
        assert live() == steady
        rows = rows_of(M, 5, 9)
        be.ctx.set_reserves(PRODUCT, rows, batches[PRODUCT].R[rows] * 1.25)
        o = synth.curve_pools(M, N, 3, seed=10)
        be.ctx.set_curve(CURVE, rows, o.R[rows], o.α[rows], o.β[rows])
        assert live() == steady
        u = batches[MULTI_TICK]
        for r in range(12):                                                               # ... and so does a regrow of the tick arrays
            if be.ctx.get_option("pool_update_regrows") >= 1:
                break
            pick = rows_of(M, M // 2, 20 + r)
            be.ctx.set_prices(MULTI_TICK, pick, moved_prices(u, 30 + r)[pick])
            assert live() == steady
        assert be.ctx.get_option("pool_update_regrows") >= 1
        be.find_arb(v)
        assert live() == steady
        be.ctx.clear()
        # what clear() keeps by design: the context-level buffers a sweep and a trade download have grown, per shard
        kept = {"d_gtab": True, "d_partials": True,                                      # (every launch has a fee-table slot and rows)
                "d_delta": True, "d_lambda": True, "d_over": True,                      # two-coin trade rows exist
                "d_xdelta": compact, "d_xlambda": compact,                              # expanded copies: compact records only
                "d_flow": False, "d_entries": False, "d_chunks": False, "d_tok_chunk_off": False, "d_chunk_sums": False}   # large-market mode only
        assert live() == baseline + shards * sum(kept.values())
        assert steady - live() == pools_only - baseline                                   # the segments' arrays, no more and no less
    finally:
        be.close()
    assert live() == before
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
