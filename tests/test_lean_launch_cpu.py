"""Which launches take the lean sweep kernels: csrc/launch_plan.cpp's lean_launch, built for the host behind
tests/native/lean_launch_host.cpp, over the configurations tests/test_gpu_lean_sweep.py sweeps on the device -- the markets
that must run lean and every configuration that must not.  No device: the predicate is a pure function of the launch's
descriptor head, its group and the arithmetic."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "native", "lean_launch_host.cpp")

OPTS = ["max_grid", "block", "bin_copies", "direct_small", "fuse_segments", "geomean_exact", "cost_geomean", "cost_univ3", "pack"]
DEFAULTS = dict(zip(OPTS, (0, 0, 0, 1, 1, 0, 10, 10, 1)))
LAUNCH = ["compact_trades", "stream_stores", "univ3_heads", "arith"]
LAUNCH_DEFAULTS = {"compact_trades": 1, "stream_stores": 0, "univ3_heads": 1, "arith": 2}
P, G, U, W, C, S = range(6)   # CFMM_KIND_*
FULL, FAST, AUTO = 0, 1, 2    # LaunchCfg::arith


def seg(kind, m, n_fees=2, packed=1, has_walk=1, n_coins=2, ticks_per_pool=2):
    return [kind, m, n_coins, ticks_per_pool * m if kind == U else 0, has_walk, packed, n_fees]


@pytest.fixture(scope="module")
def lean(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lean_launch_host") / "lean_launch_host.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O3", "-std=c++17",
                    "-ffp-contract=off", "-shared", "-fPIC", SHIM, os.path.join(CSRC, "launch_plan.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    ip = ctypes.POINTER(ctypes.c_int64)
    lib.lean_launch_host.argtypes = [ctypes.c_int, ip, ctypes.c_int, ip, ip, ip]

    def run(n, segs, **options):
        opts = np.array([options.get(k, DEFAULTS[k]) for k in OPTS], dtype=np.int64)
        launch = np.array([options.get(k, LAUNCH_DEFAULTS[k]) for k in LAUNCH], dtype=np.int64)
        assert set(options) <= set(OPTS) | set(LAUNCH)
        seg_in = np.array(segs, dtype=np.int64).reshape(len(segs), 7)
        out = np.full(len(segs), -7, dtype=np.int64)
        p = lambda a: a.ctypes.data_as(ip)
        ng = lib.lean_launch_host(n, p(opts), len(segs), p(seg_in), p(launch), p(out))
        assert 0 < ng <= len(segs)
        return [int(x) for x in out[:ng]]

    return run


FUSED = [seg(P, 1500), seg(G, 1500)]

# name: (tokens, segments, options, lean or not per launch group)
LEAN = {
    "fused_tiles_8": (8, FUSED, {"max_grid": 2}, [1]),
    "fused_tiles_257": (257, FUSED, {"max_grid": 2}, [1]),
    "fused_tiles_fast": (257, FUSED, {"max_grid": 2, "arith": FAST}, [1]),
    "fused_xcd": (256, [seg(P, 70000), seg(G, 70000)], {"max_grid": 256}, [1]),
    "fused_default_grid": (256, [seg(P, 500000), seg(G, 500000)], {}, [1]),                   # the benchmark's headline market
    "fused_three": (48, [seg(P, 5000), seg(G, 3000), seg(U, 1777)], {}, [1]),
    "product_two_blocks": (48, [seg(P, 5200)], {"block": 1024, "max_grid": 2}, [1]),
    "geomean_two_blocks": (48, [seg(G, 5200)], {"block": 1024, "max_grid": 2}, [1]),
    "univ3_two_blocks": (48, [seg(U, 5200)], {"block": 1024, "max_grid": 2}, [1]),
    "product_1m": (256, [seg(P, 1000000)], {}, [1]),
}
GENERAL = {
    "full_range_arithmetic": (257, FUSED, {"max_grid": 2, "arith": FULL}, [0]),
    "compact_trades_0": (48, FUSED, {"max_grid": 2, "compact_trades": 0}, [0]),
    "stream_stores_2": (48, FUSED, {"max_grid": 2, "stream_stores": 2}, [0]),
    "stream_stores_auto_past_the_cache": (48, [seg(P, 4000000), seg(G, 4000000)], {}, [0]),
    "fee_tiers": (48, [seg(P, 1500, n_fees=0), seg(G, 1500)], {"max_grid": 2}, [0]),
    "pack_0": (48, FUSED, {"max_grid": 2, "pack": 0}, [0]),
    "prices_without_reciprocals": (5200, FUSED, {"max_grid": 2}, [0]),
    "one_shared_bin_copy": (48, FUSED, {"max_grid": 2, "bin_copies": 1}, [0]),
    "large_market_mode": (8200, FUSED, {"max_grid": 2}, [0]),
    "direct_small": (48, [seg(P, 2048)], {}, [0]),
    "one_block_is_direct": (48, [seg(P, 2600)], {"block": 1024, "max_grid": 1}, [0]),
    "ncoin": (48, [seg(W, 700, n_coins=3, packed=0, n_fees=0)], {}, [0]),
    "solidly": (48, [seg(S, 5200)], {"block": 1024, "max_grid": 2}, [0]),
    "geomean_exact": (48, [seg(G, 5200)], {"block": 1024, "max_grid": 2, "geomean_exact": 1}, [0]),
    "univ3_without_heads": (48, [seg(U, 5200)], {"block": 1024, "max_grid": 2, "univ3_heads": 0}, [0]),
    "bounded_product_alone": (48, [seg(U, 5200, has_walk=0)], {"block": 1024, "max_grid": 2}, [0]),   # no lists: the kernel without heads
    "single_family_512": (48, [seg(P, 5200)], {"block": 512}, [0]),
    "fused_1024": (48, FUSED, {"block": 1024, "max_grid": 2}, [0]),
}
# the fused launch of a market with an N-coin segment in it stays lean; the N-coin launch has no lean kernel
MIXED = {"ncoin_between": (48, [seg(P, 3000), seg(G, 2000), seg(W, 700, n_coins=3, packed=0, n_fees=0), seg(P, 1000), seg(U, 900, has_walk=0)],
                           {}, [1, 0, 1])}
CASES = {**LEAN, **GENERAL, **MIXED}


@pytest.mark.parametrize("name", list(CASES))
def test_which_launches_are_lean(name, lean):
    n, segs, options, want = CASES[name]
    assert lean(n, segs, **options) == want


def test_the_pool_bound(lean):
    """2^26 pools x 32 bytes per pool (the UniV3 heads) = 2 GiB: what a 32-bit byte offset reaches, with a factor 2 to spare"""
    assert lean(48, [seg(P, 1 << 26)], stream_stores=1) == [1]
    assert lean(48, [seg(P, (1 << 26) + 1)], stream_stores=1) == [0]
