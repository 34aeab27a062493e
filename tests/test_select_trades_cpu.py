"""active_trades / cfmm_select_trades, the parts that need no device: the host half of the rule (plugin-seam pools), the
wrapper's argument check, the argument count across the three bindings, and the chain-following loop of
tests/test_gpu_select_trades.py on the CPU oracle (the bound it asserts holds for the reference arithmetic alone)."""
import os
import re

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FixedTrade(cr.CFMM):
    """a plugin pool (its own find_arb_, no device kernel) that always proposes the same trade"""
    kind = "fixed"

    def __init__(self, Ai, D, L):
        self.Ai = np.asarray(Ai, dtype=np.int64)
        self.D, self.L = np.asarray(D, dtype=np.float64), np.asarray(L, dtype=np.float64)

    def find_arb_(self, Δ, Λ, v):
        Δ[:] = self.D
        Λ[:] = self.L


class NoPools:
    """the device half of a router without device pools"""

    def __init__(self, n):
        self.n = n

    def eval(self, v):
        return np.zeros(self.n), 0.0

    find_arb = eval


def reference(pools, v, tau):
    idx, vals = [], []
    for i, c in enumerate(pools):
        if not (np.any(c.D != 0.0) or np.any(c.L != 0.0)):
            continue
        value = 0.0
        for k, t in enumerate(c.Ai - 1):
            value = value + (c.L[k] - c.D[k]) * v[t]
        if value < tau:
            continue
        idx.append(i)
        vals.append(value)
    return np.array(idx, dtype=np.int64), np.array(vals)


def test_active_trades_of_host_evaluated_pools():
    n = 5
    v = np.array([1.0, 2.0, 0.5, 3.0, 1.5])
    pools = [FixedTrade([1, 2], [1.0, 0.0], [0.0, 0.75]),               # trades, value 0.5
             FixedTrade([2, 3], [0.0, 0.0], [0.0, 0.0]),                # idle
             FixedTrade([3, 4, 5], [0.0, 2.0, 0.0], [1.0, 0.0, 0.1]),   # three coins, value -5.35
             FixedTrade([1, 5], [-0.0, 0.0], [0.0, -0.0]),              # -0.0 alone does not trade
             FixedTrade([4, 1], [0.0, np.nan], [0.0, 0.0]),             # NaN trades, and its NaN value is never hidden
             FixedTrade([2, 4], [0.1, 0.0], [0.0, 0.1]),                # value 0.1
             FixedTrade([5, 3], [1e-3, 0.0], [0.0, 3e-3])]              # value exactly 0.0
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), pools, n, _backend=NoPools(n))
    cr.find_arb_(r, v)
    for tau, want in ((-np.inf, [0, 2, 4, 5, 6]), (0.0, [0, 4, 5, 6]), (0.2, [0, 4]), (np.inf, [4])):
        idx, Ds, Ls, val = cr.active_trades(r, tau)
        ref_idx, ref_val = reference(pools, v, tau)
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(idx, ref_idx)
        np.testing.assert_array_equal(val, ref_val)
        assert len(Ds) == len(Ls) == len(want)
        for i, D, L in zip(idx, Ds, Ls):
            np.testing.assert_array_equal(D, pools[i].D)
            np.testing.assert_array_equal(L, pools[i].L)
    assert cr.active_trades(r)[0].tolist() == [0, 4, 5, 6]              # min_value defaults to 0.0
    # the values belong to the latest find_arb!, not to r.v
    cr.find_arb_(r, 2.0 * v)
    np.testing.assert_array_equal(cr.active_trades(r, -np.inf)[3], reference(pools, 2.0 * v, -np.inf)[1])


def test_wrapper_refuses_a_negative_capacity():
    ctx = object.__new__(cr.Context)      # no device: the check comes before the library is touched
    ctx._h = None
    with pytest.raises(cr.ArgumentError, match="capacity"):
        ctx.select_trades(0, capacity=-1)


def test_header_python_and_julia_agree_on_the_arguments():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    params = re.search(r"int\s+cfmm_select_trades\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
    c_args = [p.strip() for p in params.replace("\n", " ").split(",")]
    assert len(c_args) == 10
    assert [re.sub(r"\bconst\b", "", a).split()[0] for a in c_args] == [
        "cfmm_ctx*", "int32_t", "double*", "double", "int64_t", "int64_t*", "int64_t*", "double*", "double*", "double*"]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    argtypes = re.search(r"L\.cfmm_select_trades\.argtypes = \[(.*?)\]", py).group(1)
    assert [a.strip() for a in argtypes.split(",")] == ["_ctx", "C.c_int32", "_f64p", "C.c_double", "C.c_int64", "_i64p", "_i64p",
                                                        "_f64p", "_f64p", "_f64p"]
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_select_trades,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == ["Ptr{Cvoid}", "Int32", "Ptr{Float64}", "Float64", "Int64", "Ref{Int64}",
                                                    "Ptr{Int64}", "Ptr{Float64}", "Ptr{Float64}", "Ptr{Float64}"]
    assert "select_trades" in open(os.path.join(ROOT, "julia", "test", "runtests.jl")).read()
    assert "cfmm_select_trades" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(_lib.Context, "select_trades") and hasattr(cr.DeviceBackend, "active_trades")


def test_the_loop_on_the_cpu_oracle():
    """route!, update_reserves!, 50 moved pools, find_arb! at the same prices -- in the reference arithmetic (the CPU oracle):
    the pools that trade afterwards are a non-empty set of less than 5 % of the 20 000."""
    from helpers import OracleBackend
    from test_gpu_select_trades import N, expected, loop_market, run_loop
    batches, pi = loop_market()
    r = cr.Router(cr.LinearNonnegative(pi), batches, N, _backend=OracleBackend(N, batches, nthreads=4))
    v = run_loop(r, batches)
    D, L = r._backend.trades()
    Ai = np.concatenate([b.Ai for b in batches])
    want, value = expected(np.reshape(D, (-1, 2)), np.reshape(L, (-1, 2)), Ai, v, 0.0)
    assert 0 < want.size < 0.05 * len(Ai), want.size
