"""cfmm_swap, the parts that need no device: the argument list across the header, the Python argtypes and the Julia ccall;
and swap_ on a recording backend -- the mapping of pool numbers to (segment, row), the caller's order kept within a segment,
the answers in the caller's order, the refusal of a host-evaluated pool, the reset of the router's trades.  (The wave
numbering is a pure function of the host build: tests/test_swap_precise_cpu.py.)"""
import os
import re

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from test_quote_cpu import FixedTrade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_julia_agree_on_the_arguments():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert "NO cfmm_swap_dev" in h and "IN QUERY ORDER" in h and '"swap_refused"' in h and '"swap_ns"' in h
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    want_c = ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "int32_t*", "int32_t*", "double*", "double*"]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()

    def c_args(entry):
        params = re.search(r"int\s+" + entry + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
        return [re.sub(r"\bconst\b", "", p).split()[0] for p in params.replace("\n", " ").split(",")], \
            [p.split()[-1].lstrip("*") for p in params.replace("\n", " ").split(",")]
    types, names = c_args("cfmm_swap")
    assert types == want_c and (types, names) == c_args("cfmm_quote")           # the argument list is cfmm_quote's
    assert "cfmm_swap_dev" not in h
    argtypes = [a.strip() for a in re.search(r"L\.cfmm_swap\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert argtypes == ["_ctx", "C.c_int32", "C.c_int64", "_i64p", "_i32p", "_i32p", "_f64p", "_f64p"]
    assert argtypes == [a.strip() for a in re.search(r"L\.cfmm_quote\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_swap,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}",
                                                    "Ptr{Float64}", "Ptr{Float64}"]
    assert "function swap!(" in jl and "swap!" in re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "cfmm_swap" in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(_lib.Context, "swap") and not hasattr(_lib.Context, "swap_dev")
    assert "swap_" in cr.__all__
    mk = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "Makefile")).read()
    assert "abi_swap.cpp" in mk and "swap_kernels.h" in mk and "swap_pool.h" in mk


class RecordingContext:
    """stands in for _lib.Context: a swap answers 1000·seg + row + coin_in/10 + amount/1e6 and is recorded; the state it
    serves to the host mirror counts the swaps each row has had"""

    def __init__(self):
        self.calls, self.swapped = [], {}

    def swap(self, seg, amount_in, coin_in, coin_out=None, idx=None):
        self.calls.append((seg, list(idx), list(coin_in), None if coin_out is None else list(coin_out), list(amount_in)))
        for row in idx:
            self.swapped[(seg, row)] = self.swapped.get((seg, row), 0) + 1
        return 1000.0 * seg + np.asarray(idx) + np.asarray(coin_in) / 10.0 + np.asarray(amount_in) / 1e6

    def reserves(self, seg, m, n_coins=2):
        return np.array([[100.0 + self.swapped.get((seg, row), 0)] * n_coins for row in range(m)])


class RecordingBackend:
    def __init__(self, n):
        self.n, self.ctx = n, RecordingContext()

    def eval(self, v):
        return np.zeros(self.n), 0.0

    def find_arb(self, v):
        return np.ones(self.n), 1.0

    def trades(self):
        raise AssertionError("the trades of the old market must not be fetched after a swap")


def mixed_router(host_pool=True):
    pools = [cr.ProductTwoCoin([10.0, 20.0], 0.997, [1, 2]),                       # 0: product row 0
             cr.GeometricMeanTwoCoin([5.0, 6.0], [0.3, 0.7], 0.997, [2, 3]),        # 1: geomean row 0
             FixedTrade([1, 3]) if host_pool else cr.ProductTwoCoin([1.0, 2.0], 0.997, [1, 3]),   # 2: host (or product row 1)
             cr.ProductTwoCoin([30.0, 40.0], 0.997, [3, 4]),                        # 3: product
             cr.GeometricMean([1.0, 2.0, 3.0], [0.2, 0.3, 0.5], 0.997, [1, 2, 4]),  # 4: weighted, 3 coins
             cr.ProductTwoCoin([50.0, 60.0], 0.997, [1, 4])]                        # 5: product
    n = 4
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), pools, n, _backend=RecordingBackend(n))
    return r, pools


def test_swaps_keep_the_callers_order_within_a_segment():
    r, pools = mixed_router()
    L = r._layout
    ctx = r._backend.ctx
    cr.find_arb_(r, np.ones(4))
    assert r._trades_stale
    q_pools = [5, 0, 4, 5, 3, 0, 1, 5]                                              # pool 5 three times, pool 0 twice
    amt = np.arange(1.0, 9.0)
    cin = [0, 1, 2, 1, 0, 0, 1, 0]
    cout = [1, 0, 0, 0, 1, 1, 0, 1]
    out = cr.swap_(r, q_pools, cin, amt, cout)
    want = {}
    for q, i in enumerate(q_pools):
        _, b, row = L.locate(i)
        want.setdefault(L.seg_of[b], []).append((q, row))
    assert sorted(c[0] for c in ctx.calls) == sorted(want)                          # one call per segment
    for seg, rows, ci, co, a in ctx.calls:
        qs = [q for q, _ in want[seg]]
        assert qs == sorted(qs)                                                     # ... its swaps in the caller's order
        assert rows == [row for _, row in want[seg]]
        assert ci == [cin[q] for q in qs] and co == [cout[q] for q in qs] and a == [amt[q] for q in qs]
    for q, i in enumerate(q_pools):                                                 # the answers in the caller's order
        _, b, row = L.locate(i)
        assert out[q] == 1000.0 * L.seg_of[b] + row + cin[q] / 10.0 + amt[q] / 1e6
    # the router's trades are those of the old market: zeroed, and nothing is fetched from the backend
    assert not r._trades_stale and r._acc == 0.0 and np.all(r._psi == 0.0)
    assert all(np.all(np.asarray(x) == 0.0) for x in r.Δs) and all(np.all(np.asarray(x) == 0.0) for x in r.Λs)
    # sync_host=True (the default) refreshed the host mirror of the touched pools from the device
    assert list(pools[5].R) == [103.0, 103.0] and list(pools[0].R) == [102.0, 102.0] and list(pools[1].R) == [101.0, 101.0]
    assert list(pools[4].R) == [101.0] * 3
    # sync_host=False moves no state to the host
    ctx.calls.clear()
    cr.swap_(r, [3, 3], 1, 2.5, sync_host=False)
    assert ctx.calls == [(L.seg_of[L.locate(3)[1]], [L.locate(3)[2]] * 2, [1, 1], None, [2.5, 2.5])]
    assert list(pools[3].R) == [101.0, 101.0]                                       # (as the first call left it)


def test_swap_refuses_host_evaluated_and_unknown_pools():
    r, _ = mixed_router()
    cr.find_arb_(r, np.ones(4))
    with pytest.raises(cr.ArgumentError, match="FixedTrade is evaluated on the host by its own find_arb_ and has no device state to quote"):
        cr.swap_(r, [0, 2], 0, 1.0)
    assert r._backend.ctx.calls == []                                               # nothing was sent before the refusal
    assert not r._trades_stale                                                      # ... and _reset_trades ran all the same
    with pytest.raises(cr.ArgumentError, match="out of range"):
        cr.swap_(r, [6], 0, 1.0)
    with pytest.raises(cr.ArgumentError, match="one entry per pool"):
        cr.swap_(r, [0, 1], [0, 1, 0], 1.0)


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    with pytest.raises(cr.ArgumentError, match="idx"):
        ctx.swap(0, [1.0, 2.0], 0, idx=[0])
    with pytest.raises(cr.ArgumentError, match="coin_in"):
        ctx.swap(0, [1.0, 2.0], [0, 1, 0])
