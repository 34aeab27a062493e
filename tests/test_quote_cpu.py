"""cfmm_quote / cfmm_quote_dev, the parts that need no device: the argument lists across the header, the Python argtypes and
the Julia ccall; the router's mapping of pool numbers to (segment, row) on a mixed market with a host-evaluated pool, on a
recording backend; and the argument checks of forward_trade, which come before the library is touched."""
import os
import re

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_julia_agree_on_the_arguments():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert h.count("src/cfmms.jl:398-449") >= 2            # each entry cites what it generalises
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    want_c = ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "int32_t*", "int32_t*", "double*", "double*"]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    for entry in ("cfmm_quote", "cfmm_quote_dev"):
        params = re.search(r"int\s+" + entry + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
        c_args = [re.sub(r"\bconst\b", "", p).split()[0] for p in params.replace("\n", " ").split(",")]
        assert c_args == want_c, entry
        argtypes = [a.strip() for a in re.search(r"L\." + entry + r"\.argtypes = \[(.*?)\]", py).group(1).split(",")]
        assert len(argtypes) == len(want_c) and argtypes[:3] == ["_ctx", "C.c_int32", "C.c_int64"], entry
    host = [a.strip() for a in re.search(r"L\.cfmm_quote\.argtypes = \[(.*?)\]", py).group(1).split(",")]
    assert host[3:] == ["_i64p", "_i32p", "_i32p", "_f64p", "_f64p"]
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_quote,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}",
                                                    "Ptr{Float64}", "Ptr{Float64}"]
    assert "function forward_trade(" in jl and "function quote_swaps(" in jl
    assert "cfmm_quote" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(_lib.Context, "quote") and hasattr(_lib.Context, "quote_dev")
    assert "forward_trade" in cr.__all__ and "quote" in cr.__all__


class FixedTrade(cr.CFMM):
    """a plugin pool (its own find_arb_, no device kernel)"""
    kind = "fixed"

    def __init__(self, Ai):
        self.Ai = np.asarray(Ai, dtype=np.int64)

    def find_arb_(self, Δ, Λ, v):
        Δ[:] = 0.0
        Λ[:] = 0.0


class RecordingContext:
    """stands in for _lib.Context: answers every query with 1000·seg + row + coin_in/10 + amount/1e6"""

    def __init__(self):
        self.calls = []

    def quote(self, seg, amount_in, coin_in, coin_out=None, idx=None):
        self.calls.append((seg, list(idx), list(coin_in), None if coin_out is None else list(coin_out), list(amount_in)))
        return 1000.0 * seg + np.asarray(idx) + np.asarray(coin_in) / 10.0 + np.asarray(amount_in) / 1e6


class RecordingBackend:
    def __init__(self, n):
        self.n, self.ctx = n, RecordingContext()

    def eval(self, v):
        return np.zeros(self.n), 0.0

    find_arb = eval


def mixed_router():
    pools = [cr.ProductTwoCoin([10.0, 20.0], 0.997, [1, 2]),                       # 0: product row 0
             cr.GeometricMeanTwoCoin([5.0, 6.0], [0.3, 0.7], 0.997, [2, 3]),        # 1: geomean row 0
             FixedTrade([1, 3]),                                                   # 2: host
             cr.ProductTwoCoin([30.0, 40.0], 0.997, [3, 4]),                        # 3: product row 1
             cr.GeometricMean([1.0, 2.0, 3.0], [0.2, 0.3, 0.5], 0.997, [1, 2, 4]),  # 4: weighted, 3 coins
             cr.ProductTwoCoin([50.0, 60.0], 0.997, [1, 4])]                        # 5: product row 2
    n = 4
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), pools, n, _backend=RecordingBackend(n))
    return r, pools


def test_router_maps_pool_numbers_to_segment_rows():
    r, pools = mixed_router()
    L = r._layout
    ctx = r._backend.ctx
    q_pools = [5, 0, 4, 3, 0, 1]
    amt = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    cin = [0, 1, 2, 0, 0, 1]
    cout = [1, 0, 0, 1, 1, 0]
    out = cr.quote(r, q_pools, cin, amt, cout)
    # every query went to the segment and row update_pools_ would send that pool's change to, in one call per segment
    want = {}
    for q, i in enumerate(q_pools):
        _, b, row = L.locate(i)
        want.setdefault(L.seg_of[b], []).append((q, row))
    assert sorted(c[0] for c in ctx.calls) == sorted(want)
    for seg, rows, ci, co, a in ctx.calls:
        qs = [q for q, _ in want[seg]]
        assert rows == [row for _, row in want[seg]]
        assert ci == [cin[q] for q in qs] and co == [cout[q] for q in qs] and a == [amt[q] for q in qs]
    # ... and the answers are in the caller's order
    for q, i in enumerate(q_pools):
        _, b, row = L.locate(i)
        assert out[q] == 1000.0 * L.seg_of[b] + row + cin[q] / 10.0 + amt[q] / 1e6
    # the three product pools share a segment with rows 0, 1, 2 in router order
    seg_p = L.seg_of[L.locate(0)[1]]
    assert [L.locate(i)[2] for i in (0, 3, 5)] == [0, 1, 2] and all(L.seg_of[L.locate(i)[1]] == seg_p for i in (0, 3, 5))
    # scalars serve every query; coin_out may be left out
    ctx.calls.clear()
    cr.quote(r, [0, 3], 1, 2.5)
    assert ctx.calls == [(seg_p, [0, 1], [1, 1], None, [2.5, 2.5])]


def test_router_refuses_host_evaluated_and_unknown_pools():
    r, _ = mixed_router()
    with pytest.raises(cr.ArgumentError, match="FixedTrade"):
        cr.quote(r, [0, 2], 0, 1.0)
    assert r._backend.ctx.calls == []                      # nothing was sent before the refusal
    with pytest.raises(cr.ArgumentError, match="out of range"):
        cr.quote(r, [6], 0, 1.0)
    with pytest.raises(cr.ArgumentError, match="one entry per pool"):
        cr.quote(r, [0, 1], [0, 1, 0], 1.0)


def test_forward_trade_argument_checks():
    p2 = cr.ProductTwoCoin([10.0, 20.0], 0.997, [1, 2])
    p3 = cr.GeometricMean([1.0, 2.0, 3.0], [0.2, 0.3, 0.5], 0.997, [1, 2, 3])
    with pytest.raises(cr.ArgumentError, match="2 entries"):
        cr.forward_trade([1.0, 0.0, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="exactly one positive"):
        cr.forward_trade([1.0, 1.0], p2)
    with pytest.raises(cr.ArgumentError, match="finite and >= 0"):
        cr.forward_trade([-1.0, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="finite and >= 0"):
        cr.forward_trade([np.inf, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="coin_out= is required"):
        cr.forward_trade([1.0, 0.0, 0.0], p3)
    with pytest.raises(cr.ArgumentError, match="out of range"):
        cr.forward_trade([1.0, 0.0, 0.0], p3, coin_out=3)
    with pytest.raises(cr.ArgumentError, match="tendered coin"):
        cr.forward_trade([1.0, 0.0, 0.0], p3, coin_out=0)
    with pytest.raises(cr.ArgumentError, match="no device quote"):
        cr.forward_trade([1.0, 0.0], FixedTrade([1, 2]))
    # Δ == 0 returns 0.0 without a device (src/cfmms.jl:440-442)
    assert cr.forward_trade([0.0, 0.0], p2) == 0.0
    assert cr.forward_trade([0.0, 0.0, 0.0], p3, coin_out=1) == 0.0


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    with pytest.raises(cr.ArgumentError, match="idx"):
        ctx.quote(0, [1.0, 2.0], 0, idx=[0])
    with pytest.raises(cr.ArgumentError, match="coin_in"):
        ctx.quote(0, [1.0, 2.0], [0, 1, 0])
