"""cfmm_quote_out / cfmm_quote_out_dev, the parts that need no device: the argument lists across the header, the Python
argtypes and the Julia ccall; the router's mapping of pool numbers to (segment, row) on a mixed market with a host-evaluated
pool, on a recording backend; and the argument checks of backward_trade, which come before the library is touched."""
import os
import re

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib
from test_quote_cpu import FixedTrade, RecordingContext, mixed_router

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_python_and_julia_agree_on_the_arguments():
    h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "cfmm_amd.h")).read(), flags=re.S)
    want_c = ["cfmm_ctx*", "int32_t", "int64_t", "int64_t*", "int32_t*", "int32_t*", "double*", "double*"]
    py = open(os.path.join(ROOT, "cfmmrouter.jl_amd", "_lib.py")).read()
    names = {}
    for entry in ("cfmm_quote_out", "cfmm_quote_out_dev", "cfmm_quote", "cfmm_quote_dev"):
        params = re.search(r"int\s+" + entry + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S).group(1)
        parts = [p.strip() for p in params.replace("\n", " ").split(",")]
        assert [re.sub(r"\bconst\b", "", p).split()[0] for p in parts] == want_c, entry
        names[entry] = [p.split()[-1] for p in parts]
        argtypes = [a.strip() for a in re.search(r"L\." + entry + r"\.argtypes = \[(.*?)\]", py).group(1).split(",")]
        assert len(argtypes) == len(want_c) and argtypes[:3] == ["_ctx", "C.c_int32", "C.c_int64"], entry
    # the argument lists of the forward siblings, with the two amounts exchanged: the given one (const) before the answer
    assert names["cfmm_quote_out"][-2:] == ["amount_out", "amount_in"] and names["cfmm_quote"][-2:] == ["amount_in", "amount_out"]
    assert names["cfmm_quote_out_dev"][-2:] == ["d_amount_out", "d_amount_in"]
    assert names["cfmm_quote_out"][:-2] == names["cfmm_quote"][:-2] and names["cfmm_quote_out_dev"][:-2] == names["cfmm_quote_dev"][:-2]
    assert re.search(r"const\s+double\*\s+amount_out,\s*double\*\s+amount_in\)", h)
    for entry in ("cfmm_quote_out", "cfmm_quote_out_dev"):
        assert re.search(r"L\." + entry + r"\.argtypes = \[(.*?)\]", py).group(1) == \
            re.search(r"L\." + entry.replace("_out", "") + r"\.argtypes = \[(.*?)\]", py).group(1)
    jl = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    call = re.search(r"ccall\(\(:cfmm_quote_out,\s*LIB\),\s*Cint,\s*\((.*?)\),", jl, flags=re.S).group(1)
    assert [a.strip() for a in call.split(",")] == ["Ptr{Cvoid}", "Int32", "Int64", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Int32}",
                                                    "Ptr{Float64}", "Ptr{Float64}"]
    assert "function backward_trade(" in jl and "function quote_swaps_out(" in jl
    exported = re.search(r"^export (.*)$", jl, flags=re.M).group(1)
    assert "quote_swaps_out" in exported and "backward_trade" in exported
    tests = open(os.path.join(ROOT, "julia", "test", "runtests.jl")).read()
    assert "quote_swaps_out(" in tests and "backward_trade(" in tests
    assert "cfmm_quote_out" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(_lib.Context, "quote_out") and hasattr(_lib.Context, "quote_out_dev")
    assert "backward_trade" in cr.__all__ and "quote_out" in cr.__all__


class RecordingOutContext(RecordingContext):
    """quote_out recorded like quote; quote itself must not be called by the inverse verb"""

    def quote_out(self, seg, amount_out, coin_in, coin_out=None, idx=None):
        return RecordingContext.quote(self, seg, amount_out, coin_in, coin_out, idx)

    def quote(self, *a, **k):
        raise AssertionError("quote_out went to the forward entry")


def out_router():
    r, pools = mixed_router()
    r._backend.ctx.__class__ = RecordingOutContext          # the same recorder, answering the inverse verb only
    return r, pools


def test_router_maps_pool_numbers_to_segment_rows():
    r, pools = out_router()
    L = r._layout
    ctx = r._backend.ctx
    q_pools = [5, 0, 4, 3, 0, 1]
    amt = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    cin = [0, 1, 2, 0, 0, 1]
    cout = [1, 0, 0, 1, 1, 0]
    out = cr.quote_out(r, q_pools, cin, amt, cout)
    want = {}
    for q, i in enumerate(q_pools):
        _, b, row = L.locate(i)
        want.setdefault(L.seg_of[b], []).append((q, row))
    assert sorted(c[0] for c in ctx.calls) == sorted(want)          # one call per segment
    for seg, rows, ci, co, a in ctx.calls:
        qs = [q for q, _ in want[seg]]
        assert rows == [row for _, row in want[seg]]
        assert ci == [cin[q] for q in qs] and co == [cout[q] for q in qs] and a == [amt[q] for q in qs]
    for q, i in enumerate(q_pools):                                  # ... and the answers are in the caller's order
        _, b, row = L.locate(i)
        assert out[q] == 1000.0 * L.seg_of[b] + row + cin[q] / 10.0 + amt[q] / 1e6
    ctx.calls.clear()
    seg_p = L.seg_of[L.locate(0)[1]]
    cr.quote_out(r, [0, 3], 1, 2.5)                                  # scalars serve every query; coin_out may be left out
    assert ctx.calls == [(seg_p, [0, 1], [1, 1], None, [2.5, 2.5])]


def test_router_refuses_host_evaluated_and_unknown_pools():
    r, _ = out_router()
    with pytest.raises(cr.ArgumentError, match="FixedTrade"):
        cr.quote_out(r, [0, 2], 0, 1.0)
    assert r._backend.ctx.calls == []                      # nothing was sent before the refusal
    with pytest.raises(cr.ArgumentError, match="out of range"):
        cr.quote_out(r, [6], 0, 1.0)
    with pytest.raises(cr.ArgumentError, match="amount_out.*one entry per pool"):
        cr.quote_out(r, [0, 1], [0, 1, 0], 1.0)


def test_backward_trade_argument_checks():
    p2 = cr.ProductTwoCoin([10.0, 20.0], 0.997, [1, 2])
    p3 = cr.GeometricMean([1.0, 2.0, 3.0], [0.2, 0.3, 0.5], 0.997, [1, 2, 3])
    with pytest.raises(cr.ArgumentError, match="2 entries"):
        cr.backward_trade([1.0, 0.0, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="exactly one positive"):
        cr.backward_trade([1.0, 1.0], p2)
    with pytest.raises(cr.ArgumentError, match="finite and >= 0"):
        cr.backward_trade([-1.0, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="finite and >= 0"):
        cr.backward_trade([np.inf, 0.0], p2)
    with pytest.raises(cr.ArgumentError, match="coin_in= is required"):
        cr.backward_trade([1.0, 0.0, 0.0], p3)
    with pytest.raises(cr.ArgumentError, match="out of range"):
        cr.backward_trade([1.0, 0.0, 0.0], p3, coin_in=3)
    with pytest.raises(cr.ArgumentError, match="wanted coin"):
        cr.backward_trade([1.0, 0.0, 0.0], p3, coin_in=0)
    with pytest.raises(cr.ArgumentError, match="no device quote"):
        cr.backward_trade([1.0, 0.0], FixedTrade([1, 2]))
    # Λ == 0 returns 0.0 without a device
    assert cr.backward_trade([0.0, 0.0], p2) == 0.0
    assert cr.backward_trade([0.0, 0.0, 0.0], p3, coin_in=1) == 0.0


def test_context_wrapper_checks_shapes_before_the_library():
    ctx = object.__new__(cr.Context)
    ctx._h = None
    with pytest.raises(cr.ArgumentError, match="idx"):
        ctx.quote_out(0, [1.0, 2.0], 0, idx=[0])
    with pytest.raises(cr.ArgumentError, match="coin_in"):
        ctx.quote_out(0, [1.0, 2.0], [0, 1, 0])
