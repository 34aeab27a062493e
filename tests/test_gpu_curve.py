"""Curve (StableSwap) pools on the device (CFMM_KIND_CURVE, sweep_ncoin<CurveFamily>): N = 2..8 against the CPU reference
(tests/curve_ref.py), α = 0 against the device's own ProductTwoCoin and equal-weight weighted segments, edge cases, mixed
markets, route! against the host plugin seam, update_reserves!, multi-device parents and the error paths."""
import math

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain, synth
from cfmmrouter_amd._lib import KIND_CURVE, KIND_PRODUCT, KIND_WEIGHTED
from helpers import coin_scale, device_sweep, rel_to_max
from reduction_ref import assert_reduction_exact

import curve_ref as cv

pytestmark = pytest.mark.gpu


def _near_prices(n, seed):
    """prices within ~1e-3 of each other: the regime StableSwap pools are built for (stiff, small trades)"""
    return np.exp(1e-3 * np.random.default_rng(seed).standard_normal(n))


@pytest.mark.parametrize("nc, prices, m", [(nc, "spread", 200_000) for nc in range(2, 9)] +
                         [(nc, "near", 100_000) for nc in (2, 3, 8)])
def test_n_coin_pools_match_the_cpu_reference(nc, prices, m):
    n = 128
    b = synth.curve_pools(m, n, nc, seed=10 + nc)
    v = synth.sweep_prices(n, seed=20 + nc, spread=0.5) if prices == "spread" else _near_prices(n, 20 + nc)
    D, L, psi, acc = device_sweep(n, [b], v)
    D, L = D.reshape(m, nc), L.reshape(m, nc)
    Do, Lo = cv.sweep(b, v)
    s = coin_scale(b)
    assert np.max(np.abs(D - Do) / s) <= 1e-10 and np.max(np.abs(L - Lo) / s) <= 1e-10
    assert np.all(D >= 0) and np.all(L >= 0)
    assert np.mean(np.any(L > 0, axis=1)) > 0.3
    Ai0 = b.Ai - 1
    for i in range(0, m, 4001):   # the KKT predicate, on a sample
        assert cv.optimality_ok(v[Ai0[i]], D[i], L[i], b.R[i], b.α[i], b.β[i], b.γ[i]), i
    flows = L - D
    psi_exact = np.array([math.fsum(flows[Ai0 == t]) for t in range(n)])
    assert rel_to_max(psi, psi_exact) <= 1e-12
    vl = v[Ai0]
    acc_exact = math.fsum(np.concatenate([(L * vl).ravel(), -(D * vl).ravel()]))
    assert abs(acc - acc_exact) <= 1e-12 * max(abs(acc_exact), 1.0)
    assert_reduction_exact(D, L, Ai0, v, n, psi, acc)   # per token: exact for <= 1 flow, (c + 2)·u·Σ|t| otherwise


def test_alpha_zero_matches_device_product_and_weighted():
    n, m = 64, 100_000
    v = synth.sweep_prices(n, seed=3, spread=0.5)
    for nc in (2, 3, 4, 8):
        b = synth.curve_pools(m, n, nc, seed=30 + nc, regime="alpha0")
        assert np.all(b.α == 0)
        if nc == 2:
            other = cr.PoolBatch(KIND_PRODUCT, R=b.R, γ=b.γ, Ai=b.Ai)
        else:
            other = cr.PoolBatch(KIND_WEIGHTED, R=b.R, w=np.full((m, nc), 1.0 / nc), γ=b.γ, Ai=b.Ai)
        Dc, Lc, psic, accc = device_sweep(n, [b], v)
        Do, Lo, psio, acco = device_sweep(n, [other], v)
        s = np.repeat(coin_scale(b), nc, axis=1).ravel()
        assert np.max(np.abs(Dc - Do) / s) <= 1e-12 and np.max(np.abs(Lc - Lo) / s) <= 1e-12, nc
        assert rel_to_max(psic, psio) <= 1e-12
        assert abs(accc - acco) <= 1e-12 * abs(acco)


def test_edge_cases():
    n = 8
    v = np.array([1.0, 1.00001, 0.99999, 1e6, 1e-6, 1.0, 2.0, 0.5])
    Ai = np.array([[1, 2, 3], [1, 2, 3], [1, 4, 5], [6, 7, 8], [1, 2, 3], [6, 7, 8], [1, 4, 6]])
    bal = np.array([[1e6, 1e6, 1e6],          # balanced, prices inside the fee band: no trade
                    [1e6, 1e6, 1e6],          # the same at γ = 1: trades (small)
                    [1e6, 1e6, 1e6],          # extreme price ratios (1e12 between two coins)
                    [1e30, 2e30, 5e29],       # huge β (D ~ 1e30: β ~ 1e120)
                    [1e-6, 2e-6, 1.5e-6],     # tiny β
                    [3.0, 5.0, 2.0],          # α = 0
                    [1e6, 1e3, 1e6]])         # a drained stable pool, huge A
    A = np.array([100.0, 100.0, 50.0, 200.0, 10.0, 0.0, 5000.0])
    g = np.array([0.9996, 1.0, 0.997, 0.9996, 1.0, 0.997, 0.9996])
    al, be = chain.stableswap_params(bal, A)
    b = cr.Curve.batch(bal, g, Ai, al, be)
    D, L, psi, acc = device_sweep(n, [b], v)
    D, L = D.reshape(-1, 3), L.reshape(-1, 3)
    assert np.all(D[0] == 0) and np.all(L[0] == 0) and not np.any(np.signbit(D[0])) and not np.any(np.signbit(L[0]))
    Do, Lo = cv.sweep(b, v)
    s = coin_scale(b)
    assert np.max(np.abs(D - Do) / s) <= 1e-10 and np.max(np.abs(L - Lo) / s) <= 1e-10
    for i in range(1, len(b)):
        assert np.any(D[i] > 0) and np.any(L[i] > 0), i
        # row 2 drains a coin from 1e6 to ~5e-3: R + γΔ − Λ rounds at the old reserve's ulp, ~2e-8 of what is left
        assert cv.optimality_ok(v[Ai[i] - 1], D[i], L[i], bal[i], al[i], be[i], g[i], rtol=1e-6 if i == 2 else 1e-10), i
        # a coin that does not trade is exactly +0.0 in both arrays
        still = (D[i] == 0) & (L[i] == 0)
        assert not np.any(np.signbit(D[i][still])) and not np.any(np.signbit(L[i][still]))
    assert np.all(np.isfinite(psi)) and np.isfinite(acc)


def _mixed(n):
    return [synth.product_pools(30_000, n, seed=31), synth.geomean_pools(20_000, n, seed=32),
            synth.bounded_product_pools(10_000, n, seed=33)]


def test_mixed_market_other_rows_unchanged_and_reproducible():
    n = 48
    two = _mixed(n)
    wt = synth.weighted_pools(25_000, n, 3, seed=34)
    curves = [synth.curve_pools(25_000, n, 3, seed=35), synth.curve_pools(15_000, n, 4, seed=36)]
    v = synth.sweep_prices(n, seed=37, spread=0.5)
    m2 = sum(len(b) for b in two)
    be0 = cr.DeviceBackend(n, two + [wt])
    be = cr.DeviceBackend(n, two + [wt] + curves)
    try:
        be0.find_arb(v)
        D0, L0 = be0.trades()
        nw = 2 * m2 + 3 * 25_000
        assert be.ctx.trades_len == nw + 3 * 25_000 + 4 * 15_000
        psi1, acc1 = be.find_arb(v)
        D1, L1 = be.trades()
        np.testing.assert_array_equal(D1[:nw], D0)
        np.testing.assert_array_equal(L1[:nw], L0)
        be.eval(v * 1.1)   # another evaluation in between (alternating tile order)
        psi2, acc2 = be.find_arb(v)
        D2, L2 = be.trades()
        np.testing.assert_array_equal(D1, D2)
        np.testing.assert_array_equal(L1, L2)
        np.testing.assert_array_equal(psi1, psi2)
        assert acc1 == acc2
        p3, a3 = be.eval(v)
        p4, a4 = be.eval(v)
        np.testing.assert_array_equal(p3, p4)
        assert a3 == a4
        assert be.ctx._L.cfmm_segment_count(be.ctx._h) == 6
        Dc = D1[nw:nw + 3 * 25_000].reshape(-1, 3)
        np.testing.assert_allclose(Dc, cv.sweep(curves[0], v)[0], rtol=0, atol=1e-10 * coin_scale(curves[0]).max())
    finally:
        be0.close()
        be.close()


class HostCurve(cr.CFMM):
    """The same pool through the host plugin seam: a CFMM subclass with its own find_arb_ (curve_ref)."""

    kind = -1

    def __init__(self, R, γ, Ai, α, β):
        self.R, self.γ, self.Ai, self.α, self.β = np.array(R, float), float(γ), np.array(Ai), float(α), float(β)

    def find_arb_(self, Δ, Λ, v):
        D, L = cv.solve(self.R[None], [self.α], [self.β], [self.γ], np.asarray(v)[None])
        Δ[:] = D[0]
        Λ[:] = L[0]


@pytest.mark.parametrize("objective", ["linear", "basket"])
def test_route_matches_the_host_plugin_seam(objective):
    n = 6
    rng = np.random.default_rng(5)
    pools, host = [], []
    for k in range(12):
        nc = 2 + k % 3
        Ai = rng.choice(n, size=nc, replace=False) + 1
        R = rng.uniform(50.0, 150.0, size=nc)
        A = [0.0, 0.2, 1.0][k % 3]   # (stiffer pools turn the solver's stopping noise in v into netflow noise)
        al, be = chain.stableswap_params(R, A)
        g = [0.997, 1.0][k % 2]
        pools.append(cr.Curve(R, g, Ai, float(al), float(be)))
        host.append(HostCurve(R, g, Ai, float(al), float(be)))
    two = [cr.ProductTwoCoin([100.0, 120.0], 0.997, [1, 2]), cr.GeometricMeanTwoCoin([80.0, 50.0], [0.3, 0.7], 0.997, [2, 3])]
    obj = (lambda: cr.LinearNonnegative(np.linspace(0.5, 1.5, n))) if objective == "linear" else \
        (lambda: cr.BasketLiquidation(1, np.array([0.0, 5.0, 3.0, 0.0, 2.0, 1.0])))
    rd = cr.Router(obj(), two + pools, n)
    rh = cr.Router(obj(), two + host, n)
    try:
        cr.route_(rd, solver="native", pgtol=1e-8)   # cfmm_route: the whole route! in the library (pre-armed evaluations)
        cr.route_(rh, pgtol=1e-8)
        psi_d, psi_h = cr.netflows(rd), cr.netflows(rh)
        scale = np.max(np.abs(psi_h))
        assert np.max(np.abs(psi_d - psi_h)) <= 1e-6 * scale
        assert np.max(np.abs(rd.v - rh.v)) <= 1e-6 * np.max(np.abs(rh.v))
        assert len(rd.Δs) == len(two) + len(pools) and len(rd.Δs[2]) == 2 and len(rd.Δs[3]) == 3 and len(rd.Δs[4]) == 4
        for k in range(len(pools)):
            np.testing.assert_allclose(rd.Δs[2 + k], rh.Δs[2 + k], rtol=0, atol=1e-5 * scale)
    finally:
        rd.close()
        rh.close()


def test_update_reserves_leaves_no_arbitrage():
    n = 32
    bs = [synth.curve_pools(40_000, n, 3, seed=41), synth.curve_pools(20_000, n, 5, seed=42)]
    v = synth.sweep_prices(n, seed=43, spread=0.5)
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), bs, n)
    try:
        cr.find_arb_(r, v)
        D = [d.copy() for d in r.Δs]
        L = [l.copy() for l in r.Λs]
        R0 = [b.R.copy() for b in bs]
        al0, be0 = [b.α.copy() for b in bs], [b.β.copy() for b in bs]
        cr.update_reserves_(r)
        k = 0
        for b, R in zip(bs, R0):
            for i in range(0, len(b), 997):
                np.testing.assert_array_equal(b.R[i], (R[i] + b.γ[i] * D[k + i]) - L[k + i])
            k += len(b)
        be = r._backend
        np.testing.assert_array_equal(be.ctx.reserves(1, 20_000, 5), bs[1].R)
        for b, a0, b0 in zip(bs, al0, be0):   # α, β: the pool's parameters, unchanged
            np.testing.assert_array_equal(b.α, a0)
            np.testing.assert_array_equal(b.β, b0)
        cr.find_arb_(r, v)
        # measured against the reserves before the update: R + γΔ − Λ rounds at THEIR ulp, and that rounding is all the
        # second sweep can find (stiff pools turn it into trades of up to ~1e-10 of the pool)
        for Dn, Ln, b, R in zip(np.split(np.concatenate(r.Δs), [3 * 40_000]), np.split(np.concatenate(r.Λs), [3 * 40_000]), bs, R0):
            s = np.repeat(R.max(axis=1, keepdims=True), b.n_coins, axis=1).ravel()
            assert np.max(Dn / s) <= 1e-9 and np.max(Ln / s) <= 1e-9
            assert np.median(np.concatenate([Dn / s, Ln / s])) <= 1e-13
    finally:
        r.close()


def test_multi_device_parent_matches_single_context():
    n = 40
    bs = [synth.product_pools(10_001, n, seed=51), synth.curve_pools(30_001, n, 4, seed=52),
          synth.curve_pools(7_777, n, 3, seed=53)]
    v = synth.sweep_prices(n, seed=54, spread=0.5)
    D1, L1, psi1, acc1 = device_sweep(n, bs, v)
    D3, L3, psi3, acc3 = device_sweep(n, bs, v, device=[0, 0, 0])
    np.testing.assert_array_equal(D1, D3)
    np.testing.assert_array_equal(L1, L3)
    assert rel_to_max(psi3, psi1) <= 1e-12
    be = cr.DeviceBackend(n, bs, device=[0, 0, 0])
    try:
        be.find_arb(v)
        Dr, Lr = be.ctx.trades_range(1, 1000, 20_000, n_coins=4)
        np.testing.assert_array_equal(Dr.ravel(), D1[2 * 10_001 + 4 * 1000:2 * 10_001 + 4 * 21_000])
        be.ctx.update_reserves()
        np.testing.assert_array_equal(be.ctx.reserves(2, 7_777, 3), (bs[2].R + bs[2].γ[:, None] * D1[-3 * 7_777:].reshape(-1, 3))
                                      - L1[-3 * 7_777:].reshape(-1, 3))
    finally:
        be.close()


def test_errors():
    ctx = cr.Context(10, 0)
    try:
        R = np.ones((2, 3))
        g = np.full(2, 0.997)
        al, be = np.full(2, 100.0), np.full(2, 2.0)
        Ai = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
        with pytest.raises(cr.ArgumentError, match="coins"):
            ctx.add_curve(np.ones((2, 1)), g, np.zeros((2, 1), dtype=np.int32), al, be)
        with pytest.raises(cr.ArgumentError, match="coins"):
            ctx.add_curve(np.ones((1, 9)), g[:1], np.arange(9, dtype=np.int32)[None], al[:1], be[:1])
        with pytest.raises(cr.ArgumentError, match="distinct"):
            ctx.add_curve(R, g, np.array([[0, 1, 2], [3, 4, 3]], dtype=np.int32), al, be)
        with pytest.raises(cr.ArgumentError, match="reserves"):
            ctx.add_curve(np.array([[1.0, 0.0, 1.0], [1, 1, 1]]), g, Ai, al, be)
        with pytest.raises(cr.ArgumentError, match="reserves"):
            ctx.add_curve(np.array([[1.0, np.inf, 1.0], [1, 1, 1]]), g, Ai, al, be)
        with pytest.raises(cr.ArgumentError, match="alpha"):
            ctx.add_curve(R, g, Ai, np.array([100.0, -1.0]), be)
        with pytest.raises(cr.ArgumentError, match="alpha"):
            ctx.add_curve(R, g, Ai, np.array([100.0, np.nan]), be)
        with pytest.raises(cr.ArgumentError, match="beta"):
            ctx.add_curve(R, g, Ai, al, np.array([0.0, 1.0]))
        with pytest.raises(cr.ArgumentError, match="beta"):
            ctx.add_curve(R, g, Ai, al, np.array([np.inf, 1.0]))
        with pytest.raises(cr.ArgumentError, match="unbounded"):
            ctx.add_curve(R, np.array([0.997, 1.001]), Ai, al, be)
        with pytest.raises(cr.ArgumentError, match="gamma"):
            ctx.add_curve(R, np.array([0.997, 0.0]), Ai, al, be)
        with pytest.raises(cr.ArgumentError, match="out of range"):
            ctx.add_curve(R, g, np.array([[0, 1, 2], [3, 4, 10]], dtype=np.int32), al, be)
        assert ctx.pool_count == 0
        ctx.add_curve(R, g, Ai, al, be)
        ctx.add_product(np.ones((1, 2)), np.ones(1), np.array([[0, 1]], dtype=np.int32))
        ctx.find_arb(np.linspace(1.0, 2.0, 10))
        with pytest.raises(NotImplementedError, match="ragged"):
            ctx._check(ctx._L.cfmm_trades_dev(ctx._h, None, None))
        D, L = ctx.trades()
        assert D.shape == (2 * 3 + 2,)
    finally:
        ctx.close()
    big = cr.Context(8193, 0)
    try:
        with pytest.raises(NotImplementedError, match="8192"):
            big.add_curve(np.ones((1, 3)), [1.0], np.array([[0, 1, 2]], dtype=np.int32), [1.0], [1.0])
    finally:
        big.close()


def test_find_arb_on_a_single_pool():
    R = np.array([1.0e6, 1.2e6, 0.9e6, 1.1e6])
    al, be = chain.stableswap_params(R, 300.0)
    p = cr.Curve(R, 0.9996, [3, 1, 4, 2], float(al), float(be))
    v = np.array([1.0, 1.002, 0.998, 1.001])
    D, L = np.zeros(4), np.zeros(4)
    cr.find_arb_(D, L, p, v)
    Do, Lo = cv.solve(p.R[None], [p.α], [p.β], [p.γ], v[None])
    np.testing.assert_allclose(D, Do[0], rtol=0, atol=1e-10 * R.max())
    np.testing.assert_allclose(L, Lo[0], rtol=0, atol=1e-10 * R.max())
    assert np.any(L > 0)
    assert cv.optimality_ok(v, D, L, p.R, p.α, p.β, p.γ)
