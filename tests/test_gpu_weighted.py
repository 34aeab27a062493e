"""N-coin weighted geometric-mean pools on the device (CFMM_KIND_WEIGHTED, sweep_ncoin<WeightedFamily>): parity with the
device's own two-coin families at N = 2, with the CPU reference (tests/weighted_ref.py) at N = 3..8, edge cases, mixed markets,
route! against the host plugin seam, update_reserves!, multi-device parents and the error paths."""
import math

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_GEOMEAN, KIND_PRODUCT, KIND_WEIGHTED
from helpers import coin_scale, device_sweep, rel_to_max
from reduction_ref import assert_reduction_exact

import weighted_ref as wr

pytestmark = pytest.mark.gpu


def test_two_coin_weighted_matches_device_two_coin_families():
    n, m = 64, 100_000
    bp, bg = synth.product_pools(m, n, seed=1), synth.geomean_pools(m, n, seed=2)
    bp = cr.PoolBatch(KIND_PRODUCT, R=bp.R, γ=np.where(bp.γ > 1, 1.0, bp.γ), Ai=bp.Ai)
    bg = cr.PoolBatch(KIND_GEOMEAN, R=bg.R, w=bg.w, γ=np.where(bg.γ > 1, 1.0, bg.γ), Ai=bg.Ai)
    v = synth.sweep_prices(n, seed=3, spread=0.5)
    for two, wt in [(bp, cr.PoolBatch(KIND_WEIGHTED, R=bp.R, w=np.full((m, 2), 0.5), γ=bp.γ, Ai=bp.Ai)),
                    (bg, cr.PoolBatch(KIND_WEIGHTED, R=bg.R, w=bg.w, γ=bg.γ, Ai=bg.Ai))]:
        D2, L2, psi2, acc2 = device_sweep(n, [two], v)
        Dw, Lw, psiw, accw = device_sweep(n, [wt], v)
        s = np.repeat(coin_scale(two), 2, axis=1).ravel()
        assert np.max(np.abs(Dw - D2) / s) <= 1e-12 and np.max(np.abs(Lw - L2) / s) <= 1e-12
        assert rel_to_max(psiw, psi2) <= 1e-12
        assert abs(accw - acc2) <= 1e-12 * abs(acc2)


@pytest.mark.parametrize("nc", [3, 4, 5, 8])
def test_n_coin_pools_match_the_cpu_reference(nc):
    n, m = 128, 200_000
    b = synth.weighted_pools(m, n, nc, seed=10 + nc)
    v = synth.sweep_prices(n, seed=20 + nc, spread=0.5)
    D, L, psi, acc = device_sweep(n, [b], v)
    D, L = D.reshape(m, nc), L.reshape(m, nc)
    Do, Lo = wr.sweep(b, v)
    s = coin_scale(b)
    assert np.max(np.abs(D - Do) / s) <= 1e-11 and np.max(np.abs(L - Lo) / s) <= 1e-11
    assert np.all(D >= 0) and np.all(L >= 0)
    Ai0 = b.Ai - 1
    for i in range(0, m, 4001):   # the reference's optimality predicate (test/cfmms.jl:3-22), on a sample
        assert wr.optimality_ok(v[Ai0[i]], D[i], L[i], b.R[i], b.w[i], b.γ[i]), i
    # Ψ and acc against exactly summed values
    flows = (L - D)
    psi_exact = np.array([math.fsum(flows[Ai0 == t]) for t in range(n)])
    assert rel_to_max(psi, psi_exact) <= 1e-12
    vl = v[Ai0]
    acc_exact = math.fsum(np.concatenate([(L * vl).ravel(), -(D * vl).ravel()]))
    assert abs(acc - acc_exact) <= 1e-12 * max(abs(acc_exact), 1.0)
    assert_reduction_exact(D, L, Ai0, v, n, psi, acc)   # per token: exact for <= 1 flow, (c + 2)·u·Σ|t| otherwise


def test_edge_cases():
    n = 8
    v = np.array([1.0, 2.0, 0.5, 4.0, 1.5, 3.0, 0.25, 8.0])
    Ai = np.array([[1, 2, 3], [4, 5, 6], [1, 2, 3], [7, 8, 1], [2, 4, 6], [3, 5, 7]])
    vl = v[Ai - 1]
    w = np.array([[1, 1, 1], [1, 2, 1], [0.01, 0.99, 1.0], [0.01, 0.99, 0.5], [1, 1, 1], [1, 1, 1]], dtype=np.float64)
    wn = w / w.sum(axis=1, keepdims=True)
    R = wn / vl * 1000.0                      # exact equilibrium: R·v/w equal across the coins
    R[2] *= [1.0, 1.001, 1.0]                 # inside the fee band of γ = 0.997
    R[3] = [1e-6, 1e12, 3.0]                  # reserves over eighteen decades, tiny / dominant weights
    R[4] = [1.0, 2.0, 3.0]                    # far from equilibrium, γ = 1
    R[5] = [1e-6, 1.0, 1e12]
    g = np.array([0.997, 0.99, 0.997, 0.997, 1.0, 1.0])
    b = cr.PoolBatch(KIND_WEIGHTED, R=R, w=w, γ=g, Ai=Ai)
    D, L, psi, acc = device_sweep(n, [b], v)
    D, L = D.reshape(-1, 3), L.reshape(-1, 3)
    for i in (0, 1, 2):   # equilibrium / fee band: exact +0.0
        assert np.all(D[i] == 0) and np.all(L[i] == 0) and not np.any(np.signbit(D[i])) and not np.any(np.signbit(L[i]))
    Do, Lo = wr.sweep(b, v)
    s = coin_scale(b)
    assert np.max(np.abs(D - Do) / s) <= 1e-11 and np.max(np.abs(L - Lo) / s) <= 1e-11
    for i in (3, 4, 5):
        assert np.any(D[i] > 0) and np.any(L[i] > 0)
        Rp = R[i] + g[i] * D[i] - L[i]
        assert np.all(Rp > 0)
        # the invariant is kept up to the rounding of R + γΔ − Λ itself (a coin drained from 1e12 to ~1e2 keeps only ~1e-6 of it)
        tol = 1e-12 * max(1.0, np.abs(np.log(R[i])).max()) + 4 * np.finfo(float).eps * np.sum(wn[i] * (R[i] + D[i] + L[i]) / Rp)
        assert abs(np.sum(wn[i] * np.log(Rp)) - np.sum(wn[i] * np.log(R[i]))) <= tol


def _mixed(n):
    return [synth.product_pools(30_000, n, seed=31), synth.geomean_pools(20_000, n, seed=32),
            synth.bounded_product_pools(10_000, n, seed=33)]


def test_mixed_market_two_coin_rows_unchanged_and_reproducible():
    n = 48
    two = _mixed(n)
    wts = [synth.weighted_pools(25_000, n, 3, seed=34), synth.weighted_pools(15_000, n, 4, seed=35)]
    v = synth.sweep_prices(n, seed=36, spread=0.5)
    m2 = sum(len(b) for b in two)
    be0 = cr.DeviceBackend(n, two)
    be = cr.DeviceBackend(n, two + wts)
    try:
        be0.find_arb(v)
        D0, L0 = be0.trades()
        assert be.ctx.trades_len == 2 * m2 + 3 * 25_000 + 4 * 15_000
        psi1, acc1 = be.find_arb(v)
        D1, L1 = be.trades()
        np.testing.assert_array_equal(D1[:2 * m2].reshape(m2, 2), D0)
        np.testing.assert_array_equal(L1[:2 * m2].reshape(m2, 2), L0)
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
        kinds = [be.ctx._L.cfmm_segment_count(be.ctx._h)]
        assert kinds == [5]
        Dw = D1[2 * m2:2 * m2 + 3 * 25_000].reshape(-1, 3)
        np.testing.assert_allclose(Dw, wr.sweep(wts[0], v)[0], rtol=0, atol=1e-11 * coin_scale(wts[0]).max())
    finally:
        be0.close()
        be.close()


class HostWeighted(cr.CFMM):
    """The same pool through the host plugin seam: a CFMM subclass with its own find_arb_ (weighted_ref)."""

    kind = -1

    def __init__(self, R, w, γ, Ai):
        self.R, self.w, self.γ, self.Ai = np.array(R, float), np.array(w, float), float(γ), np.array(Ai)

    def find_arb_(self, Δ, Λ, v):
        D, L = wr.solve(self.R[None], self.w[None], [self.γ], np.asarray(v)[None])
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
        w = rng.uniform(0.2, 1.0, size=nc)
        g = [0.997, 1.0][k % 2]
        pools.append(cr.GeometricMean(R, w, g, Ai))
        host.append(HostWeighted(R, w, g, Ai))
    two = [cr.ProductTwoCoin([100.0, 120.0], 0.997, [1, 2]), cr.GeometricMeanTwoCoin([80.0, 50.0], [0.3, 0.7], 0.997, [2, 3])]
    obj = (lambda: cr.LinearNonnegative(np.linspace(0.5, 1.5, n))) if objective == "linear" else \
        (lambda: cr.BasketLiquidation(1, np.array([0.0, 5.0, 3.0, 0.0, 2.0, 1.0])))
    rd = cr.Router(obj(), two + pools, n)
    rh = cr.Router(obj(), two + host, n)
    try:
        cr.route_(rd, solver="native")   # cfmm_route: the whole route! in the library (pre-armed evaluations by default)
        cr.route_(rh)
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
    bs = [synth.weighted_pools(40_000, n, 3, seed=41), synth.weighted_pools(20_000, n, 5, seed=42)]
    v = synth.sweep_prices(n, seed=43, spread=0.5)
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), bs, n)
    try:
        cr.find_arb_(r, v)
        D = [d.copy() for d in r.Δs]
        L = [l.copy() for l in r.Λs]
        R0 = [b.R.copy() for b in bs]
        cr.update_reserves_(r)
        k = 0
        for b, R in zip(bs, R0):
            for i in range(0, len(b), 997):
                np.testing.assert_array_equal(b.R[i], (R[i] + b.γ[i] * D[k + i]) - L[k + i])
            k += len(b)
        cr.find_arb_(r, v)
        # scale: the reserves before the update -- R + γΔ − Λ rounds at THEIR ulp (a coin drained a thousandfold keeps ~1e-13 of
        # itself), and that rounding is all the second sweep can find
        for Dn, Ln, b, R in zip(np.split(np.concatenate(r.Δs), [3 * 40_000]), np.split(np.concatenate(r.Λs), [3 * 40_000]), bs, R0):
            s = np.repeat(R.max(axis=1, keepdims=True), b.n_coins, axis=1).ravel()
            assert np.max(Dn / s) <= 1e-12 and np.max(Ln / s) <= 1e-12
    finally:
        r.close()


def test_multi_device_parent_matches_single_context():
    n = 40
    bs = [synth.product_pools(10_001, n, seed=51), synth.weighted_pools(30_001, n, 4, seed=52),
          synth.weighted_pools(7_777, n, 3, seed=53)]
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
        w = np.ones((2, 3))
        g = np.full(2, 0.997)
        Ai = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
        with pytest.raises(cr.ArgumentError, match="coins"):
            ctx.add_weighted(np.ones((2, 1)), np.ones((2, 1)), g, np.zeros((2, 1), dtype=np.int32))
        with pytest.raises(cr.ArgumentError, match="coins"):
            ctx.add_weighted(np.ones((1, 9)), np.ones((1, 9)), g[:1], np.arange(9, dtype=np.int32)[None])
        with pytest.raises(cr.ArgumentError, match="distinct"):
            ctx.add_weighted(R, w, g, np.array([[0, 1, 2], [3, 4, 3]], dtype=np.int32))
        with pytest.raises(cr.ArgumentError, match="weights"):
            ctx.add_weighted(R, np.array([[1.0, 0.0, 1.0], [1, 1, 1]]), g, Ai)
        with pytest.raises(cr.ArgumentError, match="weights"):
            ctx.add_weighted(R, np.array([[1.0, 1.0, 1.0], [1, -1, 1]]), g, Ai)
        with pytest.raises(cr.ArgumentError, match="unbounded"):
            ctx.add_weighted(R, w, np.array([0.997, 1.001]), Ai)
        with pytest.raises(cr.ArgumentError, match="out of range"):
            ctx.add_weighted(R, w, g, np.array([[0, 1, 2], [3, 4, 10]], dtype=np.int32))
        assert ctx.pool_count == 0
        ctx.add_weighted(R, w, g, Ai)
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
            big.add_weighted(np.ones((1, 3)), np.ones((1, 3)), [1.0], np.array([[0, 1, 2]], dtype=np.int32))
    finally:
        big.close()


def test_find_arb_on_a_single_pool():
    p = cr.GeometricMean([100.0, 200.0, 50.0, 80.0], [0.1, 0.2, 0.3, 0.4], 0.997, [3, 1, 4, 2])
    v = np.array([1.0, 0.5, 3.0, 1.2])
    D, L = np.zeros(4), np.zeros(4)
    cr.find_arb_(D, L, p, v)
    Do, Lo = wr.solve(p.R[None], p.w[None], [p.γ], v[None])
    np.testing.assert_allclose(D, Do[0], rtol=0, atol=1e-11 * 200)
    np.testing.assert_allclose(L, Lo[0], rtol=0, atol=1e-11 * 200)
    assert wr.optimality_ok(v, D, L, p.R, p.w, p.γ)
