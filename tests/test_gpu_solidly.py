"""Solidly-style stable pairs on the device (CFMM_KIND_SOLIDLY, sweep_kernel<SolidlyOps, ...>): a million pools against
the CPU closed form (tests/solidly_ref.py), Ψ / acc against math.fsum of the device's own trades, materialising vs fused
evaluation, the single-block direct path, large-market mode, a mixed market whose other rows stay bit-equal, the device
trade views, update_reserves!, a multi-device parent, route! against the host plugin seam, and the error paths."""
import math

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_SOLIDLY
from helpers import device_sweep, rel_to_max
from reduction_ref import assert_reduction_exact

import solidly_ref as sr
from solidly_dev import dev_sweep, read_trades_dev

pytestmark = pytest.mark.gpu


def _check_against_reference(b, v, D, L, psi, acc, n, sample=4001):
    m = len(b)
    D, L = np.reshape(D, (m, 2)), np.reshape(L, (m, 2))
    Do, Lo = sr.sweep(b, v)
    s = b.R.max(axis=1, keepdims=True)
    assert np.max(np.abs(D - Do) / s) <= 1e-11 and np.max(np.abs(L - Lo) / s) <= 1e-11
    assert np.all(D >= 0) and np.all(L >= 0)
    idle = ~np.any(Do > 0, axis=1)                       # inside the band: exact +0.0, no sign bit
    assert not D[idle].any() and not L[idle].any() and not np.signbit(D[idle]).any() and not np.signbit(L[idle]).any()
    assert not np.signbit(D).any() and not np.signbit(L).any()
    Ai0 = b.Ai - 1
    for i in range(0, m, sample):
        assert sr.optimality_ok(v[Ai0[i]], D[i], L[i], b.R[i], b.γ[i]), i
    flows = L - D
    psi_exact = np.array([math.fsum(flows[Ai0 == t]) for t in range(n)])
    assert rel_to_max(psi, psi_exact) <= 1e-12
    vl = v[Ai0]
    acc_exact = math.fsum(np.concatenate([(L * vl).ravel(), -(D * vl).ravel()]))
    assert abs(acc - acc_exact) <= 1e-12 * max(np.max(np.abs(psi_exact)), abs(acc_exact))
    assert_reduction_exact(D, L, Ai0, v, n, psi, acc)   # per token: exact for <= 1 flow, (c + 2)·u·Σ|t| otherwise
    return D, L


@pytest.mark.parametrize("prices", ["near", "spread"])
def test_million_pools_match_the_cpu_reference(prices):
    n, m = 256, 1_000_000
    b = synth.solidly_pools(m, n, seed=71)
    v = synth.sweep_prices(n, seed=72, spread=1e-3 if prices == "near" else 0.5)
    be = cr.DeviceBackend(n, [b])
    try:
        psi, acc = be.find_arb(v)
        D, L = be.trades()
        D, L = _check_against_reference(b, v, D, L, psi, acc, n)
        assert 0.3 < np.mean(np.any(D > 0, axis=1)) <= 1.0
        if prices == "near":
            assert np.count_nonzero(~np.any(D > 0, axis=1)) > 1000      # the band is populated
        # materialising and fused evaluations: identical Ψ bits; two runs: identical bits.  (Consecutive sweeps walk the
        # tiles in alternating directions, option "alternate": evaluations are compared at the same direction.)
        # A materialising host call always walks forwards, and the alternation restarts behind it.)
        p1, a1 = be.eval(v)          # fused, backwards
        p2, a2 = be.eval(v)          # fused, forwards: the materialising sweep above, without the trade stores
        p3, a3 = be.find_arb(v)      # materialising, forwards: the first run again
        D2, L2 = be.trades()
        np.testing.assert_array_equal(p2, psi)
        np.testing.assert_array_equal(p3, psi)
        assert a2 == acc and a3 == acc
        assert rel_to_max(p1, psi) <= 1e-13
        np.testing.assert_array_equal(np.reshape(D2, (m, 2)), D)
        np.testing.assert_array_equal(np.reshape(L2, (m, 2)), L)
        seg = be.ctx.segments()
        assert len(seg) == 1 and seg[0]["kind"] == KIND_SOLIDLY and seg[0]["m"] == m and seg[0]["block"] == 1024
    finally:
        be.close()


def test_wide_pools_match_the_cpu_reference():
    n, m = 64, 200_000
    b = synth.solidly_pools(m, n, seed=73, wide=True)
    v = synth.sweep_prices(n, seed=74, spread=2.0)
    D, L, psi, acc = device_sweep(n, [b], v)
    _check_against_reference(b, v, D, L, psi, acc, n, sample=997)


@pytest.mark.parametrize("m", [1, 63, 512, 2048])
def test_single_block_direct_path(m):
    n = 24
    b = synth.solidly_pools(m, n, seed=75 + m)
    v = synth.sweep_prices(n, seed=76, spread=0.3)
    be = cr.DeviceBackend(n, [b])
    try:
        psi, acc = be.find_arb(v)
        D, L = be.trades()
        assert be.ctx.segments()[0]["grid"] == 1
        _check_against_reference(b, v, D, L, psi, acc, n, sample=37)
        p2, a2 = be.eval(v)
        np.testing.assert_array_equal(p2, psi)
        assert a2 == acc
        pd, ad = dev_sweep(be, v)
        np.testing.assert_array_equal(pd, psi)
        assert ad == acc
    finally:
        be.close()


def test_large_market_mode_with_a_hub_token():
    n, m = 20_000, 300_000
    b = synth.solidly_pools(m, n, seed=77)
    b.Ai[::3, 0] = 1                                    # a hub: a third of the pools trade token 1
    b.Ai[::3, 1] = np.where(b.Ai[::3, 1] == 1, 2, b.Ai[::3, 1])
    v = synth.sweep_prices(n, seed=78, spread=0.5)
    be = cr.DeviceBackend(n, [b])
    try:
        psi, acc = be.find_arb(v)
        D, L = (np.reshape(x, (m, 2)) for x in be.trades())
        Do, Lo = sr.sweep(b, v)
        s = b.R.max(axis=1, keepdims=True)
        assert np.max(np.abs(D - Do) / s) <= 1e-11 and np.max(np.abs(L - Lo) / s) <= 1e-11
        flows = (L - D).ravel()
        psi_ref = np.bincount((b.Ai - 1).ravel(), weights=flows, minlength=n)
        t = flows.reshape(m, 2)[b.Ai == 1]
        assert len(t) >= m // 3
        assert_reduction_exact(D, L, b.Ai - 1, v, n, psi, acc, be.ctx.segments())   # the hub and every other token
        assert rel_to_max(psi, psi_ref) <= 1e-11
        p2, a2 = be.eval(v)
        assert rel_to_max(p2, psi) <= 1e-12 and abs(a2 - acc) <= 1e-12 * abs(acc)
    finally:
        be.close()


def _others(n):
    return [synth.product_pools(30_000, n, seed=31), synth.geomean_pools(20_000, n, seed=32),
            synth.univ3_pools(6_000, n, 6, seed=33), synth.weighted_pools(25_000, n, 3, seed=34)]


def test_mixed_market_other_rows_bit_equal():
    n = 48
    others = _others(n)
    sol = synth.solidly_pools(40_000, n, seed=35)
    v = synth.sweep_prices(n, seed=37, spread=0.5)
    two, wt = others[:3], others[3]
    m2 = sum(len(b) for b in two)
    be0 = cr.DeviceBackend(n, two + [wt])
    be = cr.DeviceBackend(n, two + [sol, wt])
    try:
        be0.find_arb(v)
        D0, L0 = (np.ravel(x) for x in be0.trades())
        psi1, acc1 = be.find_arb(v)
        D1, L1 = (np.ravel(x) for x in be.trades())
        ms = 2 * len(sol)
        assert be.ctx.trades_len == len(D0) + ms
        np.testing.assert_array_equal(D1[:2 * m2], D0[:2 * m2])          # the fused two-coin families
        np.testing.assert_array_equal(L1[:2 * m2], L0[:2 * m2])
        np.testing.assert_array_equal(D1[2 * m2 + ms:], D0[2 * m2:])     # the weighted segment
        np.testing.assert_array_equal(L1[2 * m2 + ms:], L0[2 * m2:])
        Ds, Ls = D1[2 * m2:2 * m2 + ms].reshape(-1, 2), L1[2 * m2:2 * m2 + ms].reshape(-1, 2)
        Do, Lo = sr.sweep(sol, v)
        s = sol.R.max(axis=1, keepdims=True)
        assert np.max(np.abs(Ds - Do) / s) <= 1e-11 and np.max(np.abs(Ls - Lo) / s) <= 1e-11
        kinds = [sg["kind"] for sg in be.ctx.segments()]
        assert kinds == [0, 1, 2, KIND_SOLIDLY, 3]
        be.eval(v * 1.1)                                                  # another evaluation in between
        psi2, acc2 = be.find_arb(v)
        np.testing.assert_array_equal(psi1, psi2)
        assert acc1 == acc2
        Dr, Lr = be.ctx.trades_range(3, 100, 5_000)
        np.testing.assert_array_equal(np.reshape(Dr, (-1, 2)), Ds[100:5_100])
        np.testing.assert_array_equal(np.reshape(Lr, (-1, 2)), Ls[100:5_100])
    finally:
        be0.close()
        be.close()


def test_trades_dev_on_a_two_coin_market():
    n = 32
    bp, sol = synth.product_pools(20_000, n, seed=41), synth.solidly_pools(30_000, n, seed=42)
    v = synth.sweep_prices(n, seed=43, spread=0.4)
    be = cr.DeviceBackend(n, [bp, sol])
    try:
        be.find_arb(v)
        D, L = be.trades()
        hD, hL = read_trades_dev(be, 50_000)
        np.testing.assert_array_equal(hD, np.reshape(D, (-1, 2)))
        np.testing.assert_array_equal(hL, np.reshape(L, (-1, 2)))
        assert np.count_nonzero(hD[20_000:]) > 10_000
    finally:
        be.close()


def test_update_reserves_then_a_second_sweep_matches_a_fresh_upload():
    n, m = 40, 100_000
    sol = synth.solidly_pools(m, n, seed=44)
    v, v2 = synth.sweep_prices(n, seed=45, spread=0.5), synth.sweep_prices(n, seed=46, spread=0.5)
    be = cr.DeviceBackend(n, [sol])
    try:
        be.find_arb(v)
        D, L = (np.reshape(x, (m, 2)) for x in be.trades())
        be.ctx.update_reserves()
        Rr = be.ctx.reserves(0, m)
        np.testing.assert_array_equal(Rr, (sol.R + sol.γ[:, None] * D) - L)
        pa, aa = be.find_arb(v)                       # at the same prices: nothing but the rounding of R + γΔ − Λ is left
        Dn, Ln = (np.reshape(x, (m, 2)) for x in be.trades())
        s = sol.R.max(axis=1, keepdims=True)
        # (near balance the curve is flat: an ulp of the reserves moves the optimum by ~u/p′(t) of the pool)
        assert np.max(Dn / s) <= 1e-9 and np.max(Ln / s) <= 1e-9 and np.median(np.concatenate([Dn / s, Ln / s])) <= 1e-13
        pb, ab = be.find_arb(v2)
        DA, LA = be.trades()
    finally:
        be.close()
    fresh = cr.DeviceBackend(n, [cr.SolidlyStableTwoCoin.batch(Rr, sol.γ, sol.Ai)])
    try:
        pf, af = fresh.find_arb(v2)
        DB, LB = fresh.trades()
    finally:
        fresh.close()
    np.testing.assert_array_equal(DA, DB)
    np.testing.assert_array_equal(LA, LB)
    assert rel_to_max(pb, pf) <= 1e-12 and abs(ab - af) <= 1e-12 * abs(af)    # (the two sweeps walk the tiles in opposite directions)


def test_multi_device_parent_with_two_shards():
    n = 40
    bs = [synth.product_pools(10_001, n, seed=51), synth.solidly_pools(30_001, n, seed=52)]
    v = synth.sweep_prices(n, seed=54, spread=0.5)
    D1, L1, psi1, acc1 = device_sweep(n, bs, v)
    D2, L2, psi2, acc2 = device_sweep(n, bs, v, device=[0, 0])
    np.testing.assert_array_equal(D1, D2)
    np.testing.assert_array_equal(L1, L2)
    assert rel_to_max(psi2, psi1) <= 1e-12 and abs(acc2 - acc1) <= 1e-12 * abs(acc1)
    be = cr.DeviceBackend(n, bs, device=[0, 0])
    try:
        be.find_arb(v)
        assert [s["kind"] for s in be.ctx.segments()] == [0, KIND_SOLIDLY]
        Dr, Lr = be.ctx.trades_range(1, 1000, 20_000)
        np.testing.assert_array_equal(np.ravel(Dr), D1[2 * 10_001 + 2 * 1000:2 * 10_001 + 2 * 21_000])
        be.ctx.update_reserves()
        np.testing.assert_array_equal(be.ctx.reserves(1, 30_001), (bs[1].R + bs[1].γ[:, None] * D1[2 * 10_001:].reshape(-1, 2))
                                      - L1[2 * 10_001:].reshape(-1, 2))
    finally:
        be.close()


class HostSolidly(cr.CFMM):
    """The same pool through the host plugin seam: a CFMM subclass with its own find_arb_ (solidly_ref.solve)."""

    kind = -1

    def __init__(self, R, γ, Ai):
        self.R, self.γ, self.Ai = np.array(R, float), float(γ), np.array(Ai)

    def find_arb_(self, Δ, Λ, v):
        D, L = sr.solve(self.R[None], [self.γ], np.asarray(v, dtype=np.float64)[None])
        Δ[:] = D[0]
        Λ[:] = L[0]


def _check_feasible(r, pools, arb, TOL=1e-3):
    """test/arb.jl:5-28 with this family's φ."""
    flows = np.zeros_like(r.v)
    for Δ, Λ, c in zip(r.Δs, r.Λs, pools):
        assert np.all(Δ >= -TOL) and np.all(Λ >= -TOL)
        Rn = c.R + c.γ * Δ - Λ
        assert cr.ϕ(c, R=Rn) >= cr.ϕ(c) * (1.0 - math.sqrt(np.finfo(float).eps))
        flows[c.Ai - 1] += Λ - Δ
    assert np.max(np.abs(flows - cr.netflows(r))) <= 1e-12 * max(1.0, np.max(np.abs(flows)))
    if arb:
        assert np.all(flows >= -TOL)
    else:
        assert np.sum(flows >= -TOL) >= len(flows) - 1
    assert np.all(r.v >= cr.lower_limit(r.objective) - 1e-4) and np.all(r.v <= cr.upper_limit(r.objective) + 1e-4)


@pytest.mark.parametrize("objective", ["linear", "swap"])
def test_route_matches_the_host_plugin_seam(objective):
    """The product pools are the deep ones and set prices 20-60 % apart, so the stable pairs end well off balance.  (A
    market whose stable pairs end NEAR balance sits on the flat part of the curve, p′(1) = 0: there Ψ moves by ~1e-6 of its
    size for the 1e-16 of the dual value at which either L-BFGS-B stops, and two solvers agree to 1e-5, not 1e-6 -- the
    same effect as the stiff Curve pools of DESIGN §3.0b.)"""
    n = 6
    rng = np.random.default_rng(5)
    dev, host = [], []
    for k in range(12):
        Ai = rng.choice(n, size=2, replace=False) + 1
        R1 = rng.uniform(5.0, 15.0)
        R = [R1, R1 * math.exp(rng.uniform(-1.0, 1.0))]
        g = [0.9995, 1.0][k % 2]
        dev.append(cr.SolidlyStableTwoCoin(R, g, Ai))
        host.append(HostSolidly(R, g, Ai))
    prod = [cr.ProductTwoCoin([1000.0, 1300.0], 0.997, [1, 2]), cr.ProductTwoCoin([800.0, 500.0], 0.997, [2, 3]),
            cr.ProductTwoCoin([600.0, 900.0], 0.997, [4, 6]), cr.ProductTwoCoin([700.0, 950.0], 1.0, [5, 1]),
            cr.ProductTwoCoin([400.0, 650.0], 0.997, [3, 4])]
    obj = (lambda: cr.LinearNonnegative(np.linspace(0.5, 1.5, n))) if objective == "linear" else (lambda: cr.Swap(1, 3, 5.0, n))
    rd = cr.Router(obj(), prod + dev, n)
    rh = cr.Router(obj(), prod + host, n)
    try:
        cr.route_(rd, solver="native", pgtol=1e-8)   # cfmm_route: the whole route! in the library
        cr.route_(rh, pgtol=1e-8)
        psi_d, psi_h = cr.netflows(rd), cr.netflows(rh)
        scale = np.max(np.abs(psi_h))
        assert np.max(np.abs(psi_d - psi_h)) <= 1e-6 * scale
        _check_feasible(rd, prod + dev, arb=objective == "linear")
        assert rd.Δs.shape == (17, 2)
        assert np.count_nonzero(np.asarray(rd.Δs)[5:]) >= 6          # the stable pairs take part in the route
    finally:
        rd.close()
        rh.close()


def test_errors():
    ctx = cr.Context(10, 0)
    try:
        R = np.array([[1.0, 1.1], [2.0, 2.1]])
        g = np.array([0.9995, 1.0])
        Ai = np.array([[0, 1], [3, 4]], dtype=np.int32)
        with pytest.raises(cr.ArgumentError, match="unbounded"):
            ctx.add_solidly(R, np.array([0.9995, 1.0001]), Ai)
        with pytest.raises(cr.ArgumentError, match="gamma"):
            ctx.add_solidly(R, np.array([0.9995, 0.0]), Ai)
        with pytest.raises(cr.ArgumentError, match=r"\[2\^-150, 2\^150\]"):
            ctx.add_solidly(np.array([[1.0, 2.0 ** 151], [2.0, 2.1]]), g, Ai)
        with pytest.raises(cr.ArgumentError, match=r"\[2\^-150, 2\^150\]"):
            ctx.add_solidly(np.array([[1.0, 1.0], [2.0 ** -151, 2.1]]), g, Ai)
        with pytest.raises(cr.ArgumentError, match="reserves"):
            ctx.add_solidly(np.array([[1.0, 0.0], [2.0, 2.1]]), g, Ai)
        with pytest.raises(cr.ArgumentError, match="differ"):
            ctx.add_solidly(R, g, np.array([[0, 1], [3, 3]], dtype=np.int32))
        with pytest.raises(cr.ArgumentError, match="out of range"):
            ctx.add_solidly(R, g, np.array([[0, 1], [3, 10]], dtype=np.int32))
        with pytest.raises(cr.ArgumentError, match="shape"):
            ctx.add_solidly(R, g, np.array([[0, 1]], dtype=np.int32))
        assert ctx.pool_count == 0
        ctx.add_solidly(np.array([[2.0 ** -150, 2.0 ** 150], [2.0, 2.1]]), g, Ai)      # the ends of the range are inside it
        assert ctx.pool_count == 2
        psi, acc = ctx.eval(np.linspace(1.0, 2.0, 10))
        assert np.all(np.isfinite(psi)) and np.isfinite(acc)
    finally:
        ctx.close()


def test_find_arb_on_a_single_pool():
    p = cr.SolidlyStableTwoCoin([1.0e6, 1.02e6], 0.9995, [7, 3])
    v = np.array([1.0, 1.004])
    D, L = np.zeros(2), np.zeros(2)
    cr.find_arb_(D, L, p, v)
    Do, Lo = sr.solve(p.R[None], [p.γ], v[None])
    np.testing.assert_allclose(D, Do[0], rtol=0, atol=1e-11 * 1.02e6)
    np.testing.assert_allclose(L, Lo[0], rtol=0, atol=1e-11 * 1.02e6)
    assert D[0] > 0 and L[1] > 0 and D[1] == 0 and L[0] == 0
    assert sr.optimality_ok(v, D, L, p.R, p.γ)
