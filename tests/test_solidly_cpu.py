"""Solidly-style stable pairs, φ = x³y + xy³, on the host side: the closed form of tests/solidly_ref.py against its own
bisection solver and against the reference's optimality predicate (random, balanced and wide pools), constructors and
PoolBatch, the packing of a Router, chain intake, the synthetic market and the C header.  No GPU."""
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain, synth
from cfmmrouter_amd._lib import KIND_PRODUCT, KIND_SOLIDLY

import solidly_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _market(regime, m, seed):
    rng = np.random.default_rng(seed)
    R1 = 1000.0 * rng.random(m) + 1.0
    if regime == "balanced":
        t0, pv = np.where(rng.random(m) < 0.5, 1.0, 1.0 + 1e-9 * (2 * rng.random(m) - 1)), 1e-3
    elif regime == "wide":
        t0, pv = np.exp(3.0 * (2 * rng.random(m) - 1)), 5.0
    else:
        t0, pv = np.exp(0.05 * (2 * rng.random(m) - 1)), 0.5
    R = np.stack([R1, R1 * t0], axis=1)
    g = np.where(rng.random(m) < 0.5, 0.9995, 1.0)
    v = np.exp(pv * (2 * rng.random((m, 2)) - 1))
    return R, g, v


@pytest.mark.parametrize("regime", ["random", "balanced", "wide"])
def test_closed_form_matches_the_bisection_solver(regime):
    """The bisection stops on the sign of a marginal price, which near balance is flat (p′(1) = 0): its δ carries
    eps/p′ of the reserve, so the comparison is at 1e-11 of the larger reserve (random, balanced) and 1e-12 (wide)."""
    R, g, v = _market(regime, 4000, 7)
    D, L = sr.solve(R, g, v)
    Db, Lb = sr.solve_bisect(R, g, v)
    sc = R.max(axis=1, keepdims=True)
    tol = 1e-12 if regime == "wide" else 1e-11
    assert np.max(np.abs(D - Db) / sc) <= tol and np.max(np.abs(L - Lb) / sc) <= tol
    assert np.all(D >= 0) and np.all(L >= 0)
    assert np.all((D > 0).sum(axis=1) <= 1) and np.all((L > 0).sum(axis=1) <= 1)      # one direction at most
    assert np.count_nonzero(D) > len(g) // 2


@pytest.mark.parametrize("regime", ["random", "balanced", "wide"])
def test_closed_form_meets_the_optimality_predicate(regime):
    R, g, v = _market(regime, 600, 11)
    D, L = sr.solve(R, g, v)
    for i in range(len(g)):
        assert sr.optimality_ok(v[i], D[i], L[i], R[i], g[i]), i
    # ... and the predicate is not vacuous: half the optimal trade fails it
    i = int(np.argmax(D.max(axis=1) / R.max(axis=1)))
    assert not sr.optimality_ok(v[i], 0.5 * D[i], 0.5 * L[i], R[i], g[i])


def test_fee_band_gives_exact_zeros():
    R = np.array([[100.0, 100.0], [50.0, 50.5]])
    g = np.array([0.999, 0.99])
    v = np.array([[1.0, 1.0005], [1.0, 1.0]])
    D, L = sr.solve(R, g, v)
    assert not D.any() and not L.any() and not np.signbit(D).any() and not np.signbit(L).any()
    Db, Lb = sr.solve_bisect(R, g, v)
    assert not Db.any() and not Lb.any()


def test_invariant_and_price_at_the_optimum():
    R, g, v = _market("random", 2000, 3)
    D, L = sr.solve(R, g, v)
    Rn = R + g[:, None] * D - L
    phi = lambda X: X[:, 0] * X[:, 1] * (X[:, 0] ** 2 + X[:, 1] ** 2)
    np.testing.assert_allclose(phi(Rn), phi(R), rtol=1e-13)
    p = sr.marginal_price(Rn)
    d1, d2 = D[:, 0] > 0, D[:, 1] > 0
    np.testing.assert_allclose(g[d1] * p[d1], (v[:, 0] / v[:, 1])[d1], rtol=1e-9)    # direction 1: γ·p = v₁/v₂
    np.testing.assert_allclose(p[d2] / g[d2], (v[:, 0] / v[:, 1])[d2], rtol=1e-9)    # direction 2: p/γ = v₁/v₂


def test_constructor_phi_and_gradient():
    c = cr.SolidlyStableTwoCoin([2.0, 3.0], 0.9995, [4, 7])
    assert c.kind == KIND_SOLIDLY == 5 and len(c) == 2 and c.γ == 0.9995 and c.gamma == 0.9995
    assert cr.ϕ(c) == pytest.approx(8.0 * 3.0 + 2.0 * 27.0)
    assert cr.ϕ(c, R=[1.0, 1.0]) == pytest.approx(2.0)
    gr = np.zeros(2)
    cr.ϕ_grad_(gr, c)
    np.testing.assert_allclose(gr, [3.0 * 4.0 * 3.0 + 27.0, 8.0 + 3.0 * 2.0 * 9.0])
    assert "SolidlyStableTwoCoin" in cr.__all__
    # the single-pool find_arb_ path packs the pool with local indices
    from cfmmrouter_amd.cfmms import _with_local_idx
    loc = _with_local_idx(c)
    assert isinstance(loc, cr.SolidlyStableTwoCoin) and list(loc.Ai) == [1, 2] and np.array_equal(loc.R, c.R)


@pytest.mark.parametrize("args, msg", [
    (([1.0], 1.0, [1, 2]), "length of R must be 2"),
    (([1.0, 2.0], 1.0, [1]), "length of idx must be 2"),
    (([1.0, 2.0], 1.0, [-1, 2]), "non-negative"),
    (([1.0, 2.0], 1.01, [1, 2]), "unbounded"),
    (([1.0, 2.0], 0.0, [1, 2]), "γ"),
    (([1.0, 2.0 ** 152], 1.0, [1, 2]), "2\\^-150"),
    (([2.0 ** -151, 1.0], 1.0, [1, 2]), "2\\^-150"),
    (([1.0, -2.0], 1.0, [1, 2]), "2\\^-150"),
])
def test_constructor_validation(args, msg):
    with pytest.raises(cr.ArgumentError, match=msg):
        cr.SolidlyStableTwoCoin(*args)


def test_pool_batch():
    b = synth.solidly_pools(100, 20, seed=1)
    b2 = synth.solidly_pools(50, 20, seed=2)
    assert b.kind == KIND_SOLIDLY and b.R.shape == (100, 2) and b.Ai.shape == (100, 2) and b.γ.shape == (100,)
    assert np.all(b.Ai[:, 0] != b.Ai[:, 1]) and b.Ai.min() >= 1 and b.Ai.max() <= 20
    cat = cr.PoolBatch.concat([b, b2])
    assert len(cat) == 150 and cat.kind == KIND_SOLIDLY
    np.testing.assert_array_equal(cat.slice(100, 150).R, b2.R)
    p = cat[120]
    assert isinstance(p, cr.SolidlyStableTwoCoin) and np.array_equal(p.Ai, b2.Ai[20]) and p.γ == b2.γ[20]
    with pytest.raises(cr.ArgumentError, match="unbounded"):
        cr.SolidlyStableTwoCoin.batch([[1.0, 2.0]], [1.5], [[1, 2]])
    with pytest.raises(cr.ArgumentError, match="2\\^-150"):
        cr.SolidlyStableTwoCoin.batch([[1.0, 1e300]], [1.0], [[1, 2]])
    with pytest.raises(cr.ArgumentError, match="one pool family"):
        cr.PoolBatch.concat([b, synth.product_pools(10, 20)])


def test_synthetic_pools_are_a_pure_function_of_the_seed():
    a, b = synth.solidly_pools(1000, 64, seed=5), synth.solidly_pools(1000, 64, seed=5)
    np.testing.assert_array_equal(a.R, b.R)
    np.testing.assert_array_equal(a.Ai, b.Ai)
    np.testing.assert_array_equal(a.γ, b.γ)
    np.testing.assert_array_equal(synth.solidly_pools(100, 64, seed=5, first=900).R, a.R[900:])
    assert not np.array_equal(a.R, synth.solidly_pools(1000, 64, seed=6).R)
    t0 = a.R[:, 1] / a.R[:, 0]
    assert np.all(np.abs(np.log(t0)) <= 0.05 + 1e-12) and set(np.unique(a.γ)) == {0.9995, 1.0}
    w = synth.solidly_pools(1000, 64, seed=5, wide=True)
    lt = np.log(w.R[:, 1] / w.R[:, 0])
    assert np.all(np.abs(lt) <= 3.0 + 1e-12) and np.max(np.abs(lt)) > 2.5
    s = synth.solidly_pools(1000, 64, seed=5, spread=0.5)
    assert 0.4 < np.max(np.abs(np.log(s.R[:, 1] / s.R[:, 0]))) <= 0.5 + 1e-12


def test_segments_of_packs_solidly_pools_for_the_device():
    from cfmmrouter_amd.router import _segments_of
    pools = [cr.SolidlyStableTwoCoin([1.0, 2.0], 1.0, [1, 2]), cr.ProductTwoCoin([1.0, 2.0], 1.0, [1, 2]),
             cr.Product([1.0, 2.0, 3.0], 0.997, [1, 2, 3]), cr.SolidlyStableTwoCoin([3.0, 2.0], 0.9995, [3, 2])]
    batches, order, host = _segments_of(pools)
    assert host == []
    assert [(b.kind, len(b)) for b in batches] == [(KIND_PRODUCT, 1), (KIND_SOLIDLY, 2), (3, 1)]
    np.testing.assert_array_equal(order, [1, 0, 3, 2])


def test_chain_intake_of_solidly_stable_records():
    recs = [{"type": "solidly_stable", "tokens": ["DAI", "USDC"], "decimals": [18, 6],
             "reserves": [str(3 * 10**24), 2_900_000_000_000], "fee_bps": 5},
            {"type": "constant_product", "tokens": ["WETH", "USDC"], "decimals": [18, 6],
             "reserves": [str(10**21), 3 * 10**12], "fee_bps": 30},
            {"type": "solidly_stable", "tokens": ["USDC", "USDT"], "decimals": [6, 6], "reserves": [10**12, 10**12 + 7],
             "fee": 0.0}]
    tokens, batches = chain.load_snapshot(recs)
    assert tokens == ["DAI", "USDC", "WETH", "USDT"]
    assert [b.kind for b in batches] == [KIND_PRODUCT, KIND_SOLIDLY]
    s = batches[1]
    np.testing.assert_array_equal(s.R, [[3e6, 2.9e6], [1e6, 1000000.000007]])     # whole-token amounts
    np.testing.assert_array_equal(s.Ai, [[1, 2], [2, 4]])
    assert s.γ[0] == pytest.approx(0.9995) and s.γ[1] == 1.0
    assert isinstance(s[0], cr.SolidlyStableTwoCoin)
    with pytest.raises(cr.ArgumentError, match="two distinct"):
        chain.load_snapshot([{"type": "solidly_stable", "tokens": ["A", "A"], "reserves": [1, 1], "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="reserves must have two entries"):
        chain.load_snapshot([{"type": "solidly_stable", "tokens": ["A", "B"], "reserves": [1], "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="reserves must be > 0"):
        chain.load_snapshot([{"type": "solidly_stable", "tokens": ["A", "B"], "reserves": [0, 1], "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="exactly one of fee"):
        chain.load_snapshot([{"type": "solidly_stable", "tokens": ["A", "B"], "reserves": [1, 1]}])
    with pytest.raises(cr.ArgumentError, match="unknown pool type"):   # the record type is "solidly_stable"
        chain.load_snapshot([{"type": "stableswap", "tokens": ["A", "B"], "reserves": [1, 1], "fee_bps": 4}])


def test_header_and_lib_declare_the_solidly_entries():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert "#define CFMM_KIND_SOLIDLY 5" in h
    assert "int cfmm_pools_add_solidly(cfmm_ctx* ctx, int64_t m, const double* R, const double* gamma, const int32_t* Ai);" in h
    assert "phi(x, y) = x^3 y + x y^3" in h
    from cfmmrouter_amd import _lib
    assert _lib.KIND_SOLIDLY == 5 and cr.lib().cfmm_pools_add_solidly is not None
