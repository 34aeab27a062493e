"""Curve (StableSwap) pools, φ = α·ΣR − β·ΠR⁻¹ (Curve{T}, src/cfmms.jl:66-70), on the host side: the CPU reference solvers
(tests/curve_ref.py) against the oracle's ProductTwoCoin closed forms and the equal-weight weighted solver at α = 0, against
each other and the KKT predicate on random and stiff pools, the StableSwap mapping, constructors and PoolBatch, chain
intake and the C header.  No GPU."""
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain, synth
from cfmmrouter_amd._lib import KIND_CURVE, KIND_PRODUCT
from oracle import cfmm_oracle as orc

import curve_ref as cv
import weighted_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alpha_zero_two_coin_matches_product_closed_form():
    rng = np.random.default_rng(1)
    m = 5000
    R = rng.uniform(0.5, 1e3, size=(m, 2))
    g = rng.choice([0.997, 0.99, 1.0], size=m)
    v = rng.uniform(0.2, 5.0, size=(m, 2))
    beta = rng.uniform(0.1, 1e6, size=m)   # any β: at α = 0 the level sets are those of R₁R₂
    D, L = cv.solve(R, np.zeros(m), beta, g, v)
    Ai = np.array([[0, 1]], dtype=np.int32)
    for i in range(0, m, 97):
        Do, Lo = orc.sweep_product(R[i:i + 1], g[i:i + 1], Ai, v[i])
        s = R[i].max()
        assert np.max(np.abs(D[i] - Do[0])) <= 1e-12 * s and np.max(np.abs(L[i] - Lo[0])) <= 1e-12 * s, i


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8])
def test_alpha_zero_matches_equal_weight_weighted_solver(n):
    rng = np.random.default_rng(20 + n)
    m = 3000
    R = rng.uniform(1.0, 1e3, size=(m, n))
    g = rng.choice([0.997, 1.0], size=m)
    v = rng.uniform(0.5, 2.0, size=(m, n))
    D, L = cv.solve(R, np.zeros(m), np.full(m, 7.0), g, v)
    Dw, Lw = wr.solve(R, np.full((m, n), 1.0 / n), g, v)
    s = R.max(axis=1, keepdims=True)
    assert np.max(np.abs(D - Dw) / s) <= 1e-12 and np.max(np.abs(L - Lw) / s) <= 1e-12


def _pools(n, m, regime, seed):
    b = synth.curve_pools(m, 2 * n, n, seed=seed, regime=regime)
    rng = np.random.default_rng(seed)
    spread = 1e-3 if regime == "stableswap" else 0.5
    v = np.exp(spread * rng.standard_normal(size=(m, n)))
    return b, v


@pytest.mark.parametrize("n", [2, 3, 4, 8])
@pytest.mark.parametrize("regime", ["stableswap", "small_a", "alpha0"])
def test_bulk_solver_matches_decimal_solver(n, regime):
    """The float64 solver against the 40-digit naive (ν, P) solver: ~1e-14 of the largest reserve, stiff pools included."""
    b, v = _pools(n, 4, regime, seed=100 + n)
    D, L = cv.solve(b.R, b.α, b.β, b.γ, v)
    for i in range(len(b)):
        Dd, Ld = cv.solve_decimal(b.R[i], b.α[i], b.β[i], b.γ[i], v[i])
        s = b.R[i].max()
        assert np.max(np.abs(D[i] - Dd)) <= 1e-12 * s and np.max(np.abs(L[i] - Ld)) <= 1e-12 * s, i


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("regime", ["stableswap", "small_a", "alpha0", "mixed"])
def test_solver_meets_the_kkt_conditions(n, regime):
    b, v = _pools(n, 400, regime, seed=200 + n)
    D, L = cv.solve(b.R, b.α, b.β, b.γ, v)
    for i in range(len(b)):
        assert cv.optimality_ok(v[i], D[i], L[i], b.R[i], b.α[i], b.β[i], b.γ[i]), i
    assert np.mean(np.any(L > 0, axis=1)) > 0.5   # most pools trade at these prices
    # the predicate rejects a trade that is not optimal
    i = int(np.argmax(np.any(L > 0, axis=1)))
    assert not cv.optimality_ok(v[i], 0.5 * D[i], 0.5 * L[i], b.R[i], b.α[i], b.β[i], b.γ[i])


def test_fee_band_gives_no_trade():
    n = 3
    R = np.array([[1e6, 1e6, 1e6]])
    al, be = chain.stableswap_params(R, [100.0])
    v = np.array([[1.0, 1.0 + 1e-5, 1.0 - 1e-5]])   # ∇φ ∝ 1 at a balanced pool: inside the band of a 0.04 % fee
    D, L = cv.solve(R, al, be, [0.9996], v)
    assert np.all(D == 0) and np.all(L == 0)
    Dd, Ld = cv.solve_decimal(R[0], al[0], be[0], 0.9996, v[0])
    assert np.all(Dd == 0) and np.all(Ld == 0)


@pytest.mark.parametrize("n", [2, 3, 8])
def test_stableswap_mapping(n):
    rng = np.random.default_rng(n)
    x = rng.uniform(0.5e6, 1.5e6, size=(50, n))
    A = 10.0 ** rng.uniform(0, 3.7, size=50)
    D = chain.stableswap_D(x, A)
    Ann = A * n ** n
    # D satisfies the invariant A·nⁿ·Σx + D = A·D·nⁿ + D^{n+1}/(nⁿ·Πx)
    lhs = Ann * x.sum(axis=1) + D
    rhs = Ann * D + D ** (n + 1) / (n ** n * np.prod(x, axis=1))
    np.testing.assert_allclose(lhs, rhs, rtol=1e-13)
    al, be = chain.stableswap_params(x, A)
    np.testing.assert_array_equal(al, Ann)
    phi = al * x.sum(axis=1) - be / np.prod(x, axis=1)
    np.testing.assert_allclose(phi, Ann * D - D, rtol=1e-12)
    # a balanced pool: D = Σx
    np.testing.assert_allclose(chain.stableswap_D(np.full((1, n), 3.0), [50.0]), [3.0 * n], rtol=1e-15)


def test_curve_constructor_phi_and_gradient():
    c = cr.Curve([1.0, 2.0, 4.0], 0.997, [1, 2, 3], 3.0, 16.0)
    assert c.kind == KIND_CURVE and len(c) == 3 and c.α == 3.0 and c.β == 16.0 and c.γ == 0.997
    assert cr.ϕ(c) == pytest.approx(3.0 * 7.0 - 16.0 / 8.0)
    gr = np.zeros(3)
    cr.ϕ_grad_(gr, c)
    np.testing.assert_allclose(gr, 3.0 + 2.0 / np.array([1.0, 2.0, 4.0]))
    assert "Curve" in cr.__all__


@pytest.mark.parametrize("args, msg", [
    (([1.0], 1.0, [1], 1.0, 1.0), "coins"),
    ((np.ones(9), 1.0, np.arange(1, 10), 1.0, 1.0), "coins"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2, 2], 1.0, 1.0), "distinct"),
    (([1.0, 2.0, 3.0], 1.01, [1, 2, 3], 1.0, 1.0), "unbounded"),
    (([1.0, 2.0, 3.0], 0.0, [1, 2, 3], 1.0, 1.0), "γ"),
    (([1.0, -2.0, 3.0], 1.0, [1, 2, 3], 1.0, 1.0), "reserves"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2], 1.0, 1.0), "length of Ai"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2, 3], -1.0, 1.0), "α"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2, 3], np.inf, 1.0), "α"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2, 3], 1.0, 0.0), "β"),
    (([1.0, 2.0, 3.0], 1.0, [1, 2, 3], 1.0, np.nan), "β"),
])
def test_constructor_validation(args, msg):
    with pytest.raises(cr.ArgumentError, match=msg):
        cr.Curve(*args)


def test_pool_batch_groups_by_coin_count():
    b3 = synth.curve_pools(100, 20, 3, seed=1)
    b3b = synth.curve_pools(50, 20, 3, seed=2)
    b4 = synth.curve_pools(10, 20, 4, seed=3)
    assert b3.kind == KIND_CURVE and b3.n_coins == 3 and b3.R.shape == (100, 3) and b3.α.shape == (100,)
    assert np.all(np.sort(b3.Ai, axis=1)[:, 1:] != np.sort(b3.Ai, axis=1)[:, :-1])
    assert b3.Ai.min() >= 1 and b3.Ai.max() <= 20
    assert np.any(b3.α == 0) and np.any(b3.α > 1000 * 27) and np.all(b3.β > 0)
    cat = cr.PoolBatch.concat([b3, b3b])
    assert len(cat) == 150 and cat.n_coins == 3
    np.testing.assert_array_equal(cat.slice(100, 150).β, b3b.β)
    p = cat[120]
    assert isinstance(p, cr.Curve) and np.array_equal(p.Ai, b3b.Ai[20]) and p.α == b3b.α[20]
    with pytest.raises(cr.ArgumentError, match="coin count"):
        cr.PoolBatch.concat([b3, b4])
    with pytest.raises(cr.ArgumentError, match="coin count"):
        cr.PoolBatch.from_pools(KIND_CURVE, [b3[0], b4[0]])
    with pytest.raises(cr.ArgumentError, match="distinct"):
        cr.Curve.batch([[1.0, 2.0, 3.0]], [1.0], [[1, 1, 2]], [1.0], [1.0])
    with pytest.raises(cr.ArgumentError, match="unbounded"):
        cr.Curve.batch([[1.0, 2.0, 3.0]], [1.5], [[1, 2, 3]], [1.0], [1.0])
    with pytest.raises(cr.ArgumentError, match="β"):
        cr.Curve.batch([[1.0, 2.0, 3.0]], [1.0], [[1, 2, 3]], [1.0], [-1.0])
    with pytest.raises(cr.ArgumentError, match="shape"):
        cr.Curve.batch([[1.0, 2.0, 3.0]], [1.0], [[1, 2, 3]], [1.0, 2.0], [1.0])
    np.testing.assert_array_equal(synth.curve_pools(100, 20, 3, seed=1).β, b3.β)   # a pure function of its seed


def test_segments_of_packs_curve_pools_for_the_device():
    from cfmmrouter_amd.router import _segments_of
    pools = [cr.ProductTwoCoin([1.0, 2.0], 1.0, [1, 2]), cr.Curve([1.0, 2.0, 3.0], 0.997, [1, 2, 3], 1.0, 2.0),
             cr.Product([1.0, 2.0, 3.0], 0.997, [1, 2, 3]), cr.Curve([1.0, 2.0], 1.0, [2, 1], 0.0, 2.0),
             cr.Curve([5.0, 6.0, 7.0], 1.0, [3, 1, 2], 5.0, 9.0)]
    batches, order, host = _segments_of(pools)
    assert host == []
    assert [(b.kind, b.Ai.shape[1], len(b)) for b in batches] == [(KIND_PRODUCT, 2, 1), (3, 3, 1), (KIND_CURVE, 2, 1),
                                                                  (KIND_CURVE, 3, 2)]
    np.testing.assert_array_equal(order, [0, 2, 3, 1, 4])


def test_chain_intake_of_curve_records():
    recs = [{"type": "curve", "tokens": ["DAI", "USDC"], "decimals": [18, 6],
             "balances": [str(3 * 10**24), 2_900_000_000_000], "A": 400, "fee": 0.0004},
            {"type": "curve", "tokens": ["DAI", "USDC", "USDT"], "decimals": [18, 6, 6],
             "balances": [str(10**24), 10**12, 2 * 10**12], "A": 2000, "fee_bps": 1},
            {"type": "curve", "tokens": list("ABCDEFGH"), "balances": [10**24] * 8, "A": 100, "fee": 0.0},
            {"type": "curve", "tokens": ["USDC", "USDT"], "decimals": [6, 6], "balances": [10**12, 10**12], "A": 0,
             "fee": 0.0}]
    tokens, batches = chain.load_snapshot(recs)
    assert tokens == ["DAI", "USDC", "USDT", "A", "B", "C", "D", "E", "F", "G", "H"]
    b2, b3, b8 = batches
    assert [b.kind for b in batches] == [KIND_CURVE] * 3
    assert len(b2) == 2 and b3.n_coins == 3 and b8.n_coins == 8
    np.testing.assert_allclose(b2.R[0], [3e6, 2.9e6])
    np.testing.assert_array_equal(b2.Ai, [[1, 2], [2, 3]])
    np.testing.assert_allclose(b2.α, [400 * 4, 0.0])
    D = chain.stableswap_D(b2.R[:1], [400.0])[0]
    np.testing.assert_allclose(b2.β[0], D ** 3 / 4, rtol=1e-15)
    assert b2.γ[0] == pytest.approx(0.9996) and b3.γ[0] == pytest.approx(0.9999) and b8.γ[0] == 1.0
    np.testing.assert_allclose(b8.R, np.full((1, 8), 1e6))
    np.testing.assert_allclose(b8.β, (8e6) ** 9 / 8 ** 8, rtol=1e-13)   # balanced: D = Σx
    phi = b3.α * b3.R.sum(axis=1) - b3.β / np.prod(b3.R, axis=1)
    D3 = chain.stableswap_D(b3.R, [2000.0])
    np.testing.assert_allclose(phi, 2000 * 27 * D3 - D3, rtol=1e-12)
    with pytest.raises(cr.ArgumentError, match="distinct"):
        chain.load_snapshot([{"type": "curve", "tokens": ["A", "A"], "balances": [1, 1], "A": 10, "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="2..8"):
        chain.load_snapshot([{"type": "curve", "tokens": list("ABCDEFGHI"), "balances": [1] * 9, "A": 10, "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="amplification"):
        chain.load_snapshot([{"type": "curve", "tokens": ["A", "B"], "balances": [1, 1], "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="balances"):
        chain.load_snapshot([{"type": "curve", "tokens": ["A", "B"], "balances": [1], "A": 1, "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="unknown pool type"):   # the record type is "curve"
        chain.load_snapshot([{"type": "stableswap", "tokens": ["A", "B"], "reserves": [1, 1], "fee_bps": 4}])


def test_header_and_lib_declare_the_curve_entries():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert "#define CFMM_KIND_CURVE 4" in h
    assert ("int cfmm_pools_add_curve(cfmm_ctx* ctx, int64_t m, int32_t n_coins, const double* R, const double* gamma,"
            in h)
    assert "alpha = A n^n and beta = D^(n+1) / n^n" in h
    from cfmmrouter_amd import _lib
    assert _lib.KIND_CURVE == 4 and cr.lib().cfmm_pools_add_curve is not None
