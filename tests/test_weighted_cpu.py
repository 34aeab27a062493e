"""N-coin weighted geometric-mean pools (GeometricMean / Product, src/cfmms.jl:57-64) on the host side: the CPU
reference solver (tests/weighted_ref.py) against the oracle's two-coin closed forms and the reference's optimality
predicate, the constructors and PoolBatch, chain intake, and the C header.  No GPU."""
import os

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import chain, synth
from cfmmrouter_amd._lib import KIND_GEOMEAN, KIND_WEIGHTED
from oracle import cfmm_oracle as orc

import weighted_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _two_coin_market(m, seed):
    rng = np.random.default_rng(seed)
    R = rng.uniform(0.5, 1e3, size=(m, 2))
    g = rng.choice([0.997, 0.99, 1.0], size=m)
    v = rng.uniform(0.2, 5.0, size=(m, 2))
    return R, g, v


def test_reference_solver_matches_product_two_coin():
    m = 20_000
    R, g, v = _two_coin_market(m, 1)
    Ai = np.tile(np.array([[0, 1]], dtype=np.int32), (m, 1))
    D, L = wr.solve(R, np.full((m, 2), 0.5), g, v)
    for i in range(0, m, 997):   # the oracle's closed forms, pool by pool (local prices)
        Do, Lo = orc.sweep_product(R[i:i + 1], g[i:i + 1], Ai[:1], v[i])
        scale = R[i].max()
        assert np.max(np.abs(D[i] - Do[0])) <= 1e-12 * scale and np.max(np.abs(L[i] - Lo[0])) <= 1e-12 * scale


def test_reference_solver_matches_geomean_two_coin():
    m = 20_000
    R, g, v = _two_coin_market(m, 2)
    rng = np.random.default_rng(3)
    w1 = rng.uniform(0.05, 0.95, size=m)
    w = np.stack([w1, 1.0 - w1], axis=1)
    Ai = np.array([[0, 1]], dtype=np.int32)
    D, L = wr.solve(R, w, g, v)
    for i in range(0, m, 997):
        Do, Lo = orc.sweep_geomean(R[i:i + 1], w[i:i + 1], g[i:i + 1], Ai, v[i])
        scale = R[i].max()
        assert np.max(np.abs(D[i] - Do[0])) <= 1e-12 * scale and np.max(np.abs(L[i] - Lo[0])) <= 1e-12 * scale


@pytest.mark.parametrize("n", [3, 4, 8])
def test_reference_solver_meets_optimality_conditions(n):
    rng = np.random.default_rng(10 + n)
    m = 300
    R = rng.uniform(1.0, 100.0, size=(m, n))
    w = rng.uniform(0.05, 1.0, size=(m, n))
    g = rng.choice([0.997, 0.99, 1.0], size=m)
    v = rng.uniform(0.5, 2.0, size=(m, n))
    D, L = wr.solve(R, w, g, v)
    traded = 0
    for i in range(m):
        assert wr.optimality_ok(v[i], D[i], L[i], R[i], w[i], g[i]), i
        traded += bool(np.any(D[i] > 0))
    assert traded > m // 2   # the prices are spread enough that most pools trade


def test_product_is_equal_weight_geometric_mean():
    p = cr.Product([1.0, 2.0, 3.0], 0.997, [1, 2, 3])
    np.testing.assert_array_equal(p.w, np.full(3, 1.0 / 3.0))
    assert p.kind == KIND_WEIGHTED and len(p) == 3
    assert cr.ϕ(p) == 6.0
    gr = np.zeros(3)
    cr.ϕ_grad_(gr, p)
    np.testing.assert_allclose(gr, [6.0, 3.0, 2.0])
    q = cr.GeometricMean([1.0, 4.0], [0.5, 0.5], 1.0, [2, 1])
    assert cr.ϕ(q) == pytest.approx(2.0)
    cr.ϕ_grad_(gr[:2], q)
    np.testing.assert_allclose(gr[:2], [1.0, 0.25])


@pytest.mark.parametrize("args, msg", [
    (([1.0], [1.0], 1.0, [1]), "coins"),
    ((np.ones(9), np.ones(9), 1.0, np.arange(1, 10)), "coins"),
    (([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], 1.0, [1, 2, 2]), "distinct"),
    (([1.0, 2.0, 3.0], [1.0, 0.0, 1.0], 1.0, [1, 2, 3]), "weights"),
    (([1.0, 2.0, 3.0], [1.0, -1.0, 1.0], 1.0, [1, 2, 3]), "weights"),
    (([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], 1.01, [1, 2, 3]), "unbounded"),
    (([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], 0.0, [1, 2, 3]), "γ"),
    (([1.0, -2.0, 3.0], [1.0, 1.0, 1.0], 1.0, [1, 2, 3]), "reserves"),
    (([1.0, 2.0, 3.0], [1.0, 1.0], 1.0, [1, 2, 3]), "length of w"),
    (([1.0, 2.0, 3.0], [1.0, 1.0, 1.0], 1.0, [1, 2]), "length of Ai"),
])
def test_constructor_validation(args, msg):
    with pytest.raises(cr.ArgumentError, match=msg):
        cr.GeometricMean(*args)


def test_pool_batch_groups_by_coin_count():
    b3 = synth.weighted_pools(100, 20, 3, seed=1)
    b3b = synth.weighted_pools(50, 20, 3, seed=2)
    b4 = synth.weighted_pools(10, 20, 4, seed=3)
    assert b3.kind == KIND_WEIGHTED and b3.n_coins == 3 and b3.R.shape == (100, 3)
    np.testing.assert_allclose(b3.w.sum(axis=1), 1.0)
    assert np.all(np.sort(b3.Ai, axis=1)[:, 1:] != np.sort(b3.Ai, axis=1)[:, :-1])
    assert b3.Ai.min() >= 1 and b3.Ai.max() <= 20
    cat = cr.PoolBatch.concat([b3, b3b])
    assert len(cat) == 150 and cat.n_coins == 3
    np.testing.assert_array_equal(cat.slice(100, 150).R, b3b.R)
    p = cat[120]
    assert isinstance(p, cr.GeometricMean) and np.array_equal(p.Ai, b3b.Ai[20])
    with pytest.raises(cr.ArgumentError, match="coin count"):
        cr.PoolBatch.concat([b3, b4])
    with pytest.raises(cr.ArgumentError, match="coin count"):
        cr.PoolBatch.from_pools(KIND_WEIGHTED, [b3[0], b4[0]])
    with pytest.raises(cr.ArgumentError, match="distinct"):
        cr.GeometricMean.batch([[1.0, 2.0, 3.0]], [[1.0, 1.0, 1.0]], [1.0], [[1, 1, 2]])
    with pytest.raises(cr.ArgumentError, match="unbounded"):
        cr.GeometricMean.batch([[1.0, 2.0, 3.0]], [[1.0, 1.0, 1.0]], [1.5], [[1, 2, 3]])
    with pytest.raises(cr.ArgumentError, match="shape"):
        cr.GeometricMean.batch([[1.0, 2.0, 3.0]], [[1.0, 1.0]], [1.0], [[1, 2, 3]])
    pb = cr.Product.batch([[1.0, 2.0, 3.0, 4.0]], [0.997], [[4, 3, 2, 1]])
    np.testing.assert_array_equal(pb.w, np.full((1, 4), 0.25))
    # a synthetic market is a pure function of its seed
    np.testing.assert_array_equal(synth.weighted_pools(100, 20, 3, seed=1).R, b3.R)


def test_segments_of_packs_weighted_pools_for_the_device():
    from cfmmrouter_amd.router import _segments_of
    pools = [cr.ProductTwoCoin([1.0, 2.0], 1.0, [1, 2]), cr.Product([1.0, 2.0, 3.0], 0.997, [1, 2, 3]),
             cr.GeometricMean([1.0, 2.0, 3.0, 4.0], [1, 2, 3, 4], 0.99, [4, 3, 2, 1]),
             cr.GeometricMean([5.0, 6.0, 7.0], [1, 1, 2], 1.0, [3, 1, 2])]
    batches, order, host = _segments_of(pools)
    assert host == []
    assert [(b.kind, b.Ai.shape[1], len(b)) for b in batches] == [(0, 2, 1), (KIND_WEIGHTED, 3, 2), (KIND_WEIGHTED, 4, 1)]
    np.testing.assert_array_equal(order, [0, 1, 3, 2])


def test_chain_intake_of_three_and_five_token_weighted_pools():
    recs = [{"type": "weighted", "tokens": ["A", "B", "C"], "decimals": [18, 6, 8],
             "balances": [str(3 * 10**18), 2_000_000, 500_000_000], "weights": [1, 1, 2], "fee": 0.003},
            {"type": "weighted", "tokens": ["B", "A"], "balances": [10**18, 2 * 10**18], "weights": [0.8, 0.2], "fee": 0.001},
            {"type": "weighted", "tokens": ["A", "B", "C", "D", "E"], "balances": [10**18] * 5,
             "weights": [0.2] * 5, "fee_bps": 25}]
    tokens, batches = chain.load_snapshot(recs)
    assert tokens == ["A", "B", "C", "D", "E"]
    bg, b3, b5 = batches
    assert bg.kind == KIND_GEOMEAN and len(bg) == 1                   # two tokens: still GeometricMeanTwoCoin
    assert b3.kind == KIND_WEIGHTED and b3.n_coins == 3 and b5.n_coins == 5
    np.testing.assert_allclose(b3.R, [[3.0, 2.0, 5.0]])
    np.testing.assert_allclose(b3.w, [[0.25, 0.25, 0.5]])
    np.testing.assert_array_equal(b3.Ai, [[1, 2, 3]])
    assert b3.γ[0] == pytest.approx(0.997)
    np.testing.assert_allclose(b5.R, [[1.0] * 5])
    assert b5.γ[0] == pytest.approx(0.9975)
    with pytest.raises(cr.ArgumentError, match="distinct"):
        chain.load_snapshot([{"type": "weighted", "tokens": ["A", "B", "A"], "balances": [1, 1, 1], "weights": [1, 1, 1],
                              "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="3 positive weights"):
        chain.load_snapshot([{"type": "weighted", "tokens": ["A", "B", "C"], "balances": [1, 1, 1], "weights": [1, 1],
                              "fee": 0.0}])
    with pytest.raises(cr.ArgumentError, match="two distinct identifiers"):   # 9 tokens: not a supported pool
        chain.load_snapshot([{"type": "weighted", "tokens": list("ABCDEFGHI"), "balances": [1] * 9, "weights": [1] * 9,
                              "fee": 0.0}])


def test_header_declares_the_weighted_entries():
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    assert "#define CFMM_KIND_WEIGHTED 3" in h
    assert "int cfmm_pools_add_weighted(cfmm_ctx* ctx, int64_t m, int32_t n_coins, const double* R, const double* w," in h
    assert "int64_t cfmm_trades_len(const cfmm_ctx* ctx);" in h
    assert cr.lib().cfmm_pools_add_weighted is not None and cr.lib().cfmm_trades_len is not None
