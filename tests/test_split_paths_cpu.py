"""The contract of cfmm_split_paths (tests/split_paths_ref.py, the numpy statement of include/cfmm_amd_split.h) against the closed
form on chains of ProductTwoCoin pools.  One pool answers R_out·γx / (R_in + γx) = a·x / (b + c·x) with a = γR_out, b = R_in,
c = γ; two such forms compose to one of the same shape (a = a1·a2, b = b1·b2, c = b2·c1 + c2·a1), so every path is
a·x / (b + c·x) with marginal a·b / (b + c·x)².  The best split of A equalises the marginals of the paths it uses at a
multiplier λ: x_k = (√(a_k·b_k/λ) − b_k) / c_k on the paths with a_k/b_k > λ, which sum to A -- water filling, solved exactly
path by path in the order of a_k/b_k.  No device.

MEASURED HERE (4000 orders; the numbers quoted in the header, the docstrings and DESIGN.md), relative shortfall of total_out
against the closed form, worst / 99th percentile / median of the orders:
    1 round 1.8e-2 / 3.9e-3 / 9e-14     2 rounds 1.6e-4 / 1.2e-5 / 9e-14     3 rounds 1.8e-6 / 8.5e-8 / 5e-14
    4 rounds 1.6e-7 / 6.4e-10 / 2e-15   5 rounds 1.6e-7 / 8.0e-12 / 2e-16    6 and more 1.6e-7 / 2e-13 / 2e-16
and |share - optimum's| <= 4.7e-2, 2.3e-3, 4.7e-4 times A after 1, 2, 3 rounds and 4.7e-4 * A from then on (99% of the orders:
1.0e-6 * A at 5 rounds, 1.5e-7 * A at 6 or more -- the optimum is flat, this is sqrt(eps)); |sum of shares - A| <= 3.0e-16 * A at
every round count.  THE WORST CASE STALLS after round 4: stepping a share back ONE slice is a lower bound of the finer optimum
for two paths, but with K paths the others can each want up to a slice more, so the path that took the slack can be up to K-1
slices above its optimum, and the search never takes a share below its restart point.  The worst orders are 8-path orders in
which one path carries most of the amount.  The median order is at the rounding of the total after 5 rounds."""
import numpy as np
import pytest

from split_paths_ref import MAX_PATHS, POINTS, SPLIT_NAN, SPLIT_NONE, SPLIT_OK, SPLIT_SATURATED, split_paths_ref

N_ORDERS = 4000
SEED = 11
# what this file measured on the reference (printed by test_convergence_table), and the margins asserted over them: 10x on the shortfall and the shares, 4x on the sum
SHORTFALL_5_MEASURED = 1.6e-7
SHARE_ERR_5_MEASURED = 4.7e-4
SUM_ERR_MEASURED = 3.0e-16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def orders(n=N_ORDERS, seed=SEED):
    """K = 1 .. 8 paths per order, each a chain of 1 .. 3 pools with reserves 10^U(3, 6) and fees U(0.99, 0.9999); the amount
    10^U(1, 6)"""
    rng = np.random.default_rng(seed)
    K = rng.integers(1, MAX_PATHS + 1, n)
    first = np.concatenate(([0], np.cumsum(K)))
    P = int(first[-1])
    hops = rng.integers(1, 4, P)
    R_in, R_out = 10.0 ** rng.uniform(3, 6, (P, 3)), 10.0 ** rng.uniform(3, 6, (P, 3))
    g = rng.uniform(0.99, 0.9999, (P, 3))
    A = 10.0 ** rng.uniform(1, 6, n)
    a, b, c = g[:, 0] * R_out[:, 0], R_in[:, 0].copy(), g[:, 0].copy()
    for h in (1, 2):
        a2, b2, c2 = g[:, h] * R_out[:, h], R_in[:, h], g[:, h]
        on = hops > h
        a, b, c = np.where(on, a * a2, a), np.where(on, b * b2, b), np.where(on, b2 * c + c2 * a, c)
    return dict(first=first, K=K, hops=hops, R_in=R_in, R_out=R_out, g=g, A=A, a=a, b=b, c=c)


def quoter(m):
    def quote_path(p, x):
        y = np.asarray(x, dtype=np.float64)
        for h in range(3):
            q = m["R_out"][p, h] * (m["g"][p, h] * y / (m["R_in"][p, h] + m["g"][p, h] * y))
            y = np.where(m["hops"][p] > h, q, y)
        return y
    return quote_path


def optimum(m):
    """-> (shares [n_paths], total [orders]) of the closed form"""
    shares, total = np.zeros(m["a"].size), np.zeros(m["A"].size)
    for g_ in range(m["A"].size):
        lo, hi = int(m["first"][g_]), int(m["first"][g_ + 1])
        a, b, c = m["a"][lo:hi], m["b"][lo:hi], m["c"][lo:hi]
        order = np.argsort(-(a / b), kind="stable")
        use = 0
        for cnt in range(1, hi - lo + 1):                            # the largest set whose multiplier stays below its marginals at 0
            s = order[:cnt]
            root = (m["A"][g_] + np.sum(b[s] / c[s])) / np.sum(np.sqrt(a[s] * b[s]) / c[s])   # = 1/sqrt(λ)
            if np.all(a[s] / b[s] * root * root > 1.0):
                use, best_root = cnt, root
        s = order[:use]
        x = np.zeros(hi - lo)
        x[s] = (np.sqrt(a[s] * b[s]) * best_root - b[s]) / c[s]
        shares[lo:hi] = x
        total[g_] = np.sum(a * x / (b + c * x))
    return shares, total


@pytest.fixture(scope="module")
def market():
    m = orders()
    m["opt_shares"], m["opt_total"] = optimum(m)
    m["trace"] = []
    m["answer"] = split_paths_ref(quoter(m), m["first"], m["A"], rounds=8, trace=m["trace"])
    return m


def per_round(m):
    """the answer after r = 1 .. 8 rounds, from the trace of one 8-round run (round r does not know how many follow)"""
    G = m["A"].size
    active = np.arange(MAX_PATHS)[None, :] < m["K"][:, None]
    for r, (x, y, n, rem) in enumerate(m["trace"], start=1):
        xs = np.take_along_axis(x, n[:, :, None], axis=2)[:, :, 0]
        ys = np.take_along_axis(y, n[:, :, None], axis=2)[:, :, 0]
        total = ys[:, 0].copy()
        for k in range(1, MAX_PATHS):
            total = np.where(k < m["K"], total + ys[:, k], total)
        assert total.shape == (G,)
        yield r, xs, active, total


def test_convergence_table(market):
    m = market
    A = m["A"]
    table = {}
    for r, xs, active, total in per_round(m):
        short = (m["opt_total"] - total) / m["opt_total"]
        share_err = np.zeros(A.size)
        np.maximum.at(share_err, np.repeat(np.arange(A.size), m["K"]), np.abs(xs[active] - m["opt_shares"]))
        sums = np.array([np.sum(xs[g_, :m["K"][g_]].astype(np.longdouble)) for g_ in range(A.size)])
        sum_err = np.abs(sums - A.astype(np.longdouble)).astype(np.float64) / A
        table[r] = (short.max(), (share_err / A).max(), sum_err.max())
        print(f"rounds {r}: shortfall worst {short.max():.2e} 99% {np.quantile(short, 0.99):.2e} median {np.median(short):.2e}   "
              f"|share - optimum| / A worst {(share_err / A).max():.2e} 99% {np.quantile(share_err / A, 0.99):.2e}   "
              f"|sum of shares - A| / A worst {sum_err.max():.2e}")
    assert table[5][0] <= 10 * SHORTFALL_5_MEASURED
    assert table[5][1] <= 10 * SHARE_ERR_5_MEASURED
    assert all(table[r][2] <= 4 * SUM_ERR_MEASURED for r in table)
    assert all(table[r + 1][0] <= table[r][0] for r in range(1, 5))          # every round up to the fifth improves the worst case
    # the answer of the 8-round run is its last round's, and every path's output is the quote of its share, bit for bit
    path_in, path_out, total, status = m["answer"]
    # (beyond what the amounts' precision supports a slice is below the rounding of the outputs, an increment rounds to 0.0 and
    #  the order says SATURATED: one-path orders, whose remainder shrinks 63-fold per round, reach that at 6 rounds)
    assert np.all((status == SPLIT_OK) | (status == SPLIT_SATURATED)) and np.all(status[m["K"] > 1] == SPLIT_OK)
    np.testing.assert_array_equal(bits(path_out), bits(quoter(m)(np.arange(path_in.size), path_in)))


def test_five_rounds_is_the_default_and_matches_the_trace(market):
    m = market
    path_in, path_out, total, status = split_paths_ref(quoter(m), m["first"], m["A"])
    assert np.all(status == SPLIT_OK)
    for r, xs, active, tot in per_round(m):
        if r == 5:
            np.testing.assert_array_equal(bits(path_in), bits(xs[active]))
            np.testing.assert_array_equal(bits(total), bits(tot))


def test_one_path_gets_the_amount_bit_for_bit(market):
    """K = 1: x[0][63] of round 1 is 0 + A = A; every later base is below A and within a factor two of it, so A − base is exact
    and base + (A − base) is A again"""
    m = market
    one = np.flatnonzero(m["K"] == 1)
    assert one.size > 100
    for r, xs, active, total in per_round(m):
        np.testing.assert_array_equal(bits(xs[one, 0]), bits(m["A"][one]))
    rng = np.random.default_rng(2)
    A = np.concatenate((10.0 ** rng.uniform(-300, 300, 500), [5e-324, 1.7976931348623157e308, 1.0, 3.0, 0.1]))
    for rounds in (1, 2, 5, 16):
        trace = []
        x, y, t, st = split_paths_ref(lambda p, v: np.sqrt(v), np.arange(A.size + 1), A, rounds=rounds, trace=trace)
        np.testing.assert_array_equal(bits(x), bits(A))
        np.testing.assert_array_equal(bits(t), bits(np.sqrt(A)))
        assert all(np.all(n[:, 0] == POINTS - 1) for _, _, n, _ in trace)


def test_the_remainder_is_at_most_k_slices_after_every_round(market):
    m = market
    for r in range(len(m["trace"]) - 1):
        rem, nxt = m["trace"][r][3], m["trace"][r + 1][3]
        s = rem / (POINTS - 1)
        # K slices, and the roundings of the restart points and of their sum: fewer than 32 of at most A * 2^-53 each
        assert np.all(nxt <= m["K"] * s + 32 * 2.0 ** -53 * m["A"]), r
        assert np.all(nxt >= 0)


def test_ties_go_to_the_smaller_path():
    f = lambda p, x: 100.0 * x / (50.0 + x)
    trace = []
    x, y, t, st = split_paths_ref(f, [0, 2], [40.0], rounds=1, trace=trace)
    np.testing.assert_array_equal(trace[0][2][0, :2], [32, 31])
    assert st[0] == SPLIT_OK and x[0] > x[1]
    trace = []
    split_paths_ref(f, [0, 8], [40.0], rounds=1, trace=trace)
    np.testing.assert_array_equal(trace[0][2][0], [8, 8, 8, 8, 8, 8, 8, 7])   # 63 = 7 * 8 + 7: the last path is one short


def test_a_nan_path_gets_nothing_and_all_nan_is_split_nan():
    def f(p, x):
        return np.where(p == 1, np.nan, 100.0 * x / (50.0 + x))
    trace = []
    x, y, t, st = split_paths_ref(f, [0, 3], [40.0], rounds=3, trace=trace)
    for _, _, n, _ in trace:
        assert n[0, 1] == 0 and n[0, 0] + n[0, 2] == POINTS - 1             # the NaN path loses every step to a number
    assert st[0] == SPLIT_NAN and np.all(np.isnan(x)) and np.all(np.isnan(y)) and np.isnan(t[0])   # ... but its output is no number
    # a path that is NaN only beyond some size keeps what it got below it
    g = lambda p, v: np.where((p == 1) & (v > 5.0), np.nan, 100.0 * v / (50.0 + v))
    x, y, t, st = split_paths_ref(g, [0, 2], [40.0], rounds=5)
    assert st[0] == SPLIT_OK and 0 < x[1] <= 5.0 and abs(x[0] + x[1] - 40.0) < 1e-13
    x, y, t, st = split_paths_ref(lambda p, v: np.full(v.shape, np.nan), [0, 2, 3], [40.0, 1.0], rounds=2)
    assert np.all(st == SPLIT_NAN) and np.all(np.isnan(x)) and np.all(np.isnan(y)) and np.all(np.isnan(t))
    # an amount that is no valid number poisons its order alone
    x, y, t, st = split_paths_ref(lambda p, v: 100.0 * v / (50.0 + v), [0, 2, 3, 5], [np.nan, 7.0, -1.0], rounds=2)
    assert list(st) == [SPLIT_NAN, SPLIT_OK, SPLIT_NAN] and x[2] == 7.0 and np.all(np.isnan(x[[0, 1, 3, 4]]))


def test_saturating_paths_and_an_empty_order():
    caps = np.array([10.0, 20.0, 5.0, 50.0])
    f = lambda p, v: np.minimum(v, caps[p])
    x, y, t, st = split_paths_ref(f, [0, 3], [100.0], rounds=5)              # the paths absorb 35 of the 100
    assert st[0] == SPLIT_SATURATED and abs(t[0] - 35.0) < 1e-9 and abs(np.sum(x) - 100.0) < 1e-12
    x, y, t, st = split_paths_ref(f, [0, 3], [30.0], rounds=5)               # ... and all of 30
    assert st[0] == SPLIT_OK and abs(t[0] - 30.0) < 1e-9
    x, y, t, st = split_paths_ref(f, [0, 3, 4], [0.0, 3.0], rounds=3)
    assert list(st) == [SPLIT_NONE, SPLIT_OK]
    assert not np.any(bits(x[:3])) and not np.any(bits(y[:3])) and not bits(t)[0]   # +0.0, every one
    assert x[3] == 3.0 and t[1] == 3.0
    x, y, t, st = split_paths_ref(lambda p, v: np.zeros(v.shape), [0, 2], [9.0], rounds=2)   # paths that give nothing
    assert st[0] == SPLIT_NONE and not np.any(bits(x)) and not np.any(bits(y)) and not bits(t)[0]
