"""The contract of cfmm_size_path (tests/size_path_ref.py, the numpy statement of include/cfmm_amd_size_path.h) against the closed
form of two-pool ProductTwoCoin cycles: x -> pool A -> pool B -> back.  With a = γaγb·Ra_out·Rb_out, b = Ra_in·Rb_in and
c = γa(Rb_in + γb·Ra_out) the cycle returns a·x / (b + c·x), whose gain over x peaks at x* = (√(ab) − b)/c.  No device."""
import numpy as np
import pytest

from size_path_ref import POINTS, SIZED, SIZED_AT_LIMIT, SIZED_NONE, size_path_ref

N_CYCLES = 4000
SEED = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cycles(n=N_CYCLES, seed=SEED):
    """reserves 10^U(2, 9), fees U(0.99, 0.9999), the second pool's output reserve scaled up where needed so that a/b >= 1.001,
    max_in = x* · 10^U(0.1, 2)"""
    rng = np.random.default_rng(seed)
    Ra_in, Ra_out, Rb_in, Rb_out = (10.0 ** rng.uniform(2, 9, n) for _ in range(4))
    ga, gb = rng.uniform(0.99, 0.9999, n), rng.uniform(0.99, 0.9999, n)
    ratio = (ga * gb * Ra_out * Rb_out) / (Ra_in * Rb_in)
    Rb_out = Rb_out * np.maximum(1.0, 1.0011 / ratio)
    a, b, c = ga * gb * Ra_out * Rb_out, Ra_in * Rb_in, ga * (Rb_in + gb * Ra_out)
    assert np.all(a / b >= 1.001)
    x_star = (np.sqrt(a * b) - b) / c
    gain_star = a * x_star / (b + c * x_star) - x_star
    max_in = x_star * 10.0 ** rng.uniform(0.1, 2, n)
    return dict(Ra_in=Ra_in, Ra_out=Ra_out, Rb_in=Rb_in, Rb_out=Rb_out, ga=ga, gb=gb, x_star=x_star, gain_star=gain_star, max_in=max_in)


def product_quote(R_in, R_out, g, x):
    return R_out * (g * x / (R_in + g * x))


def quoter(m):
    def quote_path(p, x):
        y = product_quote(m["Ra_in"][p], m["Ra_out"][p], m["ga"][p], x)
        return product_quote(m["Rb_in"][p], m["Rb_out"][p], m["gb"][p], y)
    return quote_path


@pytest.fixture(scope="module")
def market():
    return cycles()


@pytest.mark.parametrize("rounds", (1, 2, 3))
def test_amount_in_is_within_the_bracket_of_the_closed_form(market, rounds):
    """the gain is concave, so x* lies in every bracket, and after r rounds the bracket is at most max_in·(2/63)^r wide"""
    x, y, g, st = size_path_ref(quoter(market), market["max_in"], rounds=rounds)
    width = market["max_in"] * (2.0 / 63.0) ** rounds
    off = np.abs(x - market["x_star"]) / width
    print(f"rounds {rounds}: worst |amount_in - x*| / bracket = {off.max():.3g}")
    assert np.all(off <= 1.0)
    assert np.all((st == SIZED) | (st == SIZED_AT_LIMIT))
    np.testing.assert_array_equal(bits(y), bits(quoter(market)(np.arange(x.size), x)))      # the round trip
    np.testing.assert_array_equal(bits(g), bits(y - x))


def test_five_rounds_reach_the_closed_form_gain(market):
    x, y, g, st = size_path_ref(quoter(market), market["max_in"], rounds=5)
    short = (market["gain_star"] - g) / market["gain_star"]
    print(f"rounds 5: worst (gain* - gain) / gain* = {short.max():.3g}")
    assert np.all(short <= 1e-9)
    assert np.all(st == SIZED)                                     # max_in >= 1.25 x*: the limit never binds


def test_trial_sizes_are_monotone_and_stay_in_the_bracket(market):
    trace = []
    size_path_ref(quoter(market), market["max_in"], rounds=8, trace=trace)
    lo, hi = np.zeros(N_CYCLES), market["max_in"]
    rows = np.arange(N_CYCLES)
    for x, g, j in trace:
        assert np.all(np.diff(x, axis=1) >= 0)
        assert np.all(x >= lo[:, None]) and np.all(x <= hi[:, None])
        np.testing.assert_array_equal(bits(x[:, 0]), bits(lo))
        np.testing.assert_array_equal(bits(x[:, POINTS - 1]), bits(hi))
        assert np.all(g[rows, j][:, None] >= g)                     # j* holds the largest gain ...
        first = np.argmax(g == g[rows, j][:, None], axis=1)
        np.testing.assert_array_equal(first, j)                     # ... and is the smallest such j
        lo, hi = x[rows, np.maximum(j - 1, 0)], x[rows, np.minimum(j + 1, POINTS - 1)]


def test_an_unprofitable_cycle_answers_none_with_three_positive_zeros(market):
    m = dict(market)
    ratio = (m["ga"] * m["gb"] * m["Ra_out"] * m["Rb_out"]) / (m["Ra_in"] * m["Rb_in"])
    m["Rb_out"] = market["Rb_out"] * (0.9 / ratio)                 # a/b = 0.9: every size loses
    for rounds in (1, 5):
        x, y, g, st = size_path_ref(quoter(m), market["max_in"], rounds=rounds)
        assert np.all(st == SIZED_NONE)
        for v in (x, y, g):
            np.testing.assert_array_equal(bits(v), np.zeros(N_CYCLES, dtype=np.uint64))
    x, y, g, st = size_path_ref(quoter(market), np.zeros(N_CYCLES), rounds=3)   # nothing to put in
    assert np.all(st == SIZED_NONE) and not np.any(bits(x)) and not np.any(bits(y)) and not np.any(bits(g))


def test_a_limit_far_below_the_optimum_binds(market):
    max_in = market["x_star"] * 1e-3
    for rounds in (1, 5):
        x, y, g, st = size_path_ref(quoter(market), max_in, rounds=rounds)
        assert np.all(st == SIZED_AT_LIMIT)
        np.testing.assert_array_equal(bits(x), bits(max_in))
        assert np.all(g > 0)
