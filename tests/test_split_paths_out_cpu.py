"""The contract of cfmm_split_paths_out (tests/split_paths_out_ref.py, the numpy statement of include/cfmm_amd_split_out.h)
against the closed form on chains of ProductTwoCoin pools -- test_split_paths_cpu.py's sample (4000 random orders, K = 1 .. 8
chains of 1 .. 3 hops).  A chain composes to out = a·x / (b + c·x), so buying y through it costs b·y / (a − c·y) up to its
capacity a/c, with marginal a·b / (a − c·y)².  The cheapest way to buy B equalises the marginals of the paths it uses at a
multiplier μ: y_k = (a_k − √(a_k·b_k/μ)) / c_k on the paths with b_k/a_k < μ, found by bisection on μ.  B is drawn from
10^U(−2.5, 0.5) times the order's joint capacity Σ a_k/c_k, so part of the sample can be bought and part cannot.  No device.

MEASURED HERE (the numbers quoted in the header and DESIGN.md; printed by test_convergence_table), on the orders below the joint
capacity that the search answers SPLIT_OK, relative EXCESS of total_in over the closed form, worst / 99th percentile / median:
    1 round 6.5 / 1.9e-1 / 1e-16          2 rounds 4.0e-1 / 2.6e-3 / 1e-16      3 rounds 4.0e-1 / 1.1e-4 / 1e-16
    4 rounds 4.0e-1 / 1.5e-6 / 1e-16      5 rounds 4.0e-1 / 1.5e-8 / 0          6 rounds 4.0e-1 / 1.4e-10 / 0
THE WORST CASE STALLS after round 2, and it is large: it belongs to orders within a few per cent of their joint capacity,
where a path's cost b*y / (a - c*y) is steep without bound, so the slice by which round 1 overfills a path (a share never
goes below its restart point: cfmm_amd_split.h says why that is up to K-1 slices) costs a multiple of the optimum.  On the
orders whose paths jointly give at least 2 B the worst excess is 4.8e-2, 4.5e-4, 2.7e-4 after 1, 2, 3 rounds and 2.7e-4 from
then on.  Shares within 2.4e-2 * B of the optimum's for all orders and within 1.2e-6 * B for 99 % of them at 5 rounds;
|sum of shares - B| <= 3.2e-16 * B at every round count.
The grid-feasibility limit, measured: of the 3347 orders of the sample below their joint capacity 18 were reported
SPLIT_UNOBTAINABLE, every one of them in round 1 and the same 18 at every round count 1 .. 8 (no later round refused an
order that round 1 had served); the largest joint capacity / B among them was 1.0581, which is 0.9698 of that order's
1 + K/63, and no order above 1.0581 was refused; the smallest joint capacity / B of a served order was 1.0092."""
import numpy as np
import pytest

from split_paths_out_ref import (BAD_INF, BAD_NAN, CLEAN, SPLIT_UNOBTAINABLE, answer_status, greedy_out, split_paths_out_ref)
from split_paths_ref import MAX_PATHS, POINTS, SPLIT_NAN, SPLIT_NONE, SPLIT_OK
from test_split_paths_cpu import N_ORDERS, bits, orders

# what this file measured on the reference against the closed form (never against the kernel); the assertions allow 2x
EXCESS_MEASURED = {1: 6.5, 2: 4.0e-1, 3: 4.0e-1, 4: 4.0e-1, 5: 4.0e-1, 6: 4.0e-1}    # worst relative excess of total_in after r rounds
ROOMY_EXCESS_MEASURED = {1: 4.8e-2, 2: 4.5e-4, 3: 2.7e-4, 4: 2.7e-4, 5: 2.7e-4, 6: 2.7e-4}   # ... of the orders with capacity / B >= 2
SHARE_ERR_5_MEASURED = 2.4e-2                                           # worst |share - optimum's| / B at 5 rounds
SUM_ERR_MEASURED = 3.2e-16                                               # worst |sum of shares - B| / B at any round count
REFUSED_UP_TO_MEASURED = 1.0581                                        # largest joint capacity / B of an UNOBTAINABLE order


def market_out(n=N_ORDERS):
    m = orders(n)
    m["cap"] = m["a"] / m["c"]
    m["C"] = np.add.reduceat(m["cap"], m["first"][:-1])
    rng = np.random.default_rng(12)
    m["B"] = m["C"] * 10.0 ** rng.uniform(-2.5, 0.5, n)
    return m


def quoter_out(m):
    """hop by hop from the last to the first: buying y of a pool costs R_in·y / (γ·(R_out − y)), +inf from y = R_out on"""
    def quote_path_out(p, y):
        y = np.asarray(y, dtype=np.float64)
        for h in (2, 1, 0):
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                q = m["R_in"][p, h] * y / (m["g"][p, h] * (m["R_out"][p, h] - y))
            q = np.where(y < m["R_out"][p, h], q, np.inf)
            y = np.where(m["hops"][p] > h, q, y)
        return y
    return quote_path_out


def optimum_out(m):
    """-> (shares [n_paths], total [orders]) of the closed form; NaN for the orders at or above the joint capacity"""
    shares, total = np.full(m["a"].size, np.nan), np.full(m["B"].size, np.nan)
    for g_ in np.flatnonzero(m["B"] < m["C"]):
        lo, hi = int(m["first"][g_]), int(m["first"][g_ + 1])
        a, b, c = (m[k][lo:hi].astype(np.longdouble) for k in "abc")
        B = np.longdouble(m["B"][g_])
        give = lambda mu: np.where(mu > b / a, (a - np.sqrt(a * b / mu)) / c, 0.0)
        lo_mu, hi_mu = np.min(b / a), np.max(b / a)
        while np.sum(give(hi_mu)) < B:
            hi_mu *= 2
        for _ in range(200):
            mid = np.sqrt(lo_mu * hi_mu)
            lo_mu, hi_mu = (mid, hi_mu) if np.sum(give(mid)) < B else (lo_mu, mid)
        y = give(hi_mu)
        y = y * (B / np.sum(y))                                         # (the bisection's last ulps)
        shares[lo:hi] = y.astype(np.float64)
        total[g_] = np.float64(np.sum(b * y / (a - c * y)))
    return shares, total


@pytest.fixture(scope="module")
def market():
    m = market_out()
    m["opt_shares"], m["opt_total"] = optimum_out(m)
    m["trace"] = []
    m["answer"] = split_paths_out_ref(quoter_out(m), m["first"], m["B"], rounds=8, trace=m["trace"])
    return m


def per_round(m):
    """the answer after r = 1 .. 8 rounds, from the trace of one 8-round run (round r does not know how many follow)"""
    active = np.arange(MAX_PATHS)[None, :] < m["K"][:, None]
    for r, (x, c, n, rem, bad) in enumerate(m["trace"], start=1):
        xs = np.take_along_axis(x, n[:, :, None], axis=2)[:, :, 0]
        cs = np.take_along_axis(c, n[:, :, None], axis=2)[:, :, 0]
        total = cs[:, 0].copy()
        with np.errstate(invalid="ignore"):
            for k in range(1, MAX_PATHS):
                total = np.where(k < m["K"], total + cs[:, k], total)
        yield r, xs, active, total, answer_status(bad, m["B"], total)


def test_convergence_table(market):
    m = market
    B, K = m["B"], m["K"]
    ratio = m["C"] / B
    table = {}
    for r, xs, active, total, status in per_round(m):
        assert np.all((status == SPLIT_OK) | (status == SPLIT_UNOBTAINABLE))
        ok = status == SPLIT_OK
        assert np.all(ratio[ok] > 1.0 - 1e-12)                              # what the paths cannot give is never reported bought
        fit = ok & (B < m["C"])
        excess = (total[fit] - m["opt_total"][fit]) / m["opt_total"][fit]
        share_err = np.zeros(B.size)
        with np.errstate(invalid="ignore"):
            np.maximum.at(share_err, np.repeat(np.arange(B.size), K), np.abs(xs[active] - m["opt_shares"]))
        sums = np.array([np.sum(xs[g_, :K[g_]].astype(np.longdouble)) for g_ in range(B.size)])
        sum_err = (np.abs(sums - B.astype(np.longdouble)).astype(np.float64) / B)[ok]
        refused = ~ok
        roomy = ratio[fit] >= 2.0                                           # away from the capacity, where the cost is not yet steep
        table[r] = dict(excess=excess.max(), share=(share_err / B)[fit].max(), sum=sum_err.max(), refused_up_to=ratio[refused].max(),
                        refused_rel=(ratio / (1 + K / 63.0))[refused].max(), accepted_down_to=ratio[ok].min(),
                        n_ok=int(ok.sum()), n_fit=int((B < m["C"]).sum()), roomy=excess[roomy].max())
        print(f"rounds {r}: ok {ok.sum()} of {(B < m['C']).sum()} below the joint capacity;  excess worst {excess.max():.2e} "
              f"99% {np.quantile(excess, 0.99):.2e} median {np.median(excess):.2e} (capacity / B >= 2: worst {excess[roomy].max():.2e});  |share - optimum| / B worst "
              f"{(share_err / B)[fit].max():.2e} 99% {np.quantile((share_err / B)[fit], 0.99):.2e};  |sum of shares - B| / B worst "
              f"{sum_err.max():.2e};  capacity / B: refused up to {ratio[refused].max():.4f} (x (1 + K/63): {table[r]['refused_rel']:.4f}), "
              f"accepted down to {ratio[ok].min():.4f}")
    for r in EXCESS_MEASURED:
        assert table[r]["excess"] <= 2 * EXCESS_MEASURED[r], r
    assert table[5]["share"] <= 2 * SHARE_ERR_5_MEASURED
    assert all(table[r]["roomy"] <= 2 * ROOMY_EXCESS_MEASURED[r] for r in ROOMY_EXCESS_MEASURED)
    assert len({table[r]["n_ok"] for r in table}) == 1                     # no round after the first refused an order
    assert all(table[r]["sum"] <= 2 * SUM_ERR_MEASURED for r in table)
    assert all(table[r]["refused_up_to"] <= REFUSED_UP_TO_MEASURED * (1 + 1e-3) for r in table)
    # the derivation of the header: round 1 refuses no order whose paths jointly give B * (1 + K/63)
    assert table[1]["refused_rel"] < 1.0
    # every path's cost is the quote of its share, bit for bit, on the orders that were answered
    share, cost, total, status = m["answer"]
    ok = np.repeat(status == SPLIT_OK, K)
    np.testing.assert_array_equal(bits(cost[ok]), bits(quoter_out(m)(np.flatnonzero(ok), share[ok])))
    bad = np.repeat(status == SPLIT_UNOBTAINABLE, K)
    assert np.all(np.isposinf(cost[bad])) and not np.any(bits(share[bad])) and np.all(np.isposinf(total[status == SPLIT_UNOBTAINABLE]))


def test_five_rounds_is_the_default_and_matches_the_trace(market):
    m = market
    share, cost, total, status = split_paths_out_ref(quoter_out(m), m["first"], m["B"])
    for r, xs, active, tot, st in per_round(m):
        if r == 5:
            np.testing.assert_array_equal(status, st)
            ok = st == SPLIT_OK
            np.testing.assert_array_equal(bits(share[np.repeat(ok, m["K"])]), bits(xs[active & ok[:, None]]))
            np.testing.assert_array_equal(bits(total[ok]), bits(tot[ok]))
    assert np.sum(status == SPLIT_OK) > 1000 and np.sum(status == SPLIT_UNOBTAINABLE) > 300


def test_one_path_gets_the_amount_bit_for_bit(market):
    """K = 1: x[0][63] of round 1 is 0 + B = B; every later base is below B and within a factor two of it, so B − base is exact
    and base + (B − base) is B again"""
    m = market
    for r, xs, active, total, status in per_round(m):
        one = np.flatnonzero((m["K"] == 1) & (status == SPLIT_OK))
        assert one.size > 100
        np.testing.assert_array_equal(bits(xs[one, 0]), bits(m["B"][one]))
    rng = np.random.default_rng(2)
    B = np.concatenate((10.0 ** rng.uniform(-300, 150, 500), [5e-324, 1.3e154, 1.0, 3.0, 0.1]))
    for rounds in (1, 2, 5, 16):
        x, c, t, st = split_paths_out_ref(lambda p, v: v * v, np.arange(B.size + 1), B, rounds=rounds)
        assert np.all(st == SPLIT_OK)
        np.testing.assert_array_equal(bits(x), bits(B))
        np.testing.assert_array_equal(bits(t), bits(B * B))


def test_ties_go_to_the_smaller_path():
    f = lambda p, y: 50.0 * y / (100.0 - y)
    trace = []
    x, c, t, st = split_paths_out_ref(f, [0, 2], [40.0], rounds=1, trace=trace)
    np.testing.assert_array_equal(trace[0][2][0, :2], [32, 31])
    assert st[0] == SPLIT_OK and x[0] > x[1]
    trace = []
    split_paths_out_ref(f, [0, 8], [40.0], rounds=1, trace=trace)
    np.testing.assert_array_equal(trace[0][2][0], [8, 8, 8, 8, 8, 8, 8, 7])   # 63 = 7 * 8 + 7: the last path is one short
    # a free slice (an increment of 0) is taken before any that costs, and is no failure
    free = lambda p, y: np.where(p == 1, np.maximum(y - 10.0, 0.0), y)
    x, c, t, st = split_paths_out_ref(free, [0, 2], [5.0], rounds=3)
    assert st[0] == SPLIT_OK and x[0] == 0.0 and x[1] == 5.0 and t[0] == 0.0 and not np.signbit(t[0])


def test_a_nan_path_gets_nothing_and_all_nan_is_split_nan():
    def f(p, y):
        return np.where(p == 1, np.nan, 50.0 * y / (100.0 - y))
    trace = []
    x, c, t, st = split_paths_out_ref(f, [0, 3], [40.0], rounds=3, trace=trace)
    for _, _, n, _, bad in trace:
        assert n[0, 1] == 0 and n[0, 0] + n[0, 2] == POINTS - 1             # the NaN path loses every step to a number
        assert bad[0] == CLEAN
    assert st[0] == SPLIT_NAN and np.all(np.isnan(x)) and np.all(np.isnan(c)) and np.isnan(t[0])   # ... but its cost is no number
    # a path that is NaN only beyond some size keeps what it got below it
    g = lambda p, v: np.where((p == 1) & (v > 5.0), np.nan, 50.0 * v / (100.0 - v))
    x, c, t, st = split_paths_out_ref(g, [0, 2], [40.0], rounds=5)
    assert st[0] == SPLIT_OK and 0 < x[1] <= 5.0 and abs(x[0] + x[1] - 40.0) < 1e-13
    x, c, t, st = split_paths_out_ref(lambda p, v: np.full(v.shape, np.nan), [0, 2, 3], [40.0, 1.0], rounds=2)
    assert np.all(st == SPLIT_NAN) and np.all(np.isnan(x)) and np.all(np.isnan(c)) and np.all(np.isnan(t))
    # an amount that is no valid number poisons its order alone
    x, c, t, st = split_paths_out_ref(lambda p, v: 50.0 * v / (100.0 - v), [0, 2, 3, 5], [np.nan, 7.0, -1.0], rounds=2)
    assert list(st) == [SPLIT_NAN, SPLIT_OK, SPLIT_NAN] and x[2] == 7.0 and np.all(np.isnan(x[[0, 1, 3, 4]]))


def capped(caps):
    caps = np.asarray(caps, dtype=np.float64)

    def f(p, y):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(y < caps[p], 50.0 * y / (caps[p] - y), np.inf)
    return f


def test_unobtainable_when_every_path_is_too_shallow():
    f = capped([10.0, 20.0, 5.0])
    for rounds in (1, 2, 5):
        x, c, t, st = split_paths_out_ref(f, [0, 3], [100.0], rounds=rounds)   # the paths give less than 35 of the 100
        assert st[0] == SPLIT_UNOBTAINABLE
        assert np.all(np.isposinf(c)) and np.isposinf(t[0]) and not np.any(bits(x))      # costs +inf, shares +0.0
    x, c, t, st = split_paths_out_ref(f, [0, 3], [30.0], rounds=5)               # ... and 30 comfortably: 35 >= 30 * (1 + 3/63)
    assert st[0] == SPLIT_OK and abs(np.sum(x) - 30.0) < 1e-12 and np.all(x < [10.0, 20.0, 5.0]) and np.isfinite(t[0])
    # no single path can give 12, the three together can: what the feature is for
    x, c, t, st = split_paths_out_ref(capped([10.0, 9.0, 8.0]), [0, 3], [12.0], rounds=5)
    assert st[0] == SPLIT_OK and np.all(np.isposinf(capped([10.0, 9.0, 8.0])(np.arange(3), np.full(3, 12.0))))
    # the grid's limit: 10 + 19 + 6 is more than 34.5, but in round 1 the paths hold only 18 + 34 + 10 = 62 whole slices of 34.5/63
    x, c, t, st = split_paths_out_ref(capped([10.0, 19.0, 6.0]), [0, 3], [34.5], rounds=5)
    assert st[0] == SPLIT_UNOBTAINABLE
    # a neighbour is untouched
    x, c, t, st = split_paths_out_ref(capped([10.0, 20.0, 5.0, 50.0]), [0, 3, 4], [100.0, 3.0], rounds=2)
    assert list(st) == [SPLIT_UNOBTAINABLE, SPLIT_OK] and x[3] == 3.0 and np.isfinite(t[1])


def test_the_first_bad_step_decides():
    j = np.arange(POINTS, dtype=np.float64)
    nan, inf = np.nan, np.inf
    full = lambda rows: np.concatenate((np.array(rows), np.full((MAX_PATHS - len(rows), POINTS), nan)))[None]
    # one path, finite to point 10, then +inf: step 11 takes +inf, steps 12 .. 63 see inf - inf = NaN and do not count
    t = j.copy(); t[11:] = inf
    n, bad = greedy_out(full([t]), np.array([1]))
    assert bad[0] == BAD_INF and n[0, 0] == POINTS - 1
    # ... NaN from point 11 on: the first bad step is no number
    t = j.copy(); t[11:] = nan
    n, bad = greedy_out(full([t]), np.array([1]))
    assert bad[0] == BAD_NAN
    # NaN before +inf and +inf before NaN
    t = j.copy(); t[5] = nan; t[20:] = inf
    assert greedy_out(full([t]), np.array([1]))[1][0] == BAD_NAN
    t = j.copy(); t[5:] = inf; t[30:] = nan
    assert greedy_out(full([t]), np.array([1]))[1][0] == BAD_INF
    # what an earlier round reported stays
    assert greedy_out(full([j]), np.array([1]), bad=np.array([BAD_INF]))[1][0] == BAD_INF
    assert greedy_out(full([j]), np.array([1]), bad=np.array([BAD_NAN]))[1][0] == BAD_NAN
    assert greedy_out(full([j]), np.array([1]))[1][0] == CLEAN
    # two paths: a +inf increment is a number, it beats the NaN path; the NaN path is never taken
    t = j.copy(); t[3:] = inf
    n, bad = greedy_out(full([np.full(POINTS, nan), t]), np.array([2]))
    assert bad[0] == BAD_INF and n[0, 0] + n[0, 1] == POINTS - 1
    # through the whole search: the status is the first's, whatever comes after
    def nan_then_inf(p, y):
        return np.where(y > 8.0, np.inf, np.where(y > 4.0, np.nan, y))
    def inf_then_nan(p, y):
        return np.where(y > 8.0, np.nan, np.where(y > 4.0, np.inf, y))
    assert split_paths_out_ref(nan_then_inf, [0, 1], [63.0], rounds=2)[3][0] == SPLIT_NAN
    x, c, t, st = split_paths_out_ref(inf_then_nan, [0, 1], [63.0], rounds=2)
    assert st[0] == SPLIT_UNOBTAINABLE and np.isposinf(c[0]) and np.isposinf(t[0]) and not bits(x)[0]


def test_an_empty_order():
    f = capped([10.0, 20.0, 5.0, 50.0])
    x, c, t, st = split_paths_out_ref(f, [0, 3, 4], [0.0, 3.0], rounds=3)
    assert list(st) == [SPLIT_NONE, SPLIT_OK]
    assert not np.any(bits(x[:3])) and not np.any(bits(c[:3])) and not bits(t)[0]   # +0.0, every one
    assert x[3] == 3.0 and t[1] == c[3]
