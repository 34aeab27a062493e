"""cfmm_swap on the device: the answer carries cfmm_quote's bits, the pools move to R + γΔ − Λ (UniV3: to the landing price,
through cfmm_pools_set_prices' own apply path), repeated rows are applied in query order, a swap that would leave an invalid
pool is refused, and the call is a state change with cfmm_pools_set_reserves' protocol.  Segments are small: every test
runs in seconds.  The 80-digit sequences are in tests/test_gpu_swap_precise.py."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
import swap_precise_ref as S
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_UNIV3, ptr
import test_gpu_pool_update as TU
from test_gpu_pool_update import assert_same, batch_with, outputs
from test_gpu_quote import N, fd_cond, pools, typical_queries

pytestmark = pytest.mark.gpu

CASES = [("product", 2), ("geomean", 2), ("solidly", 2), ("univ3", 2), ("weighted", 3), ("weighted", 8), ("curve", 3), ("curve", 8)]
IDS = [f"{k}{n}" if k in ("weighted", "curve") else k for k, n in CASES]
RESERVE = [c for c in CASES if c[0] != "univ3"]
RIDS = [i for i in IDS if i != "univ3"]
U = 2.0 ** -53
QUOTE_BLOCK = 256


V = synth.sweep_prices(N, seed=7, spread=0.3)
V2 = synth.sweep_prices(N, seed=8, spread=0.3)


def backend(batches, device=0):
    return TU.backend(batches, N, device)


def assert_equals_fresh(be, batches, v=V, device=0):
    TU.assert_equals_fresh(be, batches, N, device, v)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def state(ctx, b, seg=0):
    return ctx.prices(seg, len(b)) if b.kind == KIND_UNIV3 else ctx.reserves(seg, len(b), b.Ai.shape[1])


def with_state(b, st):
    return batch_with(b, current_price=st) if b.kind == KIND_UNIV3 else batch_with(b, R=st)


def full_co(b, ci, co):
    return (1 - ci).astype(np.int32) if co is None else co


# ---- the same bits as the quote ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
def test_swap_answers_with_the_bits_of_the_quote(kind, nc):
    m = QUOTE_BLOCK + 1                                               # one more query than a block: the grid-stride edge
    b = pools(kind, m, seed=101, n_coins=nc)
    ci, co, a = typical_queries(b, m, seed=2)
    perm = np.argsort(synth.uniform(102, 3, m)).astype(np.int64)
    for idx, sl in ((None, np.arange(m)), (perm, perm), (np.arange(64, dtype=np.int64), np.arange(64))):
        be = backend([b])
        try:
            args = (a[sl], ci[sl], None if co is None else co[sl], idx)
            q = be.ctx.quote(0, *args)
            s = be.ctx.swap(0, *args)
            assert np.all(np.isfinite(q))
            np.testing.assert_array_equal(bits(s), bits(q))
            assert be.ctx.get_option("swap_refused") == 0
            assert np.any(bits(be.ctx.quote(0, *args)) != bits(q))      # ... and the pools have moved
        finally:
            be.close()


# ---- the new state, reserve kinds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", RESERVE, ids=RIDS)
def test_new_reserves_are_exactly_R_plus_gamma_a_and_R_minus_out(kind, nc):
    m = 64
    b = pools(kind, m, seed=111, n_coins=nc)
    ci, co, a = typical_queries(b, m, seed=3)
    rows = np.arange(1, m, 3, dtype=np.int64)                          # a sparse subset: the other pools keep every bit
    a[rows[0]] = 0.0                                                  # ... and so does a pool swapped with nothing
    cof = full_co(b, ci, co)
    be = backend([b])
    try:
        out = be.ctx.swap(0, a[rows], ci[rows], None if co is None else co[rows], rows)
        R = be.ctx.reserves(0, m, b.Ai.shape[1])
    finally:
        be.close()
    want = b.R.copy()
    want[rows, ci[rows]] = b.R[rows, ci[rows]] + b.γ[rows] * a[rows]   # each operation rounded on its own
    want[rows, cof[rows]] = b.R[rows, cof[rows]] - out
    np.testing.assert_array_equal(bits(R), bits(want))
    assert out[0] == 0.0 and not np.signbit(out[0]) and np.all(out[1:] > 0)


# ---- a fresh upload of the state the swaps left ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("product", "solidly", "univ3"))
def test_after_swaps_the_context_equals_a_fresh_upload(kind):
    """Product, Solidly (no prepared constant depends on R) and UniV3 (re-prepared on the host by cfmm_pools_set_prices' own
    path): eval, find_arb, trades and state bit-identical at two price vectors; quotes in both directions and exact-output
    quotes too"""
    m = 64
    b = pools(kind, m, seed=121)
    ci, co, a = typical_queries(b, m, seed=4)
    be = backend([b])
    fresh = None
    try:
        be.ctx.swap(0, a, ci, co)
        now = with_state(b, state(be.ctx, b))
        orig = b.current_price if kind == "univ3" else b.R
        assert np.sum(np.any(bits(state(be.ctx, b)).reshape(m, -1) != bits(orig).reshape(m, -1), axis=1)) >= m // 2
        fresh = backend([now])
        for c in (ci, 1 - ci):
            np.testing.assert_array_equal(bits(be.ctx.quote(0, a, c)), bits(fresh.ctx.quote(0, a, c)))
            qo = be.ctx.quote(0, a, c) * 0.5
            np.testing.assert_array_equal(bits(be.ctx.quote_out(0, qo, c)), bits(fresh.ctx.quote_out(0, qo, c)))
        for v in (V, V2):
            assert_same(outputs(be, [now], v), outputs(fresh, [now], v))
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


def sweep_bound_two(b, Rr, v, DB, LB):
    """the scales of tests/test_gpu_precise.py's comparison of refreshed constants with a fresh upload"""
    import precise_ref as PR
    import test_gpu_precise as T
    import weighted_ref as wr
    vl = v[b.Ai - 1]
    if b.Ai.shape[1] > 2 or b.kind != 1:
        w = b.w / b.w.sum(axis=1, keepdims=True)
        Dp, Lp = wr.solve(Rr, w, b.γ, vl)
        return PR.weighted_scale(Rr, w, b.γ, vl, Dp, Lp), T.K_UPDATE["weighted"]
    Dp, Lp = T._approx_two_coin(Rr, b.w, b.γ, vl)
    return PR.two_coin_scale(Rr, b.w, b.γ, vl, Dp, Lp), T.K_UPDATE["two"]


@pytest.mark.parametrize("kind,nc", [("geomean", 2), ("weighted", 3), ("weighted", 8)], ids=["geomean", "weighted3", "weighted8"])
def test_refreshed_constants_against_a_fresh_upload_weighted(kind, nc):
    """quotes read only R and w: bit-identical.  The sweeps read the constants the swap refreshed on the device ({Q1, Q2},
    q = log(R/w): the device's log where the upload used the host's), so they agree within the bound the project already uses
    for the same comparison after cfmm_update_reserves (tests/test_gpu_precise.py: precise_ref's scales at K_UPDATE)."""
    import precise_ref as PR
    m = 64
    b = pools(kind, m, seed=131, n_coins=nc)
    ci, co, a = typical_queries(b, m, seed=5)
    v = synth.sweep_prices(N, seed=132, spread=0.3)
    be = backend([b])
    fresh = None
    try:
        be.ctx.swap(0, a, ci, co)
        Rr = be.ctx.reserves(0, m, b.Ai.shape[1])
        fresh = backend([batch_with(b, R=Rr)])
        np.testing.assert_array_equal(bits(be.ctx.quote(0, a, ci, co)), bits(fresh.ctx.quote(0, a, ci, co)))
        be.find_arb(v)
        fresh.find_arb(v)
        DA, LA = (np.reshape(x, (m, -1)) for x in be.trades())
        DB, LB = (np.reshape(x, (m, -1)) for x in fresh.trades())
    finally:
        be.close()
        if fresh is not None:
            fresh.close()
    (sD, sL), K = sweep_bound_two(b, Rr, v, DB, LB)
    r = PR.ratios(DA, LA, DB, LB, sD, sL)
    print(f"\n[swap refresh] {kind}{nc}: refreshed vs fresh upload, worst ratio {float(np.max(r)):.3g} of K = {K}")
    assert np.all(r <= K) and np.count_nonzero(DA) > m // 4


def test_refreshed_constants_against_a_fresh_upload_curve():
    """Curve: q = log R is refreshed with the device's log, the fresh upload prepares it with the host's.  The sweeps are held
    to the bound of the same comparison after cfmm_update_reserves (tests/test_gpu_curve_precise.py
    test_update_reserves_refresh_matches_a_fresh_upload): curve_precise_ref.scale of the 60-digit fixture's 3-coin pools --
    the swaps are 1% of a reserve, so the moved pools are within a trade of them, as there -- at that test's K_UPDATE.  The
    quotes read Σ log R: each is within K_q·u·(R_o + out + cond) of the exact quote of ITS logs (quote_precise_ref), and the
    two sets of logs differ by an ulp each -- a perturbation the conditioning sum covers at unit size -- so the two answers
    differ by at most (2·K_q + 1) units."""
    import curve_precise_ref as CP
    import test_gpu_curve_precise as T
    c = T.C["c_3"]
    Rt = c["R"] + c["gamma"][:, None] * c["D"] - c["L"]
    kept = np.all(Rt > 4 * CP.U * (c["R"] + c["gamma"][:, None] * c["D"] + c["L"]), axis=1)
    rows = np.flatnonzero(~CP.refused(c["R"], c["alpha"], c["beta"]) & kept)
    m, nc = len(rows), 3
    b = T._batch(c, rows)
    q = np.arange(m)
    ci, co = (q % nc).astype(np.int32), ((q + 1) % nc).astype(np.int32)
    a = 0.01 * b.R[q, ci]
    n = len(c["v"])
    be = cr.DeviceBackend(n, [b])
    fresh = None
    try:
        out = be.ctx.swap(0, a, ci, co)
        ok = np.isfinite(out)                                            # (a pool at the edge of the solve's range may refuse)
        assert ok.sum() >= m - 8
        Rr = be.ctx.reserves(0, m, nc)
        fresh = cr.DeviceBackend(n, [T._batch(c, rows, R=Rr)])
        qa, qb = be.ctx.quote(0, a, ci, co), fresh.ctx.quote(0, a, ci, co)
        be.find_arb(c["v2"])
        fresh.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, nc)) for x in be.trades())
        DB, LB = (np.reshape(x, (m, nc)) for x in fresh.trades())
    finally:
        be.close()
        if fresh is not None:
            fresh.close()
    Ri, Ro, g, al = Rr[q, ci], Rr[q, co], b.γ, b.α
    lb, srho = np.log(b.β), P.sum_logs(Rr)
    cond, gr = fd_cond(lambda ri, ro, lp, gg, aa: P.q_curve(ri, ro, 0.0, al, lp, gg, aa), [Ri, Ro, lb - srho, g, a])
    cond = cond - np.abs((lb - srho) * gr[2]) + (np.abs(lb) + np.sum(np.abs(np.log(Rr)), axis=1)) * np.abs(gr[2])
    tol = (2 * S.family_K("curve") + 1) * U * (Ro + qb + cond)
    worst_q = float(np.max(np.abs(qa - qb) / tol))
    bD, bL = CP.scale(c, rows)
    r = CP.ratios(DA, LA, DB, LB, bD + CP.U * np.abs(DB), bL + CP.U * np.abs(LB))
    print(f"\n[swap refresh] curve3: quotes worst {worst_q:.3g} of the tolerance; sweeps worst ratio {float(np.max(r)):.3g} of K = {T.K_UPDATE}")
    assert worst_q <= 1.0 and np.all(r <= T.K_UPDATE) and np.count_nonzero(DA) > m // 8


# ---- UniV3 ------------------------------------------------------------------------------------------------------------------------------
def exact_ladder():
    """three ticks with upper prices 4, 1, 1/4 and liquidity k = 16 each: every root the preparation takes of a tick EDGE is
    exact (√(16/4) = 2, √(16·1) = 4, ...), so the far edge of the first tick, s' = s_in + δmax = 4 + 4, gives
    P = 64/16 = 4 exactly -- the first tick's upper price, whatever rounding the current price brings"""
    return cr.PoolBatch(KIND_UNIV3, current_price=np.array([0.6, 0.6]), tick_off=np.array([0, 3, 6]),
                        lower_ticks=np.array([4.0, 1.0, 0.25] * 2), liquidity=np.full(6, 16.0), γ=np.array([0.997, 1.0]),
                        Ai=np.array([[1, 2], [2, 3]]))


def test_univ3_exhausting_swap_rests_at_the_first_ticks_upper_price():
    b = exact_ladder()
    be = backend([b])
    try:
        ctx = be.ctx
        whole = ctx.quote(0, [1e9, 1e9], 1)
        out = ctx.swap(0, [1e9, 1e9], 1)
        np.testing.assert_array_equal(bits(out), bits(whole))
        np.testing.assert_array_equal(ctx.prices(0, 2), [4.0, 4.0])
        after = ctx.quote(0, [1.0, 1e9], 1)
        assert np.all(bits(after) == 0)                               # +0.0: nothing is left on that side
        assert np.all(ctx.quote(0, [1.0, 1.0], 0) > 0)                  # ... and the other side has it all
        assert_equals_fresh(be, [batch_with(b, current_price=np.array([4.0, 4.0]))])
    finally:
        be.close()


def test_univ3_prices_move_the_right_way_and_zero_amount_stays():
    m = 64
    b = pools("univ3", m, seed=151)
    ci, _, a = typical_queries(b, m, seed=7)
    a[5] = 0.0
    be = backend([b])
    try:
        out = be.ctx.swap(0, a, ci)
        p = be.ctx.prices(0, m)
    finally:
        be.close()
    moved = out > 0
    assert moved.sum() >= m // 2
    assert np.all(p[moved & (ci == 0)] < b.current_price[moved & (ci == 0)])          # coin 0 in: the price falls
    assert np.all(p[moved & (ci == 1)] > b.current_price[moved & (ci == 1)])          # coin 1 in: it rises
    assert bits(p)[5] == bits(b.current_price)[5]
    top = b.lower_ticks[b.tick_off[:-1]]
    assert np.all(p <= top) and np.all(p > 0)


# ---- order ------------------------------------------------------------------------------------------------------------------------------
ORDER_ROWS = np.array([5, 2, 5, 7, 5, 2], dtype=np.int64)


def order_batch(b, seed=8):
    nc = b.Ai.shape[1]
    ci_all, co_all, a_all = typical_queries(b, len(b), seed=seed)
    ci = np.array([0, 1, 1, 0, 0, 0], dtype=np.int32)                  # row 5: coin 0, coin 1, coin 0 -- a direction reversal
    co = None if co_all is None else np.array([1, 2 % nc, 0, 1, nc - 1, 1], dtype=np.int32)
    if co is not None:
        co = np.where(co == ci, (ci + 1) % nc, co).astype(np.int32)
    scale = a_all[ORDER_ROWS] / np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    a = scale * np.array([0.05, 0.02, 0.08, 0.03, 0.04, 0.06])
    return ci, co, a


@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
@pytest.mark.parametrize("device", (0, [0, 0]), ids=("single", "multi"))
def test_a_batch_with_repeated_rows_equals_single_swaps_in_that_order(kind, nc, device):
    m = 16
    b = pools(kind, m, seed=161, n_coins=nc)
    ci, co, a = order_batch(b)
    one, batch = backend([b]), backend([b], device=device)
    try:
        singles = np.array([one.ctx.swap(0, a[q:q + 1], ci[q:q + 1], None if co is None else co[q:q + 1], ORDER_ROWS[q:q + 1])[0]
                            for q in range(6)])
        got = batch.ctx.swap(0, a, ci, co, ORDER_ROWS)
        np.testing.assert_array_equal(bits(got), bits(singles))
        np.testing.assert_array_equal(bits(state(batch.ctx, b)), bits(state(one.ctx, b)))
        assert np.all(np.isfinite(got)) and got[2] > 0 and got[4] > 0
        # the repeated row was swapped from the state its previous swap left, not from the first one
        first = backend([b])
        try:
            fresh_q = first.ctx.quote(0, a, ci, co, ORDER_ROWS)
        finally:
            first.close()
        assert bits(got)[0] == bits(fresh_q)[0] and bits(got)[2] != bits(fresh_q)[2] and bits(got)[4] != bits(fresh_q)[4]
    finally:
        one.close()
        batch.close()


# ---- path independence ----------------------------------------------------------------------------------------------------------------
def quote_units(kind, b, R, rows, ci, co, a):
    """per row: (unit = R_o + out + cond, cond, |∂q/∂R_o|) of the quote of `a` on reserves R, by finite differences on
    quote_precise_ref's numpy restatement (as tests/test_gpu_quote.py's round trip computes its conditioning)"""
    Ri, Ro, g = R[rows, ci], R[rows, co], b.γ[rows]
    if kind == "product":
        fn, xs = P.q_product, [Ri, Ro, g, a]
    elif kind == "solidly":
        fn, xs = P.q_solidly, [Ri, Ro, g, a]
    elif kind in ("geomean", "weighted"):
        w = b.w / b.w.sum(axis=1, keepdims=True)
        fn, xs = P.q_weighted, [Ri, Ro, w[rows, ci], w[rows, co], g, a]
    else:
        lb, srho, al = np.log(b.β[rows]), P.sum_logs(R[rows]), b.α[rows]
        fn = lambda ri, ro, lp, gg, aa: P.q_curve(ri, ro, 0.0, al, lp, gg, aa)
        xs = [Ri, Ro, lb - srho, g, a]
    cond, gr = fd_cond(fn, xs)
    if kind == "curve":
        cond = cond - np.abs((lb - srho) * gr[2]) + (np.abs(lb) + np.sum(np.abs(np.log(R[rows])), axis=1)) * np.abs(gr[2])
    out = fn(*xs)
    return Ro + out + cond, cond, np.abs(gr[1])


@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
def test_two_swaps_give_what_one_quote_of_the_sum_gives(kind, nc):
    """swap(a1) then swap(a2), same pool and direction, against quote(a1 + a2) on an untouched twin: exactly equal in real
    arithmetic (φ is conserved and the fee is on the input); in doubles within swap_precise_ref.path_tolerance"""
    m = 32
    b = pools(kind, m, seed=171, n_coins=nc)
    ci, co, a1 = typical_queries(b, m, seed=9)
    a2 = a1 * (0.3 + synth.uniform(172, 4, m))
    rows = np.arange(m)
    cof = full_co(b, ci, co)
    be, twin = backend([b]), backend([b])
    try:
        o1 = be.ctx.swap(0, a1, ci, co)
        mid = state(be.ctx, b)
        o2 = be.ctx.swap(0, a2, ci, co)
        q12 = twin.ctx.quote(0, a1 + a2, ci, co)
    finally:
        be.close()
        twin.close()
    K = S.family_K(kind)
    if kind == "univ3":
        prep = lambda cp, i: P.univ3_prepare(cp, b.lower_ticks[b.tick_off[i]:b.tick_off[i + 1]], b.liquidity[b.tick_off[i]:b.tick_off[i + 1]])
        tol = np.empty(m)
        for i in range(m):
            u1 = sum(P.univ3_unit(prep(b.current_price[i], i), float(b.γ[i]), int(ci[i]), float(a1[i])))
            s2, c2 = P.univ3_unit(prep(mid[i], i), float(b.γ[i]), int(ci[i]), float(a2[i]))
            u12 = sum(P.univ3_unit(prep(b.current_price[i], i), float(b.γ[i]), int(ci[i]), float(a1[i] + a2[i])))
            tol[i] = S.path_tolerance(K, U * (u1 + o1[i]), U * (s2 + c2 + o2[i]), U * (u12 + q12[i]), S.carried_univ3(c2), o1[i], o2[i])
    else:
        u1, _, _ = quote_units(kind, b, b.R, rows, ci, cof, a1)
        u2, c2, g2 = quote_units(kind, b, mid, rows, ci, cof, a2)
        u12, _, _ = quote_units(kind, b, b.R, rows, ci, cof, a1 + a2)
        tol = S.path_tolerance(K, U * u1, U * u2, U * u12, S.carried(K, U * u1, c2, g2, mid[rows, cof]), o1, o2)
    err = np.abs((o1 + o2) - q12)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.where(tol > 0, tol, 1e-300))))
    print(f"\n[path independence] {kind}{nc}: worst |out1 + out2 − quote(a1 + a2)| / tolerance = {worst:.3g} (K = {K})")
    assert np.all(np.isfinite(o1 + o2)) and worst <= 1.0


# ---- a refused swap ---------------------------------------------------------------------------------------------------------------------
def test_a_swap_that_would_empty_a_product_pool_is_refused():
    m = 8
    b = pools("product", m, seed=181)
    rows = np.array([1, 3, 3, 4, 3], dtype=np.int64)
    ci = np.zeros(5, dtype=np.int32)
    a = 0.01 * b.R[rows, 0]
    a[1] = 1e30 * b.R[3, 0]                                           # x/(R_i + x) rounds to 1: out = R_o, nothing would be left
    be, twin = backend([b]), backend([b])
    try:
        before = twin.ctx.quote(0, a, ci, None, rows)
        out = be.ctx.swap(0, a, ci, None, rows)
        assert be.ctx.get_option("swap_refused") == 1
        R = be.ctx.reserves(0, m)
        assert np.isnan(out[1]) and np.all(np.isfinite(out[[0, 2, 3, 4]]))
        assert before[1] == b.R[3, 1]
        # the later swaps of row 3 proceed from the unchanged pool: the first is the twin's quote, the second follows it
        assert bits(out)[2] == bits(before)[2] and out[4] < out[2]
        np.testing.assert_array_equal(bits(out[[0, 3]]), bits(before[[0, 3]]))
        want = b.R.copy()
        want[1] = [b.R[1, 0] + b.γ[1] * a[0], b.R[1, 1] - out[0]]
        want[4] = [b.R[4, 0] + b.γ[4] * a[3], b.R[4, 1] - out[3]]
        r3 = [b.R[3, 0] + b.γ[3] * a[2], b.R[3, 1] - out[2]]
        want[3] = [r3[0] + b.γ[3] * a[4], r3[1] - out[4]]
        np.testing.assert_array_equal(bits(R), bits(want))
        # alone in a call: the pool's bits are unchanged
        alone = twin.ctx.swap(0, a[1:2], ci[1:2], None, rows[1:2])
        assert np.isnan(alone[0]) and twin.ctx.get_option("swap_refused") == 1
        np.testing.assert_array_equal(bits(twin.ctx.reserves(0, m)), bits(b.R))
        twin.ctx.swap(0, a[:1], ci[:1], None, rows[:1])
        assert twin.ctx.get_option("swap_refused") == 0               # the count is the latest call's
    finally:
        be.close()
        twin.close()


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_names_the_query_and_changes_nothing():
    L = cr.lib()
    b, w, u = pools("product", 50, 191), pools("weighted", 50, 192), pools("univ3", 50, 193)
    be = backend([b, w, u])
    try:
        ctx = be.ctx
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        snap = lambda: [bits(ctx.reserves(0, 50)), bits(ctx.reserves(1, 50, 3)), bits(ctx.prices(2, 50))]
        was = snap()
        ci, _, a = typical_queries(b, 10)
        idx = np.arange(10, dtype=np.int64)

        def refused(match, seg=0, idx=idx, ci=ci, co=None, a=a):
            out = np.full(a.size, 7.0)
            rc = L.cfmm_swap(ctx._h, seg, a.size, ptr(idx), ptr(np.ascontiguousarray(ci, dtype=np.int32)),
                             ptr(None if co is None else np.ascontiguousarray(co, dtype=np.int32)), ptr(np.ascontiguousarray(a)), ptr(out))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and msg.startswith("cfmm_swap:") and match in msg, (rc, msg)
            assert np.all(out == 7.0)
        bad = idx.copy(); bad[4] = 50
        refused("query 4", idx=bad)
        bad = idx.copy(); bad[9] = -1
        refused("query 9", idx=bad)
        bad = ci.copy(); bad[3] = 2
        refused("query 3", ci=bad)
        refused("query 2", co=np.where(np.arange(10) == 2, ci, 1 - ci))
        for k, x in ((5, -1.0), (6, np.nan), (0, np.inf)):
            bad = a.copy(); bad[k] = x
            refused(f"query {k}", a=bad)
            refused(f"query {k}", seg=2, a=bad)
        refused("segment", seg=3)
        refused("coin_out is required", seg=1)
        for x, y in zip(snap(), was):
            np.testing.assert_array_equal(x, y)
        assert_same([np.asarray(x) for x in be.trades()], trades)         # the earlier trades are still readable
    finally:
        be.close()


# ---- the state protocol -----------------------------------------------------------------------------------------------------------------
def test_a_swap_invalidates_earlier_trades_and_the_next_sweep_sees_the_moved_pools():
    m = 64
    b = pools("product", m, seed=201)
    ci, _, a = typical_queries(b, m, seed=10)
    be = backend([b])
    fresh = None
    try:
        ctx = be.ctx
        be.find_arb(V)
        before = [np.array(x, copy=True) for x in be.trades()]
        empty = ctx.swap(0, a[:0], ci[:0])                               # count == 0 invalidates nothing
        assert empty.size == 0
        assert_same([np.asarray(x) for x in be.trades()], before)
        ctx.swap(0, a, ci)
        with pytest.raises(Exception, match="no materialised trades"):
            ctx.trades()
        now = batch_with(b, R=ctx.reserves(0, m))
        be.find_arb(V)
        after = [np.array(x, copy=True) for x in be.trades()]
        assert np.any(after[0] != before[0])
        fresh = backend([now])
        fresh.find_arb(V)
        assert_same(after, [np.asarray(x) for x in fresh.trades()])
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


def test_swaps_need_no_sweep_and_time_their_kernels():
    b = pools("geomean", 40, seed=211)
    ci, _, a = typical_queries(b, 40, seed=11)
    be = backend([b])
    try:
        be.ctx.set_option("time_kernels", 1)
        assert be.ctx.get_option("swap_ns") == 0
        be.ctx.swap(0, np.concatenate([a, a]), np.concatenate([ci, ci]), None, np.concatenate([np.arange(40), np.arange(40)]))
        assert be.ctx.get_option("swap_ns") > 0                           # two waves, both timed
    finally:
        be.close()


# ---- the fast window --------------------------------------------------------------------------------------------------------------------
def test_a_reserve_that_leaves_the_fast_window_sends_the_segment_to_full_range_arithmetic():
    """R_out = 2^-120 and x = 2^40·R_in: x/(R_in + x) = 1 − 2^-40 to rounding, so R_out' = R_out − out is about 2^-160 -- a valid
    reserve outside [2^-150, 2^150].  (The other side cannot leave upwards: an x large enough rounds the ratio to 1 and the swap is
    refused.)"""
    m = 8
    b0 = pools("product", m, seed=221)
    R = b0.R.copy()
    R[2] = [1.0, 2.0 ** -120]
    b = batch_with(b0, R=R)
    be = backend([b])
    try:
        out = be.ctx.swap(0, [2.0 ** 40 / b.γ[2]], 0, None, [2])
        Rn = be.ctx.reserves(0, m)
        assert np.isfinite(out[0]) and 0 < Rn[2, 1] < 2.0 ** -150
        assert_equals_fresh(be, [batch_with(b, R=Rn)])
        assert_equals_fresh(be, [batch_with(b, R=Rn)], v=V2)
    finally:
        be.close()


# ---- the Python front end -----------------------------------------------------------------------------------------------------------
def test_swap_through_a_router_on_a_mixed_market():
    """Product + UniV3 + Curve pools given as a list, interleaved: after swap_ the host mirror equals the device, and the next
    route_ runs on the moved market"""
    n = 6
    u = exact_ladder()
    pools = [cr.ProductTwoCoin([1e4, 2e4], 0.997, [1, 2]),
             cr.UniV3(0.6, u.lower_ticks[:3], u.liquidity[:3] * 1e4, 0.997, [2, 3]),
             cr.Curve([1e4, 1.1e4, 0.9e4], 0.9995, [1, 3, 4], 2.0, 1e16),
             cr.ProductTwoCoin([3e4, 1e4], 0.997, [3, 5]),
             cr.UniV3(2.25, u.lower_ticks[:3], u.liquidity[:3] * 1e4, 1.0, [4, 6]),
             cr.ProductTwoCoin([5e3, 5e3], 0.997, [5, 6])]
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), pools, n)
    try:
        cr.route_(r, solver="native")
        before = [np.array(x, copy=True) for x in r.Δs]
        which = [3, 1, 2, 3, 4, 0]
        cin = [0, 1, 0, 1, 0, 1]
        cout = [1, 0, 2, 0, 1, 0]
        amt = [500.0, 30.0, 200.0, 100.0, 40.0, 700.0]
        quoted = cr.quote(r, [3, 1, 2, 4, 0], [0, 1, 0, 0, 1], [500.0, 30.0, 200.0, 40.0, 700.0], [1, 0, 2, 1, 0])
        out = cr.swap_(r, which, cin, amt, cout)
        np.testing.assert_array_equal(bits(out[[0, 1, 2, 4, 5]]), bits(quoted))          # first visits: the quote's bits
        assert np.all(np.isfinite(out)) and np.all(out > 0)
        assert all(np.all(np.asarray(x) == 0) for x in r.Δs)                             # the old trades are gone
        ctx, L = r._backend.ctx, r._layout
        for i, p in enumerate(pools):                                                    # the host mirror equals the device
            _, b, row = L.locate(i)
            seg, batch = L.seg_of[b], L.batches[b]
            if isinstance(p, cr.UniV3):
                assert p.current_price == ctx.prices(seg, len(batch))[row] == batch.current_price[row]
            else:
                np.testing.assert_array_equal(bits(p.R), bits(ctx.reserves(seg, len(batch), len(p.R))[row]))
        assert pools[3].R[0] == (3e4 + 0.997 * 500.0) - out[3] and pools[1].current_price > 0.6 and pools[4].current_price < 2.25
        cr.route_(r, solver="native")
        after = [np.array(x, copy=True) for x in r.Δs]
        assert any(np.any(a != b) for a, b in zip(after, before))
    finally:
        r.close()


def test_backrun_example(capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import backrun
    before, after, got, victim = backrun.main()
    out = capsys.readouterr().out
    assert "back-run after the swaps" in out
    assert victim[-1] == victim[0] and got[-1] < got[0] * 1.0 and np.all(got > 0)      # the second swap of a pool yields less
    assert after > before and after > 0
