"""cfmm_swap_out on the device: the answer carries cfmm_quote_out's bits, the pool gives exactly the amount asked for
(R_in + γ·in, R_out − want; UniV3: where cfmm_swap of the answer leaves it), repeated rows are applied in query order, every
swap has a status, and the call is a state change with cfmm_swap's protocol.  m = 1025 pools per segment: four blocks and a
lane.  The 80-digit sequences are in tests/test_gpu_swap_out_precise.py."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_out_precise_ref as QO
import quote_precise_ref as Q
import swap_out_precise_ref as SO
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE, ptr
from test_gpu_pool_update import assert_same, batch_with, outputs
from test_gpu_quote import N, fd_cond, pools, typical_queries
from test_gpu_swap import CASES, IDS, ORDER_ROWS, RESERVE, RIDS, V, V2, backend, bits, full_co, order_batch, state, with_state

pytestmark = pytest.mark.gpu

M = 1025
U = 2.0 ** -53


def wanted(b, m, seed=1, frac=0.5):
    """(coin_in, coin_out, want) for rows 0 .. m-1: `frac` of what a typical tender yields on the pools as uploaded"""
    ci, co, a = typical_queries(b, m, seed)
    be = backend([b])
    try:
        return ci, co, frac * be.ctx.quote(0, a, ci, co)
    finally:
        be.close()


# ---- the same bits as the quote ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
def test_swap_out_answers_with_the_bits_of_quote_out(kind, nc):
    b = pools(kind, M, seed=301, n_coins=nc)
    ci, co, w = wanted(b, M, seed=2)
    perm = np.argsort(synth.uniform(302, 3, M)).astype(np.int64)
    for idx, sl in ((None, np.arange(M)), (perm, perm), (np.arange(64, dtype=np.int64), np.arange(64))):
        be = backend([b])
        try:
            args = (w[sl], ci[sl], None if co is None else co[sl], idx)
            q = be.ctx.quote_out(0, *args)
            s, st = be.ctx.swap_out(0, *args, status=True)
            assert np.all(np.isfinite(q)) and np.all(st == SWAP_APPLIED)
            np.testing.assert_array_equal(bits(s), bits(q))
            assert be.ctx.get_option("swap_refused") == 0 and be.ctx.get_option("swap_launches") == 1
            assert np.any(bits(be.ctx.quote_out(0, *args)) != bits(q))      # ... and the pools have moved
        finally:
            be.close()


# ---- the new state, reserve kinds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", RESERVE, ids=RIDS)
def test_new_reserves_are_exactly_R_plus_gamma_in_and_R_minus_want(kind, nc):
    b = pools(kind, M, seed=311, n_coins=nc)
    ci, co, w = wanted(b, M, seed=3)
    rows = np.arange(1, M, 3, dtype=np.int64)                          # a sparse subset: the other pools keep every bit
    w[rows[0]] = 0.0                                                  # ... and so does a pool asked for nothing
    cof = full_co(b, ci, co)
    be, twin = backend([b]), backend([b])
    try:
        a = be.ctx.swap_out(0, w[rows], ci[rows], None if co is None else co[rows], rows)
        R = be.ctx.reserves(0, M, b.Ai.shape[1])
        back = twin.ctx.quote(0, a, ci[rows], None if co is None else co[rows], rows)   # what tendering the answer would yield
    finally:
        be.close()
        twin.close()
    want = b.R.copy()
    want[rows, ci[rows]] = b.R[rows, ci[rows]] + b.γ[rows] * a          # each operation rounded on its own
    want[rows, cof[rows]] = b.R[rows, cof[rows]] - w[rows]              # the amount asked for, not quote(a)
    np.testing.assert_array_equal(bits(R), bits(want))
    assert a[0] == 0.0 and not np.signbit(a[0]) and np.all(a[1:] > 0)
    differ = np.flatnonzero(bits(back) != bits(w[rows]))
    assert differ.size > 0                                             # quote(quote_out(want)) is not want, bit for bit ...
    j = differ[0]
    assert R[rows[j], cof[rows[j]]] == b.R[rows[j], cof[rows[j]]] - w[rows[j]]   # ... and the pool gave want


# ---- a fresh upload of the state the swaps left ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("product", "solidly", "univ3"))
def test_after_swaps_the_context_equals_a_fresh_upload(kind):
    b = pools(kind, M, seed=321)
    ci, co, w = wanted(b, M, seed=4)
    ci_t, _, a_t = typical_queries(b, M, seed=4)
    be = backend([b])
    fresh = None
    try:
        be.ctx.swap_out(0, w, ci, co)
        now = with_state(b, state(be.ctx, b))
        orig = b.current_price if kind == "univ3" else b.R
        assert np.sum(np.any(bits(state(be.ctx, b)).reshape(M, -1) != bits(orig).reshape(M, -1), axis=1)) >= M // 2
        fresh = backend([now])
        for c in (ci, 1 - ci):
            np.testing.assert_array_equal(bits(be.ctx.quote(0, a_t, c)), bits(fresh.ctx.quote(0, a_t, c)))
            qo = be.ctx.quote(0, a_t, c) * 0.5
            np.testing.assert_array_equal(bits(be.ctx.quote_out(0, qo, c)), bits(fresh.ctx.quote_out(0, qo, c)))
        for v in (V, V2):
            assert_same(outputs(be, [now], v), outputs(fresh, [now], v))
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


# ---- the prepared constants the swap refreshed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", [("geomean", 2), ("weighted", 3), ("weighted", 8)], ids=["geomean", "weighted3", "weighted8"])
def test_refreshed_constants_against_a_fresh_upload_weighted(kind, nc):
    """quotes read only R and w: bit-identical.  The sweeps read the constants swap_out_kernel refreshed on the device ({Q1, Q2},
    q = log(R/w): the device's log where the upload used the host's), so they are held to the bound the project uses for the
    same comparison after cfmm_update_reserves and after cfmm_swap (tests/test_gpu_swap.py): precise_ref's scales at K_UPDATE.
    weighted: a stale q = log(R/w) -- the reserves moved by up to a tenth -- misses that bound by fourteen orders of magnitude
    (measured with the stores taken out of the kernel).  GeometricMean: {Q1, Q2} = log(γη) + log(R2·R1^η), η·log(γ/η) +
    log(R2·R1^η) are functions of the pool's INVARIANT, which a swap conserves, so a refreshed pair differs from the pair
    before the swap by rounding only: this case holds a WRONG store (another row, the coins exchanged, a stale reserve in the
    expression) to the bound, but no bound from an error analysis can tell a missing store from a made one (1.9 of K = 4
    measured without it).  The expression itself is pinned bit for bit on the host build
    (tests/test_swap_out_precise_cpu.py test_refreshed_constants_are_swap_pool_h_expressions_of_the_new_reserves)."""
    import precise_ref as PR
    from test_gpu_swap import sweep_bound_two
    m = 64
    b = pools(kind, m, seed=131, n_coins=nc)
    ci, co, w = wanted(b, m, seed=5)
    _, _, a_t = typical_queries(b, m, seed=5)
    v = synth.sweep_prices(N, seed=132, spread=0.3)
    be = backend([b])
    fresh = None
    try:
        _, st = be.ctx.swap_out(0, w, ci, co, status=True)
        assert np.all(st == SWAP_APPLIED)
        Rr = be.ctx.reserves(0, m, b.Ai.shape[1])
        assert np.all(np.any(bits(Rr) != bits(b.R), axis=1))
        fresh = backend([batch_with(b, R=Rr)])
        np.testing.assert_array_equal(bits(be.ctx.quote(0, a_t, ci, co)), bits(fresh.ctx.quote(0, a_t, ci, co)))
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
    print(f"\n[swap_out refresh] {kind}{nc}: refreshed vs fresh upload, worst ratio {float(np.max(r)):.3g} of K = {K}")
    assert np.all(r <= K) and np.count_nonzero(DA) > m // 4


@pytest.mark.parametrize("kind,nc", [("geomean", 2), ("weighted", 3), ("weighted", 8), ("curve", 3)], ids=["geomean", "weighted3", "weighted8", "curve3"])
def test_refreshed_constants_are_those_of_the_one_hop_path(kind, nc):
    """swap_out_kernel and pass 2 of swap_path_out_kernel leave the same reserves (bit for bit: the path tests) and refresh
    the constants with the same device functions of them, so two contexts -- one moved by swap_out, one by the same swaps as
    one-hop paths -- must agree in EVERY bit of every output of a sweep, which reads those constants: no tolerance.  This is
    what sees a store that is missing from one of the two kernels, GeometricMean's {Q1, Q2} included (a pair left from before
    the swap differs from a refreshed one by rounding only, see above, and that is a difference in bits)."""
    m = M
    b = pools(kind, m, seed=141, n_coins=nc)
    ci, co, w = wanted(b, m, seed=6)
    cof = full_co(b, ci, co)
    v = synth.sweep_prices(N, seed=142, spread=0.3)
    one, path = backend([b]), backend([b])
    try:
        a, st = one.ctx.swap_out(0, w, ci, co, status=True)
        ap, stp = path.ctx.swap_path_out(np.ones(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.arange(m, dtype=np.int64), ci, cof, w)
        assert np.all(st == SWAP_APPLIED) and np.all(stp == SWAP_APPLIED)
        np.testing.assert_array_equal(bits(a), bits(ap))
        now = batch_with(b, R=one.ctx.reserves(0, m, b.Ai.shape[1]))
        assert np.all(np.any(bits(now.R) != bits(b.R), axis=1))
        got, want = outputs(one, [now], v), outputs(path, [now], v)
        assert_same(got, want)
        assert np.count_nonzero(got[4]) > m // 4                          # ... of a sweep in which pools trade
    finally:
        one.close()
        path.close()


def test_refreshed_constants_against_a_fresh_upload_curve():
    """Curve: q = log R of the two coins that moved is refreshed with the device's log, the fresh upload prepares it with the
    host's.  The sweeps are held to the bound of the same comparison after cfmm_update_reserves and after cfmm_swap
    (tests/test_gpu_swap.py's test of the same name): curve_precise_ref.scale of the 60-digit fixture's 3-coin pools -- the
    swaps take 1% of a reserve, so the moved pools are within a trade of them -- at tests/test_gpu_curve_precise.py's K_UPDATE."""
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
    w = 0.01 * b.R[q, co]
    n = len(c["v"])
    be = cr.DeviceBackend(n, [b])
    fresh = None
    try:
        a, st = be.ctx.swap_out(0, w, ci, co, status=True)
        ok = st == SWAP_APPLIED                                          # (a pool at the edge of the solve's range may refuse)
        assert ok.sum() >= m - 8 and np.all(np.isfinite(a[ok]))
        Rr = be.ctx.reserves(0, m, nc)
        assert np.all(Rr[q[ok], co[ok]] == b.R[q[ok], co[ok]] - w[ok])
        fresh = cr.DeviceBackend(n, [T._batch(c, rows, R=Rr)])
        be.find_arb(c["v2"])
        fresh.find_arb(c["v2"])
        DA, LA = (np.reshape(x, (m, nc)) for x in be.trades())
        DB, LB = (np.reshape(x, (m, nc)) for x in fresh.trades())
    finally:
        be.close()
        if fresh is not None:
            fresh.close()
    bD, bL = CP.scale(c, rows)
    r = CP.ratios(DA, LA, DB, LB, bD + CP.U * np.abs(DB), bL + CP.U * np.abs(LB))
    print(f"\n[swap_out refresh] curve3: sweeps worst ratio {float(np.max(r)):.3g} of K = {T.K_UPDATE}")
    assert np.all(r <= T.K_UPDATE) and np.count_nonzero(DA) > m // 8


def test_univ3_rests_where_swap_of_the_answer_rests():
    b = pools("univ3", M, seed=331)
    ci, _, w = wanted(b, M, seed=5)
    w[7] = 0.0
    be, twin = backend([b]), backend([b])
    try:
        a, st = be.ctx.swap_out(0, w, ci, status=True)
        assert np.all(st == SWAP_APPLIED) and np.all(np.isfinite(a))
        twin.ctx.swap(0, a, ci)
        p = be.ctx.prices(0, M)
        np.testing.assert_array_equal(bits(p), bits(twin.ctx.prices(0, M)))
    finally:
        be.close()
        twin.close()
    moved = a > 0
    assert moved.sum() >= M // 2 and bits(p)[7] == bits(b.current_price)[7]
    assert np.all(p[moved & (ci == 0)] < b.current_price[moved & (ci == 0)])          # coin 0 in: the price falls
    assert np.all(p[moved & (ci == 1)] > b.current_price[moved & (ci == 1)])          # coin 1 in: it rises


# ---- order ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
@pytest.mark.parametrize("device", (0, [0, 0]), ids=("single", "multi"))
def test_a_batch_with_repeated_rows_equals_single_swaps_in_that_order(kind, nc, device):
    m = 16
    b = pools(kind, m, seed=161, n_coins=nc)                           # (tests/test_gpu_swap.py's market of the same test)
    ci, co, a = order_batch(b)
    q = backend([b])
    try:
        w = 0.3 * q.ctx.quote(0, a, ci, co, ORDER_ROWS)                   # outputs the pool can give three times over
        fresh_q = q.ctx.quote_out(0, w, ci, co, ORDER_ROWS)
    finally:
        q.close()
    one, batch = backend([b]), backend([b], device=device)
    try:
        singles = np.array([one.ctx.swap_out(0, w[j:j + 1], ci[j:j + 1], None if co is None else co[j:j + 1], ORDER_ROWS[j:j + 1])[0]
                            for j in range(6)])
        got, st = batch.ctx.swap_out(0, w, ci, co, ORDER_ROWS, status=True)
        np.testing.assert_array_equal(bits(got), bits(singles))
        np.testing.assert_array_equal(bits(state(batch.ctx, b)), bits(state(one.ctx, b)))
        assert np.all(st == SWAP_APPLIED) and np.all(np.isfinite(got)) and got[2] > 0 and got[4] > 0
        if device == 0:
            assert batch.ctx.get_option("swap_launches") == 3             # row 5 is named three times
        # the repeated row was swapped from the state its previous swap left, not from the first one
        assert bits(got)[0] == bits(fresh_q)[0] and bits(got)[2] != bits(fresh_q)[2] and bits(got)[4] != bits(fresh_q)[4]
    finally:
        one.close()
        batch.close()


# ---- path independence ----------------------------------------------------------------------------------------------------------------
def out_units(kind, b, R, rows, ci, co, o):
    """per row: (unit = R_i/γ + a + cond, |∂a/∂R_in|, |∂a/∂R_out|) of the exact-output quote of `o` on reserves R, by centred
    differences on quote_out_precise_ref's numpy restatement (as tests/test_gpu_quote_out.py's round trip computes them)"""
    Ri, Ro, g = R[rows, ci], R[rows, co], b.γ[rows]
    logs = None
    if kind == "product":
        fn, xs = QO.qo_product, [Ri, Ro, g, o]
    elif kind == "solidly":
        fn, xs = QO.qo_solidly, [Ri, Ro, g, o]
    elif kind in ("geomean", "weighted"):
        w = b.w / b.w.sum(axis=1, keepdims=True)
        fn, xs = QO.qo_weighted, [Ri, Ro, w[rows, ci], w[rows, co], g, o]
    else:
        lb, srho, al = np.log(b.β[rows]), Q.sum_logs(R[rows]), b.α[rows]
        fn = lambda ri, ro, lp, gg, oo: QO.qo_curve(ri, ro, 0.0, al, lp, gg, oo)
        xs = [Ri, Ro, lb - srho, g, o]
        logs = np.abs(lb) + np.sum(np.abs(np.log(R[rows])), axis=1)
    with np.errstate(all="ignore"):
        cond, gr = fd_cond(fn, xs)
        dRi, dRo = np.abs(gr[0]), np.abs(gr[1])
        if logs is not None:                                           # log P₀ stands for log β and every log R_k the device holds,
            cond = cond - np.abs(xs[2] * gr[2]) + logs * np.abs(gr[2])
            dRi, dRo = dRi + np.abs(gr[2]) / Ri, dRo + np.abs(gr[2]) / Ro   # ... and moves with the two reserves
        a = fn(*xs)
    return Ri / g + a + cond, dRi, dRo


@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
def test_two_swap_outs_cost_what_one_quote_of_the_sum_costs(kind, nc):
    """swap_out(w1) then swap_out(w2), same pool and direction, against quote_out(w1 + w2) on an untouched twin: exactly equal
    in real arithmetic (φ is conserved and the fee is on the input); in doubles within swap_out_precise_ref.path_tolerance"""
    m = 32
    b = pools(kind, m, seed=171, n_coins=nc)
    ci, co, w12 = wanted(b, m, seed=9, frac=0.6)
    w1 = w12 * (0.3 + 0.4 * synth.uniform(172, 4, m))
    w2 = w12 - w1
    rows = np.arange(m)
    cof = full_co(b, ci, co)
    be, twin = backend([b]), backend([b])
    try:
        a1 = be.ctx.swap_out(0, w1, ci, co)
        mid = state(be.ctx, b)
        a2 = be.ctx.swap_out(0, w2, ci, co)
        q12 = twin.ctx.quote_out(0, w1 + w2, ci, co)
    finally:
        be.close()
        twin.close()
    K = SO.family_K(kind)
    if kind == "univ3":
        prep = lambda cp, i: Q.univ3_prepare(cp, b.lower_ticks[b.tick_off[i]:b.tick_off[i + 1]], b.liquidity[b.tick_off[i]:b.tick_off[i + 1]])
        tol = np.full(m, np.inf)
        for i in range(m):
            if w1[i] == 0.0:                                           # a direction without liquidity: nothing asked, nothing paid
                assert a1[i] == a2[i] == q12[i] == 0.0
                continue
            g, c = float(b.γ[i]), int(ci[i])
            u1 = QO.univ3_unit(prep(b.current_price[i], i), g, c, float(w1[i]))
            pm = prep(mid[i], i)
            u2 = QO.univ3_unit(pm, g, c, float(w2[i]))
            u12 = QO.univ3_unit(prep(b.current_price[i], i), g, c, float(w1[i] + w2[i]))
            s_land = pm[0][1] if c == 0 else pm[0][2]                   # s_in of the tick the first swap landed in, at the landing price
            if None in (u1, u2, u12) or not s_land > 0:
                continue
            un = lambda u, a: U * (u[0] + a + u[1])
            tol[i] = SO.path_tolerance(K, un(u1, a1[i]), un(u2, a2[i]), un(u12, q12[i]),
                                       SO.carried_univ3(K, un(u1, a1[i]), g, s_land, u2[1]), a1[i], a2[i])
        assert np.sum(np.isfinite(tol)) >= m * 3 // 4
    else:
        u1, _, _ = out_units(kind, b, b.R, rows, ci, cof, w1)
        u2, dRi, dRo = out_units(kind, b, mid, rows, ci, cof, w2)
        u12, _, _ = out_units(kind, b, b.R, rows, ci, cof, w1 + w2)
        carry = SO.carried(K, U * u1, b.γ, mid[rows, ci], mid[rows, cof], dRi, dRo)
        tol = SO.path_tolerance(K, U * u1, U * u2, U * u12, carry, a1, a2)
    err = np.abs((a1 + a2) - q12)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.where(tol > 0, tol, 1e-300))))
    print(f"\n[path independence] {kind}{nc}: worst |in1 + in2 − quote_out(w1 + w2)| / tolerance = {worst:.3g} (K = {K})")
    assert np.all(np.isfinite(a1 + a2)) and worst <= 1.0


# ---- each status ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nc", RESERVE, ids=RIDS)
def test_an_amount_the_pool_does_not_hold_is_unobtainable(kind, nc):
    m = 8
    b = pools(kind, m, seed=351, n_coins=nc)
    rows = np.array([1, 3, 3, 4, 3], dtype=np.int64)
    ci = np.zeros(5, dtype=np.int32)
    co = np.ones(5, dtype=np.int32)
    w = 0.01 * b.R[rows, 1]
    w[1] = b.R[3, 1]                                                   # want == R_out: no finite input buys the whole reserve
    be, twin = backend([b]), backend([b])
    try:
        coa = co if kind in ("weighted", "curve") else None
        before = twin.ctx.quote_out(0, w, ci, coa, rows)
        a, st = be.ctx.swap_out(0, w, ci, coa, rows, status=True)
        assert list(st) == [SWAP_APPLIED, SWAP_UNOBTAINABLE, SWAP_APPLIED, SWAP_APPLIED, SWAP_APPLIED]
        assert a[1] == np.inf and before[1] == np.inf and be.ctx.get_option("swap_refused") == 1
        # the later swaps of row 3 proceed from the unchanged pool: the first is the twin's quote, the second follows it
        assert bits(a)[2] == bits(before)[2] and a[4] > a[2]
        alone, st1 = twin.ctx.swap_out(0, w[1:2], ci[1:2], None if coa is None else coa[1:2], rows[1:2], status=True)
        assert alone[0] == np.inf and st1[0] == SWAP_UNOBTAINABLE
        np.testing.assert_array_equal(bits(twin.ctx.reserves(0, m, b.Ai.shape[1])), bits(b.R))
    finally:
        be.close()
        twin.close()


def test_univ3_wanting_more_than_the_ladder_holds_is_unobtainable():
    """rows whose ladder holds something in both directions: more than a direction's total is unobtainable and leaves every
    bit of the price; the later swap of the row -- the other direction -- answers what quote_out answers on an untouched twin"""
    m = 16
    b = pools("univ3", m, seed=361)
    be, twin = backend([b]), backend([b])
    try:
        every = np.arange(m, dtype=np.int64)
        tot = [twin.ctx.quote(0, np.full(m, 1e300), np.full(m, c, dtype=np.int32), None, every) for c in (0, 1)]   # all a direction holds
        both = np.flatnonzero((tot[0] > 0) & (tot[1] > 0))
        assert both.size >= 2
        r0, r1 = int(both[0]), int(both[1])
        rows = np.array([r0, r0, r1, r1], dtype=np.int64)
        ci = np.array([0, 1, 1, 0], dtype=np.int32)
        total = np.array([tot[c][r] for c, r in zip(ci, rows)])
        w = np.where(np.arange(4) % 2 == 0, total * 4.0 + 1.0, 0.25 * total)
        before = twin.ctx.quote_out(0, w, ci, None, rows)
        assert before[0] == before[2] == np.inf and np.all(np.isfinite(before[[1, 3]])) and np.all(before[[1, 3]] > 0)
        # alone in a call: every bit of every price stays
        alone, st1 = be.ctx.swap_out(0, w[[0, 2]], ci[[0, 2]], None, rows[[0, 2]], status=True)
        assert np.all(st1 == SWAP_UNOBTAINABLE) and np.all(alone == np.inf) and be.ctx.get_option("swap_refused") == 2
        np.testing.assert_array_equal(bits(be.ctx.prices(0, m)), bits(b.current_price))
        # in a batch: the later swap of the same row proceeds from the unchanged pool
        a, st = be.ctx.swap_out(0, w, ci, None, rows, status=True)
        assert list(st) == [SWAP_UNOBTAINABLE, SWAP_APPLIED, SWAP_UNOBTAINABLE, SWAP_APPLIED] and a[0] == a[2] == np.inf
        np.testing.assert_array_equal(bits(a[[1, 3]]), bits(before[[1, 3]]))
        assert be.ctx.get_option("swap_refused") == 2 and be.ctx.get_option("swap_launches") == 2
        twin.ctx.swap_out(0, w[[1, 3]], ci[[1, 3]], None, rows[[1, 3]])     # ... and ends where those two swaps alone leave it
        p = be.ctx.prices(0, m)
        np.testing.assert_array_equal(bits(p), bits(twin.ctx.prices(0, m)))
        assert p[r0] > b.current_price[r0] and p[r1] < b.current_price[r1]
    finally:
        be.close()
        twin.close()


@pytest.mark.parametrize("kind,nc", CASES, ids=IDS)
def test_a_limit_one_ulp_below_the_quote_against_a_limit_equal_to_it(kind, nc):
    m = 8
    b = pools(kind, m, seed=371, n_coins=nc)
    ci, co, w = wanted(b, m, seed=6)
    be, twin = backend([b]), backend([b])
    try:
        q = twin.ctx.quote_out(0, w, ci, co)
        assert np.all(np.isfinite(q))
        live = q > 0                                                   # (a UniV3 direction without liquidity yields, and costs, nothing)
        assert live.sum() >= m - 2
        short = live & (np.arange(m) % 2 == 0)                          # even rows: a limit one ulp short; the others: the quote itself
        lim = np.where(short, np.nextafter(q, 0.0), q)
        a, st = be.ctx.swap_out(0, w, ci, co, max_in=lim, status=True)
        np.testing.assert_array_equal(bits(a), bits(q))                  # over the limit: the quote it would have cost
        assert np.all(st[short] == SWAP_OVER_LIMIT) and np.all(st[~short] == SWAP_APPLIED)
        assert be.ctx.get_option("swap_refused") == short.sum()
        now, orig = state(be.ctx, b), (b.current_price if kind == "univ3" else b.R)
        np.testing.assert_array_equal(bits(now[short]), bits(orig[short]))   # those pools keep every bit
        moved = live & ~short
        assert np.all(np.any(bits(now[moved]).reshape(moved.sum(), -1) != bits(orig[moved]).reshape(moved.sum(), -1), axis=1))
        at = np.flatnonzero(short)
        again, st2 = be.ctx.swap_out(0, w[at], ci[at], None if co is None else co[at], at, status=True)
        np.testing.assert_array_equal(bits(again), bits(q[at]))           # a later swap of the row proceeds from the unchanged pool
        assert np.all(st2 == SWAP_APPLIED)
    finally:
        be.close()
        twin.close()


# The inputs of the refused swaps were found on the host build (tests/native/swap_out_host.cpp) and are recorded here:
#   Solidly  R = {1, 2^-140}, γ = 0.997, coin 0 in, want = 2^-140·(1 − 2^-20): R_out' ≈ 2^-160 leaves [2^-150, 2^150] -> REFUSED;
#            want = 2^-141 on the same pool -> APPLIED, in = 0.26070316...
#   Curve    R = {1, 1}, α = 2, β = e^599, γ = 0.9995, coin 0 in, want = 0.9: log(P0/R_out') leaves the solve's range -> REFUSED;
#            want = 0.1 on the same pool -> APPLIED, in = 0.11116669...
REFUSED = {"solidly": dict(R=[1.0, 2.0 ** -140], γ=0.997, want=[2.0 ** -140 * (1 - 2.0 ** -20), 2.0 ** -141], then=0.26070316),
           "curve": dict(R=[1.0, 1.0], γ=0.9995, α=2.0, β=float(np.exp(599.0)), want=[0.9, 0.1], then=0.11116669)}


@pytest.mark.parametrize("kind", ("solidly", "curve"))
def test_a_swap_that_would_leave_an_invalid_pool_is_refused(kind):
    m, row = 8, 3
    c = REFUSED[kind]
    b0 = pools(kind, m, seed=381, n_coins=2)
    R, g = b0.R.copy(), b0.γ.copy()
    R[row], g[row] = c["R"], c["γ"]
    extra = {}
    if kind == "curve":
        al, be_ = b0.α.copy(), b0.β.copy()
        al[row], be_[row] = c["α"], c["β"]
        extra = dict(α=al, β=be_)
    b = batch_with(b0, R=R, γ=g, **extra)
    rows = np.array([row, row, 1], dtype=np.int64)
    ci, co = np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32)
    w = np.array(c["want"] + [0.01 * b.R[1, 1]])
    be = backend([b])
    try:
        a, st = be.ctx.swap_out(0, w, ci, co, rows, status=True)
        assert list(st) == [SWAP_REFUSED, SWAP_APPLIED, SWAP_APPLIED] and np.isnan(a[0])
        assert a[1] == pytest.approx(c["then"], rel=1e-6)               # ... from the unchanged pool
        assert be.ctx.get_option("swap_refused") == 1
        Rn = be.ctx.reserves(0, m, 2)
        assert Rn[row, 0] == np.float64(c["R"][0]) + np.float64(c["γ"]) * a[1] and Rn[row, 1] == c["R"][1] - w[1]
    finally:
        be.close()
    fresh = backend([b])
    try:                                                               # alone in a call: the pool's bits are unchanged
        a1, s1 = fresh.ctx.swap_out(0, w[:1], ci[:1], co[:1], rows[:1], status=True)
        assert np.isnan(a1[0]) and s1[0] == SWAP_REFUSED and fresh.ctx.get_option("swap_refused") == 1
        np.testing.assert_array_equal(bits(fresh.ctx.reserves(0, m, 2)), bits(b.R))
    finally:
        fresh.close()


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_names_the_query_and_changes_nothing():
    L = cr.lib()
    b, w3, u = pools("product", 50, 391), pools("weighted", 50, 392), pools("univ3", 50, 393)
    be = backend([b, w3, u])
    try:
        ctx = be.ctx
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        snap = lambda: [bits(ctx.reserves(0, 50)), bits(ctx.reserves(1, 50, 3)), bits(ctx.prices(2, 50))]
        was = snap()
        ci, _, a = typical_queries(b, 10)
        w = 0.5 * ctx.quote(0, a, ci)
        idx = np.arange(10, dtype=np.int64)

        def refused(match, seg=0, idx=idx, ci=ci, co=None, w=w, lim=None):
            out, st = np.full(w.size, 7.0), np.full(w.size, 7, dtype=np.int32)
            rc = L.cfmm_swap_out(ctx._h, seg, w.size, ptr(idx), ptr(np.ascontiguousarray(ci, dtype=np.int32)),
                                 ptr(None if co is None else np.ascontiguousarray(co, dtype=np.int32)), ptr(np.ascontiguousarray(w)),
                                 ptr(None if lim is None else np.ascontiguousarray(lim)), ptr(out), ptr(st))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and msg.startswith("cfmm_swap_out:") and match in msg, (rc, msg)
            assert np.all(out == 7.0) and np.all(st == 7)
        bad = idx.copy(); bad[4] = 50
        refused("query 4", idx=bad)
        bad = ci.copy(); bad[3] = 2
        refused("query 3", ci=bad)
        refused("query 2", co=np.where(np.arange(10) == 2, ci, 1 - ci))
        for k, x in ((5, -1.0), (6, np.nan), (0, np.inf)):
            bad = w.copy(); bad[k] = x
            refused(f"query {k}: amount_out", w=bad)
            refused(f"query {k}: amount_out", seg=2, w=bad)
            lim = np.full(10, 1e9); lim[k] = x
            refused(f"query {k}: max_amount_in", lim=lim)
        refused("segment", seg=3)
        refused("coin_out is required", seg=1)
        for x, y in zip(snap(), was):
            np.testing.assert_array_equal(x, y)
        assert_same([np.asarray(x) for x in be.trades()], trades)         # the earlier trades are still readable
    finally:
        be.close()


# ---- the state protocol -----------------------------------------------------------------------------------------------------------------
def test_a_swap_out_invalidates_earlier_trades_and_the_next_sweep_sees_the_moved_pools():
    b = pools("product", M, seed=401)
    ci, _, w = wanted(b, M, seed=10)
    be = backend([b])
    fresh = None
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        be.find_arb(V)
        before = [np.array(x, copy=True) for x in be.trades()]
        empty = ctx.swap_out(0, w[:0], ci[:0])                            # count == 0 invalidates nothing
        assert empty.size == 0
        assert_same([np.asarray(x) for x in be.trades()], before)
        ctx.swap_out(0, w, ci)
        assert ctx.get_option("swap_ns") > 0
        with pytest.raises(Exception, match="no materialised trades"):
            ctx.trades()
        now = batch_with(b, R=ctx.reserves(0, M))
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


# ---- the grid-stride loop ---------------------------------------------------------------------------------------------------------------
def test_more_swaps_than_resident_lanes():
    """2048·256 + 1 distinct Product rows: the last lane of the grid takes a second swap"""
    m = 2048 * 256 + 1
    b = pools("product", m, seed=411)
    ci = (np.arange(m) % 2).astype(np.int32)
    w = 0.01 * b.R[np.arange(m), 1 - ci]
    be = backend([b])
    try:
        q = be.ctx.quote_out(0, w, ci)
        a, st = be.ctx.swap_out(0, w, ci, status=True)
        R = be.ctx.reserves(0, m)
    finally:
        be.close()
    np.testing.assert_array_equal(bits(a), bits(q))
    assert np.all(st == SWAP_APPLIED)
    want = b.R.copy()
    r = np.arange(m)
    want[r, ci] = b.R[r, ci] + b.γ * a
    want[r, 1 - ci] = b.R[r, 1 - ci] - w
    np.testing.assert_array_equal(bits(R), bits(want))


# ---- the Python front end -----------------------------------------------------------------------------------------------------------
def test_swap_out_through_a_router_on_a_mixed_market():
    from test_gpu_swap import exact_ladder
    n = 6
    u = exact_ladder()
    pl = [cr.ProductTwoCoin([1e4, 2e4], 0.997, [1, 2]),
          cr.UniV3(0.6, u.lower_ticks[:3], u.liquidity[:3] * 1e4, 0.997, [2, 3]),
          cr.Curve([1e4, 1.1e4, 0.9e4], 0.9995, [1, 3, 4], 2.0, 1e16),
          cr.ProductTwoCoin([3e4, 1e4], 0.997, [3, 5])]
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), pl, n)
    try:
        which, cin, cout = [3, 1, 2, 3, 0], [0, 1, 0, 1, 1], [1, 0, 2, 0, 0]
        want = [100.0, 30.0, 200.0, 50.0, 1e9]
        quoted = cr.quote_out(r, which[:3], cin[:3], want[:3], cout[:3])
        a, st = cr.swap_out_(r, which, cin, want, cout, max_in=[1e9, 1e9, 1e9, 1e-3, 1e9])
        np.testing.assert_array_equal(bits(a[:3]), bits(quoted))          # first visits: the quote's bits
        assert list(st) == [SWAP_APPLIED, SWAP_APPLIED, SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_UNOBTAINABLE] and a[4] == np.inf
        ctx, L = r._backend.ctx, r._layout
        for i, p in enumerate(pl):                                        # the host mirror equals the device
            _, bt, row = L.locate(i)
            seg, batch = L.seg_of[bt], L.batches[bt]
            if isinstance(p, cr.UniV3):
                assert p.current_price == ctx.prices(seg, len(batch))[row] > 0.6
            else:
                np.testing.assert_array_equal(bits(p.R), bits(ctx.reserves(seg, len(batch), len(p.R))[row]))
        assert pl[3].R[1] == 1e4 - 100.0 and pl[3].R[0] == 3e4 + 0.997 * a[0] and pl[0].R[0] == 1e4
    finally:
        r.close()
