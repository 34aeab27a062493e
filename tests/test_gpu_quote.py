"""cfmm_quote / cfmm_quote_dev on the device beyond the 60-digit fixture (tests/test_gpu_quote_precise.py): launch geometry,
the round trip with the sweep, UniV3 against the reference's walk, ladders of sizes, live state after sparse updates,
read-only behaviour, errors and large-market mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
import cp_precise_ref as CP
import quote_precise_ref as P
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_CURVE, KIND_UNIV3, KIND_WEIGHTED, OBJ_LINEAR_NONNEGATIVE
from test_gpu_pool_update import batch_with, moved_prices, rows_of

pytestmark = pytest.mark.gpu

N = 64
KINDS = ("product", "geomean", "univ3", "weighted", "curve", "solidly")
U = 2.0 ** -53


def pools(kind, m, seed=5, n_coins=3):
    if kind == "product":
        return synth.product_pools(m, N, seed=seed)
    if kind == "geomean":
        return synth.geomean_pools(m, N, seed=seed)
    if kind == "solidly":
        return synth.solidly_pools(m, N, seed=seed, wide=True)
    if kind == "univ3":
        return synth.univ3_ragged_pools(m, N, min_ticks=1, max_ticks=64, seed=seed)
    if kind == "weighted":
        return synth.weighted_pools(m, N, n_coins, seed=seed)
    return synth.curve_pools(m, N, n_coins, seed=seed)


def typical_queries(b, count, seed=1):
    """(coin_in, coin_out, amount) for rows 0 .. count-1: alternating coins, a few percent of the tendered reserve (UniV3: of
    the pool's √liquidity scale)"""
    q = np.arange(count)
    nc = b.Ai.shape[1]
    ci = (q % nc).astype(np.int32)
    co = ((q + 1) % nc).astype(np.int32)
    f = 0.002 + 0.2 * synth.uniform(seed, 70, count)
    if b.kind == KIND_UNIV3:
        scale = np.sqrt(b.liquidity[b.tick_off[:-1]][:count] + 1.0)
        return ci, None, f * scale
    return ci, (co if b.kind in (KIND_WEIGHTED, KIND_CURVE) else None), f * b.R[q, ci]


@pytest.fixture(scope="module", params=KINDS)
def seg1025(request):
    b = pools(request.param, 1025)
    be = cr.DeviceBackend(N, [b])
    yield request.param, b, be.ctx
    be.close()


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_counts_dense_sparse_and_repeats(seg1025):
    kind, b, ctx = seg1025
    ci, co, a = typical_queries(b, 1025)
    dense = ctx.quote(0, a, ci, co)
    # (a UniV3 pool without liquidity in the asked direction yields exactly 0)
    assert np.all(np.isfinite(dense)) and np.all(dense >= 0 if kind == "univ3" else dense > 0)
    for count in (1, 63, 64, 65, 257, 1025):
        sl = slice(0, count)
        d = ctx.quote(0, a[sl], ci[sl], None if co is None else co[sl])
        s = ctx.quote(0, a[sl], ci[sl], None if co is None else co[sl], np.arange(count))
        np.testing.assert_array_equal(d, dense[sl])
        np.testing.assert_array_equal(s, dense[sl])
    pick = np.random.default_rng(4).integers(0, 1025, 1500)          # a permutation with repeats
    g = ctx.quote(0, a[pick], ci[pick], None if co is None else co[pick], pick)
    np.testing.assert_array_equal(g, dense[pick])
    # count == 0 is accepted (that it touches nothing: test_live_counts_with_the_hooks_library)
    empty = ctx.quote(0, np.zeros(0), np.zeros(0, dtype=np.int32), None if co is None else np.zeros(0, dtype=np.int32))
    assert empty.size == 0


# ---- the round trip with the sweep ----------------------------------------------------------------------------------------------
def fd_cond(fn, xs):
    """Σ_j |x_j ∂f/∂x_j| and the list of partials by central differences on the numpy restatement (relative step 1e-6: the
    tolerance needs the conditioning's size, not its digits)"""
    cond, grads = 0.0, []
    for j, x in enumerate(xs):
        h = 1e-6 * x
        up = fn(*[x + h if k == j else xs[k] for k in range(len(xs))])
        dn = fn(*[x - h if k == j else xs[k] for k in range(len(xs))])
        gj = np.where(h != 0, (up - dn) / np.where(h != 0, 2 * h, 1.0), 0.0)
        grads.append(gj)
        cond = cond + np.abs(x * gj)
    return cond, grads


K_SWEEP = 8          # the K of the sweeps' tables on well-conditioned trading pools, which is what this market holds (cp_precise_ref
                     # K_PRODUCT / K_UNIV3 <= 8; the tables' edge classes go to 16, weighted ties, and 32, Curve drained: not used here)


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_with_the_sweep(kind):
    """quote(Δ) = Λ for every pool that trades at prices v.  Tolerance, from the two documented bounds: the quote is within
    K_q·u·(R_o + out + cond) of the exact quote of the Δ it is given (K_q: the family's largest K in quote_precise_ref, cond by
    finite differences on the numpy restatement); the sweep's (Δ, Λ) are within K_s·u·κ·(2R_in + γΔ)/γ and K_s·u·κ·2R_out of
    a point on the curve (cp_precise_ref: X* + R_in, Y* + R_out; κ = 1 + the sum of the |log|s of the pool's inputs and prices for
    the log-space kinds -- precise_ref's κ without its division by e + 1, so an UPPER bound of the documented sweep bound, not
    that bound itself -- and 4 for Solidly, solidly_precise_ref.KAPPA), and
    an error dΔ in the amount moves the quote by the marginal rate ∂out/∂a.  UniV3: the sweep's scales S_in, S_out are
    cp_precise_ref.univ3_scale's, and the quote's conditioning is at most 2·S_out + 4·(∂out/∂a)·S_in (quote_precise_ref)."""
    m = 4096
    b = pools(kind, m, seed=21, n_coins=2)
    b.γ[:] = np.where(np.arange(m) % 2 == 0, 0.997, 1.0)
    v = synth.sweep_prices(N, seed=22, spread=0.5)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ctx.find_arb(v)
        D, L = ctx.trades()
        D, L = np.reshape(D, (m, 2)), np.reshape(L, (m, 2))
        trades = np.any(D != 0, axis=1) | np.any(L != 0, axis=1)
        assert trades.sum() >= m // 2, trades.sum()
        rows = np.flatnonzero(trades)
        assert np.all((D[rows] > 0).sum(axis=1) == 1) and np.all((L[rows] > 0).sum(axis=1) == 1)
        ci = np.argmax(D[rows] > 0, axis=1).astype(np.int32)
        co = np.argmax(L[rows] > 0, axis=1).astype(np.int32)
        assert np.all(ci != co)
        amt, lam = D[rows, ci], L[rows, co]
        out = ctx.quote(0, amt, ci, co if kind in ("weighted", "curve") else None, rows)
    finally:
        be.close()
    g = b.γ[rows]
    K_q = max(P.K_of(kind, c) for (f, c) in P.K_MEASURED if f == kind)
    if kind == "univ3":
        case = {"gamma": b.γ, "v": v, "cp": b.current_price, "tick_off": b.tick_off, "lower_ticks": b.lower_ticks,
                "liquidity": b.liquidity, "Ai": b.Ai}
        bD, bL = CP.univ3_scale(case, rows=rows)                       # u·S_in/γ, u·S_out at K = 1
        S_in, S_out = bD[np.arange(rows.size), ci] * g / U, bL[np.arange(rows.size), co] / U
        pr = v[b.Ai[rows, 0] - 1] / v[b.Ai[rows, 1] - 1]
        Pt = np.where(ci == 0, pr / g, g * pr)                         # the marginal price the sweep moves the pool to
        rate = np.where(ci == 0, Pt, 1.0 / Pt)
        tol = K_q * U * (2 * lam + 2 * S_out + 4 * rate * S_in) + K_SWEEP * U * (S_out + rate * S_in)
    else:
        Ri, Ro = b.R[rows, ci], b.R[rows, co]
        logs = np.abs(np.log(g)) + np.abs(np.log(Ri)) + np.abs(np.log(Ro)) + np.abs(np.log(v[b.Ai[rows, 0] - 1])) + \
            np.abs(np.log(v[b.Ai[rows, 1] - 1]))
        if kind == "product":
            cond, gr = fd_cond(P.q_product, [Ri, Ro, g, amt])
            kappa = 1.0
        elif kind == "solidly":
            cond, gr = fd_cond(P.q_solidly, [Ri, Ro, g, amt])
            kappa = 4.0
        elif kind in ("geomean", "weighted"):
            w = b.w / b.w.sum(axis=1, keepdims=True)
            wi, wo = w[rows, ci], w[rows, co]
            cond, gr = fd_cond(P.q_weighted, [Ri, Ro, wi, wo, g, amt])
            kappa = 1.0 + logs + np.abs(np.log(wi / wo))
        else:
            lb, srho = np.log(b.β[rows]), P.sum_logs(b.R[rows])
            al = b.α[rows]
            cond, gr = fd_cond(lambda ri, ro, lp, gg, aa: P.q_curve(ri, ro, 0.0, al, lp, gg, aa), [Ri, Ro, lb - srho, g, amt])
            cond = cond - np.abs((lb - srho) * gr[2]) + (np.abs(lb) + np.sum(np.abs(np.log(b.R[rows])), axis=1)) * np.abs(gr[2])
            kappa = 1.0 + logs + np.abs(lb)
        rate = np.abs(gr[-1])
        tol = K_q * U * (Ro + lam + cond) + K_SWEEP * U * kappa * (2 * Ro + rate * (2 * Ri + g * amt) / g)
    err = np.abs(out - lam)
    worst = float(np.max(err / tol))
    print(f"round trip {kind}: {rows.size} of {m} pools trade, worst |quote(Δ) − Λ| / tolerance = {worst:.3g}")
    assert np.all(np.isfinite(out)) and worst <= 1.0


# ---- UniV3 against the reference's walk ---------------------------------------------------------------------------------------
def test_univ3_against_the_oracle_walk():
    """oracle.UniV3.forward_trade (the reference's sequential walk, src/cfmms.jl:416-449) on 2048 pools with ragged 1..64-tick
    ladders (zero-liquidity ticks included), both directions, amounts log-uniform from 1e-9 to 10x the ladder's total.
    The two differ in rounding only: the device adds prefix sums where the walk subtracts tick by tick.  Each is within its
    own K of the truth in units of u·(ΣR_out walked + R_out of the landing tick + out + cond) -- the device's K of
    quote_precise_ref, the oracle's measured figure ORACLE_UNIV3_K -- so they differ by at most (K_device + K_oracle) units.
    The unit is computed per row, in doubles, from the walk actually taken (quote_precise_ref.univ3_unit, held to the
    fixture's mpmath figures on the CPU)."""
    import oracle.cfmm_oracle as O
    m = 2048
    b = synth.univ3_ragged_pools(m, N, min_ticks=1, max_ticks=64, seed=31)
    zero = synth.uniform(32, 5, b.liquidity.size) < 0.1
    b = batch_with(b, liquidity=np.where(zero, 0.0, b.liquidity))
    ci = (np.arange(m) % 2).astype(np.int32)
    P_ = [P.univ3_prepare(b.current_price[i], b.lower_ticks[b.tick_off[i]:b.tick_off[i + 1]],
                          b.liquidity[b.tick_off[i]:b.tick_off[i + 1]]) for i in range(m)]
    total = np.empty(m)
    for i in range(m):
        cur, up, lo = P_[i]
        lst = up if ci[i] == 0 else lo
        finite = [r[2] for r in lst[:-1] if np.isfinite(r[2])]
        cur_d = cur[3] if ci[i] == 0 else cur[4]
        total[i] = sum(finite) + (cur_d if np.isfinite(cur_d) and cur[0] != 0 else 0.0)
    total = np.where(total > 0, total, 1.0)
    amt = total * np.exp(np.log(1e-9) + (np.log(10.0) - np.log(1e-9)) * synth.uniform(33, 6, m)) / b.γ
    be = cr.DeviceBackend(N, [b])
    try:
        out = be.ctx.quote(0, amt, ci)
    finally:
        be.close()
    ref = np.empty(m)
    for i in range(m):
        Dl = np.zeros(2)
        Dl[ci[i]] = amt[i]
        ref[i] = O.UniV3(b.current_price[i], b.lower_ticks[b.tick_off[i]:b.tick_off[i + 1]],
                         b.liquidity[b.tick_off[i]:b.tick_off[i + 1]], b.γ[i]).forward_trade(Dl)
    K_dev = max(P.K_of("univ3", c) for (f, c) in P.K_MEASURED if f == "univ3")
    unit = np.array([sum(P.univ3_unit(P_[i], float(b.γ[i]), int(ci[i]), float(amt[i]))) for i in range(m)])
    tol = (K_dev + P.ORACLE_UNIV3_K) * U * (unit + ref)
    err = np.abs(out - ref)
    worst = float(np.max(np.where(err == 0, 0.0, err / np.where(tol > 0, tol, 1e-300))))      # (no liquidity at all: 0 == 0)
    exhausted = int(np.sum((ci == 1) & (amt * b.γ >= total)))
    print(f"UniV3 vs oracle walk: worst {worst:.3g} of the tolerance (K {K_dev} + {P.ORACLE_UNIV3_K}); {exhausted} ladders exhausted; "
          f"{int(np.sum(out == ref))} of {m} bit-identical")
    assert exhausted > 0 and np.all(np.isfinite(out)) and worst <= 1.0


# ---- a ladder of sizes ----------------------------------------------------------------------------------------------------------
def test_ladder_of_sizes(seg1025):
    kind, b, ctx = seg1025
    row = 7
    _, co, a1 = typical_queries(b, 8)
    base = a1[row] / 0.2
    sizes = base * np.exp(np.linspace(np.log(1e-6), np.log(30.0), 32))
    ci = np.full(32, row % b.Ai.shape[1], dtype=np.int32)
    cout = None if co is None else np.full(32, (row + 1) % b.Ai.shape[1], dtype=np.int32)
    out = ctx.quote(0, sizes, ci, cout, np.full(32, row))
    ulp4 = 4 * np.spacing(out)
    assert np.all(np.diff(out) >= -ulp4[1:])                                     # nondecreasing
    rate = out / sizes
    assert np.all(np.diff(rate) * sizes[1:] <= ulp4[1:])                         # out/a nonincreasing, within 4 ulp of out
    if kind != "univ3":
        assert np.all(out < b.R[row, (row + 1) % b.Ai.shape[1]])                 # out < R_o always
    else:                                                                        # ... UniV3: at most the direction's whole liquidity
        cur, up, lo = P.univ3_prepare(b.current_price[row], b.lower_ticks[b.tick_off[row]:b.tick_off[row + 1]],
                                      b.liquidity[b.tick_off[row]:b.tick_off[row + 1]])
        assert np.all(out <= (up if ci[0] == 0 else lo)[-1][6])                  # the closing record's ΣR_out


# ---- live state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_quotes_follow_sparse_updates(kind):
    m = 600
    b = pools(kind, m, seed=41)
    o = pools(kind, m, seed=42)
    rows = rows_of(m, 150, 43)
    be = cr.DeviceBackend(N, [b])
    fresh = None
    try:
        ctx = be.ctx
        if kind == "univ3":
            regrows = ctx.get_option("pool_update_regrows")
            p = b.current_price.copy()
            for rnd in range(24):                                                # enough rounds that the tick records compact
                pick = rows_of(m, m // 2, 50 + rnd)
                p[pick] = moved_prices(b, 60 + rnd)[pick]
                ctx.set_prices(0, pick, p[pick])
                if rnd >= 1 and ctx.get_option("pool_update_regrows") > regrows:
                    break
            assert ctx.get_option("pool_update_regrows") > regrows
            # a mint on `rows`: 1.5x the liquidity of every tick, the price stays
            lq = b.liquidity.copy()
            for r in rows:
                lq[b.tick_off[r]:b.tick_off[r + 1]] *= 1.5
            off = np.concatenate([[0], np.cumsum(np.diff(b.tick_off)[rows])])
            sel = np.concatenate([np.arange(b.tick_off[r], b.tick_off[r + 1]) for r in rows])
            ctx.set_ticks(0, rows, p[rows], off, b.lower_ticks[sel], lq[sel])
            new = batch_with(b, current_price=p, liquidity=lq)
        elif kind == "curve":
            ctx.set_curve(0, rows, o.R[rows], o.α[rows], o.β[rows])
            R, al, be_ = b.R.copy(), b.α.copy(), b.β.copy()
            R[rows], al[rows], be_[rows] = o.R[rows], o.α[rows], o.β[rows]
            new = batch_with(b, R=R, α=al, β=be_)
        else:
            ctx.set_reserves(0, rows, o.R[rows])
            R = b.R.copy()
            R[rows] = o.R[rows]
            new = batch_with(b, R=R)
        ci, co, a = typical_queries(new, m, seed=44)
        got = ctx.quote(0, a, ci, co)
        fresh = cr.DeviceBackend(N, [new])
        want = fresh.ctx.quote(0, a, ci, co)
        np.testing.assert_array_equal(got, want)
        assert np.any(got[rows] != be_quote_old(b, a, ci, co)[rows])
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


def be_quote_old(b, a, ci, co):
    be = cr.DeviceBackend(N, [b])
    try:
        return be.ctx.quote(0, a, ci, co)
    finally:
        be.close()


@pytest.mark.parametrize("kind", KINDS)
def test_after_update_reserves_the_former_trade_yields_less(kind):
    """every kind (weighted and Curve at N = 2, where a trade has one Δ and one Λ: their quotes read the columns -- Curve the
    uploaded log R -- that the update's own kernel must have refreshed)"""
    m = 2048
    b = pools(kind, m, seed=51, n_coins=2)
    v = synth.sweep_prices(N, seed=52, spread=0.3)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ctx.find_arb(v)
        D, L = (np.reshape(x, (m, 2)) for x in ctx.trades())
        rows = np.flatnonzero(((D > 0).sum(axis=1) == 1) & ((L > 0).sum(axis=1) == 1))
        assert rows.size >= m // 2
        ci = np.argmax(D[rows] > 0, axis=1).astype(np.int32)
        co = (1 - ci).astype(np.int32) if kind in ("weighted", "curve") else None
        before = ctx.quote(0, D[rows, ci], ci, co, rows)
        ctx.update_reserves()                                          # (the quote consumed nothing: the trades are still there)
        after = ctx.quote(0, D[rows, ci], ci, co, rows)
    finally:
        be.close()
    lam = L[rows, 1 - ci]
    assert np.all(after < lam), int(np.sum(~(after < lam)))
    assert np.all(after < before)


# ---- read-only ----------------------------------------------------------------------------------------------------------------
def test_quoting_changes_nothing_the_other_calls_see():
    batches = [pools("product", 700, 61), pools("geomean", 700, 62), pools("univ3", 300, 63), pools("solidly", 300, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)

    def run(quoting):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def q(seg):
            if quoting:
                ci, _, a = typical_queries(batches[seg], 100)
                ctx.quote(seg, a, ci)
        try:
            q(0)                                                       # needs no sweep to have run
            ctx.find_arb(v)
            q(1)
            res.append(ctx.trades())
            q(2)
            res.append(ctx.select_trades(0, 0.0))
            q(3)
            res.append((ctx.netflows(), ctx.dual_value()))
            q(0)
            ctx.update_reserves()
            q(2)
            res.append(ctx.eval(v))
            q(1)
            vr, psi, info = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=60)
            q(3)
            res.append((vr, psi, {k: info[k] for k in ("f", "proj_grad", "iterations", "evaluations", "status")}, ctx.netflows()))
        finally:
            be.close()
        return res

    a, b = run(True), run(False)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for p, q in zip(x, y):
                same(p, q)
        elif isinstance(x, dict):
            assert x == y
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    same(a, b)


COUNTERS = ("debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams")


def live_counts_body():
    probe = cr.Context(4)
    live = lambda: tuple(probe.get_option(k) for k in COUNTERS)
    base = live()
    b = pools("weighted", 500, 71)
    be = cr.DeviceBackend(N, [b])
    ci, co, a = typical_queries(b, 300)
    before = live()
    be.ctx.set_option("time_kernels", 1)
    # count == 0 touches nothing: no scratch, no staging, no event, no kernel (quote_ns stays 0), NULL arrays accepted
    be.ctx.quote(0, a[:0], ci[:0], co[:0])
    be.ctx._check(cr.lib().cfmm_quote(be.ctx._h, 0, 0, None, None, None, None, None))
    assert live() == before and be.ctx.get_option("quote_ns") == 0
    be.ctx.quote(0, a, ci, co, np.arange(300))
    first = live()
    # the first quote creates the scratch: 4 device arrays, 1 pinned buffer, 2 events (time_kernels), no stream
    assert tuple(x - y for x, y in zip(first, before)) == (4, 1, 2, 0), (before, first)
    assert be.ctx.get_option("quote_ns") > 0
    be.ctx.quote(0, a, ci, co, np.arange(300))
    be.ctx.quote(0, a[:200], ci[:200], co[:200])
    assert live() == first                                             # stable across a second quote of the same size
    be.close()
    assert live() == base                                              # everything goes with the context
    probe.close()
    print("quote-live-ok")


def test_live_counts_with_the_hooks_library():
    """the four debug_live_* counts: what the first quote creates (4 device arrays, 1 pinned buffer, 2 events under
    time_kernels) stays for the next call and goes with the context: the counts before the context and after close() are equal"""
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_quote as t\n"
            "t.live_counts_body()\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "quote-live-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_host_variant_refuses_and_names_the_query():
    L = cr.lib()
    b, w = pools("product", 50, 81), pools("weighted", 50, 82)
    be = cr.DeviceBackend(N, [b, w])
    try:
        ctx = be.ctx
        ci, co, a = typical_queries(b, 10)
        idx = np.arange(10, dtype=np.int64)

        def refused(match, seg=0, idx=idx, ci=ci, co=None, a=a):
            out = np.full(a.size, 7.0)
            from cfmmrouter_amd._lib import ptr
            rc = L.cfmm_quote(ctx._h, seg, a.size, ptr(idx), ptr(np.ascontiguousarray(ci, dtype=np.int32)),
                              ptr(None if co is None else np.ascontiguousarray(co, dtype=np.int32)), ptr(np.ascontiguousarray(a)), ptr(out))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and match in msg, (rc, msg)
            assert np.all(out == 7.0)                                  # the outputs are untouched
        bad = idx.copy(); bad[4] = 50
        refused("query 4", idx=bad)
        bad = idx.copy(); bad[9] = -1
        refused("query 9", idx=bad)
        bad = ci.copy(); bad[3] = 2
        refused("query 3", ci=bad)
        refused("query 2", co=np.where(np.arange(10) == 2, ci, 1 - ci))            # coin_out == coin_in
        bad = a.copy(); bad[5] = -1.0
        refused("query 5", a=bad)
        bad = a.copy(); bad[6] = np.nan
        refused("query 6", a=bad)
        bad = a.copy(); bad[0] = np.inf
        refused("query 0", a=bad)
        refused("segment", seg=2)
        refused("coin_out is required", seg=1)                                   # NULL coin_out on an N-coin segment
        with pytest.raises(cr.ArgumentError, match="count"):
            ctx._check(L.cfmm_quote(ctx._h, 0, -1, None, None, None, None, None))
    finally:
        be.close()


@pytest.mark.parametrize("kind", ("product", "univ3", "curve"))
def test_device_variant_poisons_exactly_the_bad_queries(kind):
    import torch
    b = pools(kind, 200, 91)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        n = 64
        ci, co, a = typical_queries(b, n)
        if co is None:
            co = (1 - ci).astype(np.int32)
        good = ctx.quote(0, a, ci, co)
        idx = np.arange(n, dtype=np.int64)
        idx[3], idx[4] = 200, -5                                                 # clamped before any read, then poisoned
        ci2, co2, a2 = ci.copy(), co.copy(), a.copy()
        ci2[10], co2[11] = b.Ai.shape[1], -1
        co2[12] = ci2[12]
        a2[20], a2[21], a2[22] = -1.0, np.nan, np.inf
        bad = np.zeros(n, dtype=bool)
        bad[[3, 4, 10, 11, 12, 20, 21, 22]] = True
        dev = torch.device("cuda:0")
        t = [torch.from_numpy(x).to(dev) for x in (idx, ci2, co2, a2)]
        t_out = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.quote_dev(0, n, t[3].data_ptr(), t[1].data_ptr(), t_out.data_ptr(), t[2].data_ptr(), t[0].data_ptr())
            torch.cuda.synchronize()
        finally:
            ctx.reset_stream()
        out = t_out.cpu().numpy()
        assert np.all(np.isnan(out[bad]))
        np.testing.assert_array_equal(out[~bad], good[~bad])
    finally:
        be.close()


# ---- large-market mode -------------------------------------------------------------------------------------------------------
def test_large_market_mode_gives_the_same_bits():
    m = 3000
    small = synth.product_pools(m, N, seed=95)
    big = batch_with(small, Ai=np.where(small.Ai == 1, 8193, small.Ai))     # one token beyond the LDS limit: n_tokens = 8193
    ci, co, a = typical_queries(small, m)
    be_s, be_b = cr.DeviceBackend(N, [small]), cr.DeviceBackend(8193, [big])
    try:
        np.testing.assert_array_equal(be_b.ctx.quote(0, a, ci), be_s.ctx.quote(0, a, ci))
        pick = np.random.default_rng(5).integers(0, m, 500)
        np.testing.assert_array_equal(be_b.ctx.quote(0, a[pick], ci[pick], None, pick), be_s.ctx.quote(0, a[pick], ci[pick], None, pick))
    finally:
        be_s.close()
        be_b.close()
