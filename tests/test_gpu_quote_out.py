"""cfmm_quote_out / cfmm_quote_out_dev on the device beyond the 80-digit fixture (tests/test_gpu_quote_out_precise.py): launch
geometry, the round trip through cfmm_quote, ladders of outputs, UniV3 against the numpy restatement of the inverse walk, the
exhausted ladder, live state after sparse updates, read-only behaviour, errors, large-market mode and the live counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_out_precise_ref as P
import quote_precise_ref as F
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import OBJ_LINEAR_NONNEGATIVE
from test_gpu_pool_update import batch_with, moved_prices, rows_of
from test_gpu_quote import COUNTERS, N, fd_cond, pools, typical_queries

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# (kind, coin count): the six kernels, the N-coin ones at every width the issue names (Curve's Σ log R switches on N)
CASES = (("product", 2), ("geomean", 2), ("solidly", 2), ("univ3", 2), ("weighted", 2), ("weighted", 3), ("weighted", 8),
         ("curve", 2), ("curve", 3), ("curve", 4), ("curve", 8))
M = 1025            # four blocks of 256 plus one lane


def K_max(table, fam):
    return max(table.K_of(fam, c) for (f, c) in table.K_MEASURED if f == fam)


def preps_of(b, rows):
    return [F.univ3_prepare(b.current_price[i], b.lower_ticks[b.tick_off[i]:b.tick_off[i + 1]],
                            b.liquidity[b.tick_off[i]:b.tick_off[i + 1]]) for i in rows]


def finite_capacity(prep, cin):
    """Σ of the finite δmax of the direction, the current tick's included"""
    cur, up, lo = prep
    d = [cur[3] if cin == 0 else cur[4]] if cur[0] != 0 else []
    return sum(x for x in d + [r[2] for r in (up if cin == 0 else lo)[:-1]] if np.isfinite(x))


def wanted(ctx, b, count, frac=0.5, seed=1):
    """(coin_in, coin_out, o): outputs the pools can give -- `frac` of what a typical tender yields"""
    ci, co, a = typical_queries(b, count, seed)
    return ci, co, frac * ctx.quote(0, a, ci, co)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}{c[1]}")
def seg(request):
    kind, nc = request.param
    b = pools(kind, M, n_coins=nc)
    be = cr.DeviceBackend(N, [b])
    yield kind, b, be.ctx
    be.close()


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_counts_dense_sparse_and_repeats(seg):
    kind, b, ctx = seg
    ci, co, o = wanted(ctx, b, M)
    dense = ctx.quote_out(0, o, ci, co)
    assert np.all(np.isfinite(dense)) and np.all(dense >= 0 if kind == "univ3" else dense > 0)
    for count in (1, 256, 257, M):
        sl = slice(0, count)
        d = ctx.quote_out(0, o[sl], ci[sl], None if co is None else co[sl])
        s = ctx.quote_out(0, o[sl], ci[sl], None if co is None else co[sl], np.arange(count))
        np.testing.assert_array_equal(d, dense[sl])
        np.testing.assert_array_equal(s, dense[sl])
    pick = np.random.default_rng(4).integers(0, M, 1500)             # a permutation with repeats
    g = ctx.quote_out(0, o[pick], ci[pick], None if co is None else co[pick], pick)
    np.testing.assert_array_equal(g, dense[pick])
    empty = ctx.quote_out(0, np.zeros(0), np.zeros(0, dtype=np.int32), None if co is None else np.zeros(0, dtype=np.int32))
    assert empty.size == 0


# ---- the round trip through the forward quote ---------------------------------------------------------------------------------
def reserve_forms(kind, b, rows, ci, co):
    """(forward form, inverse form, their arguments before the amount, the Curve log rows) on the numpy restatements"""
    g = b.γ[rows]
    Ri, Ro = b.R[rows, ci], b.R[rows, co]
    if kind == "product":
        return F.q_product, P.qo_product, [Ri, Ro, g], None
    if kind == "solidly":
        return F.q_solidly, P.qo_solidly, [Ri, Ro, g], None
    if kind in ("geomean", "weighted"):
        w = b.w / b.w.sum(axis=1, keepdims=True)
        return F.q_weighted, P.qo_weighted, [Ri, Ro, w[rows, ci], w[rows, co], g], None
    lb, srho, al = np.log(b.β[rows]), F.sum_logs(b.R[rows]), b.α[rows]
    fwd = lambda ri, ro, lp, gg, aa: F.q_curve(ri, ro, 0.0, al, lp, gg, aa)
    inv = lambda ri, ro, lp, gg, oo: P.qo_curve(ri, ro, 0.0, al, lp, gg, oo)
    return fwd, inv, [Ri, Ro, lb - srho, g], np.abs(lb) + np.sum(np.abs(np.log(b.R[rows])), axis=1)


def cond_of(fn, xs, logs):
    cond, gr = fd_cond(fn, xs)
    if logs is not None:   # Curve: argument 2 is log P₀, which stands for log β and every log R_k the device holds
        cond = cond - np.abs(xs[2] * gr[2]) + logs * np.abs(gr[2])
    return cond, np.abs(gr[-1])


def test_round_trip_through_the_forward_quote(seg):
    """quote_out(quote(a)) = a for amounts spread over 1e-9 .. 10x R_i (UniV3: of the direction's finite Σδmax).  Tolerance,
    from the two documented bounds: out = quote(a) is within K_q·u·(R_o + out + cond_q) of the exact output of a
    (quote_precise_ref); quote_out(out) is within K_o·u·(R_i/γ + a + cond_o) of the exact input of THAT out
    (quote_out_precise_ref); and an error in out moves the input by the local slope ∂a/∂out.  The slope and both conditioning
    sums come from the numpy restatements by centred differences (UniV3: from the per-row units in doubles), never from the
    device.  The worst ratio of |round trip − a| to that sum must be <= 1."""
    kind, b, ctx = seg
    rows = np.arange(M)
    nc = b.Ai.shape[1]
    ci = (rows % nc).astype(np.int32)
    co = ((rows + 1 + rows // nc % (nc - 1)) % nc).astype(np.int32) if nc > 2 else (1 - ci).astype(np.int32)
    f = np.exp(np.log(1e-9) + (np.log(10.0) - np.log(1e-9)) * synth.uniform(7, 3, M))
    K_q, K_o = K_max(F, kind), K_max(P, kind)
    if kind == "univ3":
        pr = preps_of(b, rows)
        tot = np.array([finite_capacity(p, c) for p, c in zip(pr, ci)])
        a = np.minimum(f, 0.9) * np.where(tot > 0, tot, 1.0) / b.γ
        out = ctx.quote(0, a, ci)
        back = ctx.quote_out(0, out, ci)
        tol = np.full(M, np.inf)
        for i in rows:
            if out[i] == 0.0:          # nothing to take in this direction: the smallest input for nothing is nothing
                assert back[i] == 0.0
                continue
            un = P.univ3_unit(pr[i], float(b.γ[i]), int(ci[i]), float(out[i]))
            uq = F.univ3_unit(pr[i], float(b.γ[i]), int(ci[i]), float(a[i]))
            assert un is not None
            tol[i] = K_o * U * (un[0] + a[i] + un[1]) + un[2] * K_q * U * (uq[0] + out[i] + uq[1])
    else:
        a = f * b.R[rows, ci]
        cout = co if kind in ("weighted", "curve") else None
        out = ctx.quote(0, a, ci, cout)
        back = ctx.quote_out(0, out, ci, cout)
        fwd, inv, xs, logs = reserve_forms(kind, b, rows, ci, co)
        with np.errstate(all="ignore"):
            cond_q, _ = cond_of(fwd, xs + [a], logs)
            cond_o, slope = cond_of(inv, xs + [out], logs)
            tol = K_o * U * (b.R[rows, ci] / b.γ + a + cond_o) + slope * K_q * U * (b.R[rows, co] + out + cond_q)
        # the forward quote rounded to the whole reserve: the amount is lost, no finite input yields that output.  Within
        # 1e-6 of it the centred difference reaches past the reserve and the slope is unbounded there: no tolerance either
        drained = out >= b.R[rows, co]
        assert np.all(back[drained] == np.inf) and np.all(np.isfinite(back[~drained])) and np.sum(drained) <= M // 20
        tol = np.where(np.isfinite(tol) & ~drained, tol, np.inf)
        back = np.where(drained, a, back)
        assert np.sum(np.isfinite(tol)) >= M * 9 // 10
    err = np.abs(back - a)
    worst = float(np.max(np.where(err == 0, 0.0, err / tol)))
    print(f"round trip {kind}{nc}: worst |quote_out(quote(a)) − a| / (exact-output bound + slope · exact-input bound) = {worst:.3g}")
    assert np.all(np.isfinite(back)) and worst <= 1.0


# ---- a ladder of outputs ------------------------------------------------------------------------------------------------------
def test_ladder_of_outputs_gives_strictly_increasing_inputs(seg):
    kind, b, ctx = seg
    row, nc = 7, b.Ai.shape[1]
    cin, cout = row % nc, (row + 1) % nc
    if kind == "univ3":   # the first pool from row 7 on with liquidity in the direction
        row = next(i for i in range(7, M) if P.univ3_totals(preps_of(b, [i])[0], cin)[1] > 0)
        total = P.univ3_totals(preps_of(b, [row])[0], cin)[1]
    else:
        total = b.R[row, cout]
    assert total > 0
    o = total * np.exp(np.linspace(np.log(1e-6), np.log(0.99), 48))
    a = ctx.quote_out(0, o, np.full(48, cin, dtype=np.int32), None if kind in ("product", "geomean", "solidly", "univ3")
                      else np.full(48, cout, dtype=np.int32), np.full(48, row))
    assert np.all(np.isfinite(a)) and a[0] > 0 and np.all(np.diff(a) > 0)
    assert np.all(np.diff(a / o) >= -4 * np.spacing(a[1:] / o[1:]))          # the price paid per unit never falls


# ---- UniV3 against the restatement --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged():
    m = 2048
    b = synth.univ3_ragged_pools(m, N, min_ticks=1, max_ticks=64, seed=31)
    zero = synth.uniform(32, 5, b.liquidity.size) < 0.1
    b = batch_with(b, liquidity=np.where(zero, 0.0, b.liquidity))
    be = cr.DeviceBackend(N, [b])
    yield b, be.ctx, preps_of(b, range(m))
    be.close()


def test_univ3_against_the_restatement(ragged):
    """2048 pools with ragged 1..64-tick ladders (zero-liquidity ticks included), both directions, o log-uniform from 1e-9 to
    0.999x the direction's total as the upload prepares it; 64 more rows beyond the total, which must be +inf.  The device and
    the numpy restatement run the same operations on the same prepared records and differ in the library functions and the
    records' own last bits at most: each is within its K of the truth in units of u·(scale + a + cond), so they differ by at
    most (K_device + K_restatement) units, the unit per row in doubles from the walk taken (quote_out_precise_ref.univ3_unit)."""
    b, ctx, pr = ragged
    m = b.current_price.size
    ci = (np.arange(m) % 2).astype(np.int32)
    total = np.array([P.univ3_totals(p, c)[1] for p, c in zip(pr, ci)])
    o = total * np.minimum(np.exp(np.log(1e-9) + (np.log(0.999) - np.log(1e-9)) * synth.uniform(33, 6, m)), 0.999)
    a = ctx.quote_out(0, o, ci)
    ref = np.array([P.qo_univ3(p, float(g), int(c), float(x)) for p, g, c, x in zip(pr, b.γ, ci, o)])
    K = 2 * K_max(P, "univ3")
    worst, live = 0.0, 0
    for i in range(m):
        if total[i] == 0.0:
            assert a[i] == 0.0 and ref[i] == 0.0
            continue
        un = P.univ3_unit(pr[i], float(b.γ[i]), int(ci[i]), float(o[i]))
        assert un is not None and np.isfinite(a[i])
        worst = max(worst, abs(a[i] - ref[i]) / (U * (un[0] + ref[i] + un[1])))
        live += 1
    print(f"UniV3 quote_out vs restatement: worst {worst:.3g} units of an allowance of {K}; {int(np.sum(a == ref))} of {m} rows "
          f"bit-identical; {live} rows with liquidity in the direction")
    assert live >= m // 2 and worst <= K
    far = np.flatnonzero(total > 0)[:64]
    mult = np.where(np.arange(64) % 2 == 0, 1.0000001, 5.0)
    beyond = ctx.quote_out(0, total[far] * mult, ci[far], None, far)
    assert far.size == 64 and np.all(beyond == np.inf)


def test_exhausted_ladder_reports_the_input_consumed(ragged):
    """DESIGN §8's recipe: for an amount beyond all liquidity of a direction that a finite input exhausts (coin 1 in: the price
    rises to the top of the ladder), quote gives the direction's whole ΣR_out and quote_out of THAT is the closing record's
    Σδmax/γ as the restatement computes it -- the input the pool actually consumed -- and at most the amount tendered."""
    b, ctx, pr = ragged
    rows = np.array([i for i in range(b.current_price.size) if P.univ3_totals(pr[i], 1)[1] > 0][:300])
    sd = np.array([P.univ3_totals(pr[i], 1)[0] for i in rows])
    sr = np.array([P.univ3_totals(pr[i], 1)[1] for i in rows])
    assert rows.size == 300 and np.all(np.isfinite(sd))
    a = sd / b.γ[rows] * np.where(np.arange(300) % 2 == 0, 1.5, 1e6)
    ci = np.ones(300, dtype=np.int32)
    out = ctx.quote(0, a, ci, None, rows)
    np.testing.assert_array_equal(out, sr)
    used = ctx.quote_out(0, out, ci, None, rows)
    np.testing.assert_array_equal(used, sd / b.γ[rows])
    assert np.all(used <= a)


# ---- live state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("product", "geomean", "univ3", "weighted", "curve", "solidly"))
def test_answers_follow_sparse_updates(kind):
    """set_reserves (two-coin kinds, weighted), set_curve, set_prices + set_ticks: the answers are those of a context that was
    given the new state from the start"""
    m = 600
    b = pools(kind, m, seed=41)
    o_ = pools(kind, m, seed=42)
    rows = rows_of(m, 150, 43)
    be = cr.DeviceBackend(N, [b])
    fresh = None
    try:
        ctx = be.ctx
        ci, co, want0 = wanted(ctx, b, m, seed=44)
        old = ctx.quote_out(0, want0, ci, co)
        if kind == "univ3":
            p = b.current_price.copy()
            pick = rows_of(m, m // 2, 50)
            p[pick] = moved_prices(b, 60)[pick]
            ctx.set_prices(0, pick, p[pick])
            lq = b.liquidity.copy()
            for r in rows:                                                       # a mint on `rows`: 1.5x every tick
                lq[b.tick_off[r]:b.tick_off[r + 1]] *= 1.5
            off = np.concatenate([[0], np.cumsum(np.diff(b.tick_off)[rows])])
            sel = np.concatenate([np.arange(b.tick_off[r], b.tick_off[r + 1]) for r in rows])
            ctx.set_ticks(0, rows, p[rows], off, b.lower_ticks[sel], lq[sel])
            new = batch_with(b, current_price=p, liquidity=lq)
        elif kind == "curve":
            ctx.set_curve(0, rows, o_.R[rows], o_.α[rows], o_.β[rows])
            R, al, be_ = b.R.copy(), b.α.copy(), b.β.copy()
            R[rows], al[rows], be_[rows] = o_.R[rows], o_.α[rows], o_.β[rows]
            new = batch_with(b, R=R, α=al, β=be_)
        else:
            ctx.set_reserves(0, rows, o_.R[rows])
            R = b.R.copy()
            R[rows] = o_.R[rows]
            new = batch_with(b, R=R)
        fresh = cr.DeviceBackend(N, [new])
        ci, co, want = wanted(fresh.ctx, new, m, seed=44)
        got = ctx.quote_out(0, want, ci, co)
        np.testing.assert_array_equal(got, fresh.ctx.quote_out(0, want, ci, co))
        assert np.any(ctx.quote_out(0, want0, ci, co)[rows] != old[rows])
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("kind", ("product", "geomean", "univ3", "weighted", "curve", "solidly"))
def test_after_update_reserves_the_former_output_costs_more(kind):
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
        lam = 0.5 * L[rows, 1 - ci]                                    # half of what the trade took: still there afterwards
        before = ctx.quote_out(0, lam, ci, co, rows)
        ctx.update_reserves()                                          # (the quote consumed nothing: the trades are still there)
        after = ctx.quote_out(0, lam, ci, co, rows)
    finally:
        be.close()
    assert np.all(before < D[rows, ci]) and np.all(before > 0)
    assert np.all(after > before), int(np.sum(~(after > before)))


# ---- read-only ----------------------------------------------------------------------------------------------------------------
def test_quoting_changes_nothing_the_other_calls_see():
    batches = [pools("product", 700, 61), pools("geomean", 700, 62), pools("univ3", 300, 63), pools("solidly", 300, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)

    def run(quoting):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def q(s):
            if quoting:
                ci, _, a = typical_queries(batches[s], 100)
                ctx.quote_out(s, a * 1e-3, ci)
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

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for p, q_ in zip(x, y):
                same(p, q_)
        elif isinstance(x, dict):
            assert x == y
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    same(run(True), run(False))


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
    be.ctx.quote_out(0, a[:0], ci[:0], co[:0])
    be.ctx._check(cr.lib().cfmm_quote_out(be.ctx._h, 0, 0, None, None, None, None, None))
    assert live() == before and be.ctx.get_option("quote_ns") == 0
    o = 0.5 * be.ctx.quote(0, a, ci, co, np.arange(300))
    first = live()
    # the forward quote created the scratch (4 device arrays, 1 pinned buffer, 2 events under time_kernels, no stream): the
    # inverse uses the same one and adds nothing
    assert tuple(x - y for x, y in zip(first, before)) == (4, 1, 2, 0), (before, first)
    be.ctx.quote_out(0, o, ci, co, np.arange(300))
    assert be.ctx.get_option("quote_ns") > 0                           # the latest call of either direction
    be.ctx.quote_out(0, o[:200], ci[:200], co[:200])
    be.ctx.quote(0, a, ci, co)
    assert live() == first
    be.close()
    assert live() == base                                              # everything goes with the context
    probe.close()
    print("quote-out-live-ok")


def test_live_counts_with_the_hooks_library():
    """the four debug_live_* counts are what cfmm_quote alone leaves: the inverse shares QuoteScratch and adds no buffer,
    event or stream; everything goes with the context"""
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_quote_out as t\n"
            "t.live_counts_body()\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "quote-out-live-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_host_variant_refuses_and_names_the_query():
    from cfmmrouter_amd._lib import ptr
    L = cr.lib()
    b, w = pools("product", 50, 81), pools("weighted", 50, 82)
    be = cr.DeviceBackend(N, [b, w])
    try:
        ctx = be.ctx
        ci, co, o = wanted(ctx, b, 10)
        idx = np.arange(10, dtype=np.int64)

        def refused(match, seg=0, idx=idx, ci=ci, co=None, o=o):
            ans = np.full(o.size, 7.0)
            rc = L.cfmm_quote_out(ctx._h, seg, o.size, ptr(idx), ptr(np.ascontiguousarray(ci, dtype=np.int32)),
                                  ptr(None if co is None else np.ascontiguousarray(co, dtype=np.int32)), ptr(np.ascontiguousarray(o)), ptr(ans))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and match in msg and msg.startswith("cfmm_quote_out:"), (rc, msg)
            assert np.all(ans == 7.0)                                  # the answers are untouched
        bad = idx.copy(); bad[4] = 50
        refused("query 4", idx=bad)
        bad = idx.copy(); bad[9] = -1
        refused("query 9", idx=bad)
        bad = ci.copy(); bad[3] = 2
        refused("query 3", ci=bad)
        refused("query 2", co=np.where(np.arange(10) == 2, ci, 1 - ci))            # coin_out == coin_in
        bad = o.copy(); bad[5] = -1.0
        refused("query 5: amount_out", o=bad)
        bad = o.copy(); bad[6] = np.nan
        refused("query 6", o=bad)
        bad = o.copy(); bad[0] = np.inf
        refused("query 0", o=bad)
        refused("segment", seg=2)
        refused("coin_out is required", seg=1)                                   # NULL coin_out on an N-coin segment
        with pytest.raises(cr.ArgumentError, match="count"):
            ctx._check(L.cfmm_quote_out(ctx._h, 0, -1, None, None, None, None, None))
        # more than the pool holds is an answer, not an error
        big = o.copy(); big[1] = 2.0 * b.R[1, 1 - ci[1]]
        ans = ctx.quote_out(0, big, ci)
        assert ans[1] == np.inf and np.all(np.isfinite(np.delete(ans, 1)))
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
        ci, co, o = wanted(ctx, b, n)
        if co is None:
            co = (1 - ci).astype(np.int32)
        good = ctx.quote_out(0, o, ci, co)
        idx = np.arange(n, dtype=np.int64)
        idx[3], idx[4] = 200, -5                                                 # clamped before any read, then poisoned
        ci2, co2, o2 = ci.copy(), co.copy(), o.copy()
        ci2[10], co2[11] = b.Ai.shape[1], -1
        co2[12] = ci2[12]
        o2[20], o2[21], o2[22] = -1.0, np.nan, np.inf
        bad = np.zeros(n, dtype=bool)
        bad[[3, 4, 10, 11, 12, 20, 21, 22]] = True
        dev = torch.device("cuda:0")
        t = [torch.from_numpy(x).to(dev) for x in (idx, ci2, co2, o2)]
        t_ans = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.quote_out_dev(0, n, t[3].data_ptr(), t[1].data_ptr(), t_ans.data_ptr(), t[2].data_ptr(), t[0].data_ptr())
            torch.cuda.synchronize()
        finally:
            ctx.reset_stream()
        ans = t_ans.cpu().numpy()
        assert np.all(np.isnan(ans[bad]))
        np.testing.assert_array_equal(ans[~bad], good[~bad])
    finally:
        be.close()


# ---- large-market mode -------------------------------------------------------------------------------------------------------
def test_large_market_mode_gives_the_same_bits():
    m = 3000
    small = synth.product_pools(m, N, seed=95)
    big = batch_with(small, Ai=np.where(small.Ai == 1, 8193, small.Ai))     # one token beyond the LDS limit: n_tokens = 8193
    be_s, be_b = cr.DeviceBackend(N, [small]), cr.DeviceBackend(8193, [big])
    try:
        ci, _, o = wanted(be_s.ctx, small, m)
        np.testing.assert_array_equal(be_b.ctx.quote_out(0, o, ci), be_s.ctx.quote_out(0, o, ci))
        pick = np.random.default_rng(5).integers(0, m, 500)
        np.testing.assert_array_equal(be_b.ctx.quote_out(0, o[pick], ci[pick], None, pick),
                                      be_s.ctx.quote_out(0, o[pick], ci[pick], None, pick))
    finally:
        be_s.close()
        be_b.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------
def test_the_example_sizes_the_inputs_and_the_forward_quote_confirms():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("quote_out_example", os.path.join(root, "examples", "quote_out.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    idx, D, L, want, tender, got = mod.main(m=2000, moved=10)
    assert idx.size >= 10 and np.all(np.isfinite(tender)) and np.all(tender > 0)
    assert np.all(tender < D.max(axis=1))                              # 0.9 of the output costs less than the whole input
    np.testing.assert_allclose(got, want, rtol=1e-12)
