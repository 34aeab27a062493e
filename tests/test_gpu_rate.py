"""cfmm_quote_rate / cfmm_quote_rate_dev on the device beyond the 80-digit fixture (tests/test_gpu_rate_precise.py): launch
geometry, the refusals of the host-pointer entry, the poison rule and the multi-device refusal of the device-pointer one,
read-only behaviour, the kernel span, and the router-level verbs (quote_rate, spot_price, price_impact)."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import OBJ_LINEAR_NONNEGATIVE, ptr
from test_gpu_quote import KINDS, N, pools, typical_queries

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_batches_of_1_65_and_4097_on_a_seven_pool_market(kind):
    """repeated rows: every query of a batch equals its own count-1 call, bit for bit (16 sampled per batch), and the amounts
    are cfmm_quote's"""
    b = pools(kind, 7, seed=11)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ci7, co7, a7 = typical_queries(b, 7)
        rng = np.random.default_rng(12)
        for count in (1, 65, 4097):
            rows = rng.integers(0, 7, count)
            ci, co = ci7[rows], None if co7 is None else co7[rows]
            a = a7[rows] * np.exp(rng.uniform(np.log(1e-3), np.log(30.0), count))
            a[rng.integers(0, count, max(1, count // 16))] = 0.0
            out, rate = ctx.quote_rate(0, a, ci, co, rows)
            np.testing.assert_array_equal(bits(out), bits(ctx.quote(0, a, ci, co, rows)))
            assert np.all(np.isfinite(rate)) and np.all(rate >= 0.0)
            for q in rng.choice(count, min(16, count), replace=False):
                o1, r1 = ctx.quote_rate(0, a[q:q + 1], ci[q:q + 1], None if co is None else co[q:q + 1], rows[q:q + 1])
                assert bits(o1)[0] == bits(out)[q] and bits(r1)[0] == bits(rate)[q], (kind, count, q)
        # count == 0 is a no-op that accepts NULL arrays
        ctx._check(cr.lib().cfmm_quote_rate(ctx._h, 0, 0, None, None, None, None, None, None))
    finally:
        be.close()


def test_rate_falls_along_a_ladder_and_matches_the_slope_of_the_quote():
    """every kind but UniV3 (whose rate is piecewise): the rate decreases with the amount, stays below the spot rate, and
    agrees with a central difference of cfmm_quote to 1e-5 (doubles lose half the digits: a coarse, form-independent check).
    The difference of two quotes carries their rounding, a few u·out each, over 2e·a: relative to the rate that is
    u·out/(e·a·rate), so the comparison is made where out < 1e3·a·rate (1e-7 then) -- a trade that has all but emptied the
    pool has a rate far below out/a and no finite difference in doubles resolves it."""
    for kind in ("product", "geomean", "weighted", "curve", "solidly"):
        b = pools(kind, 7, seed=13)
        be = cr.DeviceBackend(N, [b])
        try:
            ctx = be.ctx
            ci7, co7, a7 = typical_queries(b, 7)
            sizes = np.array([0.0, 0.01, 0.1, 0.5, 1.0, 3.0])
            rows = np.repeat(np.arange(7), sizes.size)
            ci, co = ci7[rows], None if co7 is None else co7[rows]
            a = a7[rows] * np.tile(sizes, 7)
            out, rate = ctx.quote_rate(0, a, ci, co, rows)
            r = rate.reshape(7, sizes.size)
            assert np.all(np.diff(r, axis=1) < 0.0) and np.all(r > 0.0), kind
            e = 1e-6
            up, dn = ctx.quote(0, a * (1 + e), ci, co, rows), ctx.quote(0, a * (1 - e), ci, co, rows)
            sel = (a > 0.0) & (out < 1e3 * a * rate)
            assert sel.sum() >= 21, (kind, sel.sum())
            fd = (up[sel] - dn[sel]) / (2 * e * a[sel])
            np.testing.assert_allclose(fd, rate[sel], rtol=1e-5, err_msg=kind)
        finally:
            be.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_host_variant_refuses_names_the_query_and_leaves_the_outputs():
    L = cr.lib()
    b, w = pools("product", 50, 81), pools("weighted", 50, 82)
    be = cr.DeviceBackend(N, [b, w])
    try:
        ctx = be.ctx
        ci, _, a = typical_queries(b, 10)
        idx = np.arange(10, dtype=np.int64)

        def refused(match, seg=0, idx=idx, ci=ci, co=None, a=a, null_out=False, null_rate=False):
            out, rate = np.full(10, 7.0), np.full(10, 7.0)
            rc = L.cfmm_quote_rate(ctx._h, seg, 10, ptr(idx), ptr(np.ascontiguousarray(ci, dtype=np.int32)),
                                   ptr(None if co is None else np.ascontiguousarray(co, dtype=np.int32)),
                                   ptr(None if a is None else np.ascontiguousarray(a)), None if null_out else ptr(out),
                                   None if null_rate else ptr(rate))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and match in msg and msg.startswith("cfmm_quote_rate:"), (rc, msg)
            assert np.all(out == 7.0) and np.all(rate == 7.0)              # the outputs are untouched
        bad = idx.copy(); bad[4] = 50
        refused("query 4: row 50 out of range", idx=bad)
        bad = idx.copy(); bad[9] = -1
        refused("query 9", idx=bad)
        bad = ci.copy(); bad[3] = 2
        refused("query 3: coin_in 2 out of range", ci=bad)
        refused("query 2: coin_in and coin_out are both", co=np.where(np.arange(10) == 2, ci, 1 - ci))
        refused("coin_out is required", seg=1)                            # NULL coin_out on a weighted segment
        bad = a.copy(); bad[5] = -1.0
        refused("query 5: amount_in must be finite and >= 0", a=bad)
        bad = a.copy(); bad[6] = np.nan
        refused("query 6", a=bad)
        bad = a.copy(); bad[0] = np.inf
        refused("query 0", a=bad)
        refused("null query array", null_rate=True)                       # a null output
        refused("null query array", null_out=True)                        # amount_out may be NULL only without amounts
        refused("query 4", idx=np.where(np.arange(10) == 4, 50, idx), a=None, null_out=True)   # no amounts: the same checks
        refused("segment", seg=2)
        with pytest.raises(cr.ArgumentError, match="count"):
            ctx._check(L.cfmm_quote_rate(ctx._h, 0, -1, None, None, None, None, None, None))
    finally:
        be.close()


@pytest.mark.parametrize("kind", ("product", "univ3", "curve"))
def test_device_variant_poisons_both_outputs_of_exactly_the_bad_queries(kind):
    import torch
    b = pools(kind, 200, 91)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        n = 64
        ci, co, a = typical_queries(b, n)
        if co is None:
            co = (1 - ci).astype(np.int32)
        good_out, good_rate = ctx.quote_rate(0, a, ci, co)
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
        t_out, t_rate = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.quote_rate_dev(0, n, t[3].data_ptr(), t[1].data_ptr(), t_out.data_ptr(), t_rate.data_ptr(), t[2].data_ptr(), t[0].data_ptr())
            torch.cuda.synchronize()
        finally:
            ctx.reset_stream()
        out, rate = t_out.cpu().numpy(), t_rate.cpu().numpy()
        assert np.all(np.isnan(out[bad])) and np.all(np.isnan(rate[bad]))
        np.testing.assert_array_equal(bits(out[~bad]), bits(good_out[~bad]))
        np.testing.assert_array_equal(bits(rate[~bad]), bits(good_rate[~bad]))
    finally:
        be.close()


def test_device_variants_are_unsupported_on_a_multi_device_context():
    multi = cr.Context(N, [0, 0])
    try:
        b = pools("product", 8, 5)
        multi.add_product(b.R, b.γ, (b.Ai - 1).astype(np.int32))
        for call in (lambda: multi.quote_rate_dev(0, 1, 8, 8, 8, 8), lambda: multi.quote_path_rate_dev(1, 1, 8, 8, 8, 8, 8, 8, 8, 8)):
            with pytest.raises(Exception) as e:
                call()
            assert "not available on a multi-device context" in str(e.value), str(e.value)
        assert multi._L.cfmm_quote_rate_dev(multi._h, 0, 1, None, None, None, None, None, None) == -4   # CFMM_ERR_UNSUPPORTED
    finally:
        multi.close()


# ---- read-only ----------------------------------------------------------------------------------------------------------------
def test_rate_calls_change_nothing_the_other_calls_see():
    """sweep, read netflows and reserves; after a batch of rate calls cfmm_netflows, cfmm_get_reserves and a pre-armed
    cfmm_route answer the same bits as on a context that made none"""
    batches = [pools("product", 300, 61), pools("geomean", 300, 62), pools("univ3", 100, 63), pools("solidly", 100, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)

    def run(rates):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def q():
            if not rates:
                return
            for seg in range(4):
                ci, _, a = typical_queries(batches[seg], 100)
                ctx.quote_rate(seg, a, ci)
                ctx.quote_rate(seg, None, ci, count=100, want_out=False)
            ctx.quote_path_rate(np.array([2], dtype=np.int32), np.array([[0, 3]], dtype=np.int32), np.array([[1, 2]], dtype=np.int64),
                                np.array([[0, 0]], dtype=np.int32), np.array([[1, 1]], dtype=np.int32), np.array([1.0]), hops=True)
        try:
            q()                                                        # needs no sweep to have run
            ctx.find_arb(v)
            res.append((ctx.netflows(), ctx.reserves(0, 300), ctx.reserves(3, 100)))
            q()
            res.append((ctx.netflows(), ctx.dual_value(), ctx.reserves(0, 300), ctx.reserves(1, 300), ctx.reserves(3, 100), ctx.trades()))
            vr, psi, info = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=40)      # leaves an evaluation armed
            q()
            vr2, psi2, info2 = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=40)   # the pre-armed route
            res.append((vr, psi, vr2, psi2, [info[k] for k in ("f", "iterations", "evaluations", "status")],
                        [info2[k] for k in ("f", "iterations", "evaluations", "status")], ctx.netflows()))
        finally:
            be.close()
        return res

    a, b = run(True), run(False)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for p, q in zip(x, y):
                same(p, q)
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    same(a, b)
    same(a[0][0], a[1][0])                                             # ... and the netflows before and after the rate calls


def test_rate_ns_is_the_latest_calls_kernel_span():
    b = pools("product", 500, 71)
    be = cr.DeviceBackend(N, [b])
    try:
        ctx = be.ctx
        ci, _, a = typical_queries(b, 300)
        ctx.set_option("time_kernels", 1)
        assert ctx.get_option("rate_ns") == 0
        ctx.quote(0, a, ci)
        assert ctx.get_option("rate_ns") == 0 and ctx.get_option("quote_ns") > 0          # cfmm_quote's span is its own
        ctx.quote_rate(0, a, ci)
        assert 0 < ctx.get_option("rate_ns") < 10_000_000
    finally:
        be.close()


# ---- the router's verbs ---------------------------------------------------------------------------------------------------------
def test_router_verbs_spot_price_and_price_impact():
    import cfmmrouter_amd as pkg
    rng = np.random.default_rng(7)
    cf = [pkg.ProductTwoCoin([1e6, 2e6], 0.997, [1, 2]), pkg.GeometricMeanTwoCoin([1e6, 1e6], [0.3, 0.7], 0.999, [2, 3]),
          pkg.ProductTwoCoin([5e5, 4e5], 1.0, [1, 3]), pkg.SolidlyStableTwoCoin([1e6, 1.1e6], 0.9995, [3, 4])]
    r = pkg.Router(pkg.LinearNonnegative(np.ones(4)), cf, 4)
    which = np.array([0, 1, 2, 3, 0, 3])
    amt = np.array([1e3, 2e3, 0.0, 5e4, 1e5, 1e2]) * (1 + rng.random(6))
    amt[2] = 0.0
    out, rate = pkg.quote_rate(r, which, 0, amt)
    np.testing.assert_array_equal(bits(out), bits(pkg.quote(r, which, 0, amt)))
    spot = pkg.spot_price(r, which, 0)
    np.testing.assert_array_equal(bits(spot), bits(pkg.quote_rate(r, which, 0, 0.0)[1]))
    every = pkg.spot_price(r)                                          # every device pool, one dense call per segment
    np.testing.assert_array_equal(bits(every[which]), bits(spot))
    assert abs(every[0] - 0.997 * 2e6 / 1e6) <= 4 * 2.0 ** -53 * every[0]
    imp = pkg.price_impact(r, which, 0, amt)
    with np.errstate(all="ignore"):
        want = np.where(amt == 0.0, 0.0, 1.0 - out / (amt * spot))
    np.testing.assert_array_equal(bits(imp), bits(want))
    assert imp[2] == 0.0 and np.all(imp[amt > 0] > 0.0) and imp[4] > imp[0]
    # paths
    paths, toks = [[0, 1], [2], [0, 1, 3]], [[1, 2, 3], [1, 3], [1, 2, 3, 4]]
    pa = np.array([1e3, 1e2, 1e4])
    pout, prate, hv, hr = pkg.quote_path_rate(r, paths, toks, pa, hops=True)
    qout, qhv = pkg.quote_path(r, paths, toks, pa, hops=True)
    np.testing.assert_array_equal(bits(pout), bits(qout))
    np.testing.assert_array_equal(bits(hv), bits(qhv))
    assert prate[0] == hr[0, 0] * hr[1, 0] and prate[1] == hr[0, 1] and prate[2] == (hr[0, 2] * hr[1, 2]) * hr[2, 2]
    pimp = pkg.path_price_impact(r, paths, toks, pa)
    assert np.all(pimp > 0.0) and np.all(pimp < 1.0)
    assert np.all(pkg.path_price_impact(r, paths, toks, 0.0) == 0.0)
