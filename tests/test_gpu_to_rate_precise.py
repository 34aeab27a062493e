"""The 80-digit to-rate fixture (tests/golden/to_rate_precise.npz) through the device: cfmm_quote_to_rate, cfmm_quote_to_rate_dev
on torch tensors, a sparse permuted idx and a 2-device-id multi-device context on one GPU, all held to BOTH K tables of
tests/to_rate_precise_ref.py -- the K the host build of the same functions is held to (tests/test_to_rate_precise_cpu.py) --
with the amounts out beside them to cfmm_quote's bits; counts 1, 64 and 65; and the _dev form's refusal of a bad row, coin or
limit, query by query.  Run with -s for the measured maxima."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
import to_rate_precise_ref as TP
from test_gpu_quote_precise import N_TOKENS, upload

pytestmark = pytest.mark.gpu


def queries(gname, g):
    """(idx, coin_in, coin_out or None, limits) of the fixture's rows: every row of the quote fixture is a pool (UniV3: the
    group's pools), and a to-rate row names the pool it was made from"""
    if gname == "univ3":
        return g["pool"].astype(np.int64), g["cin"].astype(np.int32), None, g["r"]
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    return g["row"].astype(np.int64), g["cin"].astype(np.int32), None if two else g["cout"].astype(np.int32), g["r"]


@pytest.fixture(scope="module")
def fxs():
    return TP.load()


@pytest.fixture(scope="module", params=TP.GROUPS)
def case(request, fxs):
    gname = request.param
    g = TP.group(fxs, gname)
    ctx = cr.Context(N_TOKENS, 0)
    upload(ctx, gname, P.group(fxs[0], gname))
    idx, ci, co, r = queries(gname, g)
    ref = ctx.quote_to_rate(0, r, ci, co, idx)          # computed once, shared, left unchanged
    yield gname, g, ctx, ref
    ctx.close()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_host_pointer_amounts_within_both_bounds_and_outs_are_the_quotes(case):
    gname, g, ctx, (amount, out) = case
    idx, ci, co, r = queries(gname, g)
    assert not np.any(np.isnan(amount))
    fin = np.isfinite(amount)
    back = np.zeros(r.size)
    back[fin] = ctx.quote_rate(0, amount[fin], ci[fin], None if co is None else co[fin], idx[fin])[1]   # the round trip
    ra, rr = TP.ratios(amount, g), TP.rate_ratios(back, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K, Kr = TP.K_of(gname, str(c)), TP.K_rate_of(gname, str(c))
        worst, worst_r = float(np.max(ra[sel])), float(np.max(rr[sel]))
        print(f"cfmm_quote_to_rate {gname}/{c}: amount worst {worst:.3g} of K = {K}, rate worst {worst_r:.3g} of K = {Kr}")
        assert worst <= K, (gname, c, worst, K)
        assert worst_r <= Kr, (gname, c, worst_r, Kr)
    np.testing.assert_array_equal(bits(out[fin]), bits(ctx.quote(0, amount[fin], ci[fin], None if co is None else co[fin], idx[fin])))
    zero = g["a"] == 0.0
    assert zero.sum() >= r.size // 8 and np.all(bits(amount[zero]) == 0) and np.all(bits(out[zero]) == 0)
    if gname == "univ3":   # the capacity: what cfmm_quote_out reports for everything the direction gives
        cap = g["capacity"]
        assert cap.any()
        total = ctx.quote(0, 2.0 * amount[cap], ci[cap], None, idx[cap])       # (twice the capacity: the direction's total)
        np.testing.assert_array_equal(bits(ctx.quote_out(0, total, ci[cap], None, idx[cap])), bits(amount[cap]))
    only_in, none = ctx.quote_to_rate(0, r, ci, co, idx, want_out=False)                   # amount_out == NULL
    assert none is None
    np.testing.assert_array_equal(bits(only_in), bits(amount))
    # read-only: the pools quote what they quoted
    again = ctx.quote_to_rate(0, r, ci, co, idx)
    np.testing.assert_array_equal(bits(again[0]), bits(amount))
    np.testing.assert_array_equal(bits(again[1]), bits(out))


def test_device_pointer_form_gives_the_same_bits(case):
    import torch
    gname, g, ctx, (ref_in, ref_out) = case
    idx, ci, co, r = queries(gname, g)
    dev = torch.device("cuda:0")
    t_idx = torch.from_numpy(idx).to(dev)
    t_ci = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(dev)
    t_co = None if co is None else torch.from_numpy(np.ascontiguousarray(co, dtype=np.int32)).to(dev)
    t_r = torch.from_numpy(np.ascontiguousarray(r)).to(dev)
    t_in = torch.full((r.size,), -1.0, dtype=torch.float64, device=dev)
    t_out = torch.full((r.size,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.quote_to_rate_dev(0, r.size, t_r.data_ptr(), t_ci.data_ptr(), t_in.data_ptr(), t_out.data_ptr(),
                              0 if t_co is None else t_co.data_ptr(), t_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    np.testing.assert_array_equal(bits(t_in.cpu().numpy()), bits(ref_in))
    np.testing.assert_array_equal(bits(t_out.cpu().numpy()), bits(ref_out))


def test_sparse_permuted_idx_counts_and_a_multi_device_context(case):
    gname, g, ctx, (ref_in, ref_out) = case
    idx, ci, co, r = queries(gname, g)
    perm = np.random.default_rng(3).permutation(r.size)
    sub = lambda a, s: None if a is None else a[s]   # noqa: E731
    amount, out = ctx.quote_to_rate(0, r[perm], ci[perm], sub(co, perm), idx[perm])
    np.testing.assert_array_equal(bits(amount), bits(ref_in[perm]))
    np.testing.assert_array_equal(bits(out), bits(ref_out[perm]))
    for count in (1, 64, 65):
        s = perm[:count]
        amount, out = ctx.quote_to_rate(0, r[s], ci[s], sub(co, s), idx[s])
        np.testing.assert_array_equal(bits(amount), bits(ref_in[s]))
        np.testing.assert_array_equal(bits(out), bits(ref_out[s]))
    multi = cr.Context(N_TOKENS, [0, 0])
    try:
        upload(multi, gname, P.group(TP.load()[0], gname))
        amount, out = multi.quote_to_rate(0, r[perm], ci[perm], sub(co, perm), idx[perm])
        np.testing.assert_array_equal(bits(amount), bits(ref_in[perm]))
        np.testing.assert_array_equal(bits(out), bits(ref_out[perm]))
    finally:
        multi.close()


def test_dev_form_poisons_a_bad_query_alone(case):
    import torch
    gname, g, ctx, (ref_in, ref_out) = case
    idx, ci, co, r = queries(gname, g)
    n = min(r.size, 65)
    idx, ci, r = idx[:n].copy(), ci[:n].copy(), r[:n].copy()
    co = (1 - ci if co is None else co[:n]).astype(np.int32).copy()
    m = int(idx.max()) + 1
    bad = {1: "row", 3: "row", 5: "coin", 7: "coin", 9: "same", 11: "limit", 13: "limit", 15: "limit", 17: "limit"}
    idx[1], idx[3] = -1, 1 << 40
    ci[5], co[7] = -2, 99
    co[9] = ci[9]
    r[11], r[13], r[15], r[17] = 0.0, -1.0, np.inf, np.nan
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    t_idx, t_ci, t_co, t_r = to(idx), to(ci), to(co), to(r)
    t_in = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    t_out = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.quote_to_rate_dev(0, n, t_r.data_ptr(), t_ci.data_ptr(), t_in.data_ptr(), t_out.data_ptr(), t_co.data_ptr(), t_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    got_in, got_out = t_in.cpu().numpy(), t_out.cpu().numpy()
    good = np.array([q not in bad for q in range(n)])
    assert m > 0 and np.all(np.isnan(got_in[~good])) and np.all(np.isnan(got_out[~good]))
    np.testing.assert_array_equal(bits(got_in[good]), bits(ref_in[:n][good]))
    np.testing.assert_array_equal(bits(got_out[good]), bits(ref_out[:n][good]))


def test_host_checks_name_the_query_and_leave_the_outputs(case):
    gname, g, ctx, _ = case
    idx, ci, co, r = queries(gname, g)
    for value, text in ((0.0, "rate_limit must be finite and > 0"), (-1.0, "rate_limit must be finite and > 0"),
                        (np.inf, "rate_limit must be finite and > 0"), (np.nan, "rate_limit must be finite and > 0")):
        lim = r[:4].copy()
        lim[2] = value
        with pytest.raises(cr.ArgumentError, match=f"cfmm_quote_to_rate: query 2: {text}"):
            ctx.quote_to_rate(0, lim, ci[:4], None if co is None else co[:4], idx[:4])
    bad = idx[:4].copy()
    bad[1] = 1 << 40
    with pytest.raises(cr.ArgumentError, match="cfmm_quote_to_rate: query 1: row"):
        ctx.quote_to_rate(0, r[:4], ci[:4], None if co is None else co[:4], bad)
    assert ctx.quote_to_rate(0, np.empty(0), np.empty(0, dtype=np.int32), None if co is None else np.empty(0, dtype=np.int32),
                             np.empty(0, dtype=np.int64))[0].size == 0


def test_limit_ns_reports_the_kernel_span(case):
    gname, g, ctx, (ref_in, _) = case
    idx, ci, co, r = queries(gname, g)
    ctx.set_option("time_kernels", 1)
    try:
        amount, _ = ctx.quote_to_rate(0, r, ci, co, idx)
        assert ctx.get_option("limit_ns") > 0
        np.testing.assert_array_equal(bits(amount), bits(ref_in))
    finally:
        ctx.set_option("time_kernels", 0)
