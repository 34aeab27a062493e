"""The 80-digit rate fixture (tests/golden/rate_precise.npz) through the device: cfmm_quote_rate, cfmm_quote_rate_dev on torch
tensors, a sparse permuted idx, a 2-device-id multi-device context on one GPU and the call without amounts, all held to the
bounds and the K of tests/rate_precise_ref.py -- the K the host build of the same functions is held to
(tests/test_rate_precise_cpu.py) -- and the amounts beside the rates to cfmm_quote's bits.
Run with -s for the measured maxima (profiles/rate_gpu_tests.log)."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
import rate_precise_ref as RP
from test_gpu_quote_precise import N_TOKENS, upload

pytestmark = pytest.mark.gpu


def queries(gname, g):
    """(idx, coin_in, coin_out or None, amounts) of the rate fixture's rows: every row of the quote fixture is a pool (UniV3: the
    group's pools), and a rate row names the pool it was made from"""
    if gname == "univ3":
        return g["pool"].astype(np.int64), g["cin"].astype(np.int32), None, g["a"]
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    return g["row"].astype(np.int64), g["cin"].astype(np.int32), None if two else g["cout"].astype(np.int32), g["a"]


@pytest.fixture(scope="module")
def fxs():
    return RP.load()


@pytest.fixture(scope="module", params=RP.GROUPS)
def case(request, fxs):
    gname = request.param
    g = RP.group(fxs, gname)
    ctx = cr.Context(N_TOKENS, 0)
    upload(ctx, gname, P.group(fxs[0], gname))
    idx, ci, co, a = queries(gname, g)
    ref = ctx.quote_rate(0, a, ci, co, idx)          # computed once, shared, left unchanged
    yield gname, g, ctx, ref
    ctx.close()


def check(rate, g, gname, label):
    r = RP.ratios(rate, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = RP.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert np.all(np.isfinite(rate[sel])) and worst <= K, (label, gname, c, worst, K)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_host_pointer_rates_within_the_bounds_and_amounts_are_the_quotes(case):
    gname, g, ctx, (out, rate) = case
    idx, ci, co, a = queries(gname, g)
    check(rate, g, gname, "cfmm_quote_rate")
    np.testing.assert_array_equal(bits(out), bits(ctx.quote(0, a, ci, co, idx)))         # cfmm_quote's bits
    zero = a == 0.0
    assert zero.sum() >= a.size // 8 and np.all(bits(out[zero]) == 0) and np.all(np.isfinite(rate[zero]))
    assert np.all(bits(rate[g["cls"] == "exhausted"]) == 0)                               # exactly +0.0
    if gname != "univ3":                                                                  # dense: query q is row q
        n = a.size // 2
        d_out, d_rate = ctx.quote_rate(0, a[:n], ci[:n], None if co is None else co[:n])
        np.testing.assert_array_equal(bits(d_out), bits(out[:n]))
        np.testing.assert_array_equal(bits(d_rate), bits(rate[:n]))


def test_device_pointer_rates_are_the_same_bits(case):
    import torch
    gname, g, ctx, (ref_out, ref_rate) = case
    idx, ci, co, a = queries(gname, g)
    dev = torch.device("cuda:0")
    t_idx = torch.from_numpy(idx).to(dev)
    t_ci = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(dev)
    t_co = None if co is None else torch.from_numpy(np.ascontiguousarray(co, dtype=np.int32)).to(dev)
    t_a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_out = torch.full((a.size,), -1.0, dtype=torch.float64, device=dev)
    t_rate = torch.full((a.size,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.quote_rate_dev(0, a.size, t_a.data_ptr(), t_ci.data_ptr(), t_out.data_ptr(), t_rate.data_ptr(),
                           0 if t_co is None else t_co.data_ptr(), t_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    np.testing.assert_array_equal(bits(t_out.cpu().numpy()), bits(ref_out))
    np.testing.assert_array_equal(bits(t_rate.cpu().numpy()), bits(ref_rate))


def test_sparse_permuted_idx_and_a_multi_device_context(case):
    gname, g, ctx, (ref_out, ref_rate) = case
    idx, ci, co, a = queries(gname, g)
    perm = np.random.default_rng(3).permutation(a.size)
    out, rate = ctx.quote_rate(0, a[perm], ci[perm], None if co is None else co[perm], idx[perm])
    np.testing.assert_array_equal(bits(out), bits(ref_out[perm]))
    np.testing.assert_array_equal(bits(rate), bits(ref_rate[perm]))
    multi = cr.Context(N_TOKENS, [0, 0])
    try:
        upload(multi, gname, P.group(RP.load()[0], gname))
        out, rate = multi.quote_rate(0, a[perm], ci[perm], None if co is None else co[perm], idx[perm])
        np.testing.assert_array_equal(bits(out), bits(ref_out[perm]))
        np.testing.assert_array_equal(bits(rate), bits(ref_rate[perm]))
        _, spot = multi.quote_rate(0, None, ci[perm], None if co is None else co[perm], idx[perm], want_out=False)
        np.testing.assert_array_equal(bits(spot), bits(ctx.quote_rate(0, np.zeros(a.size), ci[perm], None if co is None else co[perm], idx[perm])[1]))
    finally:
        multi.close()


def test_no_amounts_is_an_array_of_zeros(case):
    gname, g, ctx, _ = case
    idx, ci, co, a = queries(gname, g)
    z_out, z_rate = ctx.quote_rate(0, np.zeros(a.size), ci, co, idx)
    n_out, n_rate = ctx.quote_rate(0, None, ci, co, idx)                                  # amount_in == NULL
    np.testing.assert_array_equal(bits(n_out), bits(z_out))
    np.testing.assert_array_equal(bits(n_rate), bits(z_rate))
    none, o_rate = ctx.quote_rate(0, None, ci, co, idx, want_out=False)                   # ... and amount_out == NULL
    assert none is None
    np.testing.assert_array_equal(bits(o_rate), bits(z_rate))
    assert np.all(bits(z_out) == 0)
    sel = a == 0.0                                                                        # the fixture's own a = 0 rows: within K
    if gname == "univ3":
        sel &= ~g["at_boundary"]
    r = RP.ratios(z_rate, g)
    for c in np.unique(g["cls"][sel]):
        assert np.max(r[sel & (g["cls"] == c)]) <= RP.K_of(gname, str(c)), (gname, c)
