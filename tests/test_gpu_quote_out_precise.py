"""The 80-digit exact-output fixture (tests/golden/quote_out_precise.npz) through the device: cfmm_quote_out, cfmm_quote_out_dev
on torch tensors, a sparse permuted idx and a 2-device-id multi-device context on one GPU.  The four paths must agree bit for
bit, and all are held to the bounds and the K of tests/quote_out_precise_ref.py -- the K the host build of the same functions is
held to (tests/test_quote_out_precise_cpu.py); rows whose truth is +inf must be +inf.
Run with -s for the measured maxima: the device's worst ratio per class is in profiles/quote_out_gpu_tests.log."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_out_precise_ref as P
from test_gpu_quote_precise import N_TOKENS, upload

pytestmark = pytest.mark.gpu


def queries(gname, g):
    """(idx, coin_in, coin_out or None, wanted outputs): UniV3 queries name their pool, the others are row by row"""
    if gname == "univ3":
        return g["pool"].astype(np.int64), g["cin"], None, g["o"]
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    return np.arange(g["o"].size, dtype=np.int64), g["cin"], None if two else g["cout"], g["o"]


@pytest.fixture(scope="module")
def fx():
    return P.load()


@pytest.fixture(scope="module", params=P.GROUPS)
def case(request, fx):
    gname = request.param
    g = P.group(fx, gname)
    ctx = cr.Context(N_TOKENS, 0)
    upload(ctx, gname, g)
    yield gname, g, ctx
    ctx.close()


def check(a, g, gname, label):
    r = P.ratios(a, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = P.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert not np.any(np.isnan(a[sel])) and worst <= K, (label, gname, c, worst, K)
    np.testing.assert_array_equal(np.isinf(a), np.isinf(g["a"]))


def test_host_pointer_quotes_within_the_bounds(case):
    gname, g, ctx = case
    idx, ci, co, o = queries(gname, g)
    a = ctx.quote_out(0, o, ci, co, None if gname != "univ3" else idx)     # dense where query q is row q
    check(a, g, gname, "cfmm_quote_out")
    zero = ctx.quote_out(0, np.zeros(o.size), ci, co, idx)
    assert np.all(zero.view(np.uint64) == 0)                               # o == 0: +0.0 bit for bit


def test_device_pointer_quotes_are_the_same_bits(case):
    import torch
    gname, g, ctx = case
    idx, ci, co, o = queries(gname, g)
    ref = ctx.quote_out(0, o, ci, co, idx)
    dev = torch.device("cuda:0")
    t_idx = torch.from_numpy(idx).to(dev)
    t_ci = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(dev)
    t_co = None if co is None else torch.from_numpy(np.ascontiguousarray(co, dtype=np.int32)).to(dev)
    t_o = torch.from_numpy(np.ascontiguousarray(o)).to(dev)
    t_a = torch.full((o.size,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.quote_out_dev(0, o.size, t_o.data_ptr(), t_ci.data_ptr(), t_a.data_ptr(), 0 if t_co is None else t_co.data_ptr(),
                          t_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    a = t_a.cpu().numpy()
    check(a, g, gname, "cfmm_quote_out_dev")
    np.testing.assert_array_equal(a, ref)


def test_sparse_permuted_idx_and_a_multi_device_context(case):
    gname, g, ctx = case
    idx, ci, co, o = queries(gname, g)
    ref = ctx.quote_out(0, o, ci, co, idx)
    perm = np.random.default_rng(3).permutation(o.size)
    a = ctx.quote_out(0, o[perm], ci[perm], None if co is None else co[perm], idx[perm])
    np.testing.assert_array_equal(a, ref[perm])
    multi = cr.Context(N_TOKENS, [0, 0])
    try:
        upload(multi, gname, g)
        a = multi.quote_out(0, o[perm], ci[perm], None if co is None else co[perm], idx[perm])
        check(a[np.argsort(perm)], g, gname, "multi-device")
        np.testing.assert_array_equal(a, ref[perm])
    finally:
        multi.close()
