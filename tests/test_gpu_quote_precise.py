"""The 60-digit quote fixture (tests/golden/quote_precise.npz) through the device: cfmm_quote, cfmm_quote_dev on torch
tensors, a sparse permuted idx and a 2-device-id multi-device context on one GPU, all held to the bounds and the K of
tests/quote_precise_ref.py -- the K the host build of the same functions is held to (tests/test_quote_precise_cpu.py).
Run with -s for the measured maxima (profiles/quote_gpu_tests.log).

Measured on MI355X, worst ratio per family over all four paths (the paths agree bit for bit): see profiles/quote_gpu_tests.log."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P

pytestmark = pytest.mark.gpu

N_TOKENS = 8


def upload(ctx, gname, g):
    """every row of a pool group as its own pool (UniV3: the group's pools), tokens 0 .. n-1"""
    fam = P.family(gname)
    if gname == "univ3":
        p = g["current_price"].size
        Ai0 = np.tile(np.array([0, 1], dtype=np.int32), (p, 1))
        ctx.add_univ3(g["current_price"], g["pool_gamma"], Ai0, g["tick_off"], g["lower_ticks"], g["liquidity"])
        return
    m, n = g["R"].shape
    Ai0 = np.tile(np.arange(n, dtype=np.int32), (m, 1))
    if fam == "product":
        ctx.add_product(g["R"], g["gamma"], Ai0)
    elif fam == "solidly":
        ctx.add_solidly(g["R"], g["gamma"], Ai0)
    elif fam == "geomean":
        ctx.add_geomean(g["R"], g["w"], g["gamma"], Ai0)
    elif fam == "weighted":
        ctx.add_weighted(g["R"], g["w"], g["gamma"], Ai0)
    else:
        ctx.add_curve(g["R"], g["gamma"], Ai0, g["alpha"], g["beta"])


def queries(gname, g):
    """(idx, coin_in, coin_out or None, amounts): UniV3 queries name their pool, the others are row by row"""
    if gname == "univ3":
        return g["pool"].astype(np.int64), g["cin"], None, g["a"]
    two = g["R"].shape[1] == 2 and P.family(gname) not in ("weighted", "curve")
    return np.arange(g["a"].size, dtype=np.int64), g["cin"], None if two else g["cout"], g["a"]


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


def check(out, g, gname, label):
    r = P.ratios(out, g)
    for c in np.unique(g["cls"]):
        sel = g["cls"] == c
        K = P.K_of(gname, str(c))
        worst = float(np.max(r[sel]))
        print(f"{label} {gname}/{c}: worst {worst:.3g} of K = {K}")
        assert np.all(np.isfinite(out[sel])) and worst <= K, (label, gname, c, worst, K)


def test_host_pointer_quotes_within_the_bounds(case):
    gname, g, ctx = case
    idx, ci, co, a = queries(gname, g)
    out = ctx.quote(0, a, ci, co, None if gname != "univ3" else idx)       # dense where query q is row q
    check(out, g, gname, "cfmm_quote")
    zero = ctx.quote(0, np.zeros(a.size), ci, co, idx)
    assert np.all(zero.view(np.uint64) == 0)                               # a == 0: +0.0 bit for bit


def test_device_pointer_quotes_are_the_same_bits(case):
    import torch
    gname, g, ctx = case
    idx, ci, co, a = queries(gname, g)
    ref = ctx.quote(0, a, ci, co, idx)
    dev = torch.device("cuda:0")
    t_idx = torch.from_numpy(idx).to(dev)
    t_ci = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(dev)
    t_co = None if co is None else torch.from_numpy(np.ascontiguousarray(co, dtype=np.int32)).to(dev)
    t_a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_out = torch.full((a.size,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.quote_dev(0, a.size, t_a.data_ptr(), t_ci.data_ptr(), t_out.data_ptr(), 0 if t_co is None else t_co.data_ptr(),
                      t_idx.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    out = t_out.cpu().numpy()
    check(out, g, gname, "cfmm_quote_dev")
    np.testing.assert_array_equal(out, ref)


def test_sparse_permuted_idx_and_a_multi_device_context(case):
    gname, g, ctx = case
    idx, ci, co, a = queries(gname, g)
    ref = ctx.quote(0, a, ci, co, idx)
    perm = np.random.default_rng(3).permutation(a.size)
    out = ctx.quote(0, a[perm], ci[perm], None if co is None else co[perm], idx[perm])
    np.testing.assert_array_equal(out, ref[perm])
    multi = cr.Context(N_TOKENS, [0, 0])
    try:
        upload(multi, gname, g)
        out = multi.quote(0, a[perm], ci[perm], None if co is None else co[perm], idx[perm])
        check(out[np.argsort(perm)], g, gname, "multi-device")
        np.testing.assert_array_equal(out, ref[perm])
    finally:
        multi.close()
