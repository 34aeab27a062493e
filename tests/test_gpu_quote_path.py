"""cfmm_quote_path / cfmm_quote_path_out on the device: an amount carried through paths of up to eight pools of eight segments
of different kinds in ONE launch.  The pin of the whole feature is bit-equality with chaining the single-pool calls
(ctx.quote / ctx.quote_out, themselves pinned to 80-digit truths) hop level by hop level: the answer and every intermediate
amount.  Around it: launch geometry, the device-pointer entries, a multi-device parent, large-market mode, live state (the
segment table must never be stale), read-only behaviour, errors, ownership and the router-level calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import KIND_UNIV3, OBJ_LINEAR_NONNEGATIVE, ptr
from cfmmrouter_amd.cfmms import _upload
from test_gpu_pool_update import batch_with, moved_prices, rows_of
from test_gpu_quote import N, pools

pytestmark = pytest.mark.gpu

M = 257                 # pools per segment: one block plus a lane
COUNT = 1025            # paths: four blocks plus a lane
H = 8                   # max_hops
SEED = 7                # chosen on the CPU (numpy restatements of tests/quote_precise_ref.py) so that few paths end in 0.0
SEGMENTS = (("product", 2), ("geomean", 2), ("solidly", 2), ("univ3", 2), ("weighted", 3), ("weighted", 8), ("curve", 2), ("curve", 4))
PATTERNS = ("interleaved", "uniform")


def market(seed=SEED):
    """eight segments of M pools; the UniV3 ladders have 1..16 ticks, a tenth of them without liquidity"""
    out = []
    for s, (kind, nc) in enumerate(SEGMENTS):
        if kind == "univ3":
            b = synth.univ3_ragged_pools(M, N, min_ticks=1, max_ticks=16, seed=seed + s)
            zero = synth.uniform(seed + 100, 5, b.liquidity.size) < 0.1
            b = batch_with(b, liquidity=np.where(zero, 0.0, b.liquidity))
        else:
            b = pools(kind, M, seed=seed + s, n_coins=nc)
        out.append(b)
    return out


def scale_in(b):
    """[m, coins] the size an amount tendered to each coin is measured in: the reserve R_i (UniV3: the pool's √liquidity scale,
    as tests/test_gpu_quote.py typical_queries)"""
    if b.kind == KIND_UNIV3:
        return np.repeat(np.sqrt(b.liquidity[b.tick_off[:-1]] + 1.0)[:, None], 2, axis=1)
    return b.R


def make_paths(batches, pattern, count=COUNT, seed=SEED):
    """n_hops[p] = 1 + p % 8; segment (p + 3k) % 8 (neighbouring lanes in different kinds at every hop) or k % 8 (a wavefront is
    uniform); rows pseudo-random with repeats across paths; coins cycling through every ordered pair of the pool's coins; the
    first amount R_i·10^u, u uniform in [-6, 0.5]"""
    p, k = np.meshgrid(np.arange(count), np.arange(H), indexing="ij")
    n_hops = (1 + np.arange(count) % H).astype(np.int32)
    seg = ((p + 3 * k) % 8 if pattern == "interleaved" else k % 8).astype(np.int32)
    row = np.minimum((synth.uniform(seed + 200, 3, count * H).reshape(count, H) * M).astype(np.int64), M - 1)
    ci, co = np.zeros((count, H), dtype=np.int32), np.zeros((count, H), dtype=np.int32)
    for s, b in enumerate(batches):
        nc = b.Ai.shape[1]
        pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
        at = seg == s
        pick = (p[at] + k[at]) % len(pairs)
        ci[at], co[at] = pairs[pick, 0], pairs[pick, 1]
    u = -6.0 + 6.5 * synth.uniform(seed + 300, 4, count)
    first = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(count)])
    return n_hops, seg, row, ci, co, first * 10.0 ** u


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def chain(ctx, paths, nseg=len(SEGMENTS)):
    """x_{k+1} = ctx.quote(hop k, x_k), hop level by hop level and segment by segment -> (answers, [H, count] amounts leaving
    every hop, NaN in the slots a path does not use)"""
    n_hops, seg, row, ci, co, amt = paths
    x = np.array(amt, dtype=np.float64)
    hv = np.full((seg.shape[1], x.size), np.nan)
    for k in range(seg.shape[1]):
        act = n_hops > k
        for s in range(nseg):
            q = np.flatnonzero(act & (seg[:, k] == s))
            if q.size:
                x[q] = ctx.quote(s, x[q], ci[q, k], co[q, k], row[q, k])
        hv[k, act] = x[act]
    return x, hv


def chain_out(ctx, paths, want, nseg=len(SEGMENTS)):
    """y_k = ctx.quote_out(hop k, y_{k+1}) from the last hop backwards; a path whose amount has become +inf stays there (the
    single-pool call would refuse it as an input) -> (answers, [H, count] amounts to tender to every hop)"""
    n_hops, seg, row, ci, co, _ = paths
    y = np.array(want, dtype=np.float64)
    hv = np.full((seg.shape[1], y.size), np.nan)
    for k in reversed(range(seg.shape[1])):
        act = n_hops > k
        for s in range(nseg):
            q = np.flatnonzero(act & np.isfinite(y) & (seg[:, k] == s))
            if q.size:
                y[q] = ctx.quote_out(s, y[q], ci[q, k], co[q, k], row[q, k])
        hv[k, act] = y[act]
    return y, hv


def used_slots(n_hops, Hn=H):
    return np.arange(Hn)[:, None] < np.asarray(n_hops)[None, :]          # [H, count]


def sliced(paths, sl):
    return tuple(a[sl] for a in paths)


@pytest.fixture(scope="module")
def world():
    """the market on one context, both path patterns and their forward chains, computed once and left unchanged"""
    batches = market()
    be = cr.DeviceBackend(N, batches)
    paths = {pat: make_paths(batches, pat) for pat in PATTERNS}
    fwd = {pat: chain(be.ctx, paths[pat]) for pat in PATTERNS}
    yield batches, be.ctx, paths, fwd
    be.close()


# ---- the pin: the bits of the chain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_forward_is_the_chain_bit_for_bit(world, pattern):
    batches, ctx, paths, fwd = world
    p = paths[pattern]
    want, want_hops = fwd[pattern]
    got, hops = ctx.quote_path(*p, hops=True)
    used = used_slots(p[0])
    same_bits(got, want, "answers")
    same_bits(hops[used], want_hops[used], "hop_out")
    assert np.all(np.isnan(hops[~used]))                                   # unused slots can never be mistaken for amounts
    same_bits(hops[p[0] - 1, np.arange(COUNT)], got, "the last hop's amount is the answer")
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    zero = int(np.sum(got == 0.0))
    print(f"quote_path {pattern}: {COUNT} paths, {zero} end in exactly 0.0 (cap {COUNT // 10}); median answer/amount "
          f"{np.median(got[got > 0] / p[5][got > 0]):.3g}")
    assert zero <= COUNT // 10                                             # the comparison is not one of zeros


@pytest.mark.parametrize("pattern", PATTERNS)
def test_exact_output_is_the_chain_bit_for_bit(world, pattern):
    """amount_out = half the forward answer: feasible at every hop by monotonicity (each hop is asked less than the forward
    walk took from it)"""
    batches, ctx, paths, fwd = world
    p = paths[pattern]
    want_out = 0.5 * fwd[pattern][0]
    want, want_hops = chain_out(ctx, p, want_out)
    got, hops = ctx.quote_path_out(*p[:5], want_out, hops=True)
    used = used_slots(p[0])
    assert np.all(np.isfinite(want))
    same_bits(got, want, "answers")
    same_bits(hops[used], want_hops[used], "hop_in")
    assert np.all(np.isnan(hops[~used]))
    same_bits(hops[0], got, "hop_in of the first hop is the answer")
    live = fwd[pattern][0] > 0
    assert np.all(got[live] <= p[5][live] * (1 + 1e-9))                    # half the output never costs more than the whole input
    print(f"quote_path_out {pattern}: median amount_in / forward amount_in = {np.median(got[live] / p[5][live]):.3g}")


def test_an_infeasible_hop_answers_inf_from_there_to_the_first(world):
    """amount_out = R_o of the pool of the last-but-one hop, on 64 paths chosen so that the last hop can give that much and
    asks for at least as much in return: the last-but-one pool cannot give its whole reserve, so its hop_in, every earlier one
    and the answer are +inf; the last hop's hop_in is the chain's."""
    batches, ctx, paths, fwd = world
    n_hops, seg, row, ci, co, amt = paths["interleaved"]
    q = np.arange(COUNT)
    j = np.maximum(n_hops - 2, 0)
    Ro = np.array([1.0 if batches[seg[p, j[p]]].kind == KIND_UNIV3 else batches[seg[p, j[p]]].R[row[p, j[p]], co[p, j[p]]] for p in q])
    cand = (n_hops >= 2) & np.array([batches[seg[p, j[p]]].kind != KIND_UNIV3 for p in q])
    want, want_hops = chain_out(ctx, paths["interleaved"], np.where(cand, Ro, 0.0))
    last = want_hops[n_hops - 1, q]
    chosen = np.flatnonzero(cand & np.isfinite(last) & (last >= Ro))[:64]
    print(f"infeasible hop: {int(np.sum(cand & np.isfinite(last) & (last >= Ro)))} candidate paths, 64 used")
    assert chosen.size == 64
    p = sliced(paths["interleaved"], chosen)
    got, hops = ctx.quote_path_out(*p[:5], Ro[chosen], hops=True)
    assert np.all(np.isposinf(got))
    for c, path in enumerate(chosen):
        nh = n_hops[path]
        assert np.all(np.isposinf(hops[:nh - 1, c])), path
        assert np.all(np.isnan(hops[nh:, c]))
    same_bits(hops[p[0] - 1, np.arange(64)], last[chosen], "the last hop's hop_in")
    same_bits(got, want[chosen])
    # ... and without the hop amounts the answers are the same
    same_bits(ctx.quote_path_out(*p[:5], Ro[chosen]), got)


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_counts_hops_false_one_hop_and_empty(world):
    batches, ctx, paths, fwd = world
    p = paths["interleaved"]
    want, want_hops = fwd["interleaved"]
    for count in (1, 256, 257, 1025):
        sl = slice(0, count)
        got, hops = ctx.quote_path(*sliced(p, sl), hops=True)
        same_bits(got, want[sl])
        used = used_slots(p[0][sl])
        same_bits(hops[used], want_hops[:, sl][used])
        same_bits(ctx.quote_path(*sliced(p, sl)), want[sl], "hops=False")
        half = 0.5 * want[sl]
        a, _ = ctx.quote_path_out(*sliced(p, sl)[:5], half, hops=True)
        same_bits(ctx.quote_path_out(*sliced(p, sl)[:5], half), a, "hops=False, exact output")
    # max_hops = 1 is ctx.quote itself (here on one segment, so that one call of it answers)
    s = 5
    one = np.ones(COUNT, dtype=np.int32)
    col = lambda a: a[:, :1]
    seg1 = np.full((COUNT, 1), s, dtype=np.int32)
    nc = batches[s].Ai.shape[1]
    ci1, co1 = (np.arange(COUNT) % nc).astype(np.int32), ((np.arange(COUNT) + 3) % nc).astype(np.int32)
    a1 = 0.01 * batches[s].R[p[2][:, 0], ci1]
    same_bits(ctx.quote_path(one, seg1, col(p[2]), ci1, co1, a1), ctx.quote(s, a1, ci1, co1, p[2][:, 0]), "max_hops = 1")
    o1 = 0.01 * batches[s].R[p[2][:, 0], co1]
    same_bits(ctx.quote_path_out(one, seg1, col(p[2]), ci1, co1, o1), ctx.quote_out(s, o1, ci1, co1, p[2][:, 0]), "max_hops = 1, exact output")
    # count = 0 returns empty, through the library too (NULL arrays accepted)
    e = np.zeros((0, H), dtype=np.int32)
    assert ctx.quote_path(np.zeros(0, dtype=np.int32), e, e, e, e, np.zeros(0)).size == 0
    L = cr.lib()
    ctx._check(L.cfmm_quote_path(ctx._h, 0, H, None, None, None, None, None, None, None, None))
    ctx._check(L.cfmm_quote_path_out(ctx._h, 0, 1, None, None, None, None, None, None, None, None))


# ---- the same bits through other routes -----------------------------------------------------------------------------------------
def test_device_pointer_entries_give_the_same_bits(world):
    import torch
    batches, ctx, paths, fwd = world
    p = paths["interleaved"]
    want, want_hops = fwd["interleaved"]
    half = 0.5 * want
    back, back_hops = ctx.quote_path_out(*p[:5], half, hops=True)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_n, t_seg, t_row, t_ci, t_co = up(p[0]), up(p[1].T), up(p[2].T), up(p[3].T), up(p[4].T)     # hop-major, the ABI's layout
    t_amt, t_half = up(p[5]), up(half)
    t_out, t_in = (torch.zeros(COUNT, dtype=torch.float64, device=dev) for _ in range(2))
    t_hops, t_hin = (torch.zeros((H, COUNT), dtype=torch.float64, device=dev) for _ in range(2))
    t_out2 = torch.zeros(COUNT, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        args = [x.data_ptr() for x in (t_n, t_seg, t_row, t_ci, t_co)]
        ctx.quote_path_dev(COUNT, H, *args, t_amt.data_ptr(), t_out.data_ptr(), t_hops.data_ptr())
        ctx.quote_path_out_dev(COUNT, H, *args, t_half.data_ptr(), t_in.data_ptr(), t_hin.data_ptr())
        ctx.quote_path_dev(COUNT, H, *args, t_amt.data_ptr(), t_out2.data_ptr())               # no hop amounts
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    used = used_slots(p[0])
    same_bits(t_out.cpu().numpy(), want)
    same_bits(t_out2.cpu().numpy(), want)
    same_bits(t_in.cpu().numpy(), back)
    hops, hin = t_hops.cpu().numpy(), t_hin.cpu().numpy()
    same_bits(hops[used], want_hops[used])
    same_bits(hin[used], back_hops[used])
    assert np.all(np.isnan(hops[~used])) and np.all(np.isnan(hin[~used]))


def test_a_multi_device_parent_gives_the_same_bits(world):
    batches, ctx, paths, fwd = world
    multi = cr.Context(N, [0, 0])
    try:
        for b in batches:
            _upload(multi, b)
        for pattern in PATTERNS:
            p = paths[pattern]
            want, want_hops = fwd[pattern]
            got, hops = multi.quote_path(*p, hops=True)
            used = used_slots(p[0])
            same_bits(got, want)
            same_bits(hops[used], want_hops[used])
            assert np.all(np.isnan(hops[~used]))
        p = paths["interleaved"]
        half = 0.5 * fwd["interleaved"][0]
        a, ah = ctx.quote_path_out(*p[:5], half, hops=True)
        b_, bh = multi.quote_path_out(*p[:5], half, hops=True)
        same_bits(b_, a)
        same_bits(bh[used_slots(p[0])], ah[used_slots(p[0])])
        same_bits(multi.quote_path_out(*p[:5], half), a)
        # the device-pointer entry is for single-device contexts
        with pytest.raises(NotImplementedError, match="cfmm_quote_path_dev"):
            multi.quote_path_dev(1, 1, 8, 8, 8, 8, 8, 8, 8)
    finally:
        multi.close()


def test_large_market_mode_gives_the_same_bits():
    """two-coin segments only (large-market mode has no N-coin kernel), one token moved beyond the LDS limit"""
    small = market()[:4]                                                  # product, geomean, solidly, univ3
    assert len(small) == 4
    big = [batch_with(b, Ai=np.where(b.Ai == 1, 8193, b.Ai)) for b in small]
    p, k = np.meshgrid(np.arange(COUNT), np.arange(4), indexing="ij")
    n_hops = (1 + np.arange(COUNT) % 4).astype(np.int32)
    seg = ((p + 3 * k) % 4).astype(np.int32)
    row = np.minimum((synth.uniform(11, 3, COUNT * 4).reshape(COUNT, 4) * M).astype(np.int64), M - 1)
    ci = ((p + k) % 2).astype(np.int32)
    co = (1 - ci).astype(np.int32)
    amt = np.array([scale_in(small[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(COUNT)]) * 0.01
    be_s, be_b = cr.DeviceBackend(N, small), cr.DeviceBackend(8193, big)
    try:
        a, ah = be_s.ctx.quote_path(n_hops, seg, row, ci, co, amt, hops=True)
        b, bh = be_b.ctx.quote_path(n_hops, seg, row, ci, co, amt, hops=True)
        same_bits(b, a)
        used = used_slots(n_hops, 4)
        same_bits(bh[used], ah[used])
        same_bits(be_b.ctx.quote_path_out(n_hops, seg, row, ci, co, 0.5 * a), be_s.ctx.quote_path_out(n_hops, seg, row, ci, co, 0.5 * a))
        assert np.any(a > 0)
    finally:
        be_s.close()
        be_b.close()


# ---- live state: the segment table is rebuilt on every call -------------------------------------------------------------------
def test_path_quotes_follow_every_kind_of_update():
    batches = market(seed=21)
    other = market(seed=22)
    paths = make_paths(batches, "interleaved", seed=21)
    be = cr.DeviceBackend(N, batches)
    try:
        ctx = be.ctx
        before = ctx.quote_path(*paths)                                    # a first call: whatever it built must not be reused
        same_bits(before, chain(ctx, paths)[0])
        rows = rows_of(M, 100, 23)
        ctx.set_reserves(0, rows, other[0].R[rows])                        # a sparse update of the product segment
        u = batches[3]                                                     # UniV3: enough mints that the tick arrays move
        regrows = ctx.get_option("pool_update_regrows")
        price = u.current_price.copy()
        for rnd in range(40):
            pick = rows_of(M, M // 2, 50 + rnd)
            price[pick] = moved_prices(u, 60 + rnd)[pick]
            off = np.concatenate([[0], np.cumsum(np.diff(u.tick_off)[pick])])
            sel = np.concatenate([np.arange(u.tick_off[r], u.tick_off[r + 1]) for r in pick])
            ctx.set_ticks(3, pick, price[pick], off, u.lower_ticks[sel], 1.5 * u.liquidity[sel])
            if ctx.get_option("pool_update_regrows") > regrows:
                break
        assert ctx.get_option("pool_update_regrows") > regrows
        after_sparse = ctx.quote_path(*paths)
        same_bits(after_sparse, chain(ctx, paths)[0], "after set_reserves and set_ticks")
        assert np.any(bits(after_sparse) != bits(before))
        ctx.find_arb(synth.sweep_prices(N, seed=24, spread=0.3))
        ctx.update_reserves()                                              # replaces the UniV3 state, rewrites every reserve
        got, hops = ctx.quote_path(*paths, hops=True)
        want, want_hops = chain(ctx, paths)
        same_bits(got, want, "after update_reserves")
        used = used_slots(paths[0])
        same_bits(hops[used], want_hops[used])
        assert np.any(bits(got) != bits(after_sparse))
        back = ctx.quote_path_out(*paths[:5], 0.5 * got)
        same_bits(back, chain_out(ctx, paths, 0.5 * got)[0], "exact output after update_reserves")
    finally:
        be.close()


# ---- read-only ----------------------------------------------------------------------------------------------------------------
def test_path_quotes_change_nothing_the_other_calls_see():
    batches = [pools("product", 700, 61), pools("geomean", 700, 62), pools("univ3", 300, 63), pools("solidly", 300, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)
    p, k = np.meshgrid(np.arange(200), np.arange(4), indexing="ij")
    n_hops = (1 + np.arange(200) % 4).astype(np.int32)
    seg = ((p + k) % 4).astype(np.int32)
    row = ((7 * p + 13 * k) % 300).astype(np.int64)
    ci = ((p + k) % 2).astype(np.int32)
    co = (1 - ci).astype(np.int32)
    amt = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(200)]) * 0.01

    def run(quoting):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def q(out):
            if quoting:
                (ctx.quote_path_out if out else ctx.quote_path)(n_hops, seg, row, ci, co, amt, hops=out)
        try:
            q(False)                                                   # needs no sweep to have run
            ctx.find_arb(v)
            q(True)
            res.append(ctx.trades())
            q(False)
            res.append(ctx.select_trades(0, 0.0))
            q(True)
            res.append((ctx.netflows(), ctx.dual_value()))
            q(False)
            ctx.update_reserves()
            q(True)
            res.append(ctx.eval(v))
            q(False)
            vr, psi, info = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=60)
            q(True)
            res.append((vr, psi, {k_: info[k_] for k_ in ("f", "proj_grad", "iterations", "evaluations", "status")}, ctx.netflows()))
        finally:
            be.close()
        return res

    a, b = run(True), run(False)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for s, t in zip(x, y):
                same(s, t)
        elif isinstance(x, dict):
            assert x == y
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    same(a, b)


# ---- errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("cfmm_quote_path", "cfmm_quote_path_out"))
def test_host_entries_refuse_and_name_path_and_hop(world, entry):
    batches, ctx, paths, fwd = world
    L = cr.lib()
    n = 16
    n_hops, seg, row, ci, co, amt = sliced(paths["interleaved"], slice(0, n))
    amt = amt if entry == "cfmm_quote_path" else 0.5 * fwd["interleaved"][0][:n]

    def refused(match, n_hops=n_hops, seg=seg, row=row, ci=ci, co=co, amt=amt, max_hops=H, count=n):
        out, hops = np.full(n, 7.0), np.full((H, n), 7.0)
        T = lambda a, dt: np.ascontiguousarray(np.asarray(a).T, dtype=dt)
        rc = getattr(L, entry)(ctx._h, count, max_hops, ptr(np.ascontiguousarray(n_hops, dtype=np.int32)), ptr(T(seg, np.int32)),
                               ptr(T(row, np.int64)), ptr(T(ci, np.int32)), ptr(T(co, np.int32)), ptr(np.ascontiguousarray(amt)),
                               ptr(out), ptr(hops))
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith(entry + ":") and match in msg, (rc, msg)
        assert np.all(out == 7.0) and np.all(hops == 7.0)                  # the outputs are untouched

    def edit(a, p, k, value):
        a = a.copy()
        a[p, k] = value
        return a
    # path 12 has 5 hops, path 7 has 8, path 3 has 4
    refused("path 12, hop 3: row", row=edit(row, 12, 3, M))
    refused("path 7, hop 7: row -1", row=edit(row, 7, 7, -1))
    refused("path 3, hop 0: segment 8", seg=edit(seg, 3, 0, 8))
    refused("path 3, hop 2: segment -1", seg=edit(seg, 3, 2, -1))
    k2 = 2
    nc = batches[seg[12, k2]].Ai.shape[1]
    refused(f"path 12, hop 2: coin_in {nc} out of range (pool has {nc} coins)", ci=edit(ci, 12, k2, nc))
    refused("path 12, hop 2: coin_out -1", co=edit(co, 12, k2, -1))
    refused("path 7, hop 5: coin_in and coin_out are both", co=edit(co, 7, 5, ci[7, 5]))
    given_hop = {"cfmm_quote_path": 0, "cfmm_quote_path_out": 4}[entry]    # where path 12's given amount enters
    for bad in (-1.0, np.nan, np.inf):
        a = amt.copy()
        a[12] = bad
        refused(f"path 12, hop {given_hop}: amount_", amt=a)
    nh = n_hops.copy()
    nh[5] = 0
    refused("path 5: n_hops 0", n_hops=nh)
    nh[5] = 9
    refused("path 5: n_hops 9", n_hops=nh)
    refused("max_hops must be 1 .. 8", max_hops=9)
    refused("max_hops must be 1 .. 8", max_hops=0)
    refused("count must be >= 0", count=-1)
    # a slot beyond a path's hops is not a hop: garbage there is ignored (path 3 has 4 hops)
    got = ctx.quote_path(n_hops, edit(seg, 3, 6, 99), edit(row, 3, 5, -7), ci, co, sliced(paths["interleaved"], slice(0, n))[5])
    same_bits(got, fwd["interleaved"][0][:n])


def test_device_entries_poison_exactly_the_bad_paths_from_the_bad_hop_on(world):
    import torch
    batches, ctx, paths, fwd = world
    n_hops, seg, row, ci, co, amt = (a.copy() for a in paths["interleaved"])
    want, want_hops = fwd["interleaved"]
    half = 0.5 * want
    back, back_hops = ctx.quote_path_out(n_hops, seg, row, ci, co, half, hops=True)
    # (path, hop) of each bad hop; every path used here has more hops than the bad one
    bad_hops = {15: 3, 23: 0, 31: 7, 39: 2, 47: 5, 55: 1}
    seg[15, 3] = 8
    seg[23, 0] = -2
    row[31, 7] = M
    row[39, 2] = -1
    ci[47, 5] = batches[seg[47, 5]].Ai.shape[1]
    co[55, 1] = ci[55, 1]
    whole = [64, 72, 80]                                                   # the whole path is NaN: n_hops = 0, 9, and a NaN amount
    n_hops[64], n_hops[72] = 0, 9
    amt_bad, half_bad = amt.copy(), half.copy()
    amt_bad[80] = half_bad[80] = np.nan
    assert all(paths["interleaved"][0][p] > k for p, k in bad_hops.items())
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = [up(n_hops), up(seg.T), up(row.T), up(ci.T), up(co.T)]
    t_amt, t_half = up(amt_bad), up(half_bad)
    t_out, t_in = (torch.zeros(COUNT, dtype=torch.float64, device=dev) for _ in range(2))
    t_hops, t_hin = (torch.zeros((H, COUNT), dtype=torch.float64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        args = [x.data_ptr() for x in t]
        ctx.quote_path_dev(COUNT, H, *args, t_amt.data_ptr(), t_out.data_ptr(), t_hops.data_ptr())
        ctx.quote_path_out_dev(COUNT, H, *args, t_half.data_ptr(), t_in.data_ptr(), t_hin.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    out, hops, ans, hin = t_out.cpu().numpy(), t_hops.cpu().numpy(), t_in.cpu().numpy(), t_hin.cpu().numpy()
    poisoned = np.zeros(COUNT, dtype=bool)
    poisoned[list(bad_hops) + whole] = True
    used = used_slots(paths["interleaved"][0])
    assert np.all(np.isnan(out[poisoned])) and np.all(np.isnan(ans[poisoned]))
    same_bits(out[~poisoned], want[~poisoned])                             # neighbouring paths are unaffected
    same_bits(ans[~poisoned], back[~poisoned])
    clean = used & ~poisoned[None, :]
    same_bits(hops[clean], want_hops[clean])
    same_bits(hin[clean], back_hops[clean])
    for p, k in bad_hops.items():
        nh = paths["interleaved"][0][p]
        same_bits(hops[:k, p], want_hops[:k, p], f"forward, path {p}: the hops before the bad one")
        assert np.all(np.isnan(hops[k:, p])), p                            # ... NaN from the bad hop on
        same_bits(hin[k + 1:nh, p], back_hops[k + 1:nh, p], f"exact output, path {p}: the hops behind the bad one (walked first)")
        assert np.all(np.isnan(hin[:k + 1, p])), p
    for p in whole:
        assert np.all(np.isnan(hops[:, p])) and np.all(np.isnan(hin[:, p])), p


# ---- ownership ----------------------------------------------------------------------------------------------------------------
COUNTERS = ("debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams")


def live_counts_body():
    probe = cr.Context(4)
    live = lambda: tuple(probe.get_option(k) for k in COUNTERS)
    base = live()
    batches = market()
    be = cr.DeviceBackend(N, batches)
    paths = make_paths(batches, "interleaved", count=300)
    before = live()
    be.ctx.set_option("time_kernels", 1)
    be.ctx._check(cr.lib().cfmm_quote_path(be.ctx._h, 0, H, None, None, None, None, None, None, None, None))
    assert live() == before and be.ctx.get_option("quote_ns") == 0       # count == 0 touches nothing
    out, _ = be.ctx.quote_path(*paths, hops=True)
    first = live()
    # the first call creates the scratch: 6 device arrays (table, int32 columns, rows, given, answers, hop amounts), one
    # pinned staging buffer, 3 events (the guard, and {start, stop} under time_kernels), no stream
    assert tuple(x - y for x, y in zip(first, before)) == (6, 1, 3, 0), (before, first)
    assert be.ctx.get_option("quote_ns") > 0
    be.ctx.quote_path_out(*paths[:5], 0.5 * out, hops=True)
    be.ctx.quote_path(*sliced(paths, slice(0, 200)))
    assert live() == first                                               # both directions share it; stable across calls
    be.close()
    assert live() == base                                                # everything goes with the context
    probe.close()
    print("quote-path-live-ok")


def test_live_counts_with_the_hooks_library():
    """the four debug_live_* counts: what the first path call creates stays for the next and goes with the context"""
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_quote_path as t\n"
            "t.live_counts_body()\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "quote-path-live-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- the router-level calls ---------------------------------------------------------------------------------------------------
def test_router_level_calls_are_the_chain_of_router_level_quotes():
    """token-continuous paths of 1..8 different pools through a router of all eight segments: the router derives (segment, row,
    coin_in, coin_out) from pool positions and token ids, and the result is chaining cr.quote / cr.quote_out hop by hop"""
    batches = market()
    r = cr.Router(cr.LinearNonnegative(np.ones(N)), batches, N)
    L = r._layout
    total = len(batches) * M
    Ai_of = lambda i: L.batches[L.locate(i)[1]].Ai[L.locate(i)[2]]
    coins = [Ai_of(i).tolist() for i in range(total)]
    holders = {}
    for i, Ai in enumerate(coins):
        for t in Ai:
            holders.setdefault(int(t), []).append(i)
    count = 300
    plist, tlist = [], []
    for p in range(count):
        i = (p * 37) % total
        toks, pl = [int(coins[i][p % len(coins[i])])], []
        for k in range(1 + p % 8):
            outs = [int(t) for t in coins[i] if t != toks[-1]]
            pl.append(i)
            toks.append(outs[(p + k) % len(outs)])
            cands = [j for j in holders[toks[-1]] if j not in pl]
            if not cands:
                break
            i = cands[(7 * p + 13 * k) % len(cands)]
        plist.append(pl)
        tlist.append(toks)
    lengths = np.array([len(pl) for pl in plist])
    kinds = {L.locate(i)[1] for pl in plist for i in pl}
    assert lengths.max() == 8 and len(kinds) == len(batches)
    coin = lambda i, t: coins[i].index(t)
    first = np.array([scale_in(L.batches[L.locate(pl[0])[1]])[L.locate(pl[0])[2], coin(pl[0], tk[0])] for pl, tk in zip(plist, tlist)])
    amt = first * 10.0 ** (-4.0 + 3.5 * synth.uniform(SEED, 9, count))
    try:
        got, hops = cr.quote_path(r, plist, tlist, amt, hops=True)
        Hn = hops.shape[0]
        assert Hn == 8
        hop_args = lambda k, q: ([plist[j][k] for j in q], [coin(plist[j][k], tlist[j][k]) for j in q],
                                 [coin(plist[j][k], tlist[j][k + 1]) for j in q])
        x = amt.copy()
        want_hops = np.full((Hn, count), np.nan)
        for k in range(Hn):
            q = np.flatnonzero(lengths > k)
            pk, cin, cout = hop_args(k, q)
            x[q] = cr.quote(r, pk, cin, x[q], cout)
            want_hops[k, q] = x[q]
        used = used_slots(lengths, Hn)
        same_bits(got, x)
        same_bits(hops[used], want_hops[used])
        assert np.all(np.isnan(hops[~used])) and np.sum(got > 0) > count // 2
        half = 0.5 * got
        back, hin = cr.quote_path_out(r, plist, tlist, half, hops=True)
        y = half.copy()
        for k in reversed(range(Hn)):
            q = np.flatnonzero(lengths > k)
            pk, cin, cout = hop_args(k, q)
            y[q] = cr.quote_out(r, pk, cin, y[q], cout)
            same_bits(hin[k, q], y[q])
        same_bits(back, y)
        same_bits(cr.quote_path(r, plist, tlist, amt), got)
        with pytest.raises(cr.ArgumentError, match="path 0, hop 1: pool .* appears twice"):
            cr.quote_path(r, [[plist[1][0], plist[1][0]]], [[tlist[1][0], tlist[1][1], tlist[1][0]]], 1.0)
    finally:
        r.close()
