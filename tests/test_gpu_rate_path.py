"""cfmm_quote_path_rate on the device: a market holding all six kinds (eight segments of 64 pools), 200 paths with ragged
n_hops from 1 to 8.  The pins are bit-equalities: amount_out / hop_out with cfmm_quote_path, hop_rate[k] with cfmm_quote_rate on
(hop k, the amount entering it), rate with the left fold computed in numpy (tests/rate_path_ref.py).  Around them: unused
slots, a path through an exhausted UniV3 hop, the device-pointer entry and its poison rule, a multi-device parent, refusals."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import rate_path_ref as RPATH
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import ptr
from cfmmrouter_amd.cfmms import _upload
from test_gpu_pool_update import batch_with
from test_gpu_quote import N, pools
from test_gpu_quote_path import SEGMENTS, bits, same_bits, scale_in, used_slots

pytestmark = pytest.mark.gpu

M = 64                  # pools per segment
COUNT = 200             # paths
H = 8                   # max_hops
SEED = 7
UNIV3 = [s for s, (kind, _) in enumerate(SEGMENTS) if kind == "univ3"][0]


def market():
    out = []
    for s, (kind, nc) in enumerate(SEGMENTS):
        if kind == "univ3":
            b = synth.univ3_ragged_pools(M, N, min_ticks=1, max_ticks=16, seed=SEED + s)
            zero = synth.uniform(SEED + 100, 5, b.liquidity.size) < 0.1
            b = batch_with(b, liquidity=np.where(zero, 0.0, b.liquidity))
        else:
            b = pools(kind, M, seed=SEED + s, n_coins=nc)
        out.append(b)
    return out


def make_paths(batches):
    """test_gpu_quote_path.make_paths' interleaved pattern on M-pool segments: n_hops[p] = 1 + p % 8, segment (p + 3k) % 8, rows
    pseudo-random with repeats, coins cycling through every ordered pair, the first amount R_i·10^u, u uniform in [-6, 0.5];
    every eighth path starts with amount 0 (the path's spot rate)"""
    p, k = np.meshgrid(np.arange(COUNT), np.arange(H), indexing="ij")
    n_hops = (1 + np.arange(COUNT) % H).astype(np.int32)
    seg = ((p + 3 * k) % 8).astype(np.int32)
    row = np.minimum((synth.uniform(SEED + 200, 3, COUNT * H).reshape(COUNT, H) * M).astype(np.int64), M - 1)
    ci, co = np.zeros((COUNT, H), dtype=np.int32), np.zeros((COUNT, H), dtype=np.int32)
    for s, b in enumerate(batches):
        nc = b.Ai.shape[1]
        pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
        at = seg == s
        pick = (p[at] + k[at]) % len(pairs)
        ci[at], co[at] = pairs[pick, 0], pairs[pick, 1]
    u = -6.0 + 6.5 * synth.uniform(SEED + 300, 4, COUNT)
    first = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(COUNT)])
    amt = first * 10.0 ** u
    amt[::8] = 0.0
    return n_hops, seg, row, ci, co, amt


@pytest.fixture(scope="module")
def world():
    """the market on one context, the paths and the entry's answers, computed once and left unchanged"""
    batches = market()
    be = cr.DeviceBackend(N, batches)
    paths = make_paths(batches)
    ans = be.ctx.quote_path_rate(*paths, hops=True)
    yield batches, be.ctx, paths, ans
    be.close()


def test_amounts_are_quote_paths_and_every_hop_rate_is_quote_rates(world):
    batches, ctx, paths, (out, rate, hop_out, hop_rate) = world
    n_hops, seg, row, ci, co, amt = paths
    q_out, q_hops = ctx.quote_path(*paths, hops=True)
    used = used_slots(n_hops)
    same_bits(out, q_out)
    same_bits(hop_out[used], q_hops[used])
    assert np.all(np.isnan(hop_out[~used])) and np.all(np.isnan(hop_rate[~used]))              # unused slots are NaN
    assert np.all(np.isfinite(hop_rate[used])) and np.all(hop_rate[used] >= 0.0)
    # hop_rate[k] = cfmm_quote_rate on (hop k, the amount entering it), hop level by hop level and segment by segment
    x = np.array(amt)
    for k in range(H):
        act = n_hops > k
        for s in range(len(SEGMENTS)):
            q = np.flatnonzero(act & (seg[:, k] == s))
            if q.size:
                o, r = ctx.quote_rate(s, x[q], ci[q, k], co[q, k], row[q, k])
                same_bits(o, hop_out[k, q], f"hop {k} segment {s}")
                same_bits(r, hop_rate[k, q], f"hop {k} segment {s}")
        x[act] = hop_out[k, act]
    same_bits(rate, RPATH.fold_rates(n_hops, hop_rate))                                         # the left fold, in numpy
    # without the hop arrays: the same two answers
    o2, r2 = ctx.quote_path_rate(*paths)
    same_bits(o2, out)
    same_bits(r2, rate)
    assert np.all(bits(out[::8]) == 0) and np.all(np.isfinite(rate[::8]))                       # amount 0: +0.0, the spot rates' product


def test_a_path_through_an_exhausted_univ3_hop_has_rate_zero(world):
    """coin 1 in walks the price-rising list, which is finite: an amount beyond all of it exhausts the ladder.  The hop's rate is
    exactly +0.0, so is the path's, and the hops behind it are still evaluated (on what the ladder gave)"""
    batches, ctx, paths, _ = world
    huge = 1e30
    every_out, every_rate = ctx.quote_rate(UNIV3, np.full(M, huge), 1, None, np.arange(M))
    assert np.all(bits(every_rate) == 0) and np.all(np.isfinite(every_out))                    # every ladder of the segment: exactly +0.0
    pool = int(np.flatnonzero(every_out > 0.0)[0])                                              # one that had something to give
    n_hops = np.array([1, 3], dtype=np.int32)
    seg = np.array([[UNIV3, 0, 0], [UNIV3, 0, 0]], dtype=np.int32)
    row = np.array([[pool, 0, 0], [pool, 1, 2]], dtype=np.int64)
    ci = np.array([[1, 0, 0], [1, 0, 0]], dtype=np.int32)
    co = np.array([[0, 1, 1], [0, 1, 1]], dtype=np.int32)
    out, rate, hop_out, hop_rate = ctx.quote_path_rate(n_hops, seg, row, ci, co, np.array([huge, huge]), hops=True)
    o1, r1 = ctx.quote_rate(UNIV3, np.array([huge]), 1, None, np.array([pool]))
    assert bits(r1)[0] == 0 and np.isfinite(o1[0]) and o1[0] > 0.0                              # exhausted: exactly +0.0
    assert bits(rate)[0] == 0 and bits(hop_rate[0, 0]) == 0 and bits(out)[0] == bits(o1)[0]
    o2, r2 = ctx.quote_rate(0, o1, 0, None, np.array([1]))
    o3, r3 = ctx.quote_rate(0, o2, 0, None, np.array([2]))
    assert bits(hop_rate[0, 1]) == 0 and bits(rate)[1] == 0                                     # the path's rate is +0.0 ...
    assert bits(hop_out[1, 1]) == bits(o2)[0] and bits(hop_rate[1, 1]) == bits(r2)[0] and r2[0] > 0.0     # ... the later hops are evaluated
    assert bits(hop_out[2, 1]) == bits(o3)[0] and bits(hop_rate[2, 1]) == bits(r3)[0] and bits(out)[1] == bits(o3)[0]


def test_device_pointer_entry_gives_the_same_bits_and_poisons_exactly_the_bad_paths(world):
    import torch
    batches, ctx, paths, (out, rate, hop_out, hop_rate) = world
    n_hops, seg, row, ci, co, amt = paths
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def run(n_hops, seg, row, ci, co, amt):
        t = [up(n_hops), up(seg.T), up(row.T), up(ci.T), up(co.T), up(amt)]                     # hop-major, the ABI's layout
        t_out, t_rate = (torch.zeros(COUNT, dtype=torch.float64, device=dev) for _ in range(2))
        t_ho, t_hr = (torch.zeros((H, COUNT), dtype=torch.float64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.quote_path_rate_dev(COUNT, H, *(x.data_ptr() for x in t), t_out.data_ptr(), t_rate.data_ptr(), t_ho.data_ptr(), t_hr.data_ptr())
            torch.cuda.synchronize()
        finally:
            ctx.reset_stream()
        return tuple(x.cpu().numpy() for x in (t_out, t_rate, t_ho, t_hr))
    used = used_slots(n_hops)
    d_out, d_rate, d_ho, d_hr = run(*paths)
    same_bits(d_out, out)
    same_bits(d_rate, rate)
    same_bits(d_ho[used], hop_out[used])
    same_bits(d_hr[used], hop_rate[used])
    assert np.all(np.isnan(d_ho[~used])) and np.all(np.isnan(d_hr[~used]))
    # bad paths: a segment, a row, a coin out of range at some hop, equal coins, a bad amount, a bad n_hops
    n2, seg2, row2, ci2, co2, amt2 = (a.copy() for a in paths)
    seg2[15, 3] = 99           # path 15 has 8 hops: bad from hop 3 on
    row2[23, 0] = M            # path 23 (8 hops): bad from the first hop
    ci2[31, 7] = -1            # path 31 (8 hops): only the last hop
    co2[39, 2] = ci2[39, 2]    # path 39 (8 hops)
    amt2[42] = -1.0
    amt2[43] = np.nan
    n2[50], n2[51] = 0, H + 1
    bad_from = {15: 3, 23: 0, 31: 7, 39: 2, 42: 0, 43: 0}
    b_out, b_rate, b_ho, b_hr = run(n2, seg2, row2, ci2, co2, amt2)
    bad = np.zeros(COUNT, dtype=bool)
    bad[list(bad_from) + [50, 51]] = True
    assert np.all(np.isnan(b_out[bad])) and np.all(np.isnan(b_rate[bad]))                      # NaN in both outputs ...
    same_bits(b_out[~bad], out[~bad])                                                          # ... for those paths only
    same_bits(b_rate[~bad], rate[~bad])
    for p, k0 in bad_from.items():
        nh = n_hops[p]
        same_bits(b_ho[:k0, p], hop_out[:k0, p])
        same_bits(b_hr[:k0, p], hop_rate[:k0, p])
        assert np.all(np.isnan(b_ho[k0:nh, p])) and np.all(np.isnan(b_hr[k0:nh, p]))
    assert np.all(np.isnan(b_ho[:, [50, 51]])) and np.all(np.isnan(b_hr[:, [50, 51]]))         # a bad n_hops: no hop evaluated


def test_a_multi_device_parent_gives_the_same_bits(world):
    batches, ctx, paths, (out, rate, hop_out, hop_rate) = world
    multi = cr.Context(N, [0, 0])
    try:
        for b in batches:
            _upload(multi, b)
        m_out, m_rate, m_ho, m_hr = multi.quote_path_rate(*paths, hops=True)
        used = used_slots(paths[0])
        same_bits(m_out, out)
        same_bits(m_rate, rate)
        same_bits(m_ho[used], hop_out[used])
        same_bits(m_hr[used], hop_rate[used])
        assert np.all(np.isnan(m_ho[~used])) and np.all(np.isnan(m_hr[~used]))
        o2, r2 = multi.quote_path_rate(*paths)
        same_bits(o2, out)
        same_bits(r2, rate)
    finally:
        multi.close()


def test_host_entry_refuses_and_names_path_and_hop(world):
    batches, ctx, paths, _ = world
    L = cr.lib()
    n = 16
    n_hops, seg, row, ci, co, amt = (a[:n].copy() for a in paths)

    def refused(match, n_hops=n_hops, seg=seg, row=row, ci=ci, co=co, amt=amt, max_hops=H, null=None):
        out, rate = np.full(n, 7.0), np.full(n, 7.0)
        ho, hr = np.full((H, n), 7.0), np.full((H, n), 7.0)
        c = lambda a, t: np.ascontiguousarray(np.asarray(a).T if np.ndim(a) == 2 else a, dtype=t)
        rc = L.cfmm_quote_path_rate(ctx._h, n, max_hops, ptr(c(n_hops, np.int32)), ptr(c(seg, np.int32)), ptr(c(row, np.int64)),
                                    ptr(c(ci, np.int32)), ptr(c(co, np.int32)), ptr(c(amt, np.float64)),
                                    None if null == "out" else ptr(out), None if null == "rate" else ptr(rate), ptr(ho), ptr(hr))
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and match in msg and msg.startswith("cfmm_quote_path_rate:"), (rc, msg)
        assert all(np.all(a == 7.0) for a in (out, rate, ho, hr))                               # the outputs are untouched

    def edit(a, p, k, value):
        b = a.copy()
        b[p, k] = value
        return b
    refused("path 7, hop 3: segment 8 out of range", seg=edit(seg, 7, 3, 8))                    # path 7 has 8 hops
    refused("path 7, hop 0: row 64 out of range", row=edit(row, 7, 0, M))
    refused("path 15, hop 7: coin_in -1 out of range", ci=edit(ci, 15, 7, -1))
    refused("path 7, hop 2: coin_in and coin_out are both", co=edit(co, 7, 2, ci[7, 2]))
    bad = amt.copy(); bad[5] = -1.0
    refused("path 5, hop 0: amount_in must be finite and >= 0", amt=bad)
    bad = amt.copy(); bad[6] = np.inf
    refused("path 6, hop 0", amt=bad)
    bad = n_hops.copy(); bad[2] = 0
    refused("path 2: n_hops 0 out of range", n_hops=bad)
    refused("max_hops must be 1 .. 8", max_hops=9)
    refused("null path array", null="out")
    refused("null path array", null="rate")
    # slots at k >= n_hops[p] are not looked at
    out, rate = ctx.quote_path_rate(n_hops, edit(seg, 0, 5, 99), row, ci, co, amt)              # path 0 has one hop
    assert np.all(np.isfinite(rate))
