"""cfmm_swap_path_out on the device: exact-output paths of up to eight pools of eight segments of six kinds EXECUTED in query
order, each all or nothing.  test_gpu_quote_path's market and its 1025 paths of 1 to 8 hops.  No tolerance anywhere: the
amounts are held to cfmm_quote_path_out's bits on the market as it stands, the final state to chaining cfmm_swap_out hop by
hop on a twin context, a batch of paths that share pools to the same paths executed one call each.  Around the pin: each
status that is not APPLIED leaves every pool of its path as it was, bad input, a multi-device parent, the router-level call."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import KIND_UNIV3, SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE, ptr
from cfmmrouter_amd.cfmms import _upload
from test_gpu_pool_update import batch_with
from test_gpu_quote import N
from test_gpu_quote_path import COUNT, H, M, SEGMENTS, bits, chain, make_paths, market, same_bits, scale_in, sliced, used_slots
from test_gpu_swap import backend, state
from test_gpu_swap_path import explicit, mixed_pools, same_states, states, wave_count

pytestmark = pytest.mark.gpu

NSEG = len(SEGMENTS)


@pytest.fixture(scope="module")
def world():
    """the market, the interleaved paths and the outputs wanted of them: a part of what the forward walk of a small tender
    yields on the market as it stands, so that every hop can give what it is asked for.  Computed once, left unchanged."""
    batches = market()
    n_hops, seg, row, ci, co, amt = make_paths(batches, "interleaved")
    paths = (n_hops, seg, row, ci, co, amt * 1e-3)
    be = backend(batches)
    try:
        fwd, _ = chain(be.ctx, paths)
    finally:
        be.close()
    return batches, paths, fwd


def pool_disjoint(paths):
    """the paths, in query order, that share no pool with an earlier chosen one: one wave"""
    n_hops, seg, row = paths[:3]
    taken, keep = set(), []
    for p in range(len(n_hops)):
        named = {(int(seg[p, k]), int(row[p, k])) for k in range(n_hops[p])}
        if not named & taken:
            taken |= named
            keep.append(p)
    return np.array(keep)


def leaving(want, hops, n_hops):
    """[H, count] the amount leaving each hop: what the next hop is tendered; the wanted amount at the last"""
    out = np.vstack([hops[1:], np.full((1, want.size), np.nan)])
    out[n_hops - 1, np.arange(want.size)] = want
    return out


# ---- 1. one wave: the bits of the quote, the state of the chain -----------------------------------------------------------------
def test_one_wave_equals_the_quote_then_batched_swap_outs(world):
    batches, all_paths, fwd = world
    keep = pool_disjoint(all_paths)
    paths, want = sliced(all_paths, keep), 0.5 * fwd[keep]
    n_hops, seg, row, ci, co, _ = paths
    count = keep.size
    assert count >= 60 and wave_count(paths) == 1 and n_hops.max() == H
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        got, status, hops = ctx.swap_path_out(*paths[:5], want, hops=True)
        print(f"one wave: {count} paths, {int(np.sum(status != SWAP_APPLIED))} not applied, {int(np.sum(got == 0.0))} cost exactly 0.0")
        assert np.all(status == SWAP_APPLIED) and np.sum(got == 0.0) <= count // 10
        assert ctx.get_option("swap_refused") == 0 and ctx.get_option("swap_launches") == 1
        q, qh = twin.ctx.quote_path_out(*paths[:5], want, hops=True)
        used = used_slots(n_hops)
        same_bits(got, q, "amount_in")
        same_bits(hops[used], qh[used], "hop_in")
        assert np.all(np.isnan(hops[~used]))
        same_bits(hops[0], got, "hop_in of the first hop is the answer")
        # the final state: cfmm_swap_out of (hop, the amount leaving it), one batched call per (hop level, segment)
        y_out = leaving(want, qh, n_hops)
        for k in range(H):
            for s in range(NSEG):
                j = np.flatnonzero((n_hops > k) & (seg[:, k] == s))
                if j.size:
                    a, st = twin.ctx.swap_out(s, y_out[k, j], ci[j, k], co[j, k], row[j, k], status=True)
                    same_bits(a, qh[k, j], f"the twin's swaps of hop level {k}, segment {s}")
                    assert np.all(st == SWAP_APPLIED)
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
        moved = sum(int(np.sum(np.any(bits(a).reshape(M, -1) != bits(o).reshape(M, -1), axis=1)))
                    for a, o in zip(states(ctx, batches), [b.current_price if b.kind == KIND_UNIV3 else b.R for b in batches]))
        assert moved >= int(0.7 * np.sum(n_hops))                              # ... and it is a state that has moved
    finally:
        be.close()
        twin.close()


# ---- 2. shared pools, many waves --------------------------------------------------------------------------------------------------
def test_paths_that_share_pools_equal_one_path_per_call(world):
    """all 1025 paths over 257 pools per segment: most share a pool with an earlier one.  The twin executes them one call
    each, in query order; statuses, answers, hop amounts and the final state agree bit for bit"""
    batches, paths, fwd = world
    n_hops = paths[0]
    want = 0.25 * fwd
    lim = np.where(np.arange(COUNT) % 7 == 3, 0.0, 1e300)                     # every seventh path may cost nothing: over the limit
    waves = wave_count(paths)
    assert waves >= 3
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        got, status, hops = ctx.swap_path_out(*paths[:5], want, max_in=lim, hops=True)
        assert ctx.get_option("swap_launches") == waves and ctx.get_option("swap_ns") > 0
        print(f"shared pools: {waves} waves; statuses {np.bincount(status, minlength=4).tolist()}")
        assert np.sum(status == SWAP_APPLIED) >= COUNT // 2 and np.sum(status == SWAP_OVER_LIMIT) >= COUNT // 10
        assert ctx.get_option("swap_refused") == np.sum(status != SWAP_APPLIED)
        one, one_st, one_h = np.empty(COUNT), np.empty(COUNT, dtype=np.int32), np.full((H, COUNT), np.nan)
        for p in range(COUNT):
            sl = slice(p, p + 1)
            a, s, h = twin.ctx.swap_path_out(*sliced(paths[:5], sl), want[sl], max_in=lim[sl], hops=True)
            one[p], one_st[p], one_h[:, p] = a[0], s[0], h[:, 0]
        np.testing.assert_array_equal(status, one_st)
        same_bits(got, one, "amount_in")
        used = used_slots(n_hops)
        same_bits(hops[used], one_h[used], "hop_in")
        assert np.all(np.isnan(hops[~used]))
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
    finally:
        be.close()
        twin.close()


# ---- 3. all or nothing --------------------------------------------------------------------------------------------------------------
TINY, THIN, EDGE = 30, 31, 29          # rows of the doctored pools below
EPS = 2.0 ** -32


def doctored_market():
    """the market with three doctored pools.  Product row TINY holds 1e-25 of each coin: it cannot give what a later hop asks
    of it (unobtainable).  Solidly row THIN holds 2^-120 of its second coin, and Product row EDGE = {2^-120, 1} sells
    o = γ(1 − ε)/(1 + γ(1 − ε)) of its second coin for 2^-120·(1 − ε) of its first: asked for that, THIN would be left with
    2^-152 -- positive, but outside [2^-150, 2^150] (refused)."""
    batches = market()
    R = batches[0].R.copy()
    R[TINY] = [1e-25, 1e-25]
    R[EDGE] = [2.0 ** -120, 1.0]
    batches[0] = batch_with(batches[0], R=R)
    R = batches[2].R.copy()
    R[THIN] = [1.0, 2.0 ** -120]
    batches[2] = batch_with(batches[2], R=R)
    g = batches[0].γ[EDGE]
    return batches, g * (1 - EPS) / (1 + g * (1 - EPS))


@pytest.mark.parametrize("case", ("unobtainable", "refused", "over_limit"))
def test_a_path_that_is_not_applied_changes_no_pool(case):
    batches, o_edge = doctored_market()
    first, last = (1, 5, 0, 1), (4, 2, 0, 2)                                    # a GeometricMean and a weighted pool
    middle = {"unobtainable": (0, TINY, 0, 1), "refused": (2, THIN, 0, 1), "over_limit": (0, 3, 0, 1)}[case]
    if case == "refused":
        last = (0, EDGE, 0, 1)
    before = [(0, 1, 0, 1), (5, 2, 0, 3)]                                       # an ordinary path
    later = [first, (5, 3, 1, 6)]                                               # through the failing path's first pool, after it
    failing = [first, middle, last]

    def feasible(ctx, path):
        """a quarter of what a small tender to the path yields on the market as it stands: every hop can give its part"""
        s0, r0, c0, _ = path[0]
        return 0.25 * ctx.quote_path(*explicit([path], [1e-3 * scale_in(batches[s0])[r0, c0]]))[0]
    probe = backend(batches)
    try:
        w_fail = {"unobtainable": 1e-3 * batches[4].R[2, 2], "refused": o_edge}.get(case) or feasible(probe.ctx, failing)
        paths = explicit([before, failing, later], [feasible(probe.ctx, before), w_fail, feasible(probe.ctx, later)])
    finally:
        probe.close()
    assert np.all(paths[5] > 0)
    without = sliced(paths, [0, 2])
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        q, qh = twin.ctx.quote_path_out(*sliced(paths[:5], [1]), paths[5][1:2], hops=True)   # the failing path on the untouched market
        lim = None
        if case == "over_limit":
            assert 0 < q[0] < np.inf
            lim = np.array([1e300, np.nextafter(q[0], 0.0), 1e300])
        got, status, hops = ctx.swap_path_out(*paths, max_in=lim, hops=True)
        code = {"unobtainable": SWAP_UNOBTAINABLE, "refused": SWAP_REFUSED, "over_limit": SWAP_OVER_LIMIT}[case]
        assert status.tolist() == [SWAP_APPLIED, code, SWAP_APPLIED] and ctx.get_option("swap_refused") == 1
        assert np.all(np.isfinite(got[[0, 2]])) and np.all(got[[0, 2]] > 0)
        assert bits(hops[2, 1]) == bits(qh[2, 0]) and 0 < hops[2, 1] < np.inf    # the hop behind the failing one: the quote's amount
        if case == "unobtainable":
            assert qh[2, 0] >= batches[0].R[TINY, 1]                            # more than the pool holds
            assert got[1] == np.inf and np.all(hops[:2, 1] == np.inf) and q[0] == np.inf
        elif case == "refused":
            left = batches[2].R[THIN, 1] - qh[2, 0]
            print(f"Solidly: the swap would leave 2^{np.log2(left):.1f}")
            assert 0 < left < 2.0 ** -150 and np.isfinite(qh[1, 0])               # that hop's quote is finite: only the state is refused
            assert np.isnan(got[1]) and np.all(np.isnan(hops[:2, 1]))
        else:
            same_bits(got[1:2], q, "the would-be quote")
            same_bits(hops[:, 1], qh[:, 0], "hop_in")
            equal, st_eq = twin.ctx.swap_path_out(*sliced(paths[:5], [1]), paths[5][1:2], max_in=q)   # a limit that is met exactly is met
            assert st_eq.tolist() == [SWAP_APPLIED] and bits(equal)[0] == bits(q)[0]
            twin.close()
            twin = backend(batches)
        # the market is the one in which the failing path never ran: amounts, hop amounts and every bit of every segment
        want, want_st, want_hops = twin.ctx.swap_path_out(*without, hops=True)
        assert np.all(want_st == SWAP_APPLIED)
        same_bits(got[[0, 2]], want, "the other paths")
        u = used_slots(without[0], 3)
        same_bits(hops[:, [0, 2]][u], want_hops[u])
        same_states(states(ctx, batches), states(twin.ctx, batches))
    finally:
        be.close()
        twin.close()
    # alone in a call: no pool of the path changes a bit, the pools of the hops behind the failing one included
    alone = backend(batches)
    try:
        was = states(alone.ctx, batches)
        a1, s1 = alone.ctx.swap_path_out(*sliced(paths[:5], [1]), paths[5][1:2], max_in=None if lim is None else lim[1:2])
        assert s1.tolist() == [code] and alone.ctx.get_option("swap_refused") == 1
        same_states(states(alone.ctx, batches), was)
    finally:
        alone.close()


def test_zero_wanted_moves_nothing_and_one_hop_is_swap_out(world):
    batches, _, _ = world
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        every_kind = [(s, 3 + s, 0, 1) for s in range(NSEG)]
        got, status, hops = ctx.swap_path_out(*explicit([every_kind], [0.0]), max_in=0.0, hops=True)
        assert status.tolist() == [SWAP_APPLIED] and bits(got)[0] == 0 and np.all(bits(hops[:, 0]) == 0)   # +0.0 at every hop
        same_states(states(ctx, batches), was, "wanted 0")
        e = np.zeros((0, H), dtype=np.int32)
        o, s = ctx.swap_path_out(np.zeros(0, dtype=np.int32), e, e, e, e, np.zeros(0))
        assert o.size == 0 and s.size == 0
        for s_, b in enumerate(batches):                                       # a 1-hop path is cfmm_swap_out
            nc = b.Ai.shape[1]
            r = np.arange(8, 16, dtype=np.int64)
            ci1, co1 = (r % nc).astype(np.int32), ((r + 1) % nc).astype(np.int32)
            w1 = 0.25 * twin.ctx.quote(s_, 1e-3 * (np.sqrt(b.liquidity[b.tick_off[r]] + 1.0) if b.kind == KIND_UNIV3 else b.R[r, ci1]), ci1, co1, r)
            o1, st1 = ctx.swap_path_out(np.ones(8, dtype=np.int32), np.full(8, s_, dtype=np.int32), r, ci1, co1, w1)
            a1, st2 = twin.ctx.swap_out(s_, w1, ci1, co1, r, status=True)
            same_bits(o1, a1, f"one hop, segment {s_}")
            np.testing.assert_array_equal(st1, st2)
        same_states(states(ctx, batches), states(twin.ctx, batches), "one hop")
    finally:
        be.close()
        twin.close()


# ---- 4. bad input, a parent -----------------------------------------------------------------------------------------------------
def test_bad_input_names_path_and_hops_and_changes_nothing(world):
    L = cr.lib()
    batches, all_paths, fwd = world
    sl = np.arange(16)
    n_hops, seg, row, ci, co, _ = sliced(all_paths, sl)
    want = 0.25 * fwd[sl]
    be = backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        c = lambda a: np.ascontiguousarray(a.T)

        def refused(match, seg=seg, row=row, want=want, lim=None):
            out, hv, st = np.full(16, 7.0), np.full((H, 16), 7.0), np.full(16, 7, dtype=np.int32)
            rc = L.cfmm_swap_path_out(ctx._h, 16, H, ptr(n_hops), ptr(c(seg)), ptr(c(row)), ptr(c(ci)), ptr(c(co)), ptr(np.ascontiguousarray(want)),
                                      ptr(lim), ptr(out), ptr(hv), ptr(st))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and msg.startswith("cfmm_swap_path_out: ") and match in msg, (rc, msg)
            assert np.all(out == 7.0) and np.all(hv == 7.0) and np.all(st == 7)

        s2, r2 = seg.copy(), row.copy()                                        # path 5 has 6 hops: its hops 1 and 4 name one pool
        s2[5, 4], r2[5, 4] = s2[5, 1], r2[5, 1]
        refused(f"path 5, hops 1 and 4: row {r2[5, 1]} of segment {s2[5, 1]} appears twice", seg=s2, row=r2)
        bad = want.copy(); bad[7] = np.nan
        refused("path 7, hop 7: amount_out must be finite and >= 0", want=bad)  # path 7 has 8 hops: the amount enters at the last
        lim = np.zeros(16); lim[4] = -1.0
        refused("path 4, hop 0: max_amount_in must be finite and >= 0", lim=lim)
        same_states(states(ctx, batches), was)
    finally:
        be.close()


def test_a_multi_device_parent_is_unsupported_and_moves_nothing(world):
    batches, all_paths, fwd = world
    sl = np.arange(32)
    multi = cr.Context(N, [0, 0])
    try:
        for b in batches:
            _upload(multi, b)
        was = states(multi, batches)
        with pytest.raises(NotImplementedError, match="cfmm_swap_path_out is not available on a multi-device context"):
            multi.swap_path_out(*sliced(all_paths[:5], sl), 0.25 * fwd[sl])
        same_states(states(multi, batches), was)
    finally:
        multi.close()


# ---- 5. router level ----------------------------------------------------------------------------------------------------------------
def test_swap_path_out_through_a_router_equals_the_chain_of_swap_outs():
    n = 6
    path_pools = [[0, 1, 3], [2, 4, 5], [0]]
    path_tokens = [[1, 2, 3, 5], [1, 4, 6, 5], [2, 1]]
    want = [20.0, 15.0, 10.0]
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), mixed_pools(), n)
    twin = cr.Router(cr.LinearNonnegative(np.ones(n)), mixed_pools(), n)
    try:
        quoted = cr.quote_path_out(twin, path_pools[:2], path_tokens[:2], want[:2])
        got, status, hops = cr.swap_path_out_(r, path_pools, path_tokens, want, max_in=1e9, hops=True)
        assert np.all(status == SWAP_APPLIED) and np.all(got > 0)
        same_bits(got[:2], quoted, "pool-disjoint paths: the quote on the market as it stood")
        for p, (pl, tk) in enumerate(zip(path_pools, path_tokens)):
            y = want[p]
            for k in reversed(range(len(pl))):
                Ai = list(twin.cfmms[pl[k]].Ai)
                a, st = cr.swap_out_(twin, [pl[k]], [Ai.index(tk[k])], [y], [Ai.index(tk[k + 1])])
                assert st[0] == SWAP_APPLIED and bits(hops[k, p:p + 1])[0] == bits(a)[0], (p, k)
                y = a[0]
            assert bits(got[p:p + 1])[0] == bits([y])[0]
        for pool, other in zip(r.cfmms, twin.cfmms):                            # the host mirrors agree
            if isinstance(pool, cr.UniV3):
                assert pool.current_price == other.current_price
            else:
                same_bits(pool.R, other.R)
        assert r.cfmms[3].R[1] == 1e4 - 20.0                                    # the last pool of path 0 gave exactly what was asked
    finally:
        r.close()
        twin.close()
