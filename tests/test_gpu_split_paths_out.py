"""cfmm_split_paths_out on the device: a wanted amount bought through an order's 1 .. 8 paths by the greedy search stated in
include/cfmm_amd_split_out.h -- one wavefront per order, one lane per grid point, the hops walked backwards.  The pin of the
feature is bit-equality with the numpy statement of that contract (tests/split_paths_out_ref.py) driven by
ctx.quote_path_out, on test_gpu_quote_path.py's market of eight segments of every pool family: shares, costs, totals and
status.  Around it: the round trip through quote_path_out, grid geometry, the device-pointer entry and its poisoning,
execution through swap_path_out, what the split is worth, edges, read-only behaviour, a multi-device parent, large-market
mode, errors and options.

Orders: test_gpu_split_paths.py's (K cycles through 1, 2, 3, 8; path p has 1 + p % 8 hops; rows 8k + h plus an order offset,
so no pool occurs twice in an order).  The wanted amount B is the output reserve of the LAST hop of the order's first path
times 10^u, u in [-3, 0.5]: some orders are small, some exceed every path and some all paths together."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import (KIND_UNIV3, MAX_SPLIT_ROUNDS, OBJ_LINEAR_NONNEGATIVE, SPLIT_NAN, SPLIT_NONE, SPLIT_OK, SPLIT_UNOBTAINABLE,
                                 SWAP_APPLIED, ptr)
from cfmmrouter_amd.cfmms import _upload
from split_paths_out_ref import split_paths_out_ref
from test_gpu_pool_update import batch_with
from test_gpu_quote import N, pools
from test_gpu_quote_path import H, M, PATTERNS, SEED, bits, market, scale_in
from test_gpu_split_paths import COUNTS, MANY, ROUNDS, make_orders, same_bits
from test_split_paths_out_cpu import EXCESS_MEASURED

pytestmark = pytest.mark.gpu


def same_answer(got, want, first, what=""):
    """(path_amount_out, path_amount_in, total_in, status): the amounts bit for bit (NaN as NaN), the status equal"""
    np.testing.assert_array_equal(got[3], want[3], err_msg=what + " status")
    nan = want[3] == SPLIT_NAN
    nan_path = np.repeat(nan, np.diff(first))
    for name, g, w, mask in (("path_amount_out", got[0], want[0], nan_path), ("path_amount_in", got[1], want[1], nan_path),
                             ("total_in", got[2], want[2], nan)):
        assert np.all(np.isnan(g[mask])), what + " " + name
        same_bits(g[~mask], w[~mask], what + " " + name)


def make_orders_out(batches, pattern, count, seed=SEED, first_k=0, u=None):
    """make_orders' paths with the wanted amount in place of the tendered one (u: the same exponent for every order)"""
    first, _, n_hops, seg, row, ci, co = make_orders(batches, pattern, count, seed, first_k)
    u = -3.0 + 3.5 * synth.uniform(seed + 500, 4, count) if u is None else np.full(count, float(u))
    lead = first[:-1]
    last = n_hops[lead] - 1
    scale = np.array([scale_in(batches[seg[q, l]])[row[q, l], co[q, l]] for q, l in zip(lead, last)])
    return first, scale * 10.0 ** u, n_hops, seg, row, ci, co


def quoter(ctx, o):
    """the contract's market: what ctx.quote_path_out answers for amounts x wanted from paths idx of the orders o"""
    n_hops, seg, row, ci, co = o[2:7]
    return lambda idx, x: ctx.quote_path_out(n_hops[idx], seg[idx], row[idx], ci[idx], co[idx], x)


def split(ctx, o, rounds=5):
    return ctx.split_paths_out(o[0], o[1], *o[2:7], rounds)


class World:
    def __init__(self):
        self.batches = market(seed=SEED)
        self.be = cr.DeviceBackend(N, self.batches)
        self.ctx = self.be.ctx
        self.orders = {(pat, n): make_orders_out(self.batches, pat, n, first_k=n) for pat in PATTERNS for n in COUNTS + (MANY,)}
        self._ref = {}

    def ref(self, pattern, count, rounds):
        """the reference's answer, computed once and left unchanged"""
        key = (pattern, count, rounds)
        if key not in self._ref:
            o = self.orders[(pattern, count)]
            self._ref[key] = split_paths_out_ref(quoter(self.ctx, o), o[0], o[1], rounds)
        return self._ref[key]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.be.close()


# ---- the pin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("rounds", ROUNDS)
def test_the_device_is_the_reference_bit_for_bit(world, pattern, rounds):
    seen = {}
    for count in COUNTS + (MANY,):
        o = world.orders[(pattern, count)]
        got = split(world.ctx, o, rounds)
        want = world.ref(pattern, count, rounds)
        same_answer(got, want, o[0], f"{pattern}, {count} orders, rounds {rounds}")
        for s in want[3].tolist():
            seen[s] = seen.get(s, 0) + 1
        for g in np.flatnonzero(got[3] == SPLIT_OK):                      # the shares are the amount, to the rounding of their sum
            lo, hi = o[0][g], o[0][g + 1]
            assert abs(np.sum(got[0][lo:hi]) - o[1][g]) <= 8 * 2.0 ** -53 * o[1][g] and np.all(got[0][lo:hi] >= 0)
            assert np.all(np.isfinite(got[1][lo:hi])) and np.isfinite(got[2][g])
            if hi - lo == 1:
                same_bits(got[0][lo:hi], o[1][g:g + 1], "one path: the amount bit for bit")
        for g in np.flatnonzero(got[3] == SPLIT_UNOBTAINABLE):
            lo, hi = o[0][g], o[0][g + 1]
            assert np.all(np.isposinf(got[1][lo:hi])) and np.isposinf(got[2][g]) and not np.any(bits(got[0][lo:hi]))
    print(f"split_paths_out {pattern}, rounds {rounds}: statuses seen {sorted(seen.items())}")
    assert SPLIT_OK in seen and SPLIT_UNOBTAINABLE in seen and SPLIT_NAN not in seen


@pytest.mark.parametrize("pattern", PATTERNS)
def test_quote_path_out_at_the_shares_is_the_cost(world, pattern):
    o = world.orders[(pattern, MANY)]
    x, c, total, st = split(world.ctx, o)
    live = np.repeat(st == SPLIT_OK, np.diff(o[0]))
    assert live.sum() > 20
    same_bits(world.ctx.quote_path_out(*o[2:7], np.where(live, x, 0.0))[live], c[live])


def test_the_grid_and_the_batch_do_not_change_the_bits(world):
    ctx = world.ctx
    default = ctx.get_option("split_max_blocks")
    try:
        for blocks in (1, 2):
            ctx.set_option("split_max_blocks", blocks)
            for pattern in PATTERNS:
                o = world.orders[(pattern, MANY)]
                same_answer(split(ctx, o), world.ref(pattern, MANY, 5), o[0], f"split_max_blocks {blocks}, {pattern}")
    finally:
        ctx.set_option("split_max_blocks", default)
    # a slice of the orders gives the slice of the answers
    o, want = world.orders[("interleaved", MANY)], world.ref("interleaved", MANY, 5)
    for lo, hi in ((0, 1), (3, 8), (40, 70)):
        a, b = int(o[0][lo]), int(o[0][hi])
        part = (o[0][lo:hi + 1] - a, o[1][lo:hi]) + tuple(v[a:b] for v in o[2:7])
        same_answer(split(ctx, part), (want[0][a:b], want[1][a:b], want[2][lo:hi], want[3][lo:hi]), part[0], f"orders {lo}:{hi}")


# ---- the device-pointer entry -----------------------------------------------------------------------------------------------------
def test_the_device_entry_gives_the_same_bits_and_poisons_only_bad_orders(world):
    import torch
    ctx = world.ctx
    o, want = world.orders[("interleaved", MANY)], world.ref("interleaved", MANY, 5)
    first, amount = o[0], o[1]
    P = int(first[-1])
    n_hops, seg, row, ci, co = (a.copy() for a in o[2:7])
    bad_amount = amount.copy()
    # order 5: a path with n_hops 0; order 9: a row out of range; order 14: a NaN amount; order 22: a negative amount;
    # order 27: an infinite amount; order 31: n_hops 9
    n_hops[first[5]] = 0
    p9 = int(first[9]) + int(np.argmax(o[2][first[9]:first[10]] > 2))
    row[p9, 2] = M
    bad_amount[14], bad_amount[22], bad_amount[27] = np.nan, -1.0, np.inf
    n_hops[first[31] + 1 if first[32] - first[31] > 1 else first[31]] = 9
    bad = [5, 9, 14, 22, 27, 31]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_good = [up(first), up(amount), up(o[2]), up(o[3].T), up(o[4].T), up(o[5].T), up(o[6].T)]
    t_bad = [up(first), up(bad_amount), up(n_hops), up(seg.T), up(row.T), up(ci.T), up(co.T)]
    fresh = lambda: [torch.full((P,), 7.0, dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.full((MANY,), 7.0, dtype=torch.float64, device=dev), torch.full((MANY,), 7, dtype=torch.int32, device=dev)]
    wrong = first.copy()
    wrong[40] = wrong[41]                                                  # a path range that is no range: order 39 grows, order 40 has no path
    grown = int(wrong[40] - wrong[39])
    t_wrong = [up(wrong)] + t_good[1:]
    outs = [fresh(), fresh(), fresh()]
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for t, out in zip((t_good, t_bad, t_wrong), outs):
            ctx.split_paths_out_dev(MANY, t[0].data_ptr(), t[1].data_ptr(), P, H, *(x.data_ptr() for x in t[2:]), 5, *(x.data_ptr() for x in out))
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    good, poisoned, res = (tuple(x.cpu().numpy() for x in out) for out in outs)
    same_answer(good, want, first, "split_paths_out_dev")
    mask = np.zeros(MANY, dtype=bool)
    mask[bad] = True
    pmask = np.repeat(mask, np.diff(first))
    assert np.all(poisoned[3][mask] == SPLIT_NAN) and np.all(np.isnan(poisoned[2][mask]))
    assert np.all(np.isnan(poisoned[0][pmask])) and np.all(np.isnan(poisoned[1][pmask]))
    keep = lambda a: (a[0][~pmask], a[1][~pmask], a[2][~mask], a[3][~mask])
    kept_first = np.concatenate(([0], np.cumsum(np.diff(first)[~mask])))
    same_answer(keep(poisoned), keep(want), kept_first, "the neighbours of the poisoned orders")
    assert res[3][40] == SPLIT_NAN and np.isnan(res[2][40])
    if grown > 8:
        assert res[3][39] == SPLIT_NAN and np.all(res[0][wrong[39]:wrong[40]] == 7.0)    # more than 8 paths: nothing written
    others = np.ones(MANY, dtype=bool)
    others[[39, 40]] = False
    po = np.repeat(others, np.diff(first))
    same_answer((res[0][po], res[1][po], res[2][others], res[3][others]), (want[0][po], want[1][po], want[2][others], want[3][others]),
                np.concatenate(([0], np.cumsum(np.diff(first)[others]))), "the orders around a bad path range")


# ---- execution --------------------------------------------------------------------------------------------------------------------
def test_one_swap_path_out_call_executes_an_orders_split():
    batches = market(seed=SEED)
    be = cr.DeviceBackend(N, batches)
    try:
        ctx = be.ctx
        o = make_orders_out(batches, "interleaved", 4, first_k=4, u=-3.0)  # K = 1, 2, 3, 8; a thousandth of the last hop's reserve
        x, c, total, st = split(ctx, o)
        done = 0
        for g in range(4):                                                # the orders share no pool either (rows 37 g + ..)
            lo, hi = int(o[0][g]), int(o[0][g + 1])
            if st[g] != SPLIT_OK:
                continue
            want_state = [ctx.reserves(s, M) for s in (0, 1, 2)]
            quoted, quoted_hops = ctx.quote_path_out(*(a[lo:hi] for a in o[2:7]), x[lo:hi], hops=True)
            cost, status, hop_in = ctx.swap_path_out(*(a[lo:hi] for a in o[2:7]), x[lo:hi], c[lo:hi], True)
            assert np.all(status == SWAP_APPLIED), (g, status)             # the limit is the split's own cost: it holds bit for bit
            same_bits(cost, c[lo:hi], f"order {g}: the paths share no pool, so each costs its quote")
            used = np.arange(H)[:, None] < o[2][lo:hi][None, :]
            same_bits(hop_in[used], quoted_hops[used], f"order {g}: every hop takes what quote_path_out said")
            assert abs(np.sum(x[lo:hi]) - o[1][g]) <= 8 * 2.0 ** -53 * o[1][g]
            # the pools moved: a two-coin pool of the first path's first hop holds cost more of coin_in
            s0, r0, i0 = int(o[3][lo, 0]), int(o[4][lo, 0]), int(o[5][lo, 0])
            if s0 in (0, 1, 2) and x[lo] > 0:
                after = ctx.reserves(s0, M)
                assert after[r0, i0] > want_state[s0][r0, i0]
            done += 1
        print(f"executed {done} of 4 orders; statuses {st}")
        assert done >= 2
    finally:
        be.close()


# ---- it is worth having -----------------------------------------------------------------------------------------------------------
def test_four_equal_pools_fill_what_no_single_pool_can_and_reach_the_closed_form():
    R, g_ = 1.0e5, 0.997
    r = cr.Router(cr.LinearNonnegative(np.ones(2)), [cr.ProductTwoCoin([R, R], g_, [1, 2]) for _ in range(4)], 2)
    try:
        paths, toks = [[0], [1], [2], [3]], [[1, 2]] * 4
        # half a pool's reserve: one path can give it, four give it for far less
        B = 0.5 * R
        single = cr.quote_path_out(r, [[0]], [[1, 2]], B)[0]
        x, c, total, st = cr.split_paths_out(r, [paths], [toks], B)
        best = 4.0 * (R * (B / 4) / (g_ * (R - B / 4)))
        print(f"split over four equal pools: {total[0]:.9g} against {single:.9g} through one; closed form {best:.9g}; shares {x[0]}")
        assert st[0] == cr.SPLIT_OK and total[0] < single
        assert total[0] <= single * (1 + 2 * EXCESS_MEASURED[5])
        assert abs(total[0] - best) / best <= 1e-9                         # equal pools: the grid holds the optimum, equal shares
        assert np.all(np.abs(x[0] - B / 4) <= 4 * (B / 63) * (4 / 63) ** 4)   # four slices of the fifth round, each 4/63 of the round before's
        same_bits(cr.quote_path_out(r, paths, toks, x[0]), c[0])
        # twice a pool's reserve: every single path answers +inf, the four together suffice
        B2 = 2.0 * R
        assert np.all(np.isposinf(cr.quote_path_out(r, paths, toks, B2)))
        x2, c2, total2, st2 = cr.split_paths_out(r, [paths], [toks], B2)
        assert st2[0] == cr.SPLIT_OK and np.isfinite(total2[0]) and abs(np.sum(x2[0]) - B2) <= 8 * 2.0 ** -53 * B2 and np.all(x2[0] < R)
        # ... and five times the reserve is more than all four hold
        x3, c3, total3, st3 = cr.split_paths_out(r, [paths], [toks], 5.0 * R)
        assert st3[0] == cr.SPLIT_UNOBTAINABLE and np.isposinf(total3[0]) and np.all(np.isposinf(c3[0])) and not np.any(bits(x3[0]))
        # the router's refusals are split_paths'
        with pytest.raises(cr.ArgumentError, match="order 0: paths 0 and 2 share pool 0"):
            cr.split_paths_out(r, [[[0], [1], [0]]], [[[1, 2]] * 3], B)
        with pytest.raises(cr.ArgumentError, match="order 0: its paths must all start at the same token and end at the same token"):
            cr.split_paths_out(r, [[[0], [1]]], [[[1, 2], [2, 1]]], B)
        with pytest.raises(cr.ArgumentError, match="order 0: 9 paths"):
            cr.split_paths_out(r, [[[0]] * 9], [[[1, 2]] * 9], B)
        # executing the answer buys exactly the shares for exactly the costs
        cost, status = cr.swap_path_out_(r, paths, toks, x[0], max_in=c[0])
        assert np.all(status == SWAP_APPLIED)
        same_bits(cost, c[0])
    finally:
        r.close()


def test_product_orders_cost_no_more_than_the_cheapest_single_path(world):
    """on product-only orders (segment 0, one hop per path) total_in is at most the cheapest single path's quote at B times
    (1 + 2 x the CPU test's measured worst excess at 5 rounds)"""
    ctx, b = world.ctx, world.batches[0]
    G, K = 12, 4
    first = np.arange(0, G * K + 1, K, dtype=np.int64)
    rows = ((11 * np.arange(G * K)) % M).astype(np.int64).reshape(-1, 1)
    assert all(len(set(rows[g * K:(g + 1) * K, 0].tolist())) == K for g in range(G))
    cin = (np.arange(G * K) % 2).astype(np.int32).reshape(-1, 1)
    hops = (np.ones(G * K, dtype=np.int32), np.zeros((G * K, 1), dtype=np.int32), rows, cin, 1 - cin)
    Rout = b.R[rows[:, 0], 1 - cin[:, 0]].reshape(G, K)
    B = Rout.min(axis=1) * np.linspace(0.05, 0.9, G)                        # every path can give it alone
    x, c, total, st = ctx.split_paths_out(first, B, *hops, 5)
    single = ctx.quote_path_out(*hops, np.repeat(B, K)).reshape(G, K)
    assert np.all(st == SPLIT_OK) and np.all(np.isfinite(single))
    print("total_in / cheapest single path:", np.array2string(total / single.min(axis=1), precision=4))
    assert np.all(total <= single.min(axis=1) * (1 + 2 * EXCESS_MEASURED[5]))


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_edges_zero_amount_dry_and_exhausted_univ3_no_orders_no_pools(world):
    ctx, u = world.ctx, world.batches[3]
    assert u.kind == KIND_UNIV3
    o = world.orders[("interleaved", 5)]
    got = ctx.split_paths_out(o[0], np.zeros(5), *o[2:7], 3)
    want = split_paths_out_ref(quoter(ctx, o), o[0], np.zeros(5), 3)
    same_answer(got, want, o[0], "B = 0")
    assert np.any(got[3] == SPLIT_NONE)
    none = got[3] == SPLIT_NONE
    assert not np.any(bits(got[2][none])) and not np.any(bits(got[0][np.repeat(none, np.diff(o[0]))]))
    # one-hop paths on a UniV3 segment of its own; the first eight pools hold no liquidity at all
    tick_pool = np.repeat(np.arange(M), np.diff(u.tick_off))
    u2 = batch_with(u, liquidity=np.where(tick_pool < 8, 0.0, u.liquidity))
    be = cr.DeviceBackend(N, [u2])
    try:
        c2 = be.ctx
        rows = np.tile(np.arange(M), 2)
        cin = np.repeat(np.array([0, 1], dtype=np.int32), M)
        scale = np.sqrt(u.liquidity[u.tick_off[:-1]] + 1.0)[rows]
        small, huge = (c2.quote(0, f * scale, cin, None, rows) for f in (1e-3, 1e10))
        dry = np.flatnonzero(huge == 0.0)
        live = np.flatnonzero(small > 0)
        assert dry.size >= 1 and live.size >= 3
        one = lambda a, dt: np.asarray(a, dtype=dt).reshape(-1, 1)

        def hops(q):
            q = np.asarray(q)
            return np.ones(q.size, dtype=np.int32), one(np.zeros(q.size), np.int32), one(rows[q], np.int64), one(cin[q], np.int32), one(1 - cin[q], np.int32)
        # a dry pool on one path of three: it can give nothing, so it gets nothing; the others give everything
        pick = [q for q in live if rows[q] != rows[dry[0]]]
        pick = [pick[0]] + [q for q in pick[1:] if rows[q] != rows[pick[0]]][:1]
        order = [pick[0], dry[0], pick[1]]
        B = 0.25 * min(small[pick[0]], small[pick[1]])                     # (what 1e-3 of the scale buys: each live path can give it)
        first = np.array([0, 3], dtype=np.int64)
        got = c2.split_paths_out(first, [B], *hops(order), 5)
        same_answer(got, split_paths_out_ref(quoter(c2, (first, None) + hops(order)), first, [B], 5), first, "a dry path")
        assert got[3][0] == SPLIT_OK and not bits(got[0][1:2])[0] and abs(got[0][0] + got[0][2] - B) <= 4 * 2.0 ** -53 * B and got[2][0] > 0
        # every path exhausted: more than the three ladders hold together
        B = 4.0 * huge[order].max() + 1.0
        got = c2.split_paths_out(first, [B], *hops(order), 5)
        same_answer(got, split_paths_out_ref(quoter(c2, (first, None) + hops(order)), first, [B], 5), first, "exhausted ladders")
        assert got[3][0] == SPLIT_UNOBTAINABLE and np.isposinf(got[2][0])
    finally:
        be.close()
    # count == 0: empty answers, and NULL arrays through the library
    e = np.zeros((0, H), dtype=np.int32)
    out = ctx.split_paths_out(np.zeros(1, dtype=np.int64), np.zeros(0), np.zeros(0, dtype=np.int32), e, e, e, e)
    assert all(a.size == 0 for a in out)
    ctx._check(cr.lib().cfmm_split_paths_out(ctx._h, 0, None, None, 0, H, None, None, None, None, None, 5, None, None, None, None))
    # a context without pools: the path checks refuse
    empty = cr.Context(4)
    try:
        with pytest.raises(cr.ArgumentError, match=r"cfmm_split_paths_out: order 0: path 0, hop 0: segment 0 out of range \(the context has 0\)"):
            empty.split_paths_out([0, 1], [1.0], [1], [0], [0], [0], [1])
    finally:
        empty.close()


# ---- read-only --------------------------------------------------------------------------------------------------------------------
def test_splitting_changes_nothing_the_other_calls_see():
    batches = [pools("product", 700, 61), pools("geomean", 700, 62), pools("univ3", 300, 63), pools("solidly", 300, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)
    p, k = np.meshgrid(np.arange(200), np.arange(4), indexing="ij")
    n_hops = (1 + np.arange(200) % 4).astype(np.int32)
    seg = ((p + k) % 4).astype(np.int32)
    row = ((7 * p + 13 * k) % 300).astype(np.int64)                     # paths 2g and 2g + 1 share no pool
    ci = ((p + k) % 2).astype(np.int32)
    co = (1 - ci).astype(np.int32)
    first = np.arange(0, 201, 2, dtype=np.int64)
    last = n_hops[::2] - 1
    amt = 0.2 * np.array([scale_in(batches[seg[q, l]])[row[q, l], co[q, l]] for q, l in zip(range(0, 200, 2), last)])

    def run(splitting):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def s():
            if splitting:
                ctx.split_paths_out(first, amt, n_hops, seg, row, ci, co, 3)
        try:
            s()                                                        # needs no sweep to have run
            ctx.find_arb(v)
            s()
            res.append(ctx.trades())
            s()
            res.append((ctx.netflows(), ctx.dual_value()))
            s()
            res.append([ctx.reserves(0, 700), ctx.reserves(1, 700), ctx.reserves(3, 300)])
            ctx.update_reserves()
            s()
            res.append(ctx.eval(v))
            s()
            vr, psi, info = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=60)
            s()
            res.append((vr, psi, {k_: info[k_] for k_ in ("f", "proj_grad", "iterations", "evaluations", "status")}, ctx.netflows()))
            res.append(ctx.split_paths(first, amt, n_hops, seg, row, ci, co, 2))   # the forward split answers the same, too
        finally:
            be.close()
        return res

    a, b = run(True), run(False)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for s_, t in zip(x, y):
                same(s_, t)
        elif isinstance(x, dict) or x is None:
            assert x == y
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    same(a, b)


# ---- other contexts ---------------------------------------------------------------------------------------------------------------
def test_a_multi_device_parent_gives_the_same_bits(world):
    multi = cr.Context(N, [0, 0])
    try:
        for b in world.batches:
            _upload(multi, b)
        multi.set_option("time_kernels", 1)
        for pattern, count, rounds in (("interleaved", MANY, 5), ("uniform", 5, 2), ("interleaved", 4, 1)):
            o = world.orders[(pattern, count)]
            same_answer(split(multi, o, rounds), world.ref(pattern, count, rounds), o[0], f"parent: {pattern}, {count}, {rounds}")
            assert multi.get_option("split_launches") == rounds and multi.get_option("split_ns") > 0
        with pytest.raises(NotImplementedError, match="cfmm_split_paths_out_dev"):
            multi.split_paths_out_dev(1, 8, 8, 1, 1, 8, 8, 8, 8, 8, 5, 8, 8, 8, 8)
    finally:
        multi.close()


def test_large_market_mode_gives_the_same_bits():
    """two-coin segments only (large-market mode has no N-coin kernel), one token moved beyond the LDS limit"""
    small = market()[:4]
    big = [batch_with(b, Ai=np.where(b.Ai == 1, 8193, b.Ai)) for b in small]
    o = list(make_orders(market(), "interleaved", MANY))
    o[3] = o[3] % 4                                                      # the four two-coin segments
    o[5], o[6] = o[5] % 2, 1 - o[5] % 2
    lead = o[0][:-1]
    last = o[2][lead] - 1
    o[1] = np.array([scale_in(small[o[3][q, l]])[o[4][q, l], o[6][q, l]] for q, l in zip(lead, last)]) * 0.01
    be_s, be_b = cr.DeviceBackend(N, small), cr.DeviceBackend(8193, big)
    try:
        a, b = split(be_s.ctx, o), split(be_b.ctx, o)
        same_answer(b, a, o[0])
        print("large market: statuses", np.bincount(a[3], minlength=5))
        assert np.sum(a[3] == SPLIT_OK) >= 10
    finally:
        be_s.close()
        be_b.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_the_host_entry_refuses_names_the_order_and_leaves_the_outputs(world):
    ctx, L = world.ctx, cr.lib()
    o = world.orders[("interleaved", 5)]
    first, amount, n_hops, seg, row, ci, co = o
    G, P = 5, int(first[-1])

    def refused(match, first=first, amount=amount, n_hops=n_hops, seg=seg, row=row, rounds=5, outputs=True, n_paths=P):
        out = [np.full(P, 7.0), np.full(P, 7.0), np.full(G, 7.0), np.full(G, 7, dtype=np.int32)]
        T = lambda a, dt: np.ascontiguousarray(np.asarray(a).T, dtype=dt)
        rc = L.cfmm_split_paths_out(ctx._h, G, ptr(np.ascontiguousarray(first, dtype=np.int64)), ptr(np.ascontiguousarray(amount)), n_paths, H,
                                    ptr(np.ascontiguousarray(n_hops, dtype=np.int32)), ptr(T(seg, np.int32)), ptr(T(row, np.int64)),
                                    ptr(T(ci, np.int32)), ptr(T(co, np.int32)), rounds, ptr(out[0]), ptr(out[1]), ptr(out[2] if outputs else None),
                                    ptr(out[3]))
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_split_paths_out:") and match in msg, (rc, msg)
        assert all(np.all(a == 7) for a in out)                            # the outputs are untouched

    def edit(a, at, value):
        a = a.copy()
        a[at] = value
        return a
    K = np.diff(first)
    g8 = int(np.argmax(K == 8))                                            # the 8-path order, and a path of it with 4 or more hops
    p_long = int(first[g8]) + int(np.argmax(n_hops[first[g8]:first[g8 + 1]] >= 4))
    refused("rounds must be 1 .. 16 (got 0)", rounds=0)
    refused("rounds must be 1 .. 16 (got 17)", rounds=MAX_SPLIT_ROUNDS + 1)
    refused("order 0: order_first[0] must be 0 (got 1)", first=edit(first, 0, 1))
    refused(f"order {g8}: order_first decreases", first=edit(first, g8 + 1, first[g8] - 1))
    refused(f"order {g8}: 9 paths (an order has 1 .. 8)", first=edit(first, g8 + 1, first[g8 + 1] + 1))
    refused(f"order_first[count] must be n_paths {P + 1}", n_paths=P + 1)
    refused("order 3: amount_out must be finite and >= 0", amount=edit(amount, 3, np.nan))
    refused("order 1: amount_out must be finite and >= 0", amount=edit(amount, 1, -1.0))
    refused("order 2: amount_out must be finite and >= 0", amount=edit(amount, 2, np.inf))
    refused(f"order {g8}: path {p_long - int(first[g8])}, hop 3: row", row=edit(row, (p_long, 3), M))
    refused(f"order {g8}: path {p_long - int(first[g8])}: n_hops 0", n_hops=edit(n_hops, p_long, 0))
    refused("null order array", outputs=False)
    # two paths of the 8-path order through one pool: path 1's hop 0 made path 6's hop 0
    a, b = int(first[g8]) + 1, int(first[g8]) + 6
    refused(f"order {g8}: paths 1 and 6 share pool (segment {int(seg[a, 0])}, row {int(row[a, 0])})",
            seg=edit(seg, (b, 0), seg[a, 0]), row=edit(row, (b, 0), row[a, 0]))
    with pytest.raises(cr.ArgumentError, match=f"order {g8}: paths 1 and 6 share pool"):
        ctx.split_paths_out(first, amount, n_hops, edit(seg, (b, 0), seg[a, 0]), edit(row, (b, 0), row[a, 0]), ci, co)


# ---- options ----------------------------------------------------------------------------------------------------------------------
def test_the_kernel_span_and_the_launch_count(world):
    ctx = world.ctx
    ctx.set_option("time_kernels", 1)
    try:
        o = world.orders[("uniform", MANY)]
        same_answer(split(ctx, o), world.ref("uniform", MANY, 5), o[0])
        assert ctx.get_option("split_ns") > 0 and ctx.get_option("split_launches") == 1      # one launch, whatever the rounds
        print(f"split_paths_out: {MANY} orders over {int(o[0][-1])} paths, 5 rounds: kernel span {ctx.get_option('split_ns')} ns")
    finally:
        ctx.set_option("time_kernels", 0)
