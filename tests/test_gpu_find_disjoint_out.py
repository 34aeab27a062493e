"""cfmm_find_disjoint_paths_out on the device: up to 8 paths per query that share no pool, for a WANTED OUTPUT, by successive runs
of cfmm_find_path_out's layered search with a per-query bitmap of absent pools.  The pin is bit-equality with the successive
search on the host (tests/find_disjoint_out_ref.py) driven by ctx.quote_out -- every output, every slot, with the layers folded
through LDS and without.  Around it: the contract's consequences (slot 0 is find_path_out, amounts do not decrease, no pool
twice, contiguous slots, the none values, quote_path_out answers the same bits), cycles, chunking, errors and special contexts.

The market is test_gpu_find_disjoint.py's (test_gpu_quote_path.py's eight segments of 257 pools on 65 tokens plus one token no
pool holds); the queries are test_gpu_find_path_out.py's: the wanted amounts 10^u of the median reserve of token_out, every
17th exactly 0.0, token_in == token_out in every 13th."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import FOUND, FOUND_NONE, FOUND_REPEATS, ptr
from cfmmrouter_amd.cfmms import _upload
from find_disjoint_out_ref import find_disjoint_out_ref
from test_gpu_find_path import tables
from test_gpu_find_path_out import NT, make_queries
from test_gpu_pool_update import batch_with
from test_gpu_quote import N
from test_gpu_quote_path import M, bits, market, same_bits

pytestmark = pytest.mark.gpu

COUNT = 1025
COUNTS = (1, 65, 1025)
PATHS = (1, 2, 8)
HOPS = (1, 3, 8)
NAMES = ("n_paths", "amount_in", "n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out", "status")


def assert_same(got, want, what=""):
    """(n_paths, amount_in, n_hops, seg, row, ci, co, status) bit for bit"""
    for k, name in enumerate(NAMES):
        assert got[k].shape == want[k].shape, f"{what} {name}: shape {got[k].shape} vs {want[k].shape}"
        if name == "amount_in":
            same_bits(got[k], want[k], f"{what} {name}")
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {name}")


def leading(ref, count, K):
    """the answer for the first `count` queries and max_paths K of a reference for more of both: queries are independent and the
    rounds successive, so it is the leading part; n_paths is recounted"""
    cutk = [a[:count, :K] for a in ref[1:]]
    return (np.sum(cutk[-1] != FOUND_NONE, axis=1).astype(np.int32), *cutk)


class World:
    def __init__(self):
        self.batches = market()
        self.be = cr.DeviceBackend(NT, self.batches)
        self.ctx = self.be.ctx
        self.tok = tables(self.batches)
        self.queries = make_queries(self.batches, NT, COUNT)
        self._refs = {}

    def ref(self, max_hops):
        """the reference for 8 paths and every query at that max_hops, computed once and left unchanged"""
        if max_hops not in self._refs:
            tin, tout, amt = self.queries
            self._refs[max_hops] = find_disjoint_out_ref(self.tok, self.ctx.quote_out, NT, tin, tout, amt, max(PATHS), max_hops)
        return self._refs[max_hops]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.be.close()


# ---- 1. the pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("max_paths", PATHS)
@pytest.mark.parametrize("max_hops", HOPS)
def test_the_device_is_the_successive_search_bit_for_bit(world, max_hops, max_paths, count):
    ctx, (tin, tout, amt) = world.ctx, world.queries
    sl = slice(0, count)
    want = leading(world.ref(max_hops), count, max_paths)
    assert ctx.get_option("find_lds") == 1
    got = ctx.find_disjoint_paths_out(tin[sl], tout[sl], amt[sl], max_paths, max_hops)
    assert got[0].shape == (count,) and got[1].shape == got[2].shape == got[7].shape == (count, max_paths)
    assert got[3].shape == got[4].shape == got[5].shape == got[6].shape == (count, max_paths, max_hops)
    assert_same(got, want, f"max_hops {max_hops}, max_paths {max_paths}, count {count}:")
    assert ctx.get_option("find_launches") == max_paths * (3 * max_hops + 3)   # one chunk: init, relax x H, select, (claim, advance) x H, finish per round
    ctx.set_option("find_lds", 0)
    try:
        assert_same(ctx.find_disjoint_paths_out(tin[sl], tout[sl], amt[sl], max_paths, max_hops), want, f"find_lds 0, {max_hops}, {max_paths}, {count}:")
    finally:
        ctx.set_option("find_lds", 1)
    n_paths = got[0]
    print(f"find_disjoint_paths_out max_hops {max_hops}, max_paths {max_paths}, count {count}: n_paths histogram "
          f"{np.bincount(n_paths, minlength=max_paths + 1).tolist()}, statuses {np.bincount(got[7].reshape(-1), minlength=3).tolist()}")
    if count == COUNT and max_paths == 8:                                  # the comparison is not one of empty answers
        assert np.sum(n_paths >= 2) >= count // 2
        if max_hops > 1:
            assert np.any(got[2] > 1)
    if max_paths == 1:                                                     # max_paths == 1 is cfmm_find_path_out bit for bit
        one = ctx.find_path_out(tin[sl], tout[sl], amt[sl], max_hops)
        same_bits(got[1][:, 0], one[0], "max_paths 1 amount_in")
        for k, j in ((2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6)):
            np.testing.assert_array_equal(got[k][:, 0], one[j], err_msg=f"max_paths 1 {NAMES[k]}")


# ---- 2. the consequences of the contract ---------------------------------------------------------------------------------------
def test_slot_0_is_find_path_out_and_the_slots_are_ordered_disjoint_contiguous_and_quotable(world):
    ctx, tok, (tin, tout, amt) = world.ctx, world.tok, world.queries
    K, H = 8, 3
    n_paths, cost, n_hops, seg, row, ci, co, status = ctx.find_disjoint_paths_out(tin, tout, amt, K, H)
    one = ctx.find_path_out(tin, tout, amt, H)
    same_bits(cost[:, 0], one[0], "slot 0 amount_in")
    for got, want, name in ((n_hops, one[1], "n_hops"), (seg, one[2], "seg"), (row, one[3], "row"), (ci, one[4], "ci"), (co, one[5], "co"),
                            (status, one[6], "status")):
        np.testing.assert_array_equal(got[:, 0], want, err_msg=f"slot 0 {name}")
    assert np.all(cost[:, 1:] >= cost[:, :-1])                             # each round minimises over a subset of the one before
    found = status != FOUND_NONE
    np.testing.assert_array_equal(n_paths, found.sum(axis=1))
    assert np.all(found == (np.arange(K)[None, :] < n_paths[:, None]))     # the found slots are the leading ones
    # empty slots: find_path_out's none value -- +inf, or +0.0 where amount_out is 0 -- 0 hops and -1
    zero = np.broadcast_to((amt == 0.0)[:, None], found.shape)
    assert np.any(zero) and np.all(~found[zero]) and not np.any(bits(cost[zero]))
    assert np.all(np.isposinf(cost[~found & ~zero])) and np.all(n_hops[~found] == 0)
    unused = np.arange(H)[None, None, :] >= n_hops[:, :, None]
    for a in (seg, row, ci, co):
        assert np.all(a[unused] == -1) and np.all(a[~unused] >= 0)
    assert np.all((n_hops > 0) == found) and np.all(np.isfinite(cost[found]) & (cost[found] > 0))
    for q in range(COUNT):                                                 # no (segment, row) in two paths of a query
        seen = set()
        for r in range(n_paths[q]):
            mine = {(int(seg[q, r, k]), int(row[q, r, k])) for k in range(n_hops[q, r])}
            assert not seen & mine, (q, r)
            assert (len(mine) < n_hops[q, r]) == (status[q, r] == FOUND_REPEATS)
            seen |= mine
    q, r = np.nonzero(status == FOUND)                                     # cfmm_quote_path_out refuses a walk that repeats a pool
    again = ctx.quote_path_out(n_hops[q, r], seg[q, r], row[q, r], ci[q, r], co[q, r], amt[q])
    same_bits(again, cost[q, r], "quote_path_out on every found path")
    assert q.size > 2 * COUNT
    for j in range(0, q.size, 17):                                         # token-continuous, from token_in to token_out
        path = [(tok[seg[q[j], r[j], k]][row[q[j], r[j], k], ci[q[j], r[j], k]], tok[seg[q[j], r[j], k]][row[q[j], r[j], k], co[q[j], r[j], k]])
                for k in range(n_hops[q[j], r[j]])]
        assert path[0][0] == tin[q[j]] and path[-1][1] == tout[q[j]] and all(a[1] == b[0] for a, b in zip(path, path[1:]))
    # token_in == token_out: cycles are found, slot after slot, and the unheld token reaches nothing
    cyc = tin == tout
    assert np.any(cyc & (n_paths >= 2)) and np.all(n_paths[(tin == NT - 1) | (tout == NT - 1)] == 0)


def test_batching_does_not_change_the_bits(world):
    ctx, (tin, tout, amt) = world.ctx, world.queries
    order = np.arange(COUNT)[::-1][:100]                                   # other queries, another order: other chunk rows, other lanes
    got = ctx.find_disjoint_paths_out(tin[order], tout[order], amt[order], 8, 3)
    assert_same(got, tuple(a[order] for a in world.ref(3)), "reversed batch:")


# ---- 3. exact ties and a walk that re-enters a pool ----------------------------------------------------------------------------
def test_two_identical_pools_are_taken_one_after_the_other():
    """two identical pools in parallel, in two segments: round 0 takes the smaller (segment, row), round 1 the other at the same
    cost bit for bit -- the banned twin ties the layer word and must not be claimed -- and round 2 finds nothing"""
    twin = lambda: cr.ProductTwoCoin.batch(np.array([[5e5, 7e5], [3e5, 2e5]]), np.array([0.997, 0.997]), np.array([[1, 2], [2, 3]]))
    be = cr.DeviceBackend(3, [twin(), twin()])
    try:
        got = be.ctx.find_disjoint_paths_out([0, 0], [1, 2], [1000.0, 1000.0], 3, 2)
        n_paths, cost, n_hops, seg, row, ci, co, status = got
        assert n_paths.tolist() == [2, 2] and status.tolist() == [[FOUND, FOUND, FOUND_NONE]] * 2
        assert seg[0, :, 0].tolist() == [0, 1, -1] and row[0, :, 0].tolist() == [0, 0, -1] and n_hops[0].tolist() == [1, 1, 0]
        assert bits(cost[0, 0]) == bits(cost[0, 1]) and cost[0, 0] > 0 and np.isposinf(cost[0, 2])
        # two hops: the first path takes both pools of segment 0, the second both of segment 1 -- never one of each
        assert n_hops[1].tolist() == [2, 2, 0] and seg[1, 0].tolist() == [0, 0] and seg[1, 1].tolist() == [1, 1] and row[1, 0].tolist() == [0, 1]
        assert bits(cost[1, 0]) == bits(cost[1, 1])
        assert_same(got, find_disjoint_out_ref(tables([twin(), twin()]), be.ctx.quote_out, 3, [0, 0], [1, 2], [1000.0, 1000.0], 3, 2), "twins:")
    finally:
        be.close()


# ---- 4. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunks_of_a_large_market_call_equal_single_queries():
    """test_gpu_find_disjoint.py's large-market device: 65536 tokens and 8 hops make a query's layers 4.5 MiB, so the 256 MiB
    budget cuts 120 queries into three chunks.  A ban row that is not cleared per chunk, or that is indexed by the call's query
    number and not the chunk's, shows in the second round of the later chunks."""
    n_big = 65536
    small = market()[:4]                                                   # product, geomean, solidly, univ3
    big = [batch_with(b, Ai=np.where(b.Ai == 1, n_big, b.Ai)) for b in small]
    be = cr.DeviceBackend(n_big, big)
    try:
        count, H, K = 120, 8, 2
        per_query = ((H + 1) * n_big + (4 * M + 63) // 64) * 8
        assert 2 * ((256 << 20) // per_query) < count <= 3 * ((256 << 20) // per_query)   # three chunks
        tin, tout, amt = make_queries(small, N, count, seed=5)
        tin[::7], tout[3::11] = n_big - 1, n_big - 1                       # the moved token, as source and as destination
        whole = be.ctx.find_disjoint_paths_out(tin, tout, amt, K, H)
        assert be.ctx.get_option("find_launches") == 3 * K * (3 * H + 3)
        singles = [be.ctx.find_disjoint_paths_out(tin[q:q + 1], tout[q:q + 1], amt[q:q + 1], K, H) for q in range(count)]
        assert_same(whole, tuple(np.concatenate([s[k] for s in singles]) for k in range(8)), "chunked vs one by one:")
        assert np.sum(whole[0] == 2) > count // 3                          # second rounds that found something, in every chunk
        assert all(np.any(whole[0][c0:c0 + 56] == 2) for c0 in (0, 56, 112))
        # ... and the reference, on a few of them (its layers are [9, queries, 65536] doubles), from every chunk
        f = np.array([3, 40, 60, 100, 115, 119])
        want = find_disjoint_out_ref(tables(big), be.ctx.quote_out, n_big, tin[f], tout[f], amt[f], K, H)
        assert_same(tuple(a[f] for a in whole), want, "large-market mode vs the reference:")
    finally:
        be.close()


# ---- 5. errors and special contexts -------------------------------------------------------------------------------------------
def test_refusals_name_the_query_and_launch_nothing(world):
    ctx, (tin, tout, amt) = world.ctx, world.queries
    L = cr.lib()
    n, K, H = 16, 3, 3
    ok = ctx.find_disjoint_paths_out(tin[:n], tout[:n], amt[:n], K, H)
    launches = ctx.get_option("find_launches")
    assert launches == K * (3 * H + 3)

    def refused(match, tin=tin[:n], tout=tout[:n], amt=amt[:n], max_paths=K, max_hops=H, count=n, null=None):
        npaths, out = np.full(n, 7, dtype=np.int32), np.full((8, n), 7.0)
        nh, st = (np.full((8, n), 7, dtype=np.int32) for _ in range(2))
        seg, ci, co = (np.full((8, 8, n), 7, dtype=np.int32) for _ in range(3))
        row = np.full((8, 8, n), 7, dtype=np.int64)
        args = [ptr(np.ascontiguousarray(tin, dtype=np.int32)), ptr(np.ascontiguousarray(tout, dtype=np.int32)), ptr(np.ascontiguousarray(amt)),
                ptr(npaths), ptr(out), ptr(nh), ptr(st), ptr(seg), ptr(row), ptr(ci), ptr(co)]
        if null is not None:
            args[null] = None
        rc = L.cfmm_find_disjoint_paths_out(ctx._h, count, max_paths, max_hops, *args)
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_find_disjoint_paths_out:") and match in msg, (rc, msg)
        for a in (npaths, out, nh, st, seg, ci, co, row):
            assert np.all(a == 7)                                          # the outputs are untouched
        assert ctx.get_option("find_launches") == launches                 # nothing was launched

    def edit(a, q, value):
        a = np.array(a, copy=True)
        a[q] = value
        return a
    refused(f"query 12: token_in {NT} out of range (the market has {NT} tokens)", tin=edit(tin[:n], 12, NT))
    refused(f"query 15: token_out {NT + 5} out of range", tout=edit(tout[:n], 15, NT + 5))
    for bad in (-1.0, np.nan, np.inf):
        refused("query 7: amount_out must be finite and >= 0", amt=edit(amt[:n], 7, bad))
    refused("max_paths must be 1 .. 8 (got 0)", max_paths=0)
    refused("max_paths must be 1 .. 8 (got 9)", max_paths=9)
    refused("max_hops must be 1 .. 8 (got 9)", max_hops=9)
    refused("count must be >= 0", count=-1)
    for k in range(11):                                                    # n_paths (3) among them
        refused("null query array", null=k)
    with pytest.raises(cr.ArgumentError, match="query 1: token_out"):
        ctx.find_disjoint_paths_out([0, 1], [1, NT], 1.0)
    with pytest.raises(cr.ArgumentError, match="amount_out must be scalars or have one entry per query"):
        ctx.find_disjoint_paths_out([0, 1], [1, 2, 3], 1.0)
    # count == 0 is a no-op, NULL arrays accepted
    ctx._check(L.cfmm_find_disjoint_paths_out(ctx._h, 0, K, H, *([None] * 11)))
    empty = ctx.find_disjoint_paths_out([], [], [], K, H)
    assert empty[0].shape == (0,) and empty[1].shape == (0, K) and empty[3].shape == (0, K, H)
    assert_same(ctx.find_disjoint_paths_out(tin[:n], tout[:n], amt[:n], K, H), ok, "after the refusals:")
    assert_same(ok, leading(world.ref(H), n, K), "the answer itself:")


def test_a_context_without_pools_finds_nothing_and_a_parent_is_unsupported(world):
    empty = cr.Context(4)
    try:
        n_paths, cost, n_hops, seg, row, ci, co, status = empty.find_disjoint_paths_out([0, 1], [1, 1], [1.0, 0.0], 3, 2)
        assert n_paths.tolist() == [0, 0] and np.all(status == FOUND_NONE) and np.all(n_hops == 0)
        assert np.all(np.isposinf(cost[0])) and not np.any(bits(cost[1]))  # +inf, and +0.0 where nothing is wanted
        assert np.all(seg == -1) and np.all(row == -1) and np.all(ci == -1) and np.all(co == -1) and seg.shape == (2, 3, 2)
    finally:
        empty.close()
    multi = cr.Context(NT, [0, 0])
    try:
        for b in world.batches[:2]:
            _upload(multi, b)
        with pytest.raises(NotImplementedError, match="cfmm_find_disjoint_paths_out is not available on a multi-device context"):
            multi.find_disjoint_paths_out(0, 1, 1.0)
    finally:
        multi.close()
