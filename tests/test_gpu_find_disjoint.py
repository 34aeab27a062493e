"""cfmm_find_disjoint_paths on the device: up to 8 paths per query that share no pool, by successive runs of cfmm_find_path's
layered search with a per-query bitmap of absent pools.  The pin is bit-equality with the successive search on the host
(tests/find_disjoint_ref.py) driven by ctx.quote -- every output, every slot.  Around it: the contract's consequences (slot 0 is
find_path, amounts do not increase, no pool twice, contiguous slots, quote_path answers the same bits), both layer kernels, exact
ties, a walk that re-enters a pool, chunking, live state, errors and special contexts, the router-level calls.

The market is test_gpu_quote_path.py's: 8 segments of 257 pools on 65 tokens -- 2056 pools, no multiple of 64, and no segment
but the first starts on a multiple of 64, so ban words straddle segment boundaries."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import FOUND, FOUND_NONE, FOUND_REPEATS, KIND_UNIV3, PATH_APPLIED, SPLIT_NONE, SPLIT_OK, ptr
from cfmmrouter_amd.cfmms import _upload
from find_disjoint_ref import find_disjoint_ref
from test_gpu_find_path import NT, make_queries, tables
from test_gpu_pool_update import batch_with
from test_gpu_quote import N
from test_gpu_quote_path import M, bits, market, same_bits

pytestmark = pytest.mark.gpu

COUNT = 257
COUNTS = (1, 65, 257)
PATHS = (1, 2, 8)
HOPS = (1, 3)
NAMES = ("n_paths", "amount_out", "n_hops", "hop_seg", "hop_row", "hop_coin_in", "hop_coin_out", "status")


def assert_same(got, want, what=""):
    """(n_paths, amount_out, n_hops, seg, row, ci, co, status) bit for bit"""
    for k, name in enumerate(NAMES):
        assert got[k].shape == want[k].shape, f"{what} {name}: shape {got[k].shape} vs {want[k].shape}"
        if name == "amount_out":
            same_bits(got[k], want[k], f"{what} {name}")
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {name}")


def leading(ref, count, K):
    """the answer for the first `count` queries and max_paths K of a reference for more of both: queries are independent and the
    rounds successive, so it is the leading part; n_paths is recounted"""
    cutk = [a[:count, :K] for a in ref[1:]]
    return (np.sum(cutk[-1] != FOUND_NONE, axis=1).astype(np.int32), *cutk)


@pytest.fixture(scope="module")
def world():
    """the eight-segment market on one context of NT tokens, make_queries' queries, and the reference for 8 paths at 1 and 3 hops,
    computed once and left unchanged"""
    batches = market()
    assert sum(b.Ai.shape[0] for b in batches) == 8 * M == 2056 and 2056 % 64 and all((s * M) % 64 for s in range(1, 8))
    be = cr.DeviceBackend(NT, batches)
    tok = tables(batches)
    tin, tout, amt = make_queries(batches, NT, COUNT)
    refs = {H: find_disjoint_ref(tok, be.ctx.quote, NT, tin, tout, amt, max(PATHS), H) for H in HOPS}
    yield batches, be.ctx, tok, (tin, tout, amt), refs
    be.close()


# ---- 1. the pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("max_paths", PATHS)
@pytest.mark.parametrize("max_hops", HOPS)
def test_the_device_is_the_successive_search_bit_for_bit(world, max_hops, max_paths, count):
    batches, ctx, tok, (tin, tout, amt), refs = world
    sl = slice(0, count)
    want = leading(refs[max_hops], count, max_paths)
    got = ctx.find_disjoint_paths(tin[sl], tout[sl], amt[sl], max_paths, max_hops)
    assert got[0].shape == (count,) and got[1].shape == got[2].shape == got[7].shape == (count, max_paths)
    assert got[3].shape == got[4].shape == got[5].shape == got[6].shape == (count, max_paths, max_hops)
    assert_same(got, want, f"max_hops {max_hops}, max_paths {max_paths}, count {count}:")
    n_paths = got[0]
    print(f"find_disjoint_paths max_hops {max_hops}, max_paths {max_paths}, count {count}: n_paths histogram "
          f"{np.bincount(n_paths, minlength=max_paths + 1).tolist()}, statuses {np.bincount(got[7].reshape(-1), minlength=3).tolist()}")
    assert ctx.get_option("find_launches") == max_paths * (3 * max_hops + 3)   # one chunk: init, relax x H, select, (claim, advance) x H, finish per round
    if count == COUNT and max_paths == 8:                                  # the comparison is not one of empty answers
        assert np.sum(n_paths >= 2) >= count // 2
        if max_hops == 1:
            assert np.any((n_paths > 0) & (n_paths < 8))                   # some queries run out of direct pools on the way
        else:
            assert np.any(n_paths == 8) and np.any(got[2] > 1)
    if max_paths == 1:                                                     # max_paths == 1 is cfmm_find_path bit for bit
        one = ctx.find_path(tin[sl], tout[sl], amt[sl], max_hops)
        same_bits(got[1][:, 0], one[0], "max_paths 1 amount_out")
        for k, j in ((2, 1), (3, 2), (4, 3), (5, 4), (6, 5), (7, 6)):
            np.testing.assert_array_equal(got[k][:, 0], one[j], err_msg=f"max_paths 1 {NAMES[k]}")


# ---- 2. the consequences of the contract ---------------------------------------------------------------------------------------
def test_slot_0_is_find_path_and_the_slots_are_ordered_disjoint_contiguous_and_quotable(world):
    batches, ctx, tok, (tin, tout, amt), refs = world
    K, H = 8, 3
    n_paths, out, n_hops, seg, row, ci, co, status = ctx.find_disjoint_paths(tin, tout, amt, K, H)
    one = ctx.find_path(tin, tout, amt, H)
    same_bits(out[:, 0], one[0], "slot 0 amount_out")
    for got, want, name in ((n_hops, one[1], "n_hops"), (seg, one[2], "seg"), (row, one[3], "row"), (ci, one[4], "ci"), (co, one[5], "co"),
                            (status, one[6], "status")):
        np.testing.assert_array_equal(got[:, 0], want, err_msg=f"slot 0 {name}")
    assert np.all(out[:, 1:] <= out[:, :-1])                               # each round maximises over a subset of the one before
    found = status != FOUND_NONE
    np.testing.assert_array_equal(n_paths, found.sum(axis=1))
    assert np.all(found == (np.arange(K)[None, :] < n_paths[:, None]))     # the found slots are the leading ones
    assert np.all(out[~found] == 0.0) and not np.any(np.signbit(out[~found])) and np.all(n_hops[~found] == 0)
    unused = np.arange(H)[None, None, :] >= n_hops[:, :, None]
    for a in (seg, row, ci, co):
        assert np.all(a[unused] == -1) and np.all(a[~unused] >= 0)
    assert np.all((n_hops > 0) == found) and np.all(out[found] > 0)
    for q in range(COUNT):                                                 # no (segment, row) in two paths of a query
        seen = set()
        for r in range(n_paths[q]):
            mine = {(int(seg[q, r, k]), int(row[q, r, k])) for k in range(n_hops[q, r])}
            assert not seen & mine, (q, r)
            assert (len(mine) < n_hops[q, r]) == (status[q, r] == FOUND_REPEATS)
            seen |= mine
    q, r = np.nonzero(status == FOUND)                                     # cfmm_quote_path refuses a walk that repeats a pool
    again = ctx.quote_path(n_hops[q, r], seg[q, r], row[q, r], ci[q, r], co[q, r], amt[q])
    same_bits(again, out[q, r], "quote_path on every found path")
    assert q.size > 4 * COUNT
    for j in range(0, q.size, 7):                                          # token-continuous, from token_in to token_out
        path = [(tok[seg[q[j], r[j], k]][row[q[j], r[j], k], ci[q[j], r[j], k]], tok[seg[q[j], r[j], k]][row[q[j], r[j], k], co[q[j], r[j], k]])
                for k in range(n_hops[q[j], r[j]])]
        assert path[0][0] == tin[q[j]] and path[-1][1] == tout[q[j]] and all(a[1] == b[0] for a, b in zip(path, path[1:]))


# ---- 3. the layer kernels -------------------------------------------------------------------------------------------------------
def test_both_layer_kernels_give_the_same_bits(world):
    """option "find_lds": the layers folded through a per-block LDS copy (the default here) or straight into global memory"""
    batches, ctx, tok, (tin, tout, amt), refs = world
    assert ctx.get_option("find_lds") == 1
    ctx.set_option("find_lds", 0)
    try:
        for H in HOPS:
            assert_same(ctx.find_disjoint_paths(tin, tout, amt, 8, H), refs[H], f"find_lds 0, max_hops {H}:")
    finally:
        ctx.set_option("find_lds", 1)


def test_batching_does_not_change_the_bits(world):
    batches, ctx, tok, (tin, tout, amt), refs = world
    order = np.arange(COUNT)[::-1][:100]                                   # other queries, another order: other chunk rows, other lanes
    got = ctx.find_disjoint_paths(tin[order], tout[order], amt[order], 8, 3)
    assert_same(got, tuple(a[order] for a in refs[3]), "reversed batch:")


# ---- 4. exact ties ----------------------------------------------------------------------------------------------------------
def test_two_identical_pools_are_taken_one_after_the_other():
    """two identical pools in parallel, in two segments: round 0 takes the smaller (segment, row), round 1 the other with the same
    amount bit for bit -- the banned twin ties the layer word and must not be claimed -- and round 2 finds nothing"""
    twin = lambda: cr.ProductTwoCoin.batch(np.array([[5e5, 7e5], [3e5, 2e5]]), np.array([0.997, 0.997]), np.array([[1, 2], [2, 3]]))
    be = cr.DeviceBackend(3, [twin(), twin()])
    try:
        n_paths, out, n_hops, seg, row, ci, co, status = be.ctx.find_disjoint_paths([0, 0], [1, 2], [1000.0, 1000.0], 3, 2)
        assert n_paths.tolist() == [2, 2] and status.tolist() == [[FOUND, FOUND, FOUND_NONE]] * 2
        assert seg[0, :, 0].tolist() == [0, 1, -1] and row[0, :, 0].tolist() == [0, 0, -1] and n_hops[0].tolist() == [1, 1, 0]
        assert bits(out[0, 0]) == bits(out[0, 1]) and out[0, 0] > 0 and out[0, 2] == 0.0
        # two hops: the first path takes both pools of segment 0, the second both of segment 1 -- never one of each
        assert n_hops[1].tolist() == [2, 2, 0] and seg[1, 0].tolist() == [0, 0] and seg[1, 1].tolist() == [1, 1] and row[1, 0].tolist() == [0, 1]
        assert bits(out[1, 0]) == bits(out[1, 1])
        assert_same((n_paths, out, n_hops, seg, row, ci, co, status),
                    find_disjoint_ref(tables([twin(), twin()]), be.ctx.quote, 3, [0, 0], [1, 2], [1000.0, 1000.0], 3, 2), "twins:")
    finally:
        be.close()


# ---- 5. a walk that re-enters a pool ----------------------------------------------------------------------------------------
def test_a_walk_that_re_enters_a_pool_keeps_its_slot_and_its_pools_are_banned():
    """test_gpu_find_path.py's A -> B -> A -> B market (pool 0 deep and one for one, pool 1 gives four A for a B) and a shallow
    third pool: round 0 is the walk through pools 0, 1, 0; round 1 may use neither and finds the shallow pool; round 2 nothing"""
    pools = cr.ProductTwoCoin.batch(np.array([[1e9, 1e9], [4e6, 1e6], [1e3, 1e3]]), np.array([0.997] * 3), np.array([[1, 2]] * 3))
    be = cr.DeviceBackend(3, [pools])
    try:
        ctx = be.ctx
        got = ctx.find_disjoint_paths([0], [1], [1000.0], 4, 3)
        n_paths, out, n_hops, seg, row, ci, co, status = got
        assert status[0].tolist() == [FOUND_REPEATS, FOUND, FOUND_NONE, FOUND_NONE] and n_paths.tolist() == [2]
        assert row[0, 0].tolist() == [0, 1, 0] and row[0, 1].tolist() == [2, -1, -1] and n_hops[0].tolist() == [3, 1, 0, 0]
        assert out[0, 0] > 3000.0 and 400.0 < out[0, 1] < 500.0
        same_bits(ctx.quote_path(n_hops[:, 1], seg[:, 1], row[:, 1], ci[:, 1], co[:, 1], [1000.0]), out[:, 1], "the second path is quote_path's")
        assert_same(got, find_disjoint_ref(tables([pools]), ctx.quote, 3, [0], [1], [1000.0], 4, 3), "re-entering walk:")
        # within one hop nothing repeats: the three pools, deepest first
        one = ctx.find_disjoint_paths([0], [1], [1000.0], 4, 1)
        assert one[7][0].tolist() == [FOUND, FOUND, FOUND, FOUND_NONE] and one[4][0, :, 0].tolist() == [0, 2, 1, -1]   # about 997, 499 and 249 out
        assert_same(one, find_disjoint_ref(tables([pools]), ctx.quote, 3, [0], [1], [1000.0], 4, 1), "one hop:")
    finally:
        be.close()


# ---- 6. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunks_of_a_large_market_call_equal_single_queries():
    """test_gpu_find_path.py's large-market device: 65536 tokens and 8 hops make a query's layers 4.5 MiB, so the 256 MiB budget
    cuts 120 queries into three chunks.  A ban row that is not cleared per chunk, or that is indexed by the call's query number
    and not the chunk's, shows in the second round of the later chunks."""
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
        whole = be.ctx.find_disjoint_paths(tin, tout, amt, K, H)
        assert be.ctx.get_option("find_launches") == 3 * K * (3 * H + 3)
        singles = [be.ctx.find_disjoint_paths(tin[q:q + 1], tout[q:q + 1], amt[q:q + 1], K, H) for q in range(count)]
        assert_same(whole, tuple(np.concatenate([s[k] for s in singles]) for k in range(8)), "chunked vs one by one:")
        assert np.sum(whole[0] == 2) > count // 2                          # second rounds that found something, in every chunk
        assert all(np.any(whole[0][c0:c0 + 56] == 2) for c0 in (0, 56, 112))
        # ... and the reference, on a few of them (its layers are [9, queries, 65536] doubles), from every chunk
        f = np.array([3, 40, 60, 100, 115, 119])
        want = find_disjoint_ref(tables(big), be.ctx.quote, n_big, tin[f], tout[f], amt[f], K, H)
        assert_same(tuple(a[f] for a in whole), want, "large-market mode vs the reference:")
    finally:
        be.close()


# ---- 7. live state --------------------------------------------------------------------------------------------------------------
def test_the_answer_follows_the_market_and_the_call_changes_nothing():
    batches = market(seed=41)
    be = cr.DeviceBackend(NT, batches)
    try:
        ctx = be.ctx
        tok = tables(batches)
        tin, tout, amt = make_queries(batches, NT, 65, seed=9)
        K, H = 4, 3
        first = ctx.find_disjoint_paths(tin, tout, amt, K, H)
        assert_same(first, find_disjoint_ref(tok, ctx.quote, NT, tin, tout, amt, K, H), "before:")
        n_paths, out, n_hops, seg, row, ci, co, status = first
        q = int(np.flatnonzero((status[:, 0] == FOUND) & (n_paths >= 2))[0])   # a swap_ on the first pool of its slot 0's path
        ctx.swap(int(seg[q, 0, 0]), [amt[q]], [ci[q, 0, 0]], [co[q, 0, 0]], [row[q, 0, 0]])
        R_before = [ctx.reserves(s, M, b.Ai.shape[1]) for s, b in enumerate(batches) if b.kind != KIND_UNIV3]
        refused = ctx.get_option("swap_refused")
        v = synth.sweep_prices(NT, seed=43, spread=0.3)
        ctx.find_arb(v)
        trades = ctx.trades()
        probe = ctx.quote(0, amt[:8], [0] * 8, [1] * 8, np.arange(8))
        one = ctx.find_path(tin, tout, amt, H)
        a = ctx.find_disjoint_paths(tin, tout, amt, K, H)
        b = ctx.find_disjoint_paths(tin, tout, amt, K, H)
        assert_same(a, b, "twice in a row:")
        assert_same(a, find_disjoint_ref(tok, ctx.quote, NT, tin, tout, amt, K, H), "after the swap:")
        assert bits(a[1][q, 0]) != bits(out[q, 0])                          # the market did move under that query
        # read-only: reserves, trades, a quote, find_path and the refusal count are where they were
        for R0, R1 in zip(R_before, [ctx.reserves(s, M, b_.Ai.shape[1]) for s, b_ in enumerate(batches) if b_.kind != KIND_UNIV3]):
            np.testing.assert_array_equal(R0, R1)
        for t0, t1 in zip(trades, ctx.trades()):
            np.testing.assert_array_equal(np.asarray(t0), np.asarray(t1))
        same_bits(ctx.quote(0, amt[:8], [0] * 8, [1] * 8, np.arange(8)), probe, "a quote after the call")
        again = ctx.find_path(tin, tout, amt, H)
        same_bits(again[0], one[0], "find_path after the call")
        for x, y in zip(again[1:], one[1:]):
            np.testing.assert_array_equal(x, y)
        assert ctx.get_option("swap_refused") == refused
        np.testing.assert_array_equal(ctx.netflows(), ctx.netflows())
    finally:
        be.close()


# ---- 8. errors and special contexts -------------------------------------------------------------------------------------------
def test_refusals_name_the_query_and_launch_nothing(world):
    batches, ctx, tok, (tin, tout, amt), refs = world
    L = cr.lib()
    n, K, H = 16, 3, 3
    ok = ctx.find_disjoint_paths(tin[:n], tout[:n], amt[:n], K, H)
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
        rc = L.cfmm_find_disjoint_paths(ctx._h, count, max_paths, max_hops, *args)
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_find_disjoint_paths:") and match in msg, (rc, msg)
        for a in (npaths, out, nh, st, seg, ci, co, row):
            assert np.all(a == 7)                                          # the outputs are untouched
        assert ctx.get_option("find_launches") == launches                 # nothing was launched

    def edit(a, q, value):
        a = np.array(a, copy=True)
        a[q] = value
        return a
    refused(f"query 12: token_in {NT} out of range (the market has {NT} tokens)", tin=edit(tin[:n], 12, NT))
    refused("query 3: token_in -1", tin=edit(tin[:n], 3, -1))
    refused(f"query 15: token_out {NT + 5} out of range", tout=edit(tout[:n], 15, NT + 5))
    for bad in (-1.0, np.nan, np.inf):
        refused("query 7: amount_in must be finite and >= 0", amt=edit(amt[:n], 7, bad))
    refused("query 2: token_in", tin=edit(tin[:n], 2, NT), amt=edit(amt[:n], 9, -1.0))   # the first bad query is named
    refused("max_paths must be 1 .. 8 (got 0)", max_paths=0)
    refused("max_paths must be 1 .. 8 (got 9)", max_paths=9)
    refused("max_hops must be 1 .. 8 (got 0)", max_hops=0)
    refused("max_hops must be 1 .. 8 (got 9)", max_hops=9)
    refused("count must be >= 0", count=-1)
    for k in range(11):                                                    # n_paths (3) among them
        refused("null query array", null=k)
    with pytest.raises(cr.ArgumentError, match="query 1: token_out"):
        ctx.find_disjoint_paths([0, 1], [1, NT], 1.0)
    with pytest.raises(cr.ArgumentError, match="max_paths"):
        ctx.find_disjoint_paths(0, 1, 1.0, max_paths=9)
    with pytest.raises(cr.ArgumentError, match="one entry per query"):
        ctx.find_disjoint_paths([0, 1], [1, 2, 3], 1.0)
    # count == 0 is a no-op, NULL arrays accepted
    ctx._check(L.cfmm_find_disjoint_paths(ctx._h, 0, K, H, *([None] * 11)))
    empty = ctx.find_disjoint_paths([], [], [], K, H)
    assert empty[0].shape == (0,) and empty[1].shape == (0, K) and empty[3].shape == (0, K, H)
    assert_same(ctx.find_disjoint_paths(tin[:n], tout[:n], amt[:n], K, H), ok, "after the refusals:")
    assert_same(ok, leading(refs[H], n, K), "the answer itself:")


def test_a_context_without_pools_finds_nothing_and_a_parent_is_unsupported(world):
    batches = world[0]
    empty = cr.Context(4)
    try:
        n_paths, out, n_hops, seg, row, ci, co, status = empty.find_disjoint_paths([0, 1], [1, 1], [1.0, 2.0], 3, 2)
        assert n_paths.tolist() == [0, 0] and np.all(status == FOUND_NONE) and np.all(out == 0.0) and np.all(n_hops == 0)
        assert np.all(seg == -1) and np.all(row == -1) and np.all(ci == -1) and np.all(co == -1) and seg.shape == (2, 3, 2)
    finally:
        empty.close()
    multi = cr.Context(NT, [0, 0])
    try:
        for b in batches[:2]:
            _upload(multi, b)
        with pytest.raises(NotImplementedError, match="cfmm_find_disjoint_paths is not available on a multi-device context"):
            multi.find_disjoint_paths(0, 1, 1.0)
    finally:
        multi.close()


def test_round_spans_fall_once_queries_have_ended(world):
    """under "time_kernels" every round reports its layer and walk spans; they add up to the call's"""
    batches, ctx, tok, (tin, tout, amt), refs = world
    ctx.set_option("time_kernels", 1)
    try:
        ctx.find_disjoint_paths(tin, tout, amt, 8, 3)
        relax = [ctx.get_option(f"find_round_relax_ns_{r}") for r in range(1, 9)]
        walk = [ctx.get_option(f"find_round_walk_ns_{r}") for r in range(1, 9)]
        print(f"per-round relax ns {relax}, walk ns {walk}")
        assert all(x > 0 for x in relax + walk)
        assert sum(relax) == ctx.get_option("find_relax_ns") and sum(walk) == ctx.get_option("find_walk_ns")
        ctx.find_disjoint_paths(tin, tout, amt, 2, 3)
        assert [ctx.get_option(f"find_round_relax_ns_{r}") > 0 for r in range(1, 9)] == [True, True] + [False] * 6
        ctx.find_path(tin, tout, amt, 3)                                   # the other entries have one round
        assert ctx.get_option("find_round_relax_ns_1") == ctx.get_option("find_relax_ns") > 0 and ctx.get_option("find_round_relax_ns_2") == 0
    finally:
        ctx.set_option("time_kernels", 0)


COUNTERS = ("debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams")


def live_counts_body():
    probe = cr.Context(4)
    live = lambda: tuple(probe.get_option(k) for k in COUNTERS)
    base = live()
    batches = market()
    be = cr.DeviceBackend(NT, batches)
    tin, tout, amt = make_queries(batches, NT, 65)
    before = live()
    be.ctx._check(cr.lib().cfmm_find_disjoint_paths(be.ctx._h, 0, 4, 3, *([None] * 11)))
    assert live() == before                                              # count == 0 touches nothing
    be.ctx.find_disjoint_paths(tin, tout, amt, 4, 3)
    first = live()
    # the first call creates the search's scratch and the ban rows: 7 device arrays (table, layers, edges, int32 columns, rows,
    # amounts, ban), one pinned staging buffer, no event without time_kernels, no stream
    assert tuple(x - y for x, y in zip(first, before)) == (7, 1, 0, 0), (before, first)
    be.ctx.find_disjoint_paths(tin[:10], tout[:10], amt[:10], 8, 2)
    be.ctx.find_path(tin, tout, amt, 3)                                  # find_path shares the scratch
    be.ctx.find_disjoint_paths(tin, tout, amt, 4, 3)
    assert live()[1:] == first[1:] and live()[0] == first[0]             # stable across calls (arrays grow in place)
    be.close()
    assert live() == base                                                # everything goes with the context
    probe.close()
    print("find-disjoint-live-ok")


def test_live_counts_with_the_hooks_library():
    """the four debug_live_* counts return to where they were: the ban rows follow the DevBuf owner pattern"""
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_find_disjoint as t\n"
            "t.live_counts_body()\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "find-disjoint-live-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- 9. the router-level calls ------------------------------------------------------------------------------------------------
def five_pools():
    """examples/split_order.py's market: three pools 1 -> 2 of different depth and the detour 1 -> 3 -> 2"""
    return [cr.ProductTwoCoin([1.0e5, 1.0e5], 0.997, [1, 2]), cr.ProductTwoCoin([5.0e4, 5.0e4], 0.999, [1, 2]),
            cr.ProductTwoCoin([2.0e4, 2.0e4], 0.997, [1, 2]), cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [1, 3]),
            cr.ProductTwoCoin([8.0e4, 8.0e4], 0.997, [3, 2])]


def test_router_level_find_split_execute_and_route_order():
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), five_pools(), 3)
    try:
        A = 1.0e5
        out, pools, tokens, status = cr.find_disjoint_paths(r, [1, 2, 1], [2, 1, 1], [A, 0.0, A], max_paths=8, max_hops=3)
        assert {tuple(p) for p in pools[0]} == {(0,), (1,), (2,), (3, 4)} and len(pools[0]) == 4 and pools[0][0] == [0]
        assert tokens[0] == [[1, 3, 2] if p == [3, 4] else [1, 2] for p in pools[0]] and status[0].tolist() == [FOUND] * 4
        assert pools[1] == [] and tokens[1] == [] and out[1].size == 0     # amount 0: nothing found
        # the cycles through token 1: on this market the best one always goes out and back through the SAME pool -- walks that
        # repeat a pool, which split_paths would refuse, so none is listed; usable_only=False shows them, each pool banned in turn
        assert pools[2] == [] and tokens[2] == [] and status[2].size == 0
        _, walks, wtok, wst = cr.find_disjoint_paths(r, 1, 1, A, max_paths=8, max_hops=3, usable_only=False)
        assert wst[0].tolist() == [FOUND_REPEATS] * 4 and walks[0][0] == [0, 0] and sorted(walks[0]) == [[0, 0], [1, 1], [2, 2], [3, 3]]
        assert all(tk[0] == tk[-1] == 1 and len(tk) == 3 for tk in wtok[0])
        same_bits(cr.quote_path(r, pools[0], tokens[0], np.full(4, A)), out[0], "cr.quote_path on cr.find_disjoint_paths")
        assert np.all(out[0][1:] <= out[0][:-1])
        single, path, _, _ = cr.find_path(r, 1, 2, A, max_hops=3)
        assert path[0] == pools[0][0] and bits(single[0]) == bits(out[0][0])
        x, y, total, st = cr.split_paths(r, [pools[0]], [tokens[0]], A)
        assert st.tolist() == [SPLIT_OK] and total[0] > out[0][0] and abs(np.sum(x[0]) - A) <= 1e-15 * A
        routed = cr.route_order(r, [1, 2], [2, 1], [A, 0.0], max_paths=8, max_hops=3)
        assert routed[0] == [pools[0], []] and routed[1] == [tokens[0], []]
        same_bits(routed[2][0], x[0], "route_order's shares")
        same_bits(routed[3][0], y[0], "route_order's outputs")
        assert bits(routed[4][0]) == bits(total[0]) and routed[4][1] == 0.0 and routed[5].tolist() == [SPLIT_OK, SPLIT_NONE]
        assert routed[2][1].size == 0 and routed[3][1].size == 0
        quarter = cr.route_order(r, 1, 2, A, max_paths=2, probe=A / 4)     # two paths, probed with a share's size
        assert len(quarter[0][0]) == 2 and quarter[5].tolist() == [SPLIT_OK] and quarter[4][0] < total[0]
        got, applied = cr.swap_path_(r, pools[0], tokens[0], x[0])         # find -> split -> execute
        assert np.all(applied == PATH_APPLIED)
        same_bits(got, y[0], "swap_path_ gives what split_paths promised")
        after = cr.route_order(r, 1, 2, A, max_paths=8, max_hops=3)
        assert after[4][0] < total[0]                                      # the market it left is worse
    finally:
        r.close()
