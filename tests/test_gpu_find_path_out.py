"""cfmm_find_path_out on the device: the cheapest swap walk of at most max_hops hops that BUYS an exact amount, found by the
layered search run backwards from the wanted output -- one launch per layer with one lane per pool, an integer atomic min on the
doubles' bits -- and walked forward.  The pin of the whole feature is bit-equality with the layered search on the host
(tests/find_path_out_ref.py) driven by ctx.quote_out: amount, n_hops, the four hop arrays and the status.  Around it: both
layer kernels, cfmm_quote_path_out on the result, the tie-break, brute force over every walk of a small market, chunking, live
state, the statuses and the two NONE amounts, execution with the found amount as the limit, errors."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import FOUND, FOUND_NONE, FOUND_REPEATS, KIND_UNIV3, SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, ptr
from cfmmrouter_amd.cfmms import _upload
from find_path_out_ref import find_path_out_ref, layers_out
from find_path_ref import brute_force_walks
from test_gpu_find_path import small_market, tables
from test_gpu_pool_update import batch_with
from test_gpu_quote import N
from test_gpu_quote_path import M, bits, market, same_bits

pytestmark = pytest.mark.gpu

NT = N + 1              # one token more than the pools use: token NT - 1 is held by no pool
COUNT = 1025
HOPS = (1, 3, 8)
COUNTS = (1, 65, 1025)
U_LO, U_HI = -6.0, -1.5  # the wanted amounts: 10^u of the median reserve of token_out, u uniform in [U_LO, U_HI]


def reserve_scale(batches, n_tokens):
    """per token the median reserve of it over the non-UniV3 pools that hold it; 1.0 for a token none of them holds"""
    per = [[] for _ in range(n_tokens)]
    for b in batches:
        if b.kind == KIND_UNIV3:
            continue
        for c in range(b.Ai.shape[1]):
            for t, x in zip((b.Ai[:, c] - 1).tolist(), b.R[:, c].tolist()):
                per[t].append(x)
    return np.array([np.median(p) if p else 1.0 for p in per])


def query_tokens(n_tokens, count):
    """token_in = q mod n_tokens (65 queries cover every token, the unheld one included); token_out walks through every token at
    another stride, equals token_in in every 13th query (a cycle) and is the unheld token in every 65th"""
    q = np.arange(count)
    tin = (q % n_tokens).astype(np.int32)
    tout = ((7 * q + q // n_tokens + 1) % n_tokens).astype(np.int32)
    tout[q % 13 == 5] = tin[q % 13 == 5]
    tout[q % 65 == 33] = n_tokens - 1
    return tin, tout


def amounts_out(scale, tout, seed):
    """10^u of the scale of token_out, u uniform in [U_LO, U_HI]; every 17th exactly 0.0"""
    count = len(tout)
    amt = scale[tout] * 10.0 ** (U_LO + (U_HI - U_LO) * synth.uniform(seed, 8, count))
    amt[np.arange(count) % 17 == 11] = 0.0
    return amt


def make_queries(batches, n_tokens, count, seed=3):
    tin, tout = query_tokens(n_tokens, count)
    return tin, tout, amounts_out(reserve_scale(batches, n_tokens), tout, seed)


def assert_same(got, want, what=""):
    """(amount_in, n_hops, seg, row, ci, co, status) bit for bit"""
    same_bits(got[0], want[0], what + " amount_in")
    for k, name in ((1, "n_hops"), (2, "hop_seg"), (3, "hop_row"), (4, "hop_coin_in"), (5, "hop_coin_out"), (6, "status")):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {name}")


def assert_none_is_well_formed(got, amt):
    cost, n_hops, seg, row, ci, co, status = got
    none = status == FOUND_NONE
    assert np.all(n_hops[none] == 0) and np.all(seg[none] == -1) and np.all(row[none] == -1) and np.all(ci[none] == -1) and np.all(co[none] == -1)
    zero = none & (amt == 0.0)
    assert np.all(bits(cost[zero]) == 0)                                   # +0.0: buying nothing costs nothing
    assert np.all(np.isposinf(cost[none & (amt != 0.0)]))                  # +inf: token_in is not reached
    assert np.all(np.isfinite(cost[~none]) & (cost[~none] > 0))
    unused = np.arange(seg.shape[1])[None, :] >= n_hops[:, None]
    assert np.all(seg[unused] == -1) and np.all(row[unused] == -1) and np.all(ci[unused] == -1) and np.all(co[unused] == -1)


@pytest.fixture(scope="module")
def world():
    """the eight-segment market on one context of NT tokens, the queries, and the reference's layers for 8 hops, computed once
    and left unchanged (layer h is the same whatever max_hops is)"""
    batches = market()
    be = cr.DeviceBackend(NT, batches)
    tok = tables(batches)
    tin, tout, amt = make_queries(batches, NT, COUNT)
    need = layers_out(tok, be.ctx.quote_out, NT, tout, amt, max(HOPS))
    yield batches, be.ctx, tok, (tin, tout, amt), need
    be.close()


# ---- 1. the pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("max_hops", HOPS)
def test_find_path_out_is_the_layered_search_bit_for_bit(world, max_hops, count):
    batches, ctx, tok, (tin, tout, amt), need = world
    sl = slice(0, count)
    want = find_path_out_ref(tok, ctx.quote_out, NT, tin[sl], tout[sl], amt[sl], max_hops, need=need[:, sl])
    got = ctx.find_path_out(tin[sl], tout[sl], amt[sl], max_hops)
    assert got[2].shape == got[3].shape == got[4].shape == got[5].shape == (count, max_hops)
    cost, n_hops, seg, row, ci, co, status = got
    print(f"find_path_out max_hops {max_hops}, count {count}: hops histogram {np.bincount(n_hops, minlength=max_hops + 1).tolist()}, "
          f"statuses {np.bincount(status, minlength=3).tolist()}")
    assert_same(got, want, f"max_hops {max_hops}, count {count}:")
    assert_none_is_well_formed(got, amt[sl])
    none = status == FOUND_NONE
    assert np.all((amt[sl] == 0.0) <= none) and np.all((tout[sl] == NT - 1) <= none) and np.all((tin[sl] == NT - 1) <= none)
    if count == COUNT:
        assert np.sum(status != FOUND_NONE) > count // 2                   # the comparison is not one of empty answers
        if max_hops > 1:
            assert np.any(n_hops > 1) and np.any((tin[sl] == tout[sl]) & (status != FOUND_NONE))   # cycles are found


# ---- 2. both layer kernels ------------------------------------------------------------------------------------------------------
def test_both_layer_kernels_give_the_same_bits(world):
    """option "find_lds": the layers folded through a per-block LDS copy (default where n_tokens lets one fit) or straight into
    global memory (what a market of more than 4096 tokens gets) -- integer minima either way"""
    batches, ctx, tok, (tin, tout, amt), need = world
    assert ctx.get_option("find_lds") == 1
    with_lds = {H: ctx.find_path_out(tin, tout, amt, H) for H in (3, 8)}
    ctx.set_option("find_lds", 0)
    try:
        for max_hops in (3, 8):
            got = ctx.find_path_out(tin, tout, amt, max_hops)
            assert_same(got, with_lds[max_hops], f"find_lds 0 vs 1, max_hops {max_hops}:")
            assert_same(got, find_path_out_ref(tok, ctx.quote_out, NT, tin, tout, amt, max_hops, need=need), f"find_lds 0, max_hops {max_hops}:")
    finally:
        ctx.set_option("find_lds", 1)


# ---- 3. cfmm_quote_path_out on the result ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_hops", (3, 8))
def test_quote_path_out_on_the_result_answers_the_same_bits(world, max_hops):
    batches, ctx, tok, (tin, tout, amt), need = world
    cost, n_hops, seg, row, ci, co, status = ctx.find_path_out(tin, tout, amt, max_hops)
    f = np.flatnonzero(status != FOUND_NONE)
    again, hops = ctx.quote_path_out(n_hops[f], seg[f], row[f], ci[f], co[f], amt[f], hops=True)
    same_bits(again, cost[f], "quote_path_out on the found hops")
    for j, q in enumerate(f):                                              # hop k is tendered the layer value of the token it leaves
        h = n_hops[q]
        for k in range(h):
            t = tok[seg[q, k]][row[q, k], ci[q, k]]
            assert bits(hops[k, j]) == bits(need[h - k, q, t]), (q, k)
        assert tok[seg[q, 0]][row[q, 0], ci[q, 0]] == tin[q] and tok[seg[q, h - 1]][row[q, h - 1], co[q, h - 1]] == tout[q]
        for k in range(1, h):                                              # token-continuous
            assert tok[seg[q, k]][row[q, k], ci[q, k]] == tok[seg[q, k - 1]][row[q, k - 1], co[q, k - 1]]


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_smaller_segment_row_and_coins():
    """the segment most found hops run through, once more in its own later rows AND as a last segment: every edge of it has two
    exact twins, and the one in the smallest (segment, row) must be the hop"""
    base = market()
    tin, tout, amt = make_queries(base, NT, 195)
    be0 = cr.DeviceBackend(NT, base)
    try:
        plain = be0.ctx.find_path_out(tin, tout, amt, 3)
    finally:
        be0.close()
    used = np.arange(3)[None, :] < plain[1][:, None]
    twin = int(np.argmax(np.bincount(plain[2][used], minlength=len(base))))
    dup = base[:twin] + [cr.PoolBatch.concat([base[twin], base[twin]])] + base[twin + 1:] + [base[twin]]
    be = cr.DeviceBackend(NT, dup)
    try:
        tok = tables(dup)
        got = be.ctx.find_path_out(tin, tout, amt, 3)
        assert_same(got, find_path_out_ref(tok, be.ctx.quote_out, NT, tin, tout, amt, 3), "ties:")
        _, n_hops, seg, row, _, _, status = got
        used = np.arange(3)[None, :] < n_hops[:, None]
        print(f"ties: {int(np.sum(used & (seg == twin)))} hops of {int(np.sum(used))} run through segment {twin}")
        assert np.sum(used & (seg == twin)) > 0                            # the segment is on found paths ...
        assert not np.any(used & (seg == len(dup) - 1)) and not np.any(used & (seg == twin) & (row >= M))   # ... its twins on none
        assert_same(plain, got, "without the twins: the same amounts through the same pools")
    finally:
        be.close()


# ---- 5. brute force -------------------------------------------------------------------------------------------------------------
SMALL_N = 6


def test_brute_force_over_every_walk_of_a_small_market():
    """Every walk of 1 .. 3 hops between the query's tokens on the 40-pool market, priced by ONE ctx.quote_path_out call.  The
    expected excess of the found amount over the enumeration's minimum is exactly 0; it may exceed it only where rounding breaks
    a quote_out's monotonicity.  The allowance is the margin tests/test_gpu_find_path.py takes: max_hops x the per-quote bound
    K u (R + in* + cond) of tests/quote_precise_ref.py with K = K_CAP, R = the largest reserve of token_in any first hop can
    add to, in* = the minimum itself, and cond left out -- which only makes it tighter.  The measured excess is printed."""
    batches = small_market()
    be = cr.DeviceBackend(SMALL_N, batches)
    try:
        tok = tables(batches)
        scale = reserve_scale(batches, SMALL_N)
        # every token as source and as destination, to its neighbour and back to itself (the cheapest cycle), small and larger amounts
        queries = [(a, b, scale[b] * 10.0 ** (-4.0 if (a + b) % 2 else -2.0)) for a in range(SMALL_N) for b in ((a + 1) % SMALL_N, a)]
        tin, tout, amt = (np.array(x) for x in zip(*queries))
        H = 3
        cost, n_hops, seg, row, ci, co, status = be.ctx.find_path_out(tin, tout, amt, H)
        walks, owner = [], []
        for q, (a, b, _) in enumerate(queries):
            w = brute_force_walks(tok, a, b, H)
            walks += w
            owner += [q] * len(w)
        owner = np.array(owner)
        print(f"brute force: {len(queries)} queries, {len(walks)} walks")
        assert 10_000 < len(walks) < 1_000_000
        wn = np.array([len(w) for w in walks], dtype=np.int32)
        cols = np.zeros((4, len(walks), H), dtype=np.int64)
        for j, w in enumerate(walks):
            cols[:, j, :len(w)] = np.array(w).T
        priced = be.ctx.quote_path_out(wn, cols[0].astype(np.int32), cols[1], cols[2].astype(np.int32), cols[3].astype(np.int32), amt[owner])
        priced = np.where(np.isfinite(priced) & (priced > 0), priced, np.inf)
        low = np.full(len(queries), np.inf)
        np.minimum.at(low, owner, priced)
        assert np.all(np.isfinite(low)) and np.all(status != FOUND_NONE)   # every query is answered: none is skipped
        Rmax = np.zeros(SMALL_N)
        for b in batches:
            if b.kind != KIND_UNIV3:
                np.maximum.at(Rmax, (b.Ai - 1).reshape(-1), b.R.reshape(-1))
        allowed = H * P.bound(P.K_CAP, Rmax[tin], low, 0.0)
        excess = cost - low
        print(f"brute force: largest excess found - min = {excess.max():.3e} (relative {np.max(excess / low):.3e}), "
              f"smallest allowance {allowed.min():.3e}; found below the enumeration nowhere: {bool(np.all(cost >= low))}")
        assert np.all(cost >= low)                                         # the found walk is one of the enumeration
        assert np.all(excess <= allowed)
    finally:
        be.close()


# ---- 6. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunks_of_a_large_market_call_equal_single_queries():
    """large-market mode (65536 tokens, plain Ai arrays); 8 hops make a query's layers 4.5 MiB, so the 256 MiB budget cuts 120
    queries into three chunks"""
    n_big = 65536
    small = market()[:4]                                                   # product, geomean, solidly, univ3
    big = [batch_with(b, Ai=np.where(b.Ai == 1, n_big, b.Ai)) for b in small]
    be = cr.DeviceBackend(n_big, big)
    try:
        count, H = 120, 8
        assert 2 * ((256 << 20) // ((H + 1) * n_big * 8)) < count          # at least three chunks
        tin, tout = query_tokens(N, count)
        tin[::7], tout[3::11] = n_big - 1, n_big - 1                       # the moved token, as source and as destination
        amt = amounts_out(reserve_scale(big, n_big), tout, seed=5)
        whole = be.ctx.find_path_out(tin, tout, amt, H)
        launches = be.ctx.get_option("find_launches")
        assert launches == 3 * (3 * H + 3)
        singles = [be.ctx.find_path_out(tin[q:q + 1], tout[q:q + 1], amt[q:q + 1], H) for q in range(count)]
        assert_same(whole, tuple(np.concatenate([s[k] for s in singles]) for k in range(7)), "chunked vs one by one:")
        assert np.sum(whole[6] != FOUND_NONE) > count // 2
        # ... and the reference, on a few of them (its layers are [9, queries, 65536] doubles): large-market mode gives its bits
        f = np.arange(0, count, 17)
        want = find_path_out_ref(tables(big), be.ctx.quote_out, n_big, tin[f], tout[f], amt[f], H)
        assert_same(tuple(a[f] for a in whole), want, "large-market mode vs the reference:")
    finally:
        be.close()


# ---- 7. live state --------------------------------------------------------------------------------------------------------------
def test_find_path_out_follows_the_market_and_changes_nothing():
    batches = market(seed=41)
    other = market(seed=42)
    be = cr.DeviceBackend(NT, batches)
    try:
        ctx = be.ctx
        tok = tables(batches)
        tin, tout, amt = make_queries(batches, NT, 130, seed=9)
        first = ctx.find_path_out(tin, tout, amt, 3)
        assert_same(first, find_path_out_ref(tok, ctx.quote_out, NT, tin, tout, amt, 3), "before:")
        # execute hops of the found paths (the first visit of every pool) with swap_, and rewrite eighty reserves
        cost, n_hops, seg, row, ci, co, status = first
        seen = set()
        for q in np.flatnonzero(status == FOUND)[:40]:
            x = cost[q]
            for k in range(n_hops[q]):
                if (seg[q, k], row[q, k]) in seen:
                    break
                seen.add((seg[q, k], row[q, k]))
                x = ctx.swap(int(seg[q, k]), [x], [ci[q, k]], [co[q, k]], [row[q, k]])[0]
        rows = np.arange(0, M, 3)[:80].astype(np.int64)
        ctx.set_reserves(0, rows, other[0].R[rows])
        R_before = [ctx.reserves(s, M, b.Ai.shape[1]) for s, b in enumerate(batches) if b.kind != KIND_UNIV3]
        refused = ctx.get_option("swap_refused")
        v = synth.sweep_prices(NT, seed=43, spread=0.3)
        ctx.find_arb(v)
        trades = ctx.trades()
        a = ctx.find_path_out(tin, tout, amt, 3)
        b = ctx.find_path_out(tin, tout, amt, 3)
        assert_same(a, b, "twice in a row:")
        assert_same(a, find_path_out_ref(tok, ctx.quote_out, NT, tin, tout, amt, 3), "after swaps and set_reserves:")
        assert np.any(bits(a[0]) != bits(first[0]))                        # the market did move
        # read-only: reserves, trades, outputs and the refusal count are where they were
        for R0, R1 in zip(R_before, [ctx.reserves(s, M, b_.Ai.shape[1]) for s, b_ in enumerate(batches) if b_.kind != KIND_UNIV3]):
            np.testing.assert_array_equal(R0, R1)
        for t0, t1 in zip(trades, ctx.trades()):
            np.testing.assert_array_equal(np.asarray(t0), np.asarray(t1))
        assert ctx.get_option("swap_refused") == refused
        np.testing.assert_array_equal(ctx.netflows(), ctx.netflows())
    finally:
        be.close()


# ---- 8. statuses and edges ------------------------------------------------------------------------------------------------------
def test_statuses_the_two_none_amounts_and_a_walk_that_re_enters_a_pool():
    """A -> B -> A -> B: pool 0 trades A and B one for one and is deep; pool 1 gives four A for a B.  The cheapest way to buy B
    with A within 3 hops buys it from pool 0 with A that was bought from pool 1 with B that was bought from pool 0: pool 0 twice."""
    pools = cr.ProductTwoCoin.batch(np.array([[1e9, 1e9], [4e6, 1e6]]), np.array([0.997, 0.997]), np.array([[1, 2], [1, 2]]))
    be = cr.DeviceBackend(3, [pools])
    try:
        ctx = be.ctx
        cost, n_hops, seg, row, ci, co, status = ctx.find_path_out([0, 0], [1, 1], [1000.0, 1000.0], 3)
        assert status.tolist() == [FOUND_REPEATS] * 2 and n_hops.tolist() == [3, 3]
        assert row[0].tolist() == [0, 1, 0] and ci[0].tolist() == [0, 1, 0] and co[0].tolist() == [1, 0, 1]   # path order
        assert 250.0 < cost[0] < 260.0
        same_bits(ctx.quote_path_out(n_hops, seg, row, ci, co, [1000.0, 1000.0]), cost, "the amounts are quote_path_out's")
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_path_out: path 0"):
            ctx.swap_path_out(n_hops, seg, row, ci, co, [1000.0, 1000.0])
        one = ctx.find_path_out([0], [1], [1000.0], 1)                     # within one hop: the deep pool, no repeat
        assert one[6].tolist() == [FOUND] and one[1].tolist() == [1] and one[3][0].tolist() == [0] and 1003.0 < one[0][0] < 1003.1
        two = ctx.find_path_out([0], [1], [1000.0], 2)                     # no two hops lead from A to B: the same answer
        assert_same(tuple(a[:, :1] if a.ndim == 2 else a for a in two), one, "max_hops 2:")
        # NONE: more than any pool holds (+inf) -- at 1e9 itself, one ulp below it is still obtainable in one hop;
        # token 2 is held by no pool, as source and as destination (+inf); nothing to buy (+0.0), whatever the tokens
        none = ctx.find_path_out([0, 0, 2, 0, 0, 2], [1, 1, 0, 2, 1, 2], [1e9, 2e9, 1.0, 1.0, 0.0, 0.0], 3)
        assert none[6].tolist() == [FOUND_NONE] * 6 and np.all(none[1] == 0) and np.all(none[3] == -1) and np.all(none[2] == -1)
        assert np.all(np.isposinf(none[0][:4])) and bits(none[0][4:]).tolist() == [0, 0]
        assert ctx.find_path_out([0], [1], [np.nextafter(1e9, 0.0)], 1)[6].tolist() == [FOUND]
    finally:
        be.close()


def test_a_found_path_executes_with_its_own_amount_as_the_limit():
    batches = market(seed=51)
    be = cr.DeviceBackend(NT, batches)
    try:
        tin, tout, amt = make_queries(batches, NT, 65, seed=11)
        cost, n_hops, seg, row, ci, co, status = be.ctx.find_path_out(tin, tout, amt, 3)
        f = np.flatnonzero(status == FOUND)
        assert f.size > 20
        q = f[np.argmax(n_hops[f])]                                        # one path (a batch would move shared pools in between)
        s = slice(q, q + 1)
        paid, st = be.ctx.swap_path_out(n_hops[s], seg[s], row[s], ci[s], co[s], amt[s], max_in=cost[s])
        assert st[0] in (SWAP_APPLIED, SWAP_REFUSED) and st[0] != SWAP_OVER_LIMIT   # the limit is the quote itself: never over it
        print(f"executing a found path of {n_hops[q]} hops with max_in = amount_in: status {st[0]}")
        if st[0] == SWAP_APPLIED:
            same_bits(paid, cost[s], "swap_path_out costs what find_path_out promised")
            after = be.ctx.find_path_out(tin[s], tout[s], amt[s], 3)
            assert after[0][0] > cost[q]                                   # the same order afterwards costs more
        else:
            assert np.isnan(paid[0])                                       # refused by a state condition: nothing moved
    finally:
        be.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_query_and_launch_nothing(world):
    batches, ctx, tok, (tin, tout, amt), need = world
    L = cr.lib()
    n, H = 16, 3
    ok = ctx.find_path_out(tin[:n], tout[:n], amt[:n], H)
    launches = ctx.get_option("find_launches")
    assert launches == 3 * H + 3

    def refused(match, tin=tin[:n], tout=tout[:n], amt=amt[:n], max_hops=H, count=n, null=None):
        out, nh, st = np.full(n, 7.0), np.full(n, 7, dtype=np.int32), np.full(n, 7, dtype=np.int32)
        seg, ci, co = (np.full((8, n), 7, dtype=np.int32) for _ in range(3))
        row = np.full((8, n), 7, dtype=np.int64)
        args = [ptr(np.ascontiguousarray(tin, dtype=np.int32)), ptr(np.ascontiguousarray(tout, dtype=np.int32)), ptr(np.ascontiguousarray(amt)),
                ptr(out), ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(st)]
        if null is not None:
            args[null] = None
        rc = L.cfmm_find_path_out(ctx._h, count, max_hops, *args)
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_find_path_out:") and match in msg, (rc, msg)   # CFMM_ERR_INVALID_ARG
        for a in (out, nh, st, seg, ci, co, row):
            assert np.all(a == 7)                                          # the outputs are untouched
        assert ctx.get_option("find_launches") == launches                 # nothing was launched

    def edit(a, q, value):
        a = np.array(a, copy=True)
        a[q] = value
        return a
    refused(f"query 12: token_in {NT} out of range (the market has {NT} tokens)", tin=edit(tin[:n], 12, NT))
    refused("query 3: token_in -1", tin=edit(tin[:n], 3, -1))
    refused(f"query 15: token_out {NT + 5} out of range", tout=edit(tout[:n], 15, NT + 5))
    refused("query 0: token_out -2", tout=edit(tout[:n], 0, -2))
    for bad in (-1.0, np.nan, np.inf):
        refused("query 7: amount_out must be finite and >= 0", amt=edit(amt[:n], 7, bad))
    refused("query 2: token_in", tin=edit(tin[:n], 2, NT), amt=edit(amt[:n], 9, -1.0))   # the first bad query is named
    refused("max_hops must be 1 .. 8 (got 0)", max_hops=0)
    refused("max_hops must be 1 .. 8 (got 9)", max_hops=9)
    refused("count must be >= 0", count=-1)
    for k in range(10):
        refused("null query array", null=k)
    # through the wrapper the refusals are ArgumentErrors
    with pytest.raises(cr.ArgumentError, match="query 1: token_out"):
        ctx.find_path_out([0, 1], [1, NT], 1.0, 3)
    with pytest.raises(cr.ArgumentError, match="query 0: amount_out"):
        ctx.find_path_out(0, 1, np.nan)
    with pytest.raises(cr.ArgumentError, match="max_hops"):
        ctx.find_path_out(0, 1, 1.0, max_hops=9)
    # count == 0 is a no-op, NULL arrays accepted
    ctx._check(L.cfmm_find_path_out(ctx._h, 0, 3, None, None, None, None, None, None, None, None, None, None))
    assert ctx.find_path_out([], [], [], 3)[0].size == 0
    assert_same(ctx.find_path_out(tin[:n], tout[:n], amt[:n], H), ok, "after the refusals:")
    # the exact-input entry still answers, and the latest call is the one the options describe
    ctx.find_path(tin[:n], tout[:n], amt[:n], 1)
    assert ctx.get_option("find_launches") == 3 * 1 + 3


def test_a_context_without_pools_finds_nothing_and_a_parent_is_unsupported(world):
    batches = world[0]
    empty = cr.Context(4)
    try:
        cost, n_hops, seg, row, ci, co, status = empty.find_path_out([0, 1], [1, 1], [1.0, 0.0], 2)
        assert status.tolist() == [FOUND_NONE] * 2 and np.isposinf(cost[0]) and bits(cost[1:]).tolist() == [0] and np.all(n_hops == 0)
        assert np.all(seg == -1) and np.all(row == -1) and np.all(ci == -1) and np.all(co == -1)
    finally:
        empty.close()
    multi = cr.Context(NT, [0, 0])
    try:
        for b in batches[:2]:
            _upload(multi, b)
        with pytest.raises(NotImplementedError, match="cfmm_find_path_out is not available on a multi-device context"):
            multi.find_path_out(0, 1, 1.0)
    finally:
        multi.close()


# ---- the router-level call ------------------------------------------------------------------------------------------------------
def test_router_level_find_quote_execute():
    batches = market(seed=61)
    r = cr.Router(cr.LinearNonnegative(np.ones(NT)), batches, NT)
    try:
        tin, tout, amt = make_queries(batches, NT, 65, seed=13)
        cost, pools, tokens, status = cr.find_path_out(r, tin + 1, tout + 1, amt, max_hops=3)
        f = [q for q in range(65) if status[q] == FOUND]
        assert len(f) > 20
        same_bits(cr.quote_path_out(r, [pools[q] for q in f], [tokens[q] for q in f], amt[f]), cost[f], "cr.quote_path_out on cr.find_path_out")
        for q in range(65):
            if status[q] == FOUND_NONE:
                assert pools[q] == [] and tokens[q] == [] and (cost[q] == 0.0 if amt[q] == 0.0 else np.isposinf(cost[q]))
            else:
                assert tokens[q][0] == tin[q] + 1 and tokens[q][-1] == tout[q] + 1 and len(tokens[q]) == len(pools[q]) + 1
        q = f[0]
        paid, st = cr.swap_path_out_(r, [pools[q]], [tokens[q]], amt[q], max_in=cost[q])
        assert st[0] in (SWAP_APPLIED, SWAP_REFUSED)
        if st[0] == SWAP_APPLIED:
            assert bits(paid)[0] == bits(cost[q:q + 1])[0]
            again, _, _, _ = cr.find_path_out(r, tin[q] + 1, tout[q] + 1, amt[q], max_hops=3)
            assert again[0] > cost[q]
    finally:
        r.close()
