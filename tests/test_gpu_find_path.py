"""cfmm_find_path on the device: the best swap walk of at most max_hops hops between two tokens, found by layers -- one launch
per layer with one lane per pool -- and walked back.  The pin of the whole feature is bit-equality with the layered search on
the host (tests/find_path_ref.py) driven by ctx.quote: amount, n_hops, the four hop arrays and the status.  Around it:
cfmm_quote_path on the result, the tie-break, brute force over every walk of a small market, chunking, live state, the three
statuses, errors."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import FOUND, FOUND_NONE, FOUND_REPEATS, KIND_UNIV3, PATH_APPLIED, ptr
from cfmmrouter_amd.cfmms import _upload
from find_path_ref import brute_force_walks, find_path_ref, layers
from test_gpu_pool_update import batch_with
from test_gpu_quote import N
from test_gpu_quote_path import M, SEGMENTS, bits, market, same_bits, scale_in

pytestmark = pytest.mark.gpu

NT = N + 1              # one token more than the pools use: token NT - 1 is held by no pool
COUNT = 1025
HOPS = (1, 3, 8)
COUNTS = (1, 65, 1025)


def tables(batches):
    return [np.ascontiguousarray(b.Ai - 1, dtype=np.int64) for b in batches]


def token_scale(batches, n_tokens):
    """per token the median size of an amount tendered to it (scale_in over the pools that hold it); 1.0 for a token no pool holds"""
    per = [[] for _ in range(n_tokens)]
    for b in batches:
        s = scale_in(b)
        for c in range(b.Ai.shape[1]):
            for t, x in zip((b.Ai[:, c] - 1).tolist(), s[:, c].tolist()):
                per[t].append(x)
    return np.array([np.median(p) if p else 1.0 for p in per])


def make_queries(batches, n_tokens, count, seed=3):
    """token_in = q mod n_tokens (65 queries cover every token, the unheld one included); token_out walks through every token
    at another stride, equals token_in in every 13th query and is the unheld token in every 65th; amounts 10^u of the token's
    scale, u uniform in [-6, 0.5], every 17th exactly 0.0"""
    q = np.arange(count)
    tin = (q % n_tokens).astype(np.int32)
    tout = ((7 * q + q // n_tokens + 1) % n_tokens).astype(np.int32)
    tout[q % 13 == 5] = tin[q % 13 == 5]
    tout[q % 65 == 33] = n_tokens - 1
    amt = token_scale(batches, n_tokens)[tin] * 10.0 ** (-6.0 + 6.5 * synth.uniform(seed, 8, count))
    amt[q % 17 == 11] = 0.0
    return tin, tout, amt


def assert_same(got, want, what=""):
    """(amount_out, n_hops, seg, row, ci, co, status) bit for bit"""
    same_bits(got[0], want[0], what + " amount_out")
    for k, name in ((1, "n_hops"), (2, "hop_seg"), (3, "hop_row"), (4, "hop_coin_in"), (5, "hop_coin_out"), (6, "status")):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {name}")


@pytest.fixture(scope="module")
def world():
    """the eight-segment market on one context of NT tokens, the queries, and the reference's layers for 8 hops, computed once
    and left unchanged (layer h is the same whatever max_hops is)"""
    batches = market()
    be = cr.DeviceBackend(NT, batches)
    tok = tables(batches)
    tin, tout, amt = make_queries(batches, NT, COUNT)
    best = layers(tok, be.ctx.quote, NT, tin, amt, max(HOPS))
    yield batches, be.ctx, tok, (tin, tout, amt), best
    be.close()


# ---- 1. the pin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("max_hops", HOPS)
def test_find_path_is_the_layered_search_bit_for_bit(world, max_hops, count):
    batches, ctx, tok, (tin, tout, amt), best = world
    sl = slice(0, count)
    want = find_path_ref(tok, ctx.quote, NT, tin[sl], tout[sl], amt[sl], max_hops, best=best[:, sl])
    got = ctx.find_path(tin[sl], tout[sl], amt[sl], max_hops)
    assert got[2].shape == got[3].shape == got[4].shape == got[5].shape == (count, max_hops)
    assert_same(got, want, f"max_hops {max_hops}, count {count}:")
    out, n_hops, seg, row, ci, co, status = got
    none = status == FOUND_NONE
    assert np.all(out[none] == 0.0) and np.all(n_hops[none] == 0) and np.all(seg[none] == -1) and np.all(row[none] == -1)
    assert np.all((amt[sl] == 0.0) <= none) and np.all((tout[sl] == NT - 1) <= none) and np.all((tin[sl] == NT - 1) <= none)
    unused = np.arange(max_hops)[None, :] >= n_hops[:, None]
    assert np.all(seg[unused] == -1) and np.all(row[unused] == -1) and np.all(ci[unused] == -1) and np.all(co[unused] == -1)
    print(f"find_path max_hops {max_hops}, count {count}: hops histogram {np.bincount(n_hops, minlength=max_hops + 1).tolist()}, "
          f"statuses {np.bincount(status, minlength=3).tolist()}")
    if count == COUNT:
        assert np.sum(status != FOUND_NONE) > count // 2                   # the comparison is not one of empty answers
        if max_hops > 1:
            assert np.any(n_hops > 1) and np.any((tin[sl] == tout[sl]) & (status != FOUND_NONE))   # cycles are found


def test_both_layer_kernels_give_the_same_bits(world):
    """option "find_lds": the layers folded through a per-block LDS copy (default where n_tokens lets one fit) or straight into
    global memory (what a market of more than 4096 tokens gets) -- integer maxima either way"""
    batches, ctx, tok, (tin, tout, amt), best = world
    assert ctx.get_option("find_lds") == 1
    ctx.set_option("find_lds", 0)
    try:
        for max_hops in (3, 8):
            got = ctx.find_path(tin, tout, amt, max_hops)
            assert_same(got, find_path_ref(tok, ctx.quote, NT, tin, tout, amt, max_hops, best=best), f"find_lds 0, max_hops {max_hops}:")
    finally:
        ctx.set_option("find_lds", 1)


# ---- 2. cfmm_quote_path on the result ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_hops", (3, 8))
def test_quote_path_on_the_result_answers_the_same_bits(world, max_hops):
    batches, ctx, tok, (tin, tout, amt), best = world
    out, n_hops, seg, row, ci, co, status = ctx.find_path(tin, tout, amt, max_hops)
    f = np.flatnonzero(status != FOUND_NONE)
    again, hops = ctx.quote_path(n_hops[f], seg[f], row[f], ci[f], co[f], amt[f], hops=True)
    same_bits(again, out[f], "quote_path on the found hops")
    for j, q in enumerate(f):                                              # hop k leaves the layer value of the token it reaches
        for k in range(n_hops[q]):
            t = tok[seg[q, k]][row[q, k], co[q, k]]
            assert bits(hops[k, j]) == bits(best[k + 1, q, t]), (q, k)
        assert tok[seg[q, 0]][row[q, 0], ci[q, 0]] == tin[q] and t == tout[q]
        for k in range(1, n_hops[q]):                                      # token-continuous
            assert tok[seg[q, k]][row[q, k], ci[q, k]] == tok[seg[q, k - 1]][row[q, k - 1], co[q, k - 1]]


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------
TWIN = 5                # the segment that gets twins: the 8-coin weighted pools, which most best paths of this market run through


def test_exact_ties_go_to_the_smaller_segment_row_and_coins():
    """segment TWIN's pools once more in its own later rows AND as a last segment: every edge of it has two exact twins, and
    the one in the smallest (segment, row) must be the hop"""
    base = market()
    dup = base[:TWIN] + [cr.PoolBatch.concat([base[TWIN], base[TWIN]])] + base[TWIN + 1:] + [base[TWIN]]
    be = cr.DeviceBackend(NT, dup)
    try:
        tok = tables(dup)
        tin, tout, amt = make_queries(base, NT, 195)
        got = be.ctx.find_path(tin, tout, amt, 3)
        assert_same(got, find_path_ref(tok, be.ctx.quote, NT, tin, tout, amt, 3), "ties:")
        _, n_hops, seg, row, _, _, status = got
        used = np.arange(3)[None, :] < n_hops[:, None]
        print(f"ties: {int(np.sum(used & (seg == TWIN)))} hops of {int(np.sum(used))} run through segment {TWIN}")
        assert np.sum(used & (seg == TWIN)) > 50                           # the segment is on many paths ...
        assert not np.any(used & (seg == len(dup) - 1)) and not np.any(used & (seg == TWIN) & (row >= M))   # ... its twins on none
        # the same queries on the market without the twins: the same amounts through the same pools
        be0 = cr.DeviceBackend(NT, base)
        try:
            assert_same(be0.ctx.find_path(tin, tout, amt, 3), got, "without the twins:")
        finally:
            be0.close()
    finally:
        be.close()


# ---- 4. brute force -------------------------------------------------------------------------------------------------------------
SMALL_M, SMALL_N = 5, 6


def small_market(seed=31):
    """5 pools per segment of the same eight segments on 6 tokens (the weighted segment of 8 coins becomes one of 5)"""
    out = []
    for s, (kind, nc) in enumerate(SEGMENTS):
        nc = min(nc, SMALL_N - 1)
        if kind == "product":
            b = synth.product_pools(SMALL_M, SMALL_N, seed=seed + s)
        elif kind == "geomean":
            b = synth.geomean_pools(SMALL_M, SMALL_N, seed=seed + s)
        elif kind == "solidly":
            b = synth.solidly_pools(SMALL_M, SMALL_N, seed=seed + s, wide=True)
        elif kind == "univ3":
            b = synth.univ3_ragged_pools(SMALL_M, SMALL_N, min_ticks=1, max_ticks=16, seed=seed + s)
        elif kind == "weighted":
            b = synth.weighted_pools(SMALL_M, SMALL_N, nc, seed=seed + s)
        else:
            b = synth.curve_pools(SMALL_M, SMALL_N, nc, seed=seed + s)
        out.append(b)
    return out


def test_brute_force_over_every_walk_of_a_small_market():
    """Every walk of 1 .. 3 hops between the query's tokens, priced by ONE ctx.quote_path call.  The found amount may fall
    short of the enumeration's maximum only where rounding breaks a quote's monotonicity.  The precise tests hold one quote to
    |out - out*| <= K u (R_o + out* + cond) with K <= K_CAP (tests/quote_precise_ref.py bound(), K_of()); the bound here is
    max_hops of those with K = K_CAP, R_o = the largest reserve of token_out any last hop can draw on, out* = the maximum
    itself, and cond left out -- which only makes it tighter.  Largest shortfall seen: printed (DESIGN records it; 0 on
    this market)."""
    batches = small_market()
    be = cr.DeviceBackend(SMALL_N, batches)
    try:
        tok = tables(batches)
        scale = token_scale(batches, SMALL_N)
        # every token as source and as destination, to its neighbour and back to itself (the best cycle), small and large amounts
        queries = [(a, b, scale[a] * 10.0 ** (-4.0 if (a + b) % 2 else -1.0)) for a in range(SMALL_N) for b in ((a + 1) % SMALL_N, a)]
        tin, tout, amt = (np.array(x) for x in zip(*queries))
        H = 3
        out, n_hops, seg, row, ci, co, status = be.ctx.find_path(tin, tout, amt, H)
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
        priced = be.ctx.quote_path(wn, cols[0].astype(np.int32), cols[1], cols[2].astype(np.int32), cols[3].astype(np.int32), amt[owner])
        priced = np.where(np.isfinite(priced) & (priced > 0), priced, 0.0)
        top = np.zeros(len(queries))
        np.maximum.at(top, owner, priced)
        assert np.all(status != FOUND_NONE) and np.all(top > 0)            # every query is answered: none is skipped
        Ro = np.zeros(SMALL_N)
        for b in batches:
            np.maximum.at(Ro, (b.Ai - 1).reshape(-1), scale_in(b).reshape(-1))
        allowed = H * P.bound(P.K_CAP, Ro[tout], top, 0.0)
        short = top - out
        print(f"brute force: largest shortfall max - found = {short.max():.3e} (relative {np.max(short / top):.3e}), "
              f"smallest allowance {allowed.min():.3e}; found above the enumeration nowhere: {bool(np.all(out <= top))}")
        assert np.all(out <= top)                                          # the found walk is one of the enumeration
        assert np.all(short <= allowed)
    finally:
        be.close()


# ---- 5. chunking ----------------------------------------------------------------------------------------------------------------
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
        tin, tout, amt = make_queries(small, N, count, seed=5)
        tin[::7], tout[3::11] = n_big - 1, n_big - 1                       # the moved token, as source and as destination
        whole = be.ctx.find_path(tin, tout, amt, H)
        launches = be.ctx.get_option("find_launches")
        assert launches == 3 * (3 * H + 3)
        singles = [be.ctx.find_path(tin[q:q + 1], tout[q:q + 1], amt[q:q + 1], H) for q in range(count)]
        assert_same(whole, tuple(np.concatenate([s[k] for s in singles]) for k in range(7)), "chunked vs one by one:")
        assert np.sum(whole[6] != FOUND_NONE) > count // 2
        # ... and the reference, on a few of them (its layers are [9, queries, 65536] doubles)
        f = np.arange(0, count, 17)
        want = find_path_ref(tables(big), be.ctx.quote, n_big, tin[f], tout[f], amt[f], H)
        assert_same(tuple(a[f] for a in whole), want, "large-market mode vs the reference:")
    finally:
        be.close()


# ---- 6. live state --------------------------------------------------------------------------------------------------------------
def test_find_path_follows_the_market_and_changes_nothing():
    batches = market(seed=41)
    other = market(seed=42)
    be = cr.DeviceBackend(NT, batches)
    try:
        ctx = be.ctx
        tok = tables(batches)
        tin, tout, amt = make_queries(batches, NT, 130, seed=9)
        first = ctx.find_path(tin, tout, amt, 3)
        assert_same(first, find_path_ref(tok, ctx.quote, NT, tin, tout, amt, 3), "before:")
        # execute the found paths' hops (the first visit of every pool), and rewrite a hundred reserves
        out, n_hops, seg, row, ci, co, status = first
        seen = set()
        for q in np.flatnonzero(status == FOUND)[:40]:
            x = amt[q]
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
        a = ctx.find_path(tin, tout, amt, 3)
        b = ctx.find_path(tin, tout, amt, 3)
        assert_same(a, b, "twice in a row:")
        assert_same(a, find_path_ref(tok, ctx.quote, NT, tin, tout, amt, 3), "after swaps and set_reserves:")
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


# ---- 7. statuses ----------------------------------------------------------------------------------------------------------------
def test_a_walk_that_re_enters_a_pool_is_found_and_flagged():
    """A -> B -> A -> B: pool 0 trades A and B one for one and is deep; pool 1 gives four A for a B.  The best walk of 3 hops
    from A to B goes through pool 0, back through pool 1, and through pool 0 AGAIN."""
    pools = cr.ProductTwoCoin.batch(np.array([[1e9, 1e9], [4e6, 1e6]]), np.array([0.997, 0.997]), np.array([[1, 2], [1, 2]]))
    be = cr.DeviceBackend(3, [pools])
    try:
        ctx = be.ctx
        out, n_hops, seg, row, ci, co, status = ctx.find_path([0, 0], [1, 1], [1000.0, 1000.0], [3][0])
        assert status.tolist() == [FOUND_REPEATS] * 2 and n_hops.tolist() == [3, 3]
        assert row[0].tolist() == [0, 1, 0] and ci[0].tolist() == [0, 1, 0] and co[0].tolist() == [1, 0, 1]
        assert out[0] > 3000.0
        same_bits(ctx.quote_path(n_hops, seg, row, ci, co, [1000.0, 1000.0]), out, "the amounts are quote_path's")
        with pytest.raises(cr.ArgumentError, match="cfmm_swap_path: path 0"):
            ctx.swap_path(n_hops, seg, row, ci, co, [1000.0, 1000.0])
        one = ctx.find_path([0], [1], [1000.0], 1)                         # within one hop: the deep pool, no repeat
        assert one[6].tolist() == [FOUND] and one[1].tolist() == [1] and one[3][0].tolist() == [0] and 990.0 < one[0][0] < 997.0
        two = ctx.find_path([0], [1], [1000.0], 2)                         # two hops cannot end at B with more: the same answer
        assert_same(tuple(a[:, :1] if a.ndim == 2 else a for a in two), one, "max_hops 2:")
        none = ctx.find_path([2, 0, 0], [0, 2, 1], [1.0, 1.0, 0.0], 3)     # token 2 is held by no pool; amount 0
        assert none[6].tolist() == [FOUND_NONE] * 3 and np.all(none[0] == 0.0) and np.all(none[1] == 0) and np.all(none[3] == -1)
    finally:
        be.close()


def test_a_found_path_executes_with_its_own_amount_as_the_limit(world):
    batches = market(seed=51)
    be = cr.DeviceBackend(NT, batches)
    try:
        tin, tout, amt = make_queries(batches, NT, 65, seed=11)
        out, n_hops, seg, row, ci, co, status = be.ctx.find_path(tin, tout, amt, 3)
        f = np.flatnonzero(status == FOUND)
        assert f.size > 20
        q = f[np.argmax(n_hops[f])]                                        # one path (a batch would move shared pools in between)
        assert n_hops[q] >= 2
        got, st = be.ctx.swap_path(n_hops[q:q + 1], seg[q:q + 1], row[q:q + 1], ci[q:q + 1], co[q:q + 1], amt[q:q + 1], min_out=out[q:q + 1])
        assert st.tolist() == [PATH_APPLIED]
        same_bits(got, out[q:q + 1], "swap_path gives what find_path promised")
        after = be.ctx.find_path(tin[q:q + 1], tout[q:q + 1], amt[q:q + 1], 3)
        assert after[0][0] < out[q]                                        # the same query afterwards finds a worse price
    finally:
        be.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_query_and_launch_nothing(world):
    batches, ctx, tok, (tin, tout, amt), best = world
    L = cr.lib()
    n, H = 16, 3
    ok = ctx.find_path(tin[:n], tout[:n], amt[:n], H)
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
        rc = L.cfmm_find_path(ctx._h, count, max_hops, *args)
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_find_path:") and match in msg, (rc, msg)
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
        refused("query 7: amount_in must be finite and >= 0", amt=edit(amt[:n], 7, bad))
    refused("query 2: token_in", tin=edit(tin[:n], 2, NT), amt=edit(amt[:n], 9, -1.0))   # the first bad query is named
    refused("max_hops must be 1 .. 8 (got 0)", max_hops=0)
    refused("max_hops must be 1 .. 8 (got 9)", max_hops=9)
    refused("count must be >= 0", count=-1)
    for k in range(10):
        refused("null query array", null=k)
    # through the wrapper the refusals are ArgumentErrors
    with pytest.raises(cr.ArgumentError, match="query 1: token_out"):
        ctx.find_path([0, 1], [1, NT], 1.0, 3)
    with pytest.raises(cr.ArgumentError, match="query 0: amount_in"):
        ctx.find_path(0, 1, np.nan)
    with pytest.raises(cr.ArgumentError, match="max_hops"):
        ctx.find_path(0, 1, 1.0, max_hops=9)
    # count == 0 is a no-op, NULL arrays accepted
    ctx._check(L.cfmm_find_path(ctx._h, 0, 3, None, None, None, None, None, None, None, None, None, None))
    assert ctx.find_path([], [], [], 3)[0].size == 0
    assert_same(ctx.find_path(tin[:n], tout[:n], amt[:n], H), ok, "after the refusals:")


def test_a_context_without_pools_finds_nothing_and_a_parent_is_unsupported(world):
    batches = world[0]
    empty = cr.Context(4)
    try:
        out, n_hops, seg, row, ci, co, status = empty.find_path([0, 1], [1, 1], [1.0, 2.0], 2)
        assert status.tolist() == [FOUND_NONE] * 2 and np.all(out == 0.0) and np.all(n_hops == 0)
        assert np.all(seg == -1) and np.all(row == -1) and np.all(ci == -1) and np.all(co == -1)
    finally:
        empty.close()
    multi = cr.Context(NT, [0, 0])
    try:
        for b in batches[:2]:
            _upload(multi, b)
        with pytest.raises(NotImplementedError, match="cfmm_find_path is not available on a multi-device context"):
            multi.find_path(0, 1, 1.0)
    finally:
        multi.close()


# ---- the router-level call ------------------------------------------------------------------------------------------------------
def test_router_level_find_quote_execute():
    batches = market(seed=61)
    r = cr.Router(cr.LinearNonnegative(np.ones(NT)), batches, NT)
    try:
        tin, tout, amt = make_queries(batches, NT, 65, seed=13)
        out, pools, tokens, status = cr.find_path(r, tin + 1, tout + 1, amt, max_hops=3)
        f = [q for q in range(65) if status[q] == FOUND]
        assert len(f) > 20
        same_bits(cr.quote_path(r, [pools[q] for q in f], [tokens[q] for q in f], amt[f]), out[f], "cr.quote_path on cr.find_path")
        for q in range(65):
            if status[q] == FOUND_NONE:
                assert pools[q] == [] and tokens[q] == [] and out[q] == 0.0
            else:
                assert tokens[q][0] == tin[q] + 1 and tokens[q][-1] == tout[q] + 1 and len(tokens[q]) == len(pools[q]) + 1
        q = f[0]
        got, st = cr.swap_path_(r, [pools[q]], [tokens[q]], amt[q], min_out=out[q])
        assert st.tolist() == [PATH_APPLIED] and bits(got)[0] == bits(out[q:q + 1])[0]
        again, _, _, _ = cr.find_path(r, tin[q] + 1, tout[q] + 1, amt[q], max_hops=3)
        assert again[0] < out[q]
    finally:
        r.close()
