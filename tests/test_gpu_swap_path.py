"""cfmm_swap_path on the device: paths of up to eight pools of eight segments of six kinds EXECUTED in query order, each all or
nothing.  There is no tolerance anywhere: every comparison is bit equality against calls the project already has -- the
amounts against cfmm_quote_path on the market as it stands, the final state against chaining cfmm_swap hop by hop, path by
path, on a twin context.  Around the pin: shared pools (many waves, with and without UniV3), a refused hop in the middle of a
path, the limit, zero amounts and NULL outputs, the state protocol, a multi-device parent, bad input, the router-level call.
Segments are small: every test runs in seconds.

The inputs of the three equality tests (one wave, shared pools, router) must make no path refuse and let at most 5 % of the
paths end in exactly 0.0 (a comparison of zeros shows nothing); both are asserted where the paths run.  What decides both is
not the first amount (10^-4 .. 10^-2 of the tendered reserve; 10^-5 .. 10^-3.5 where pools are shared) but the amounts the
later hops inherit: a pool of one segment can hand a pool of the next fifty times its reserve, which empties a reserve pool
(refused) or exhausts a UniV3 direction, after which every swap of that direction answers 0.0.  The market keeps synth's UniV3
ladders as they are (test_gpu_quote_path's zeroes a tenth of the ticks).  The seeds were fixed on the CPU with reference_walk:
the walk restated with the numpy forms of tests/quote_precise_ref.py, the reserve tests and the UniV3 landing price of
csrc/swap_pool.h, on the market as it stands (one wave) or moved path by path (shared pools).  SEED 39 refuses no one-wave
path and lets 3 of 257 end in 0.0 (seed 31 refused one); SHARED_SEED 62 refuses none of the 300 and lets 0 / 4 end in 0.0
(without / with UniV3; most seeds exceed the cap of 15 with UniV3 at the larger amounts).  The tests assert both conditions
on the restatement before the device is asked, and on the device's own answers after."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import quote_precise_ref as P
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import (KIND_CURVE, KIND_GEOMEAN, KIND_PRODUCT, KIND_SOLIDLY, KIND_UNIV3, KIND_WEIGHTED, OBJ_LINEAR_NONNEGATIVE,
                                 PATH_APPLIED, PATH_BELOW_LIMIT, PATH_REFUSED, ptr)
from cfmmrouter_amd.cfmms import _upload
from test_gpu_pool_update import assert_same, batch_with
from test_gpu_quote import N, pools
from test_gpu_quote_path import H, M, SEGMENTS, bits, same_bits, scale_in, used_slots
from test_gpu_swap import V, assert_equals_fresh, backend, exact_ladder, state, with_state

pytestmark = pytest.mark.gpu

SEED = 39                 # the one-wave market and paths
SHARED_SEED = 62          # the shared-pool market and paths
NSEG = len(SEGMENTS)


def market(m=M, seed=SEED, univ3=True):
    """test_gpu_quote_path's eight segments of six kinds, m pools each, the UniV3 ladders (1..16 ticks) as synth makes them;
    univ3=False: a second Product segment in UniV3's place"""
    out = []
    for s, (kind, nc) in enumerate(SEGMENTS):
        if kind == "univ3":
            out.append(synth.univ3_ragged_pools(m, N, min_ticks=1, max_ticks=16, seed=seed + s) if univ3 else pools("product", m, seed=seed + 50))
        else:
            out.append(pools(kind, m, seed=seed + s, n_coins=nc))
    return out


def coins_for(batches, seg, p, k):
    ci, co = np.zeros(seg.shape, dtype=np.int32), np.zeros(seg.shape, dtype=np.int32)
    for s, b in enumerate(batches):
        nc = b.Ai.shape[1]
        pairs = np.array([(i, j) for i in range(nc) for j in range(nc) if i != j], dtype=np.int32)
        at = seg == s
        pick = (p[at] + k[at]) % len(pairs)
        ci[at], co[at] = pairs[pick, 0], pairs[pick, 1]
    return ci, co


def make_paths(batches, count, rows, seed=SEED, lo=-4.0, hi=-2.0):
    """n_hops[p] = 1 + p % 8; hop k of path p in segment (p + 3k) % 8, so a path never visits a segment twice; rows[s][p] is its
    row there; coins cycling through every ordered pair; the first amount R_i·10^u, u uniform in [lo, hi]"""
    p, k = np.meshgrid(np.arange(count), np.arange(H), indexing="ij")
    n_hops = (1 + np.arange(count) % H).astype(np.int32)
    seg = ((p + 3 * k) % NSEG).astype(np.int32)
    row = np.zeros((count, H), dtype=np.int64)
    for s in range(NSEG):
        row[seg == s] = rows[s][p[seg == s]]
    ci, co = coins_for(batches, seg, p, k)
    u = lo + (hi - lo) * synth.uniform(seed + 300, 4, count)
    first = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(count)])
    return n_hops, seg, row, ci, co, first * 10.0 ** u


def explicit(paths, amounts):
    """paths as lists of (segment, row, coin_in, coin_out) -> the six path arguments"""
    count, Hn = len(paths), max(len(p) for p in paths)
    n_hops = np.array([len(p) for p in paths], dtype=np.int32)
    cols = [np.zeros((count, Hn), dtype=np.int64 if j == 1 else np.int32) for j in range(4)]
    for p, path in enumerate(paths):
        for k, hop in enumerate(path):
            for j in range(4):
                cols[j][p, k] = hop[j]
    return (n_hops, *cols, np.asarray(amounts, dtype=np.float64))


def sliced(paths, sl):
    return tuple(a[sl] for a in paths)


def states(ctx, batches):
    return [state(ctx, b, s) for s, b in enumerate(batches)]


def same_states(got, want, what=""):
    for s, (x, y) in enumerate(zip(got, want)):
        same_bits(x, y, f"{what} segment {s}")


def entering(paths, hops):
    """[H, count] the amount entering each hop: the given amount, then what left the hop before"""
    return np.vstack([paths[5][None, :], hops[:-1]])


def wave_count(paths):
    """the planner's rule (csrc/swap_path_waves.h), restated: a path runs in the first wave in which all its pools are free"""
    n_hops, seg, row = paths[:3]
    free, waves = {}, 0
    for p in range(len(n_hops)):
        named = [(int(seg[p, k]), int(row[p, k])) for k in range(n_hops[p])]
        w = max([free.get(x, 0) for x in named])
        for x in named:
            free[x] = w + 1
        waves = max(waves, w + 1)
    return waves


def univ3_landing_price(cp, prep, g, cin, a):
    """csrc/swap_pool.h swap_univ3_price on the records of quote_precise_ref.univ3_prepare"""
    cur, up, lo = prep
    d = g * a
    if a == 0.0:
        return cp
    k = cur[0]
    s_in, dmax = (cur[1], cur[3]) if cin == 0 else (cur[2], cur[4])
    if k != 0.0 and d < dmax:
        kk, ss, dt = k, s_in, d
    else:
        lst = up if cin == 0 else lo
        cnt = len(lst) - 1
        lo_i, hi_i = 0, cnt + 1
        while hi_i - lo_i > 1:
            mid = lo_i + ((hi_i - lo_i) >> 1)
            if lst[mid][5] <= d:
                lo_i = mid
            else:
                hi_i = mid
        if lo_i == cnt:
            if cnt > 0:
                kk, ss, dt = lst[cnt - 1][0], lst[cnt - 1][1], lst[cnt - 1][2]
            elif k != 0.0:
                kk, ss, dt = k, s_in, dmax
            else:
                return cp
        else:
            e = lst[lo_i]
            kk, ss, dt = e[0], e[1], min(max(d - e[5], 0.0), e[2])
    sp = ss + dt
    return kk / (sp * sp) if cin == 0 else (sp * sp) / kk


def reference_walk(batches, paths, advance=False):
    """The paths walked with the numpy restatements of csrc/quote_pool.h -> (answers, refused [count]).  A hop is refused by
    the reserve tests of csrc/swap_pool.h restated here (new reserves finite and > 0, Solidly inside [2^-150, 2^150]) and its
    path then answers NaN.  advance=False: every path on the market as it stands; advance=True: in query order, every path
    that is not refused moves its pools -- the reserve kinds to R_in + γ·a, R_out − out, UniV3 to the landing price clamped to
    the first tick's upper price and prepared again."""
    n_hops, seg, row, ci, co, amt = paths
    R = [None if b.kind == KIND_UNIV3 else b.R.copy() for b in batches]
    prep, cp = {}, {}
    out, refused = np.array(amt, dtype=np.float64), np.zeros(len(n_hops), dtype=bool)
    window = lambda v: 2.0 ** -150 <= v < 2.0 ** 151
    for p in range(len(n_hops)):
        x = np.float64(amt[p])
        moves = []
        for k in range(n_hops[p]):
            s, r, i, o = seg[p, k], row[p, k], ci[p, k], co[p, k]
            b = batches[s]
            g = np.float64(b.γ[r])
            if b.kind == KIND_UNIV3:
                a_, b_ = b.tick_off[r], b.tick_off[r + 1]
                if r not in prep:
                    cp[r] = float(b.current_price[r])
                    prep[r] = P.univ3_prepare(cp[r], b.lower_ticks[a_:b_], b.liquidity[a_:b_])
                price = univ3_landing_price(cp[r], prep[r], float(g), int(i), float(x))
                if not 0 < price < np.inf:
                    refused[p] = True
                    break
                moves.append((s, r, None, None, min(price, float(b.lower_ticks[a_])), None))
                x = np.float64(P.q_univ3(prep[r], float(g), int(i), float(x)))
                continue
            Ri, Ro = R[s][r, i], R[s][r, o]
            if b.kind == KIND_PRODUCT:
                y = P.q_product(Ri, Ro, g, x)
            elif b.kind == KIND_SOLIDLY:
                y = np.float64(P.q_solidly(Ri, Ro, g, x))
            elif b.kind in (KIND_GEOMEAN, KIND_WEIGHTED):
                y = P.q_weighted(Ri, Ro, b.w[r, i], b.w[r, o], g, x)
            else:
                assert b.kind == KIND_CURVE
                y = P.q_curve(Ri, Ro, P.sum_logs(R[s][r:r + 1])[0], b.α[r], np.log(b.β[r]), g, x)
            if x != 0.0:
                ni, no = Ri + g * x, Ro - y
                if not (0 < ni < np.inf and 0 < no < np.inf) or (b.kind == KIND_SOLIDLY and not (window(ni) and window(no))):
                    refused[p] = True
                    break
                moves.append((s, r, i, o, ni, no))
            x = y
        out[p] = np.nan if refused[p] else x
        if advance and not refused[p]:
            for s, r, i, o, ni, no in moves:
                if i is None:
                    b = batches[s]
                    cp[r] = ni
                    prep[r] = P.univ3_prepare(ni, b.lower_ticks[b.tick_off[r]:b.tick_off[r + 1]], b.liquidity[b.tick_off[r]:b.tick_off[r + 1]])
                else:
                    R[s][r, i], R[s][r, o] = ni, no
    return out, refused


def input_conditions(status, out, what):
    zero = int(np.sum(out == 0.0))
    print(f"{what}: {out.size} paths, {int(np.sum(status != PATH_APPLIED))} not applied, {zero} end in exactly 0.0 (cap {out.size // 20})")
    assert np.all(status == PATH_APPLIED), "an input condition of the test: no path may be refused"
    assert zero <= out.size // 20, "an input condition of the test: at most 5 % of the paths end in 0.0"
    assert np.all(np.isfinite(out)) and np.all(out >= 0)


# ---- 1. one wave ----------------------------------------------------------------------------------------------------------------
def test_one_wave_equals_the_quote_then_batched_swaps():
    """257 paths of 1..8 hops, path p on row π_s(p) of segment s: every pool of the batch is distinct, so the call is one
    launch, its amounts are quote_path's on the market as it stands and its final state is that of one batched ctx.swap per
    (hop level, segment)"""
    batches = market()
    rows = [np.argsort(synth.uniform(SEED + 400 + s, 6, M)).astype(np.int64) for s in range(NSEG)]
    paths = make_paths(batches, M, rows)
    n_hops, seg, row, ci, co, amt = paths
    ref, ref_refused = reference_walk(batches, paths)
    print(f"numpy restatement: {int(np.sum(ref_refused))} of {M} paths refused, {int(np.sum(ref == 0.0))} end in exactly 0.0")
    assert not np.any(ref_refused) and np.all(np.isfinite(ref)) and np.all(ref >= 0) and np.sum(ref == 0.0) <= M // 20
    assert wave_count(paths) == 1
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        out, status, hops = ctx.swap_path(*paths, hops=True)
        input_conditions(status, out, "one wave")
        assert ctx.get_option("swap_refused") == 0 and ctx.get_option("swap_launches") == 1
        want, want_hops = twin.ctx.quote_path(*paths, hops=True)
        used = used_slots(n_hops)
        same_bits(out, want, "amount_out")
        same_bits(hops[used], want_hops[used], "hop_out")
        assert np.all(np.isnan(hops[~used]))
        live = ref > 0
        np.testing.assert_allclose(out[live], ref[live], rtol=1e-6)              # (the restatement describes these very paths)
        x_in = entering(paths, want_hops)
        for k in range(H):
            for s in range(NSEG):
                q = np.flatnonzero((n_hops > k) & (seg[:, k] == s))
                if q.size:
                    got = twin.ctx.swap(s, x_in[k, q], ci[q, k], co[q, k], row[q, k])
                    same_bits(got, want_hops[k, q], f"the twin's swaps of hop level {k}, segment {s}")
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
        moved = sum(int(np.sum(np.any(bits(a).reshape(M, -1) != bits(state_of).reshape(M, -1), axis=1)))
                    for a, state_of in zip(states(ctx, batches), [b.current_price if b.kind == KIND_UNIV3 else b.R for b in batches]))
        assert moved >= int(0.9 * np.sum(n_hops))                              # ... and it is a state that has moved
    finally:
        be.close()
        twin.close()


def test_after_paths_the_context_equals_a_fresh_upload():
    """Product, Solidly (no prepared constant depends on R) and UniV3 (re-prepared on the host): after a batch of paths every
    output of the context equals that of a context freshly uploaded at the state it reports"""
    batches = [pools("product", M, seed=41), pools("solidly", M, seed=42), synth.univ3_ragged_pools(M, N, min_ticks=1, max_ticks=16, seed=43)]
    p, k = np.meshgrid(np.arange(M), np.arange(3), indexing="ij")
    n_hops = (1 + np.arange(M) % 3).astype(np.int32)
    seg = ((p + k) % 3).astype(np.int32)
    row = ((p * 5 + 7 * seg) % M).astype(np.int64)                             # (5 is coprime to 257: distinct rows per segment)
    ci = ((p + k) % 2).astype(np.int32)
    amt = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(M)]) * 0.01
    be = backend(batches)
    try:
        out, status = be.ctx.swap_path(n_hops, seg, row, ci, 1 - ci, amt)
        input_conditions(status, out, "three segments")
        now = [with_state(b, state(be.ctx, b, s)) for s, b in enumerate(batches)]
        assert_equals_fresh(be, now)
    finally:
        be.close()


# ---- 2. shared pools, many waves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("univ3", (False, True), ids=("no_univ3", "univ3"))
def test_shared_pools_equal_single_swaps_in_query_order(univ3):
    """300 paths drawn uniformly over 32 rows per segment: most paths share a pool with an earlier one.  The twin replays the
    batch by single-query ctx.swap calls, path by path and hop by hop"""
    m, count = 32, 300
    batches = market(m=m, seed=SHARED_SEED, univ3=univ3)
    rows = [np.minimum((synth.uniform(SHARED_SEED + 500 + s, 7, count) * m).astype(np.int64), m - 1) for s in range(NSEG)]
    paths = make_paths(batches, count, rows, seed=SHARED_SEED, lo=-5.0, hi=-3.5)
    n_hops, seg, row, ci, co, amt = paths
    waves = wave_count(paths)
    assert waves > 10
    ref, ref_refused = reference_walk(batches, paths, advance=True)
    print(f"numpy restatement: {int(np.sum(ref_refused))} of {count} paths refused, {int(np.sum(ref == 0.0))} end in exactly 0.0")
    assert not np.any(ref_refused) and np.all(np.isfinite(ref)) and np.sum(ref == 0.0) <= count // 20
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        ctx.set_option("time_kernels", 1)
        out, status, hops = ctx.swap_path(*paths, hops=True)
        input_conditions(status, out, f"shared pools ({waves} waves)")
        assert ctx.get_option("swap_launches") == waves and ctx.get_option("swap_ns") > 0
        want, want_hops = np.zeros(count), np.full((H, count), np.nan)
        for p in range(count):
            if status[p] != PATH_APPLIED:
                continue
            x = amt[p:p + 1]
            for k in range(n_hops[p]):
                x = twin.ctx.swap(int(seg[p, k]), x, ci[p, k:k + 1], co[p, k:k + 1], row[p, k:k + 1])
                want_hops[k, p] = x[0]
            want[p] = x[0]
        used = used_slots(n_hops)
        same_bits(out, want, "amount_out")
        same_bits(hops[used], want_hops[used], "hop_out")
        assert np.all(np.isnan(hops[~used]))
        same_states(states(ctx, batches), states(twin.ctx, batches), "final state")
    finally:
        be.close()
        twin.close()


# ---- 3. all or nothing --------------------------------------------------------------------------------------------------------------
FUNNEL, TINY, THIN = 29, 30, 31       # rows of the doctored pools below


def doctored_market(m=32):
    """the market with three doctored pools: Product row FUNNEL gives about 4000 whatever comes in; Product row TINY holds so
    little that 4000 coming in makes x/(R + x) round to 1 (nothing would be left: refused); Solidly row THIN holds 2^-120 of
    its second coin, of which 4000 of the first leaves about 2^-156 -- positive, but outside [2^-150, 2^150] (refused)"""
    batches = market(m=m, seed=42)        # (UniV3 row 4 of this market answers both directions: reference_walk)
    R = batches[0].R.copy()
    R[FUNNEL] = [1e-6, 4000.0]
    R[TINY] = [1e-25, 1e-25]
    batches[0] = batch_with(batches[0], R=R)
    R = batches[2].R.copy()
    R[THIN] = [1.0, 2.0 ** -120]
    batches[2] = batch_with(batches[2], R=R)
    return batches


@pytest.mark.parametrize("case", ("product", "solidly", "univ3"))
def test_a_refused_hop_leaves_the_whole_path_unapplied(case):
    batches = doctored_market()
    u3 = 0.01 * scale_in(batches[3])[4, 0]
    g1 = 0.01 * batches[1].R[5, 0]
    first = (3, 4, 0, 1) if case == "univ3" else (1, 5, 0, 1)                  # hop 0: a UniV3 pool, or a GeometricMean pool
    last = (2, THIN, 0, 1) if case == "solidly" else (0, TINY, 0, 1)
    refused = [first, (0, FUNNEL, 0, 1), last]
    before = [(0, 1, 0, 1), (4, 2, 0, 2)]                                       # an ordinary path
    later = [first, (5, 3, 1, 6)]                                               # through hop 0's pool, after the refused path
    a0 = u3 if case == "univ3" else g1
    paths = explicit([before, refused, later, [(0, FUNNEL, 0, 1)]], [0.01 * batches[0].R[1, 0], a0, a0, 1.0])
    without = sliced(paths, [0, 2, 3])
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        q, qh = twin.ctx.quote_path(*sliced(paths, [1]), hops=True)            # the refused path, quoted on the untouched market
        if case == "solidly":
            left = batches[2].R[THIN, 1] - qh[2, 0]
            print(f"Solidly: the swap would leave 2^{np.log2(left):.1f}")
            assert 0 < left < 2.0 ** -150
        else:
            assert qh[2, 0] == batches[0].R[TINY, 1]                           # the whole reserve: nothing would be left
        out, status, hops = ctx.swap_path(*paths, hops=True)
        assert status.tolist() == [PATH_APPLIED, PATH_REFUSED, PATH_APPLIED, PATH_APPLIED] and ctx.get_option("swap_refused") == 1
        assert np.isnan(out[1]) and np.all(np.isfinite(out[[0, 2, 3]])) and np.all(out[[0, 2, 3]] > 0)
        same_bits(hops[:2, 1], qh[:2, 0], "hop_out before the refusing hop")
        assert np.all(hops[:2, 1] > 0) and np.isnan(hops[2, 1])
        # the market is the one in which the refused path never ran: amounts, hop amounts and every bit of every segment
        want, want_st, want_hops = twin.ctx.swap_path(*without, hops=True)
        assert np.all(want_st == PATH_APPLIED)
        same_bits(out[[0, 2, 3]], want, "the other paths")
        same_bits(hops[:, [0, 2, 3]][used_slots(without[0], 3)], want_hops[used_slots(without[0], 3)])
        same_states(states(ctx, batches), states(twin.ctx, batches))
        # ... in particular the later path moved hop 0's pool from where it stood, and the doctored pool is untouched
        s_last, r_last = last[0], last[1]
        same_bits(state(ctx, batches[s_last], s_last)[r_last], batches[s_last].R[r_last])
    finally:
        be.close()
        twin.close()


def test_a_refused_path_alone_changes_no_bit():
    batches = doctored_market()
    paths = explicit([[(3, 4, 1, 0), (1, 5, 0, 1), (0, FUNNEL, 0, 1), (0, TINY, 1, 0)]], [0.01 * scale_in(batches[3])[4, 1]])
    be = backend(batches)
    try:
        was = states(be.ctx, batches)
        out, status, hops = be.ctx.swap_path(*paths, hops=True)
        assert status.tolist() == [PATH_REFUSED] and np.isnan(out[0]) and np.all(hops[:3, 0] > 0) and np.isnan(hops[3, 0])
        same_states(states(be.ctx, batches), was)
        assert be.ctx.get_option("swap_refused") == 1
    finally:
        be.close()


# ---- 4. the limit -------------------------------------------------------------------------------------------------------------------
def test_the_limit_stops_the_second_execution_of_a_cycle():
    batches = market(m=32, seed=44)           # (reference_walk: the cycle below returns 44.6, then 25.8, then 17.1)
    cycle = [(0, 3, 0, 1), (3, 7, 1, 0), (6, 2, 1, 0), (1, 9, 0, 1)]
    a = 0.001 * batches[0].R[3, 0]
    one = explicit([cycle], [a])
    be, twin = backend(batches), backend(batches)
    try:
        r1, st1 = twin.ctx.swap_path(*one)
        q2 = twin.ctx.quote_path(*one)                                         # what a second execution would give
        assert st1.tolist() == [PATH_APPLIED] and 0 < q2[0] < r1[0]
        limit = 0.5 * (r1[0] + q2[0])
        assert q2[0] < limit < r1[0]
        out, status, hops = be.ctx.swap_path(*explicit([cycle, cycle], [a, a]), min_out=[limit, limit], hops=True)
        assert status.tolist() == [PATH_APPLIED, PATH_BELOW_LIMIT] and be.ctx.get_option("swap_refused") == 1
        same_bits(out, [r1[0], q2[0]])                                         # the second: the quote on the moved market
        same_bits(hops[3], out)
        same_states(states(be.ctx, batches), states(twin.ctx, batches), "only the first was executed")
        # a limit that is met exactly is met; a scalar serves every path
        out3, st3 = be.ctx.swap_path(*one, min_out=q2[0])
        assert st3.tolist() == [PATH_APPLIED] and bits(out3)[0] == bits(q2)[0]
    finally:
        be.close()
        twin.close()


# ---- 5. zero and edges ------------------------------------------------------------------------------------------------------------
def test_zero_amounts_empty_calls_null_outputs_and_one_hop():
    batches = market(m=32, seed=48)
    L = cr.lib()
    be, twin = backend(batches), backend(batches)
    try:
        ctx = be.ctx
        was = states(ctx, batches)
        every_kind = [(s, 3 + s, 0, 1) for s in range(NSEG)]
        out, status, hops = ctx.swap_path(*explicit([every_kind], [0.0]), min_out=0.0, hops=True)
        assert status.tolist() == [PATH_APPLIED] and out[0] == 0.0 and np.all(hops[:, 0] == 0.0)
        same_states(states(ctx, batches), was, "amount 0")
        # count == 0 invalidates nothing, through the wrapper and through the library with NULL arrays
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        e = np.zeros((0, H), dtype=np.int32)
        o, s = ctx.swap_path(np.zeros(0, dtype=np.int32), e, e, e, e, np.zeros(0))
        assert o.size == 0 and s.size == 0
        ctx._check(L.cfmm_swap_path(ctx._h, 0, H, None, None, None, None, None, None, None, None, None, None))
        assert_same([np.asarray(x) for x in be.trades()], trades)
        # hop_out, status and min_amount_out as NULL
        paths = explicit([[(0, 1, 0, 1), (4, 2, 0, 2)], [(6, 5, 1, 0)]], [0.01 * batches[0].R[1, 0], 0.01 * batches[6].R[5, 1]])
        n_hops, seg, row, ci, co, amt = paths
        c = lambda a: np.ascontiguousarray(a.T)
        got = np.full(2, 7.0)
        ctx._check(L.cfmm_swap_path(ctx._h, 2, 2, ptr(n_hops), ptr(c(seg)), ptr(c(row)), ptr(c(ci)), ptr(c(co)), ptr(amt), None, ptr(got), None, None))
        want, st = twin.ctx.swap_path(*paths)
        same_bits(got, want)
        same_states(states(ctx, batches), states(twin.ctx, batches), "NULL outputs")
        # a 1-hop path is cfmm_swap
        for s_, b in enumerate(batches):
            nc = b.Ai.shape[1]
            r = np.arange(8, 16, dtype=np.int64)
            ci1, co1 = (r % nc).astype(np.int32), ((r + 1) % nc).astype(np.int32)
            a1 = 0.01 * scale_in(b)[r, ci1]
            o1, st1 = ctx.swap_path(np.ones(8, dtype=np.int32), np.full(8, s_, dtype=np.int32), r, ci1, co1, a1)
            same_bits(o1, twin.ctx.swap(s_, a1, ci1, co1, r), f"one hop, segment {s_}")
            assert np.all(st1 == PATH_APPLIED)
        same_states(states(ctx, batches), states(twin.ctx, batches), "one hop")
    finally:
        be.close()
        twin.close()


# ---- 6. protocol --------------------------------------------------------------------------------------------------------------------
def three_segments(m=64):
    batches = [pools("product", m, seed=51), pools("solidly", m, seed=52), synth.univ3_ragged_pools(m, N, min_ticks=1, max_ticks=16, seed=53)]
    p, k = np.meshgrid(np.arange(m), np.arange(3), indexing="ij")
    seg = ((p + k) % 3).astype(np.int32)
    row = ((p * 3 + 5 * k) % m).astype(np.int64)                               # rows shared between paths: several waves
    ci = ((p + k) % 2).astype(np.int32)
    amt = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(m)]) * 0.005
    return batches, ((1 + np.arange(m) % 3).astype(np.int32), seg, row, ci, (1 - ci).astype(np.int32), amt)


def test_a_call_invalidates_trades_cancels_an_armed_route_and_the_next_sweep_sees_the_moved_market():
    batches, paths = three_segments()
    c = synth.linear_prices(N, seed=3)
    be = backend(batches)
    fresh = None
    try:
        ctx = be.ctx
        ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N))                 # pre-armed evaluations (option "armed" is on)
        be.find_arb(V)
        be.trades()
        out, status = ctx.swap_path(*paths)
        assert np.all(status == PATH_APPLIED)
        with pytest.raises(Exception, match="no materialised trades"):
            ctx.trades()
        now = [with_state(b, state(ctx, b, s)) for s, b in enumerate(batches)]
        assert_equals_fresh(be, now)                                           # eval, find_arb, trades, state
        fresh = backend(now)
        a, b_ = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N)), fresh.ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N))
        np.testing.assert_array_equal(a[0], b_[0])
        np.testing.assert_array_equal(a[1], b_[1])
    finally:
        be.close()
        if fresh is not None:
            fresh.close()


def test_large_market_mode_gives_the_same_bits():
    """two-coin segments only (large-market mode has no N-coin kernel), one token moved beyond the LDS limit"""
    small, paths = three_segments()
    big = [batch_with(b, Ai=np.where(b.Ai == 1, 8193, b.Ai)) for b in small]
    be_s, be_b = cr.DeviceBackend(N, small), cr.DeviceBackend(8193, big)
    try:
        a, sa, ah = be_s.ctx.swap_path(*paths, hops=True)
        b, sb, bh = be_b.ctx.swap_path(*paths, hops=True)
        same_bits(b, a)
        assert np.array_equal(sa, sb) and np.all(sa == PATH_APPLIED)
        same_bits(bh[used_slots(paths[0], 3)], ah[used_slots(paths[0], 3)])
        same_states(states(be_b.ctx, big), states(be_s.ctx, small))
    finally:
        be_s.close()
        be_b.close()


def test_a_multi_device_parent_is_unsupported_and_moves_nothing():
    batches, paths = three_segments()
    multi = cr.Context(N, [0, 0])
    try:
        for b in batches:
            _upload(multi, b)
        was = states(multi, batches)
        with pytest.raises(NotImplementedError, match="cfmm_swap_path is not available on a multi-device context"):
            multi.swap_path(*paths)
        same_states(states(multi, batches), was)
        multi.quote_path(*paths)                                              # ... while the read-only call is
    finally:
        multi.close()


def test_bad_input_names_path_and_hop_and_changes_nothing():
    L = cr.lib()
    batches, paths = three_segments()
    n_hops, seg, row, ci, co, amt = paths
    be = backend(batches)
    try:
        ctx = be.ctx
        be.find_arb(V)
        trades = [np.array(x, copy=True) for x in be.trades()]
        was = states(ctx, batches)
        c = lambda a: np.ascontiguousarray(a.T)

        def refused(match, seg=seg, row=row, ci=ci, co=co, amt=amt, lim=None):
            out, hv, st = np.full(amt.size, 7.0), np.full((3, amt.size), 7.0), np.full(amt.size, 7, dtype=np.int32)
            rc = L.cfmm_swap_path(ctx._h, amt.size, 3, ptr(n_hops), ptr(c(seg)), ptr(c(row)), ptr(c(ci)), ptr(c(co)), ptr(np.ascontiguousarray(amt)),
                                  ptr(lim), ptr(out), ptr(hv), ptr(st))
            msg = L.cfmm_last_error(ctx._h).decode()
            assert rc == -1 and msg.startswith("cfmm_swap_path: ") and match in msg, (rc, msg)
            assert np.all(out == 7.0) and np.all(hv == 7.0) and np.all(st == 7)

        def edit(a, p, k, value):
            a = a.copy()
            a[p, k] = value
            return a
        refused("path 5, hop 2: row 64 out of range (segment 1 has 64 pools)", row=edit(row, 5, 2, 64))     # path 5 has 3 hops
        refused("path 2, hops 0 and 2: row 9 of segment 2 appears twice", seg=edit(edit(seg, 2, 0, 2), 2, 2, 2), row=edit(edit(row, 2, 0, 9), 2, 2, 9))
        refused("path 1, hop 0: coin_in 2 out of range", ci=edit(ci, 1, 0, 2))
        bad = amt.copy(); bad[7] = np.nan
        refused("path 7, hop 0: amount_in must be finite and >= 0", amt=bad)
        lim = np.zeros(amt.size); lim[4] = -1.0
        refused("path 4, hop 1: min_amount_out must be finite and >= 0", lim=lim)
        assert L.cfmm_swap_path(ctx._h, 1, 9, *([None] * 10)) == -1 and "max_hops" in L.cfmm_last_error(ctx._h).decode()
        same_states(states(ctx, batches), was)
        assert_same([np.asarray(x) for x in be.trades()], trades)                # the earlier trades are still readable
    finally:
        be.close()


# ---- 7. router level ----------------------------------------------------------------------------------------------------------------
def mixed_pools():
    u = exact_ladder()
    return [cr.ProductTwoCoin([1e4, 2e4], 0.997, [1, 2]),
            cr.UniV3(0.6, u.lower_ticks[:3], u.liquidity[:3] * 1e4, 0.997, [2, 3]),
            cr.Curve([1e4, 1.1e4, 0.9e4], 0.9995, [1, 3, 4], 2.0, 1e16),
            cr.ProductTwoCoin([3e4, 1e4], 0.997, [3, 5]),
            cr.UniV3(2.25, u.lower_ticks[:3], u.liquidity[:3] * 1e4, 1.0, [4, 6]),
            cr.ProductTwoCoin([5e3, 5e3], 0.997, [5, 6])]


def test_swap_path_through_a_router_equals_the_chain_of_swaps():
    n = 6
    path_pools = [[0, 1, 3], [2, 4, 5], [3, 5, 4], [0]]
    path_tokens = [[1, 2, 3, 5], [1, 4, 6, 5], [3, 5, 6, 4], [2, 1]]
    amt = [50.0, 40.0, 30.0, 20.0]
    r = cr.Router(cr.LinearNonnegative(np.ones(n)), mixed_pools(), n)
    twin = cr.Router(cr.LinearNonnegative(np.ones(n)), mixed_pools(), n)
    try:
        cr.route_(r, solver="native")
        out, status, hops = cr.swap_path_(r, path_pools, path_tokens, amt, min_out=0.0, hops=True)
        input_conditions(status, out, "router")
        assert all(np.all(np.asarray(x) == 0) for x in r.Δs)                    # the old trades are gone
        for p, (pl, tk) in enumerate(zip(path_pools, path_tokens)):
            x = amt[p]
            for k, i in enumerate(pl):
                Ai = list(twin.cfmms[i].Ai)
                x = cr.swap_(twin, [i], [Ai.index(tk[k])], [x], [Ai.index(tk[k + 1])])[0]
                assert bits(hops[k, p:p + 1])[0] == bits([x])[0], (p, k)
            assert bits(out[p:p + 1])[0] == bits([x])[0]
        ctx, L = r._backend.ctx, r._layout
        for i, (pool, other) in enumerate(zip(r.cfmms, twin.cfmms)):           # the host mirror equals the device and the twin
            _, b, row = L.locate(i)
            s, batch = L.seg_of[b], L.batches[b]
            if isinstance(pool, cr.UniV3):
                assert pool.current_price == ctx.prices(s, len(batch))[row] == other.current_price
            else:
                same_bits(pool.R, ctx.reserves(s, len(batch), len(pool.R))[row])
                same_bits(pool.R, other.R)
        assert r.cfmms[1].current_price < 0.6 and r.cfmms[0].R[0] != 1e4          # (coin 0 went into the UniV3 pool: its price fell)
        cr.route_(r, solver="native")                                          # ... and the router routes on
    finally:
        r.close()
        twin.close()

