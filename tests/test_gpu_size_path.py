"""cfmm_size_path on the device: the input of a path that maximises its gain, by the bracketing search stated in
include/cfmm_amd_size_path.h -- one wavefront per path, one lane per trial size.  The pin of the feature is bit-equality with the
numpy statement of that contract (tests/size_path_ref.py) driven by ctx.quote_path, on test_gpu_quote_path.py's market of eight
segments of every pool family: amount_in, amount_out, gain and status.  Around it: the round trip through quote_path, grid
geometry, the device-pointer entry and its poisoning, edges, live state, read-only behaviour, a multi-device parent, large-market
mode, errors, options, ownership and the router-level call.

261 paths: 65 blocks of four wavefronts and one wavefront more.  With x0 the path's first amount and y0 = quote_path(x0):
value_out = 1, value_in = 0.5·y0/x0 (1 where y0 is 0), max_in = 64·x0 -- so a path gains at x0 whenever y0 > 0, shallow paths
bind at the limit and deep ones turn over inside it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from cfmmrouter_amd._lib import (KIND_UNIV3, MAX_SIZE_ROUNDS, OBJ_LINEAR_NONNEGATIVE, SIZED, SIZED_AT_LIMIT, SIZED_NAN, SIZED_NONE,
                                 ptr)
from cfmmrouter_amd.cfmms import _upload
from size_path_ref import size_path_ref
from test_gpu_pool_update import batch_with, moved_prices, rows_of
from test_gpu_quote import N, pools
from test_gpu_quote_path import H, M, PATTERNS, SEED, bits, make_paths, market, scale_in

pytestmark = pytest.mark.gpu

COUNT = 261             # 65 blocks of 4 wavefronts plus one wavefront
ROUNDS = (1, 2, 5, 16)
VALUES = ("both", "in", "out", "none")                  # which of value_in / value_out the call gives


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def same_answer(got, want, what=""):
    """(amount_in, amount_out, gain, status): the three amounts bit for bit (NaN as NaN), the status equal"""
    np.testing.assert_array_equal(got[3], want[3], err_msg=what + " status")
    nan = want[3] == SIZED_NAN
    for name, g, w in zip(("amount_in", "amount_out", "gain"), got, want):
        assert np.all(np.isnan(g[nan])), what + " " + name
        same_bits(g[~nan], w[~nan], what + " " + name)


def quoter(ctx, p):
    """the contract's market: what ctx.quote_path answers for amounts x through paths idx of p"""
    n_hops, seg, row, ci, co = p[:5]
    return lambda idx, x: ctx.quote_path(n_hops[idx], seg[idx], row[idx], ci[idx], co[idx], x)


def inputs(ctx, p):
    x0 = p[5]
    y0 = ctx.quote_path(*p)
    live = y0 > 0
    vi = np.where(live, 0.5 * y0 / x0, 1.0)
    vo = np.where(live, 2.0 * x0 / np.where(live, y0, 1.0), 1.0)   # the same ratio put on the other side
    return dict(max_in=64.0 * x0, vi=vi, vo=vo, y0=y0)


def values_of(inp, which):
    one = np.ones(inp["vi"].size)
    return {"both": (inp["vi"], one), "in": (inp["vi"], None), "out": (None, inp["vo"]), "none": (None, None)}[which]


class World:
    def __init__(self):
        self.batches = market(seed=SEED)
        self.be = cr.DeviceBackend(N, self.batches)
        self.ctx = self.be.ctx
        self.paths = {pat: make_paths(self.batches, pat, count=COUNT, seed=SEED) for pat in PATTERNS}
        self.inp = {pat: inputs(self.ctx, self.paths[pat]) for pat in PATTERNS}
        self._ref = {}

    def ref(self, pattern, which, rounds):
        """the reference's answer, computed once and left unchanged"""
        key = (pattern, which, rounds)
        if key not in self._ref:
            vi, vo = values_of(self.inp[pattern], which)
            self._ref[key] = size_path_ref(quoter(self.ctx, self.paths[pattern]), self.inp[pattern]["max_in"], vi, vo, rounds)
        return self._ref[key]

    def size(self, pattern, which, rounds, ctx=None):
        vi, vo = values_of(self.inp[pattern], which)
        return (ctx or self.ctx).size_path(*self.paths[pattern][:5], self.inp[pattern]["max_in"], vi, vo, rounds)


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.be.close()


# ---- the condition on the inputs, on the reference alone -------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_inputs_bind_and_turn_over(world, pattern):
    """each of SIZED and SIZED_AT_LIMIT is at least a tenth of the paths: the comparison below is one of searches that end inside
    the bracket AND of searches that end at its upper end"""
    st = world.ref(pattern, "both", 5)[3]
    frac = {name: float(np.mean(st == code)) for name, code in (("SIZED", SIZED), ("AT_LIMIT", SIZED_AT_LIMIT), ("NONE", SIZED_NONE), ("NAN", SIZED_NAN))}
    print(f"size_path inputs {pattern}: {frac}")
    assert frac["SIZED"] >= 0.1 and frac["AT_LIMIT"] >= 0.1 and frac["NAN"] == 0.0


# ---- the pin ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("rounds", ROUNDS)
def test_the_device_is_the_reference_bit_for_bit(world, pattern, rounds):
    for which in VALUES:
        got = world.size(pattern, which, rounds)
        same_answer(got, world.ref(pattern, which, rounds), f"{pattern}, rounds {rounds}, values {which}")
        sized = (got[3] == SIZED) | (got[3] == SIZED_AT_LIMIT)
        assert np.all(got[2][sized] > 0) and np.all(got[0][sized] <= world.inp[pattern]["max_in"][sized])
        same_bits(got[0][got[3] == SIZED_AT_LIMIT], world.inp[pattern]["max_in"][got[3] == SIZED_AT_LIMIT], "the limit binds bit for bit")
        none = got[3] == SIZED_NONE
        assert not np.any(bits(got[0][none])) and not np.any(bits(got[1][none])) and not np.any(bits(got[2][none]))   # three +0.0


@pytest.mark.parametrize("pattern", PATTERNS)
def test_quote_path_at_the_answer_is_amount_out(world, pattern):
    x, y, g, st = world.size(pattern, "both", 5)
    same_bits(world.ctx.quote_path(*world.paths[pattern][:5], x), y)
    vi, vo = values_of(world.inp[pattern], "both")
    same_bits(g, vo * y - vi * x)


def test_the_grid_does_not_change_the_bits(world):
    ctx = world.ctx
    default = ctx.get_option("size_max_blocks")
    assert default >= 1
    try:
        for blocks in (1, 2):
            ctx.set_option("size_max_blocks", blocks)
            for pattern in PATTERNS:
                same_answer(world.size(pattern, "both", 5), world.ref(pattern, "both", 5), f"size_max_blocks {blocks}, {pattern}")
        with pytest.raises(cr.ArgumentError, match="size_max_blocks"):
            ctx.set_option("size_max_blocks", 0)
    finally:
        ctx.set_option("size_max_blocks", default)
    # ... and neither does the batch: a slice of the paths gives the slice of the answers
    p, inp = world.paths["interleaved"], world.inp["interleaved"]
    for sl in (slice(0, 1), slice(3, 8), slice(100, 261)):
        got = ctx.size_path(*(a[sl] for a in p[:5]), inp["max_in"][sl], inp["vi"][sl], None, 5)
        same_answer(got, tuple(a[sl] for a in world.ref("interleaved", "in", 5)), str(sl))


# ---- the device-pointer entry -----------------------------------------------------------------------------------------------------
def test_the_device_entry_gives_the_same_bits_and_poisons_only_bad_paths(world):
    import torch
    ctx = world.ctx
    p, inp = world.paths["interleaved"], world.inp["interleaved"]
    want = world.ref("interleaved", "both", 5)
    n_hops, seg, row, ci, co = (a.copy() for a in p[:5])
    max_in, vi = inp["max_in"].copy(), inp["vi"].copy()
    bad = {40: "n_hops 0", 77: "a row out of range", 130: "a negative max_in", 131: "a value of 0", 200: "n_hops 9", 201: "a NaN max_in"}
    n_hops[40], n_hops[200] = 0, 9
    assert p[0][77] > 2
    row[77, 2] = M
    max_in[130], max_in[201] = -1.0, np.nan
    vi[131] = 0.0
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t_good = [up(p[0]), up(p[1].T), up(p[2].T), up(p[3].T), up(p[4].T), up(inp["max_in"]), up(inp["vi"])]
    t_bad = [up(n_hops), up(seg.T), up(row.T), up(ci.T), up(co.T), up(max_in), up(vi)]
    outs = [[torch.full((COUNT,), 7.0, dtype=torch.float64, device=dev) for _ in range(3)] + [torch.full((COUNT,), 7, dtype=torch.int32, device=dev)]
            for _ in range(2)]
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for t, o in zip((t_good, t_bad), outs):
            ctx.size_path_dev(COUNT, H, *(x.data_ptr() for x in t), 0, 5, *(x.data_ptr() for x in o))
        torch.cuda.synchronize()
    finally:
        ctx.reset_stream()
    good, poisoned = (tuple(x.cpu().numpy() for x in o) for o in outs)
    same_answer(good, want, "size_path_dev")
    mask = np.zeros(COUNT, dtype=bool)
    mask[list(bad)] = True
    assert np.all(poisoned[3][mask] == SIZED_NAN)
    for v in poisoned[:3]:
        assert np.all(np.isnan(v[mask]))
    same_answer(tuple(a[~mask] for a in poisoned), tuple(a[~mask] for a in want), "the neighbours of the poisoned paths")


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_edges_zero_limit_dry_and_exhausted_univ3_and_no_paths(world):
    ctx, u = world.ctx, world.batches[3]
    assert u.kind == KIND_UNIV3
    p, inp = world.paths["interleaved"], world.inp["interleaved"]
    # max_in == 0: nothing to put in
    x, y, g, st = ctx.size_path(*p[:5], np.zeros(COUNT), None, None, 3)
    assert np.all(st == SIZED_NONE) and not np.any(bits(x)) and not np.any(bits(y)) and not np.any(bits(g))
    # one-hop paths on a UniV3 segment of its own, both directions of every pool; the first eight pools hold no liquidity at all
    tick_pool = np.repeat(np.arange(M), np.diff(u.tick_off))
    u2 = batch_with(u, liquidity=np.where(tick_pool < 8, 0.0, u.liquidity))
    be = cr.DeviceBackend(N, [u2])
    try:
        c2 = be.ctx
        rows = np.tile(np.arange(M), 2)
        cin = np.repeat(np.array([0, 1], dtype=np.int32), M)
        scale = np.sqrt(u.liquidity[u.tick_off[:-1]] + 1.0)[rows]
        one = lambda a, dt: np.asarray(a, dtype=dt).reshape(-1, 1)
        hop = (np.ones(2 * M, dtype=np.int32), one(np.zeros(2 * M), np.int32), one(rows, np.int64), one(cin, np.int32), one(1 - cin, np.int32))
        big, huge = (c2.quote(0, f * scale, cin, None, rows) for f in (1e7, 1e10))
        dry = np.flatnonzero(huge == 0.0)                              # a direction without liquidity
        full = np.flatnonzero((huge > 0) & (huge == big))              # a ladder that the limit exhausts a thousand times over
        print(f"size_path UniV3 edges: {dry.size} dry directions, {full.size} exhausted ladders of {2 * M}")
        assert dry.size >= 16 and full.size >= 8
        max_in = 1e10 * scale
        vi = np.where(huge > 0, 0.5 * huge / max_in, 1.0)              # half the whole ladder's worth at the limit
        q = quoter(c2, hop + (None,))
        for rounds in (1, 5):
            got = c2.size_path(*hop, max_in, vi, None, rounds)
            same_answer(got, size_path_ref(q, max_in, vi, None, rounds), f"UniV3 one-hop paths, rounds {rounds}")
            assert np.all(got[3][dry] == SIZED_NONE)
            # beyond the ladder's end the output is flat and the cost rises: the answer lies below the limit
            assert np.all(got[3][full] == SIZED) and np.all(got[0][full] < max_in[full]) and np.all(got[1][full] <= huge[full])
    finally:
        be.close()
    # count == 0: empty answers, and NULL arrays through the library
    e = np.zeros((0, H), dtype=np.int32)
    out = ctx.size_path(np.zeros(0, dtype=np.int32), e, e, e, e, np.zeros(0))
    assert all(a.size == 0 for a in out)
    ctx._check(cr.lib().cfmm_size_path(ctx._h, 0, H, None, None, None, None, None, None, None, None, 5, None, None, None, None))


# ---- live state: the segment table is rebuilt on every call ----------------------------------------------------------------------
def test_sizing_follows_swaps_and_tick_updates():
    batches = market(seed=21)
    paths = make_paths(batches, "interleaved", count=COUNT, seed=21)
    be = cr.DeviceBackend(N, batches)
    try:
        ctx = be.ctx
        inp = inputs(ctx, paths)
        size = lambda: ctx.size_path(*paths[:5], inp["max_in"], inp["vi"], None, 5)
        ref = lambda: size_path_ref(quoter(ctx, paths), inp["max_in"], inp["vi"], None, 5)
        before = size()
        same_answer(before, ref(), "before")
        rows = rows_of(M, 100, 23)
        ctx.swap(0, 0.2 * batches[0].R[rows, 0], np.zeros(100, dtype=np.int32), None, rows)      # the product segment moves
        u = batches[3]
        pick = rows_of(M, M // 2, 50)
        price = moved_prices(u, 60)[pick]
        off = np.concatenate([[0], np.cumsum(np.diff(u.tick_off)[pick])])
        sel = np.concatenate([np.arange(u.tick_off[r], u.tick_off[r + 1]) for r in pick])
        ctx.set_ticks(3, pick, price, off, u.lower_ticks[sel], 1.5 * u.liquidity[sel])            # a mint on half the UniV3 pools
        after = size()
        same_answer(after, ref(), "after swap and set_ticks")
        assert np.any(bits(after[0]) != bits(before[0]))
    finally:
        be.close()


# ---- read-only --------------------------------------------------------------------------------------------------------------------
def test_sizing_changes_nothing_the_other_calls_see():
    batches = [pools("product", 700, 61), pools("geomean", 700, 62), pools("univ3", 300, 63), pools("solidly", 300, 64)]
    v = synth.sweep_prices(N, seed=65, spread=0.3)
    c = synth.linear_prices(N, seed=66)
    p, k = np.meshgrid(np.arange(200), np.arange(4), indexing="ij")
    n_hops = (1 + np.arange(200) % 4).astype(np.int32)
    seg = ((p + k) % 4).astype(np.int32)
    row = ((7 * p + 13 * k) % 300).astype(np.int64)
    ci = ((p + k) % 2).astype(np.int32)
    co = (1 - ci).astype(np.int32)
    amt = np.array([scale_in(batches[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(200)])

    def run(sizing):
        be = cr.DeviceBackend(N, batches)
        ctx = be.ctx
        res = []

        def s():
            if sizing:
                ctx.size_path(n_hops, seg, row, ci, co, amt, 0.01, None, 3)
        try:
            s()                                                        # needs no sweep to have run
            ctx.find_arb(v)
            s()
            res.append(ctx.trades())
            s()
            res.append(ctx.select_trades(0, 0.0))
            s()
            res.append((ctx.netflows(), ctx.dual_value()))
            s()
            ctx.update_reserves()
            s()
            res.append(ctx.eval(v))
            s()
            vr, psi, info = ctx.route(OBJ_LINEAR_NONNEGATIVE, c, 0, v0=np.ones(N), maxfun=60)     # pre-armed evaluations
            s()
            res.append((vr, psi, {k_: info[k_] for k_ in ("f", "proj_grad", "iterations", "evaluations", "status")}, ctx.netflows()))
        finally:
            be.close()
        return res

    a, b = run(True), run(False)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for s_, t in zip(x, y):
                same(s_, t)
        elif isinstance(x, dict):
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
        for pattern, which, rounds in (("interleaved", "both", 5), ("uniform", "out", 2), ("interleaved", "none", 1)):
            same_answer(world.size(pattern, which, rounds, ctx=multi), world.ref(pattern, which, rounds), f"parent: {pattern}, {which}, {rounds}")
            assert multi.get_option("size_launches") == rounds and multi.get_option("size_ns") > 0
        with pytest.raises(NotImplementedError, match="cfmm_size_path_dev"):
            multi.size_path_dev(1, 1, 8, 8, 8, 8, 8, 8, 0, 0, 5, 8, 8, 8, 8)
    finally:
        multi.close()


def test_large_market_mode_gives_the_same_bits():
    """two-coin segments only (large-market mode has no N-coin kernel), one token moved beyond the LDS limit"""
    small = market()[:4]
    big = [batch_with(b, Ai=np.where(b.Ai == 1, 8193, b.Ai)) for b in small]
    p, k = np.meshgrid(np.arange(COUNT), np.arange(4), indexing="ij")
    n_hops = (1 + np.arange(COUNT) % 4).astype(np.int32)
    seg = ((p + 3 * k) % 4).astype(np.int32)
    row = np.minimum((synth.uniform(11, 3, COUNT * 4).reshape(COUNT, 4) * M).astype(np.int64), M - 1)
    ci = ((p + k) % 2).astype(np.int32)
    co = (1 - ci).astype(np.int32)
    x0 = np.array([scale_in(small[seg[q, 0]])[row[q, 0], ci[q, 0]] for q in range(COUNT)]) * 0.01
    be_s, be_b = cr.DeviceBackend(N, small), cr.DeviceBackend(8193, big)
    try:
        inp = inputs(be_s.ctx, (n_hops, seg, row, ci, co, x0))
        a = be_s.ctx.size_path(n_hops, seg, row, ci, co, inp["max_in"], inp["vi"], None, 5)
        b = be_b.ctx.size_path(n_hops, seg, row, ci, co, inp["max_in"], inp["vi"], None, 5)
        same_answer(b, a)
        assert np.sum(np.isin(a[3], (SIZED, SIZED_AT_LIMIT))) > COUNT // 2
    finally:
        be_s.close()
        be_b.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_the_host_entry_refuses_names_the_path_and_leaves_the_outputs(world):
    ctx, L = world.ctx, cr.lib()
    n = 16
    p, inp = world.paths["interleaved"], world.inp["interleaved"]
    n_hops, seg, row, ci, co = (a[:n] for a in p[:5])
    max_in, vi = inp["max_in"][:n], inp["vi"][:n]

    def refused(match, n_hops=n_hops, row=row, max_in=max_in, vi=vi, vo=None, rounds=5, outputs=True):
        out = [np.full(n, 7.0) for _ in range(3)] + [np.full(n, 7, dtype=np.int32)]
        T = lambda a, dt: np.ascontiguousarray(np.asarray(a).T, dtype=dt)
        rc = L.cfmm_size_path(ctx._h, n, H, ptr(np.ascontiguousarray(n_hops, dtype=np.int32)), ptr(T(seg, np.int32)), ptr(T(row, np.int64)),
                              ptr(T(ci, np.int32)), ptr(T(co, np.int32)), ptr(np.ascontiguousarray(max_in)),
                              ptr(None if vi is None else np.ascontiguousarray(vi)), ptr(None if vo is None else np.ascontiguousarray(vo)),
                              rounds, ptr(out[0]), ptr(out[1]), ptr(out[2] if outputs else None), ptr(out[3]))
        msg = L.cfmm_last_error(ctx._h).decode()
        assert rc == -1 and msg.startswith("cfmm_size_path:") and match in msg, (rc, msg)
        assert all(np.all(a == 7) for a in out)                            # the outputs are untouched

    def edit(a, at, value):
        a = a.copy()
        a[at] = value
        return a
    refused("rounds must be 1 .. 16 (got 0)", rounds=0)
    refused("rounds must be 1 .. 16 (got 17)", rounds=MAX_SIZE_ROUNDS + 1)
    refused("path 9, hop 0: value_in must be finite and > 0", vi=edit(vi, 9, 0.0))
    refused("path 4, hop 0: value_out must be finite and > 0", vo=edit(np.ones(n), 4, 0.0))
    refused("path 11, hop 0: max_amount_in must be finite and >= 0", max_in=edit(max_in, 11, np.nan))
    refused("path 11, hop 0: max_amount_in", max_in=edit(max_in, 11, -1.0))
    refused("path 12, hop 3: row", row=edit(row, (12, 3), M))              # path 12 has 5 hops
    refused("path 5: n_hops 0", n_hops=edit(n_hops, 5, 0))
    refused("null path array", outputs=False)
    with pytest.raises(cr.ArgumentError, match="path 12, hop 3: row"):
        ctx.size_path(n_hops, seg, edit(row, (12, 3), -1), ci, co, max_in)


# ---- options ----------------------------------------------------------------------------------------------------------------------
def test_the_kernel_span_and_the_launch_count(world):
    ctx = world.ctx
    ctx.set_option("time_kernels", 1)
    try:
        same_answer(world.size("uniform", "both", 5), world.ref("uniform", "both", 5))
        assert ctx.get_option("size_ns") > 0 and ctx.get_option("size_launches") == 1
        print(f"size_path: {COUNT} paths, 5 rounds: kernel span {ctx.get_option('size_ns')} ns")
    finally:
        ctx.set_option("time_kernels", 0)


# ---- ownership --------------------------------------------------------------------------------------------------------------------
COUNTERS = ("debug_live_allocs", "debug_live_pinned", "debug_live_events", "debug_live_streams")


def live_counts_body():
    probe = cr.Context(4)
    live = lambda: tuple(probe.get_option(k) for k in COUNTERS)
    base = live()
    batches = market()
    be = cr.DeviceBackend(N, batches)
    paths = make_paths(batches, "interleaved", count=COUNT)
    before = live()
    be.ctx.set_option("time_kernels", 1)
    be.ctx._check(cr.lib().cfmm_size_path(be.ctx._h, 0, H, None, None, None, None, None, None, None, None, 5, None, None, None, None))
    assert live() == before and be.ctx.get_option("size_ns") == 0        # count == 0 touches nothing
    be.ctx.size_path(*paths[:5], 64.0 * paths[5], 0.01, None, 5)
    first = live()
    # the first call creates the scratch: 6 device arrays (table, int32 columns, rows, limits and values, answers, statuses), one
    # pinned staging buffer, 3 events (the guard, and {start, stop} under time_kernels), no stream
    assert tuple(x - y for x, y in zip(first, before)) == (6, 1, 3, 0), (before, first)
    assert be.ctx.get_option("size_ns") > 0
    be.ctx.size_path(*(a[:100] for a in paths[:5]), paths[5][:100], None, 2.0, 16)
    assert live() == first                                               # stable across calls
    be.close()
    assert live() == base                                                # everything goes with the context
    probe.close()
    print("size-path-live-ok")


def test_live_counts_with_the_hooks_library():
    """the four debug_live_* counts: what the first sizing call creates stays for the next and goes with the context"""
    from cfmmrouter_amd._lib import LIB_PATH
    hooks = os.path.join(os.path.dirname(LIB_PATH), "libcfmm_amd_hooks.so")
    assert os.path.exists(hooks), "build it: make -C cfmmrouter.jl_amd/csrc hooks (__graft_entry__.build() does)"
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_size_path as t\n"
            "t.live_counts_body()\n") % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CFMM_AMD_LIB=hooks), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "size-path-live-ok" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


# ---- the router-level call --------------------------------------------------------------------------------------------------------
def test_the_router_level_call_beats_the_ladder_of_the_example():
    """examples/execute_cycle.py's market and its ladder of 20 sizes: the search's gain is at least the ladder's best"""
    cycle_pools = [cr.ProductTwoCoin([1.00e5, 2.00e5], 0.997, [1, 2]),
                   cr.GeometricMeanTwoCoin([2.00e5, 1.04e5], [0.5, 0.5], 0.997, [2, 3]),
                   cr.Curve([1.0e5, 1.0e5], 0.9995, [3, 1], 2.0, 1e15)]
    r = cr.Router(cr.LinearNonnegative(np.ones(3)), cycle_pools, 3)
    try:
        cycle, tokens = [0, 1, 2], [1, 2, 3, 1]
        sizes = 50.0 * 1.25 ** np.arange(20)
        quoted = cr.quote_path(r, [cycle] * sizes.size, [tokens] * sizes.size, sizes)
        ladder = float(np.max(quoted - sizes))
        x, y, g, st = cr.size_path(r, [cycle], [tokens], sizes[-1])
        print(f"size_path on the example's cycle: {x[0]:.9g} in -> gain {g[0]:.9g}; the ladder's best gain {ladder:.9g}")
        assert st[0] == cr.SIZED and ladder > 0 and g[0] >= ladder
        same_bits(cr.quote_path(r, [cycle], [tokens], x), y)
        x2, _, g2, st2 = cr.size_path(r, [cycle, cycle], [tokens, tokens], [sizes[-1], 100.0], rounds=5)    # one limit per path
        same_bits(x2[:1], x)
        assert st2[1] == cr.SIZED_AT_LIMIT and x2[1] == 100.0
        with pytest.raises(cr.ArgumentError, match="path 0, hop 1: token 1 is not a coin of pool 1"):
            cr.size_path(r, [cycle], [[1, 2, 1, 1]], 100.0)                                               # a token break
        with pytest.raises(cr.ArgumentError, match="path 0, hop 1: pool 0 appears twice"):
            cr.size_path(r, [[0, 0]], [[1, 2, 1]], 100.0)
        with pytest.raises(cr.ArgumentError, match="max_in must be a scalar or have one entry per path"):
            cr.size_path(r, [cycle], [tokens], [1.0, 2.0])
    finally:
        r.close()
