"""Ψ and the dual value against EXACT sums of the device's own trades (tests/reduction_ref.py), at every geometry of the
reduction chain: the LDS bin scatter (private copies / one shared copy), finish_row, the single-block direct publish,
reduce_partials at 2 / 63..65 / 255..257 partial rows x every column-group edge, fused launches under both block -> segment
maps, N-coin and Solidly rows, large-market mode (gather_chunks / token_fold at their chunk, lane and block edges), and
reduce_gather with up to 16 ranks -- both peer passes, own rank on either side of 8, sequence tags across their wrap.

Markets are ill-scaled (token amounts over 2^-40 .. 2^40, the numeraire on top, tokens of degree 0 and 1 at the bottom): a
flow that is dropped, doubled or booked on the wrong token is 10^-24 of max|Ψ| there and 10^16 bounds here.  Every case
prints its geometry and the worst |error| / bound it saw -- the margin the kernels have, a record and not a threshold.
"""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from helpers import dev_sweep
import reduction_ref as rr

pytestmark = pytest.mark.gpu


def _uneven(total, count, seed):
    """`count` degrees that share about `total` stubs unevenly."""
    w = 0.25 + synth.uniform(seed, 210, count)
    return np.floor(total * w / w.sum()).astype(np.int64)


def _degrees(n, m, seed, special=(0, 1, 1, 0, 1, 2, 3), hub=None):
    """Degrees of the non-hub tokens and the hub's, for about m pools: the hub meets a third of the pools unless told (all of
    them when the market has fewer than 16 tokens), `special` sits on tokens 1.., the other tokens share the rest unevenly."""
    deg = np.zeros(n, dtype=np.int64)
    if n < 16:
        deg[1:] = _uneven(m, n - 1, seed)
        deg[1] += m - deg.sum()
        return deg, m
    hub = m // 3 if hub is None else hub
    free = np.arange(1 + len(special), n)
    deg[free] = _uneven(2 * m - hub - sum(special), free.size, seed)
    deg[1:1 + len(special)] = special
    return deg, hub


_markets = {}


def _market(n, m, seed, families=("product",), **scale):
    key = (n, m, seed, families, tuple(sorted(scale.items())))
    if key not in _markets:
        deg, hub = _degrees(n, m, seed)
        batches, v, _ = rr.ill_scaled_market(n, deg, hub, seed, families, **scale)
        _markets[key] = (batches, v, rr.flat_tokens(batches))
    return _markets[key]


def _backend(n, batches, **opts):
    be = cr.DeviceBackend(n, batches)
    for k, val in opts.items():
        be.ctx.set_option(k, val)
    return be


def _check_every_path(be, n, v, Ai0, label, bit_equal=False, ill=None):
    """A materialising sweep gives the trades; its {Ψ, acc}, those of the two fused evaluations behind it (option
    "alternate": the first walks backwards, the second forwards again) and those of device-pointer sweeps, fused and
    materialising, all go through the exact reference.  bit_equal: same direction => the same bits (fixed-order geometries)."""
    geo = be.ctx.segments()
    psi, acc = be.find_arb(v)
    D, L = (np.ravel(x) for x in be.trades())
    if ill is not None:                      # the batches of an ill-scaled market: it must be what the case needs
        rr.assert_ill_scaled(D, L, Ai0, n, ill)
    worst = {"find_arb": rr.assert_reduction_exact(D, L, Ai0, v, n, psi, acc, (label, "find_arb", geo))}
    back, fwd = be.eval(v), be.eval(v)
    worst["eval<-"] = rr.assert_reduction_exact(D, L, Ai0, v, n, back[0], back[1], (label, "eval backwards", geo))
    worst["eval->"] = rr.assert_reduction_exact(D, L, Ai0, v, n, fwd[0], fwd[1], (label, "eval forwards", geo))
    for mat in (False, True):
        pd, ad = dev_sweep(be, v, materialize=mat)
        if mat:
            D2, L2 = (np.ravel(x) for x in be.trades())
            np.testing.assert_array_equal(D2, D)
            np.testing.assert_array_equal(L2, L)
        worst[f"dev{int(mat)}"] = rr.assert_reduction_exact(D, L, Ai0, v, n, pd, ad, (label, f"sweep_dev mat={mat}", geo))
    if bit_equal:
        np.testing.assert_array_equal(fwd[0], psi)
        assert fwd[1] == acc
    print(f"[reduction] {label}: segments {[(s['kind'], s['m'], s['block'], s['grid']) for s in geo]} "
          f"worst/bound " + " ".join(f"{k}={w:.3f}" for k, w in worst.items()))
    return psi, acc, D, L


# ---- the row fold: partial rows x column groups --------------------------------------------------------------------------

@pytest.mark.parametrize("n1", [3, 8, 9, 16, 17, 128, 129, 136])
@pytest.mark.parametrize("rows", [2, 63, 64, 65, 255, 256, 257])
def test_fold_rows_and_column_groups(rows, n1):
    """reduce_partials: 64 row-lanes x batches of 4 rows (tails at 63 / 65 / 255 / 257 rows), 8 columns per block, the
    pair of groups of a line dealt to one XCD (n + 1 = 129: the first group of the second deal; 136: its line complete)."""
    n = n1 - 1
    m = rows * 512 + 77                      # more tiles than blocks: some lanes sweep two pools
    batches, v, Ai0 = _market(n, m, seed=300 + n1)
    be = _backend(n, batches, block=512, max_grid=rows, direct_small=0)
    try:
        seg = be.ctx.segments()
        assert len(seg) == 1 and seg[0]["block"] == 512 and seg[0]["grid"] == rows and seg[0]["m"] > rows * 512
        _check_every_path(be, n, v, Ai0, f"fold rows={rows} n+1={n1} fold_grid={rr.fold_grid(n1)}",
                          ill=batches if n >= 16 else None)
    finally:
        be.close()


# ---- the LDS bins: private copies per wavefront, or one shared copy ---------------------------------------------------------

@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("block", [512, 1024])
@pytest.mark.parametrize("copies", [1, 2, 0])
def test_bin_copies_on_both_sides_of_the_auto_threshold(copies, block, side):
    n = rr.auto_threshold(block) + (0 if side == "below" else 1)
    planned = rr.planned_copies(n, copies, block)
    assert planned == (1 if copies == 1 or (copies == 0 and side == "above") else block // 64)
    batches, v, Ai0 = _market(n, 40_000, seed=400 + block // 512)
    be = _backend(n, batches, block=block, bin_copies=copies)
    try:
        seg = be.ctx.segments()
        assert seg[0]["block"] == block and seg[0]["grid"] == -(-seg[0]["m"] // block)
        _check_every_path(be, n, v, Ai0, f"bins n={n} block={block} bin_copies={copies} -> {planned} copies", ill=batches)
    finally:
        be.close()


TINY = 1e-25


@pytest.mark.parametrize("shape", ["private", "shared", "direct"])
def test_flows_far_below_every_other_are_still_summed(shape):
    """Eleven tokens at scale 2^-100, degrees 0 / 1 / 2 / 3 and a few hundred: their flows are about 1e-29, nonzero.  The
    scatter may leave out a flow that IS zero and nothing else: a rule that takes a small flow for none leaves +0.0 where the
    reference expects the flow, bit for bit (one flow) or within the bound (several) -- on private bin copies, on one shared
    copy and in a single-block launch."""
    n, rows = 128, 3                         # 1613 pools: one block of 1024 threads takes them all, or three of 512
    batches, v, Ai0 = _market(n, rows * 512 + 77, seed=460, bottom=-100, n_bottom=11)
    opts = {} if shape == "direct" else dict(block=512, max_grid=rows, direct_small=0, bin_copies=1 if shape == "shared" else 2)
    be = _backend(n, batches, **opts)
    try:
        seg = be.ctx.segments()
        assert len(seg) == 1 and seg[0]["grid"] == (1 if shape == "direct" else rows)
        copies = rr.planned_copies(n, opts.get("bin_copies", 0), seg[0]["block"])
        assert copies == (1 if shape == "shared" else seg[0]["block"] // 64)
        _, _, D, L = _check_every_path(be, n, v, Ai0, f"tiny flows, {shape}: {copies} copies", ill=batches)
        f = L - D
        tiny = (f != 0.0) & (np.abs(f) < TINY)
        per_token = np.bincount(Ai0[tiny], minlength=n)
        assert np.count_nonzero(tiny) >= 40 and np.any(per_token == 1) and np.any(per_token >= 8), per_token[:12]
        print(f"[reduction] tiny flows, {shape}: {np.count_nonzero(tiny)} nonzero flows below {TINY:g} "
              f"(smallest {np.abs(f[tiny]).min():.3e}) on {np.count_nonzero(per_token)} tokens")
    finally:
        be.close()


def test_the_largest_market_that_keeps_its_bins_in_lds():
    n = 8192
    batches, v, Ai0 = _market(n, 60_000, seed=450)
    be = _backend(n, batches)
    try:
        assert rr.planned_copies(n, 0, be.ctx.segments()[0]["block"]) == 1
        _check_every_path(be, n, v, Ai0, f"LDS limit n={n} copies=1", ill=batches)
    finally:
        be.close()


# ---- single-block launches: the block's row is the result -----------------------------------------------------------------

@pytest.mark.parametrize("n1", [8, 9, 16, 17])
@pytest.mark.parametrize("m", [1, 64, 2048])
def test_direct_publish(m, n1):
    """finish_row's direct form: host granules (find_arb / eval) and plain stores to a device output (sweep_dev)."""
    n = n1 - 1
    full, v, _ = _market(n, 2048, seed=500 + n1)
    batches = [full[0].slice(0, m)]
    Ai0 = rr.flat_tokens(batches)
    be = _backend(n, batches)
    try:
        seg = be.ctx.segments()
        assert len(seg) == 1 and seg[0]["grid"] == 1 and seg[0]["block"] == 1024 and seg[0]["m"] == m
        _check_every_path(be, n, v, Ai0, f"direct m={m} n+1={n1}", bit_equal=True)
    finally:
        be.close()


# ---- fused multi-family launches -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("families,max_grid,grid", [
    (("product", "geomean", "univ3"), 200, 198),
    (("product", "geomean", "univ3", "product"), 200, 200),
    (("product", "geomean", "univ3", "product"), 256, 256)])
def test_fused_launches_under_both_block_maps(families, max_grid, grid):
    """Families that share small tokens in one launch: b % nseg (grid no multiple of 256) and the XCD-aware map (256)."""
    n = 200
    batches, v, Ai0 = _market(n, 132_000, seed=600 + len(families), families=families)
    be = _backend(n, batches, max_grid=max_grid)
    try:
        seg = be.ctx.segments()
        assert len(seg) == len(families) and all(s["block"] == 512 for s in seg) and sum(s["grid"] for s in seg) == grid
        _check_every_path(be, n, v, Ai0, f"fused {'+'.join(families)} max_grid={max_grid} xcd_map={int(grid % 256 == 0)}",
                          ill=batches)
    finally:
        be.close()


def test_ncoin_and_solidly_rows():
    """One mixed market: Product and Solidly pairs, 3-coin weighted and 4-coin Curve pools (ragged trades)."""
    n = 64
    batches = [synth.product_pools(9_000, n - 2, seed=701), synth.solidly_pools(7_001, n - 2, seed=702),
               synth.weighted_pools(5_003, n - 2, 3, seed=703), synth.curve_pools(4_099, n - 2, 4, seed=704)]
    for b in batches:                        # drawn on n - 2 tokens: tokens 1 and 2 (0-based) stay out of the market ...
        b.Ai[b.Ai >= 2] += 2
    batches[0].Ai[0] = (3, 1)                # ... but for token 2 in one Product pool
    v = synth.sweep_prices(n, seed=705, spread=0.5)
    Ai0 = rr.flat_tokens(batches)
    be = _backend(n, batches)
    try:
        assert [s["kind"] for s in be.ctx.segments()] == [b.kind for b in batches]
        psi, _, D, L = _check_every_path(be, n, v, Ai0, "mixed product+solidly+weighted3+curve4")
        assert psi[1] == 0.0 and not np.signbit(psi[1]) and np.count_nonzero(Ai0 == 1) == 0
        assert np.count_nonzero(Ai0 == 2) == 1 and psi[2] == (L - D)[Ai0 == 2][0]
    finally:
        be.close()


# ---- large-market mode ---------------------------------------------------------------------------------------------------

LARGE_DEGREES = (0, 1, 1, 15, 16, 17, 511, 512, 513, 1025, 0, 1)


def _large_market(n):
    key = ("large", n)
    if key not in _markets:
        deg, hub = _degrees(n, 136_000, 800, special=LARGE_DEGREES, hub=20_000)
        deg[n - 1] = 513                     # the last token (token_fold's last lane) ends on a chunk of one entry
        e = rr.token_exponents(n, 800)
        e[1:4] = -40
        Ai = rr.prescribed_pairs(n, deg, hub, 800)
        cut = len(Ai) - 500                  # the GeometricMean segment: one tile
        batches = [rr.rescale(synth.product_pools(cut, n, seed=801), Ai[:cut], e),
                   rr.rescale(rr.tame_weights(synth.geomean_pools(len(Ai) - cut, n, seed=802)), Ai[cut:], e)]
        got = np.bincount(rr.flat_tokens(batches), minlength=n)
        assert tuple(got[1:1 + len(LARGE_DEGREES)]) == LARGE_DEGREES and 20_000 <= got[rr.HUB] <= 21_000
        _markets[key] = (batches, rr.ill_prices(n, e, 803), rr.flat_tokens(batches))
    return _markets[key]


@pytest.mark.parametrize("fuse,max_grid,rows", [(0, 1, 2), (0, 254, 255), (0, 255, 256), (0, 256, 257),
                                                (1, 2, 2), (1, 254, 254), (1, 256, 256), (1, 258, 258)])
@pytest.mark.parametrize("n", [8193, 8448, 8449])
def test_large_market_mode(n, fuse, max_grid, rows):
    """gather_chunks (16 lanes per chunk, chunks of 512 entries: degrees 15..17, 511..513, 1025, a hub of ~20 000) and
    token_fold (256 tokens per block: n = 8193 / 8448 / 8449; the acc column over 1 / 255..257 rows).  Separate launches put
    rows = max_grid + 1 (the GeometricMean segment is one tile); a fused launch has an even number of rows by construction.
    Ψ is pulled in a fixed order: materialising and fused evaluations in the same direction agree bit for bit."""
    batches, v, Ai0 = _large_market(n)
    be = _backend(n, batches, fuse_segments=fuse, max_grid=max_grid)
    try:
        seg = be.ctx.segments()
        assert all(s["block"] == 512 for s in seg) and sum(s["grid"] for s in seg) == rows
        psi, acc, D, L = _check_every_path(be, n, v, Ai0, f"large n={n} fuse={fuse} rows={rows}", bit_equal=True,
                                              ill=batches)
        back = be.eval(v)                    # the other direction reorders the dual column only
        np.testing.assert_array_equal(back[0], psi)
    finally:
        be.close()


def test_large_market_single_row():
    n = 8449
    batches, v, Ai0 = _large_market(n)
    be = _backend(n, batches[:1], max_grid=1)
    try:
        assert [s["grid"] for s in be.ctx.segments()] == [1]
        _check_every_path(be, n, v, Ai0[:2 * len(batches[0])], f"large n={n} rows=1", bit_equal=True, ill=batches[:1])
    finally:
        be.close()


# ---- fold + gather: up to 16 ranks, one of them live ----------------------------------------------------------------------

SEQS = [0, 1, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 1, 2 ** 40 + 2]


def _payloads(world, n1, seed, wild, rank):
    """[world, n1] columns the other ranks 'computed'.  Column kind by index: ordinary, ill-scaled, -0.0 / denormals, bit
    patterns with an all-ones low half, and two kinds with the high half full of ones: wild makes them +-inf and all-ones
    (NaNs) -- device outputs only: a host-pointer evaluation reports a non-finite result as an error -- tame makes them
    finite: ONE rank (the one after `rank`, which carries its own local columns) holds +-1.79e308 (high half 0x7FEFFFFF /
    0xFFEFFFFF), so the SUM has that high half too and the host's reassembly of the output granules (b << 32) sees it."""
    u = synth.uniform(seed, 220, world * n1).reshape(world, n1)
    x = (u - 0.5) * 1000.0
    kind = np.arange(n1) % 6
    x[:, kind == 1] *= 2.0 ** np.floor(80 * synth.uniform(seed, 221, world)[:, None] - 40)
    tiny = np.array([-0.0, 5e-324, -2.5e-310, 0.0, 2.2250738585072014e-308])
    x[:, kind == 2] = tiny[(np.arange(world)[:, None] + np.arange(np.count_nonzero(kind == 2))) % tiny.size]
    bits = x.view(np.uint64)
    bits[:, kind == 3] |= np.uint64(0xFFFFFFFF)
    if wild:
        x[:, kind == 4] = np.where(u[:, kind == 4] < 0.5, np.inf, -np.inf) if seed % 2 else np.inf
        bits[:, kind == 5] |= np.uint64(0xFFFFFFFF00000000)
    elif world > 1:
        other = (rank + 1) % world
        low = bits[other] & np.uint64(0xFFFFFFFF)
        bits[other, kind == 4] = (np.uint64(0x7FEFFFFF) << np.uint64(32)) | low[kind == 4]
        bits[other, kind == 5] = (np.uint64(0xFFEFFFFF) << np.uint64(32)) | low[kind == 5]
    return x


def _same_bits(got, want, what):
    nan = np.isnan(want)                     # (IEEE 754 leaves the payload and sign of a produced NaN to the implementation)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), \
        (what, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)))


@pytest.mark.parametrize("world", [1, 2, 8, 9, 16])
def test_gather_with_up_to_16_ranks(world, monkeypatch):
    """reduce_gather in ONE process with ONE live rank: the other ranks' granule buffers ([parity][col][half], include/
    cfmm_amd.h) are written by the test under the tags of the two coming launches, so nothing ever waits.  The output must be
    the rank-ordered sum bit for bit -- both peer passes (p >= 8), own rank on either side of 8, sequence numbers across the
    tag's wrap at 2^32 - 1 -- on a device output (cfmm_sweep_dev) and on host granules (cfmm_eval), and the live rank's own
    buffer must afterwards hold its local columns under the right tag and parity."""
    import torch
    monkeypatch.setenv("CFMM_AMD_PEER_TIMEOUT_S", "2")      # a wrong tag ends as NaN at once instead of a long wait
    n = 20
    n1 = n + 1
    batches, v, Ai0 = _market(n, 5_000, seed=900)
    be = _backend(n, batches, alternate=0, armed=0)
    try:
        seg = be.ctx.segments()
        rows = seg[0]["grid"]
        assert rows == -(-seg[0]["m"] // 512) and rows > 8 and seg[0]["block"] == 512
        be.ctx.set_peers([], 0, 0, 0)                        # sharding off: this rank's own columns
        psi, acc, D, L = _check_every_path(be, n, v, Ai0, f"gather world={world}: local", bit_equal=True, ill=batches)
        local = np.concatenate([psi, [acc]])
        done = []
        for rank in sorted({0, 7, 8, world - 1} & set(range(world))):
            for k, s0 in enumerate(SEQS):
                seq = [s0 + 1, s0 + 2]                       # the two launches behind set_peers(seq = s0)
                pay = [_payloads(world, n1, 1000 + 16 * k + rank, True, rank), _payloads(world, n1, 2000 + 16 * k + rank, False, rank)]
                want = []
                host = np.zeros((world, 2, n1, 2), dtype=np.uint64)
                for q in range(2):
                    pay[q][rank] = local
                    want.append(rr.gather_sum(pay[q]))
                    assert seq[0] & 1 != seq[1] & 1
                    for p in range(world):
                        host[p, seq[q] & 1] = rr.granules(pay[q][p], seq[q])
                host[rank] = 0
                bufs = [torch.from_numpy(host[p].view(np.int64).copy()).cuda() for p in range(world)]
                torch.cuda.synchronize()
                be.ctx.set_peers([b.data_ptr() for b in bufs], world, rank, s0)
                pd, ad = dev_sweep(be, v, materialize=False)                 # launch s0 + 1: plain stores to d_out
                _same_bits(np.concatenate([pd, [ad]]), want[0], (world, rank, s0, "sweep_dev"))
                ph, ah = be.eval(v)                                          # launch s0 + 2: host granules
                _same_bits(np.concatenate([ph, [ah]]), want[1], (world, rank, s0, "eval"))
                if world > 1:                                                # the sum kept the high halves full of ones
                    assert {0x7FEFFFFF, 0xFFEFFFFF} <= set((want[1].view(np.uint64) >> np.uint64(32)).tolist())
                assert be.ctx.get_option("peer_seq") == s0 + 2
                torch.cuda.synchronize()
                own = bufs[rank].cpu().numpy().view(np.uint64)
                if world > 1:
                    for q in range(2):
                        assert np.array_equal(own[seq[q] & 1], rr.granules(local, seq[q])), (world, rank, s0, q)
                else:
                    assert not own.any()                                     # a world of one rank: the plain fold, no exchange
                for p in range(world):
                    if p != rank:
                        assert np.array_equal(bufs[p].cpu().numpy().view(np.uint64), host[p]), "a peer's buffer was written"
                done.append((rank, s0))
        be.ctx.set_peers([], 0, 0, 0)
        print(f"[reduction] gather world={world} n+1={n1} rows={rows}: {len(done)} (rank, seq) cases x 2 launches bit-equal: "
              f"ranks {sorted({r for r, _ in done})} seqs {SEQS}")
    finally:
        be.close()
