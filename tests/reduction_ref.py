"""The one reference for the REDUCTION of a sweep's trades -- Ψ (per-token netflows) and the dual scalar acc -- and the
ill-scaled markets that make a wrong reduction visible.

What route! consumes is not the trades but their sums, formed on the device by a chain of hand-written pieces (the LDS bin
scatter, finish_row, the direct publish, reduce_partials, reduce_gather, gather_chunks / token_fold).  A correct sum in ANY
order of c nonzero terms t stays within

    |s − fsum(t)|  <=  (c + 2) · u · Σ|t|,      u = 2⁻⁵³

(c − 1 additions, each rounding a partial sum bounded by Σ|t|, plus the rounding of forming each term: Λ − Δ for Ψ, Λ·v and
Δ·v for acc).  Nothing here is fitted to what the kernels return: a token without a nonzero flow must be +0.0, a token with
one nonzero flow must be that flow bit for bit, everything else must meet the bound.  max-error over max-|Ψ|
(helpers.rel_to_max) cannot see a flow that is dropped, doubled or booked on the wrong token when the token is 10⁻¹³ of the
market's largest -- tests/test_reduction_exact_cpu.py puts numbers on that.
"""
import math

import numpy as np

from cfmmrouter_amd import synth

U = 2.0 ** -53


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def token_terms(D, L, Ai0, n):
    """Flows Λ − Δ grouped by token: (flows sorted by token, starts [n + 1]); token j owns fs[starts[j]:starts[j + 1]]."""
    f = np.ravel(np.asarray(L, dtype=np.float64)) - np.ravel(np.asarray(D, dtype=np.float64))
    idx = np.ravel(np.asarray(Ai0)).astype(np.int64)
    assert f.size == idx.size and (idx.size == 0 or (idx.min() >= 0 and idx.max() < n))
    order = np.argsort(idx, kind="stable")
    return f[order], np.searchsorted(idx[order], np.arange(n + 1))


def reduction_report(D, L, Ai0, v, n, psi, acc):
    """-> (failures, worst): the violations as strings and the largest |error| / bound over the tokens (and acc) that are
    held to the bound (c >= 2): the margin the reduction really has -- a record, never a threshold."""
    psi = np.asarray(psi, dtype=np.float64)
    assert psi.shape == (n,)
    fs, starts = token_terms(D, L, Ai0, n)
    nz = fs != 0.0                                          # (NaN counts as a term)
    cnt = np.add.reduceat(np.concatenate([nz, [False]]).astype(np.int64), starts[:-1]) * (np.diff(starts) > 0)
    deg = np.diff(starts)
    fails, worst = [], 0.0
    for j in np.flatnonzero(cnt == 0):
        if psi[j] != 0.0 or np.signbit(psi[j]):
            fails.append(f"token {j} (degree {deg[j]}, no nonzero flow): psi = {psi[j]!r}, expected +0.0")
    for j in np.flatnonzero(cnt == 1):
        t = fs[starts[j]:starts[j + 1]]
        one = t[t != 0.0][0]
        if _bits(psi[j]) != _bits(one):
            fails.append(f"token {j} (degree {deg[j]}, one nonzero flow): psi = {psi[j]!r} is not the flow {one!r} bit for bit")
    for j in np.flatnonzero(cnt >= 2):
        t = fs[starts[j]:starts[j + 1]]
        bound = (cnt[j] + 2) * U * float(np.sum(np.abs(t)))
        err = abs(psi[j] - math.fsum(t))
        frac = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        if not frac <= 1.0:
            fails.append(f"token {j} (degree {deg[j]}, {cnt[j]} nonzero flows): |psi - fsum| = {err:.3e} = {frac:.3g} x bound")
        worst = max(worst, frac) if frac == frac else math.inf
    vl = np.asarray(v, dtype=np.float64)[np.ravel(Ai0)]
    terms = np.concatenate([np.ravel(L) * vl, -(np.ravel(D) * vl)])
    bound = (np.count_nonzero(terms) + 2) * U * float(np.sum(np.abs(terms)))
    err = abs(float(acc) - math.fsum(terms))
    frac = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    if not frac <= 1.0:
        fails.append(f"acc ({np.count_nonzero(terms)} nonzero terms): |acc - fsum| = {err:.3e} = {frac:.3g} x bound")
    worst = max(worst, frac) if frac == frac else math.inf
    return fails, worst


def assert_reduction_exact(D, L, Ai0, v, n, psi, acc, geometry=None):
    """Ψ / acc against the exact sums of the flat per-entry trades D, L (entry k belongs to token Ai0[k]; any family, two-coin
    or N-coin).  `geometry`: what to name in a failure (ctx.segments() and the like).  Returns the worst |error| / bound."""
    fails, worst = reduction_report(D, L, Ai0, v, n, psi, acc)
    assert not fails, f"{len(fails)} reduction violations, geometry {geometry}:\n  " + "\n  ".join(fails[:12])
    return worst


# ---- ill-scaled markets ---------------------------------------------------------------------------------------------------

HUB = 0   # the numeraire: token 0, at the top of the scale


def token_exponents(n, seed, lo=-40, hi=40):
    """Token j's amounts live at scale 2^e[j]: e spread over [lo, hi], the numeraire at the top."""
    e = np.floor(lo + (hi - lo + 1) * synth.uniform(seed, 200, n)).astype(np.int64).clip(lo, hi)
    e[HUB] = hi
    return e


def prescribed_pairs(n, degrees, hub_degree, seed):
    """Token pairs (1-based [m, 2]) in which token j != HUB is in exactly degrees[j] pools and the hub in about hub_degree:
    the tokens' stubs are shuffled, the first hub_degree of them meet the hub, the rest meet each other in order (two stubs of
    one token: both go to the hub instead).  Which side a token takes is drawn per pool."""
    degrees = np.asarray(degrees, dtype=np.int64).copy()
    degrees[HUB] = 0
    stubs = np.repeat(np.arange(n), degrees)
    stubs = stubs[np.argsort(synth.uniform(seed, 201, stubs.size), kind="stable")]
    h = min(int(hub_degree), stubs.size)
    h += (stubs.size - h) & 1
    h = min(h, stubs.size)
    a, b = stubs[h::2], stubs[h + 1::2]
    assert a.size == b.size
    same = a == b
    first = np.concatenate([stubs[:h], a[same], b[same], a[~same]])
    second = np.concatenate([np.full(h + 2 * int(same.sum()), HUB), b[~same]])
    flip = synth.uniform(seed, 202, first.size) < 0.5
    Ai = np.where(flip[:, None], np.stack([second, first], axis=1), np.stack([first, second], axis=1))
    Ai = Ai[np.argsort(synth.uniform(seed, 203, first.size), kind="stable")]
    got = np.bincount(Ai.ravel(), minlength=n)
    assert np.array_equal(np.delete(got, HUB), np.delete(degrees, HUB))
    return Ai + 1


def rescale(batch, Ai, e):
    """`batch` (a synth two-coin batch of len(Ai) pools) on the token pairs Ai with token j's amounts scaled by 2^e[j]:
    reserves per side, UniV3 prices by 2^(e₂ − e₁) and invariants by 2^(e₁ + e₂).  Powers of two: the pools trade as before."""
    from cfmmrouter_amd._lib import KIND_UNIV3
    assert len(batch) == len(Ai)
    batch.Ai = np.ascontiguousarray(Ai, dtype=np.int64)
    ea = e[batch.Ai - 1].astype(np.float64)
    if batch.kind == KIND_UNIV3:
        nt = np.diff(batch.tick_off)
        batch.current_price = batch.current_price * 2.0 ** (ea[:, 1] - ea[:, 0])
        batch.lower_ticks = batch.lower_ticks * np.repeat(2.0 ** (ea[:, 1] - ea[:, 0]), nt)
        batch.liquidity = batch.liquidity * np.repeat(2.0 ** (ea[:, 0] + ea[:, 1]), nt)
    else:
        batch.R = batch.R * 2.0 ** ea
    return batch


def tame_weights(b):
    """GeometricMean weights into [0.4, 0.6]: the pool's closed form raises price ratios to η = w₁/w₂, and ratios of 2^80
    to the power 49 leave the double range (in the reference's own arithmetic as well)."""
    w1 = 0.4 + 0.2 * b.w[:, 0]
    b.w = np.stack([w1, 1.0 - w1], axis=1)
    return b


def ill_prices(n, e, seed, spread=0.2):
    """Prices inverse to the scales, so that every pool sees the price ratios of an ordinary market."""
    return synth.sweep_prices(n, seed=seed, spread=spread) * 2.0 ** (-e.astype(np.float64))


def default_degrees(n, seed, typical=12, special=(0, 1, 1, 0, 1, 2, 3)):
    """Degrees for the non-hub tokens: about `typical` each, with `special` on tokens 1.. (degree 0 and 1 among them)."""
    d = 1 + np.floor(2 * (typical - 1) * synth.uniform(seed, 204, n)).astype(np.int64)
    d[1:1 + len(special)] = special
    return d


def ill_scaled_market(n, degrees, hub_degree, seed, families=("product",), ticks=4, bottom=-40, n_bottom=3):
    """-> (batches, v, e): a market on prescribed token degrees whose tokens span 2^-40 .. 2^40, split evenly over
    `families` ("product" / "geomean" / "univ3"), the first n_bottom tokens after the hub pinned to scale 2^bottom."""
    e = token_exponents(n, seed)
    e[1:1 + n_bottom] = bottom                             # the degree-0 / degree-1 tokens sit 2^80 below the hub
    Ai = prescribed_pairs(n, degrees, hub_degree, seed)
    m = len(Ai)
    cuts = [m * k // len(families) for k in range(len(families) + 1)]
    batches = []
    for k, fam in enumerate(families):
        lo, hi = cuts[k], cuts[k + 1]
        if fam == "product":
            b = synth.product_pools(hi - lo, n, seed=seed + 10 * k)
        elif fam == "geomean":
            b = synth.geomean_pools(hi - lo, n, seed=seed + 10 * k)
            tame_weights(b)
        else:
            b = synth.univ3_pools(hi - lo, n, ticks, seed=seed + 10 * k)
        batches.append(rescale(b, Ai[lo:hi], e))
    return batches, ill_prices(n, e, seed + 1), e


def flat_tokens(batches):
    """0-based token of every flat trade entry, in packed (segment) order."""
    return np.concatenate([(b.Ai - 1).ravel() for b in batches])


def assert_ill_scaled(D, L, Ai0, n, batches):
    """The market is what the tests need: most pools trade, there are tokens without a flow and with exactly one, the token
    scales span 2^60, and every reserve sits inside the window of the fast arithmetic [2^-150, 2^150]."""
    fs, starts = token_terms(D, L, Ai0, n)
    mass = np.add.reduceat(np.concatenate([np.abs(fs), [0.0]]), starts[:-1]) * (np.diff(starts) > 0)
    cnt = np.add.reduceat(np.concatenate([fs != 0.0, [False]]).astype(np.int64), starts[:-1]) * (np.diff(starts) > 0)
    trading = np.any(np.reshape(np.asarray(L, dtype=np.float64), (-1, 2)) != 0.0, axis=1)
    assert np.mean(trading) >= 0.5, np.mean(trading)
    assert np.any(np.diff(starts) == 0) and np.any(cnt == 0) and np.any(cnt == 1)
    assert np.any(np.diff(starts) == 1)
    assert mass.max() / mass[mass > 0].min() >= 2.0 ** 60
    for b in batches:
        for name in ("R", "liquidity", "lower_ticks", "current_price"):
            x = getattr(b, name, None)
            if x is not None:
                x = x[x != 0.0]
                assert x.min() >= 2.0 ** -150 and x.max() <= 2.0 ** 150, name
    return cnt


# ---- the fold's geometry and the gather's arithmetic, restated -----------------------------------------------------------

REDUCE_COLS = 8


def fold_colblock(b):
    """fold_kernels.h: block b -> column group.  The two groups of one 128-byte line go to two blocks of the same XCD."""
    x, q = b & 7, b >> 3
    return 2 * (x + 8 * (q >> 1)) + (q & 1)


def fold_grid(n1):
    groups = (n1 + REDUCE_COLS - 1) // REDUCE_COLS
    pairs = (groups + 1) // 2
    return 16 * ((pairs + 7) // 8)


def gather_tag(seq):
    """The 32-bit tag of the launch with sequence number seq (never 0 = an empty buffer) -- seq is what the launch uses,
    i.e. one more than the number handed to cfmm_set_peers before it."""
    return seq % 0xFFFFFFFF + 1


def gather_sum(columns):
    """The rank-ordered sum of reduce_gather: columns [world, n1] -> [n1], s = 0.0; for p: s += x[p]."""
    s = np.zeros(np.shape(columns)[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for x in np.asarray(columns, dtype=np.float64):
            s = s + x
    return s


def granules(values, seq):
    """One parity's granules of `values` [n1] under the tag of launch seq: [n1, 2] uint64 {tag, low half}, {tag, high half}."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    tag = np.uint64(gather_tag(seq)) << np.uint64(32)
    return np.stack([tag | (bits & np.uint64(0xFFFFFFFF)), tag | (bits >> np.uint64(32))], axis=1)


# ---- the plan's bin-copy rule, restated (launch_plan.cpp: bin_copies, stage_pairs; sweep.h: sweep_lds_bytes) ---------------

def lds_words(n_pad, copies, block, need_logv, gtab_n, stage_y):
    return n_pad * ((2 if stage_y else 1) + (1 if need_logv else 0) + copies) + 2 * gtab_n + 2 * (block // 64) + 2


def planned_copies(n, option, block):
    """launch_plan.cpp's rule (bin_copies): private copies while the blocks of the geometry fit a CU's LDS together."""
    n_pad = (n + 1) & ~1
    waves = block // 64
    stage_y = 8 * lds_words(n_pad, 1, block, 1, 256, 1) <= 160 * 1024
    per_wave = 8 * lds_words(n_pad, waves, block, 1, 256, stage_y)
    if n > 8192 or option == 1:
        return 1
    if option == 2:
        return waves if per_wave <= 160 * 1024 else 1
    return waves if per_wave <= (128 if block == 1024 else 64) * 1024 else 1


def auto_threshold(block):
    lo, hi = 2, 8192                         # copies(lo) == waves, copies(hi) == 1: bisect the rule
    assert planned_copies(lo, 0, block) == block // 64 and planned_copies(hi, 0, block) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if planned_copies(mid, 0, block) > 1 else (lo, mid)
    return lo
