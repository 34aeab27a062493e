"""Chain-data intake: on-chain pool state -> the pool batches of a Router.

The reference constructs its pools by hand in Julia (`examples/*.jl`); it has no loader.  Real markets arrive as
snapshots of contract state: raw integer reserves, token decimals, fees in basis points or pips, and -- for
concentrated liquidity -- `sqrtPriceX96`, the initialized ticks and their `liquidityNet`.  This module converts one
such snapshot (JSON lines, one pool per line; integers may be decimal strings, as RPC clients deliver them) into
the package's `PoolBatch`es, in human units, with the token universe numbered in order of first appearance.

One line per pool:

    {"type": "constant_product", "tokens": ["0xA..", "0xB.."], "decimals": [18, 6],
     "reserves": ["123..", "456.."], "fee_bps": 30}                                    Uniswap-v2 style pairs
    {"type": "weighted", "tokens": [...], "decimals": [...], "balances": [...],
     "weights": [0.8, 0.2], "fee": 0.001}                                              Balancer-style 2-token pools
                                     (3..8 tokens: one GeometricMean batch per token count, weights normalised)
    {"type": "curve", "tokens": [...], "decimals": [...], "balances": [...], "A": 200,
     "fee": 0.0004}                                                                     StableSwap pools, 2..8 tokens
    {"type": "solidly_stable", "tokens": ["0xA..", "0xB.."], "decimals": [18, 6],
     "reserves": ["123..", "456.."], "fee_bps": 5}                                     Solidly-family stable pairs
                                     (Velodrome, Aerodrome, ...: x³y + xy³ on the decimal-normalised balances)
    {"type": "concentrated", "tokens": [token0, token1], "decimals": [d0, d1], "fee_pips": 3000,
     "sqrt_price_x96": "...", "liquidity": "...", "ticks": [[index, liquidity_net], ...]}   Uniswap-v3 style pools

Fees: exactly one of "fee" (fraction), "fee_bps" (1e-4) or "fee_pips" (1e-6); γ = 1 − fee.

StableSwap -> the reference's `Curve(R, γ, Ai, α, β)` (src/cfmms.jl:66-70), one batch per token count: D is the
invariant of the balances (StableSwap's Newton iteration, float64), α = A·nⁿ and β = D^{n+1}/nⁿ, so that
φ(R) = α·ΣR − β·ΠR⁻¹ is the invariant with D held fixed.  "A" is the amplification coefficient itself (contracts that
store A·nⁿ⁻¹ or A·100 must be converted by the caller).  The fee is charged on the input like every family here
(γ = 1 − fee), not on the output as the contracts do (which also grows D).

Concentrated liquidity -> the reference's `UniV3(current_price, lower_ticks, liquidity, γ, Ai)` (src/cfmms.jl:226-245):
  * price = amount of token1 per token0 = (sqrtPriceX96 / 2^96)², in human units × 10^(d0 − d1); the reference's
    coin 1 is token0 and coin 2 is token1 (`curr_price = (R₂+β)/(R₁+α)`, :283);
  * between two adjacent initialized ticks t_j < t_{j+1} the active liquidity is L_j = Σ_{i ≤ j} liquidityNet_i; the
    reference's per-interval `liquidity` is k = L² (`α = sqrt(k/p₊)`, `β = sqrt(k·p₋)`, :294-300), in human units
    L² / 10^(d0 + d1);
  * the reference lists, in DESCENDING order, the UPPER price of every interval (`tick_high_price`, :249; the field is
    called `lower_ticks`), the last interval reaching down to price 0 (:252-257): one entry per pair of adjacent
    initialized ticks, plus an empty interval below the lowest tick (and one above the highest when the pool's price
    sits there).
"""
from __future__ import annotations

import json
from fractions import Fraction

import numpy as np

from ._lib import ArgumentError
from .cfmms import MAX_COINS, Curve, GeometricMean, GeometricMeanTwoCoin, ProductTwoCoin, SolidlyStableTwoCoin, UniV3

Q96 = 1 << 96
TICK_BASE = 1.0001


def _int(x, what):
    try:
        return int(x)
    except (TypeError, ValueError):
        raise ArgumentError(f"{what}: not an integer: {x!r}") from None


def _gamma(rec, where):
    keys = [k for k in ("fee", "fee_bps", "fee_pips") if k in rec]
    if len(keys) != 1:
        raise ArgumentError(f"{where}: give exactly one of fee / fee_bps / fee_pips")
    fee = float(rec[keys[0]]) * {"fee": 1.0, "fee_bps": 1e-4, "fee_pips": 1e-6}[keys[0]]
    if not 0.0 <= fee < 1.0:
        raise ArgumentError(f"{where}: fee {fee} outside [0, 1)")
    return 1.0 - fee


def _amount(raw, decimals, where):
    v = _int(raw, where)
    if v <= 0:
        raise ArgumentError(f"{where}: reserves must be > 0")
    return float(Fraction(v, 10 ** int(decimals)))          # exact rational, one rounding


def tick_price(index, d0=0, d1=0):
    """Price (token1 per token0, human units) at a tick index: 1.0001^index · 10^(d0 − d1)."""
    return TICK_BASE ** int(index) * 10.0 ** (int(d0) - int(d1))


def concentrated_to_univ3(sqrt_price_x96, ticks, d0, d1, liquidity=None, where="pool"):
    """-> (current_price, upper_prices descending, k per interval) in the reference's UniV3 parametrisation."""
    s = _int(sqrt_price_x96, where + ".sqrt_price_x96")
    if s <= 0:
        raise ArgumentError(f"{where}: sqrt_price_x96 must be > 0")
    scale = 10.0 ** (int(d0) - int(d1))
    price = float(Fraction(s * s, Q96 * Q96)) * scale
    init = sorted((int(t), _int(net, where + ".ticks")) for t, net in ticks)
    if len(init) < 2:
        raise ArgumentError(f"{where}: at least two initialized ticks are needed")
    if any(a[0] == b[0] for a, b in zip(init, init[1:])):
        raise ArgumentError(f"{where}: duplicate tick index")
    L, active = [], 0
    for t, net in init[:-1]:
        active += net
        if active < 0:
            raise ArgumentError(f"{where}: liquidityNet sums to a negative liquidity at tick {t}")
        L.append(active)
    if active + init[-1][1] != 0:
        raise ArgumentError(f"{where}: liquidityNet does not sum to zero over the initialized ticks")
    unit = 10.0 ** (-(int(d0) + int(d1)))
    uppers = [tick_price(t, d0, d1) for t, _ in init[1:]]          # upper price of interval j = price at t_{j+1}
    ks = [float(l) * float(l) * unit for l in L]
    uppers, ks = uppers[::-1], ks[::-1]                             # descending, as the reference stores them
    uppers.append(tick_price(init[0][0], d0, d1))                   # below the lowest tick: empty, down to price 0
    ks.append(0.0)
    if price > uppers[0]:                                           # above the highest tick: empty as well
        uppers.insert(0, price * TICK_BASE)
        ks.insert(0, 0.0)
    if liquidity is not None:                                       # cross-check against the pool's own `liquidity` slot
        want = float(_int(liquidity, where + ".liquidity")) ** 2 * unit
        idx = int(np.searchsorted(-np.asarray(uppers), -price, side="right")) - 1   # searchsortedlast(rev=true), 0-based
        have = ks[max(idx, 0)]
        if abs(have - want) > 1e-9 * max(have, want, 1e-300):
            raise ArgumentError(f"{where}: active liquidity {want:g} (liquidity slot) does not match the ticks ({have:g})")
    return price, uppers, ks


def load_snapshot(source):
    """source: path to a JSON-lines file, or an iterable of dicts / JSON strings.
    -> (tokens, batches): the token identifiers in index order (index k+1 is the reference's 1-based token id) and the
    pool batches [ProductTwoCoin..., GeometricMeanTwoCoin..., UniV3..., SolidlyStableTwoCoin..., then the N-coin
    families] (families that do not occur are omitted)."""
    if isinstance(source, (str, bytes)):
        with open(source) as f:
            records = [json.loads(line) for line in f if line.strip() and not line.lstrip().startswith("#")]
    else:
        records = [json.loads(r) if isinstance(r, (str, bytes)) else r for r in source]
    tokens, index = [], {}

    def tid(name):
        if name not in index:
            index[name] = len(tokens) + 1
            tokens.append(name)
        return index[name]

    prod, geo, conc, multi, curve, solid = [], [], [], {}, {}, []
    for k, rec in enumerate(records):
        where = f"pool {k}"
        toks = rec.get("tokens")
        if rec.get("type") == "curve":
            c = _curve(rec, toks, tid, where)
            curve.setdefault(len(c[0]), []).append(c)
            continue
        if rec.get("type") == "weighted" and isinstance(toks, (list, tuple)) and 3 <= len(toks) <= MAX_COINS:
            multi.setdefault(len(toks), []).append(_weighted_n(rec, toks, tid, where))
            continue
        if not isinstance(toks, (list, tuple)) or len(toks) != 2 or toks[0] == toks[1]:
            raise ArgumentError(f"{where}: tokens must be two distinct identifiers")
        dec = rec.get("decimals", [18, 18])
        if len(dec) != 2:
            raise ArgumentError(f"{where}: decimals must have two entries")
        ai = [tid(toks[0]), tid(toks[1])]
        g = _gamma(rec, where)
        kind = rec.get("type")
        if kind == "constant_product":
            r = rec.get("reserves")
            prod.append(([_amount(r[0], dec[0], where), _amount(r[1], dec[1], where)], g, ai))
        elif kind == "solidly_stable":
            # whole-token amounts: the normalisation these contracts apply before they evaluate x³y + xy³
            r = rec.get("reserves")
            if r is None or len(r) != 2:
                raise ArgumentError(f"{where}: reserves must have two entries")
            solid.append(([_amount(r[0], dec[0], where), _amount(r[1], dec[1], where)], g, ai))
        elif kind == "weighted":
            r, w = rec.get("balances"), [float(x) for x in rec.get("weights", ())]
            if len(w) != 2 or min(w) <= 0:
                raise ArgumentError(f"{where}: two positive weights are needed")
            tot = w[0] + w[1]
            geo.append(([_amount(r[0], dec[0], where), _amount(r[1], dec[1], where)], [w[0] / tot, w[1] / tot], g, ai))
        elif kind == "concentrated":
            p, up, ks = concentrated_to_univ3(rec.get("sqrt_price_x96"), rec.get("ticks", ()), dec[0], dec[1],
                                              rec.get("liquidity"), where)
            conc.append((p, up, ks, g, ai))
        else:
            raise ArgumentError(f"{where}: unknown pool type {kind!r}")
    batches = []
    if prod:
        batches.append(ProductTwoCoin.batch([p[0] for p in prod], [p[1] for p in prod], [p[2] for p in prod]))
    if geo:
        batches.append(GeometricMeanTwoCoin.batch([p[0] for p in geo], [p[1] for p in geo], [p[2] for p in geo],
                                                  [p[3] for p in geo]))
    if conc:
        off = np.zeros(len(conc) + 1, dtype=np.int64)
        np.cumsum([len(c[1]) for c in conc], out=off[1:])
        batches.append(UniV3.batch([c[0] for c in conc], off, np.concatenate([c[1] for c in conc]),
                                   np.concatenate([c[2] for c in conc]), [c[3] for c in conc], [c[4] for c in conc]))
    if solid:
        batches.append(SolidlyStableTwoCoin.batch([p[0] for p in solid], [p[1] for p in solid], [p[2] for p in solid]))
    for n in sorted(multi):   # 3..8-token weighted pools: one batch per coin count (GeometricMean, src/cfmms.jl:60-63)
        pools = multi[n]
        batches.append(GeometricMean.batch([p[0] for p in pools], [p[1] for p in pools], [p[2] for p in pools],
                                           [p[3] for p in pools]))
    for n in sorted(curve):   # StableSwap pools: one Curve batch per coin count
        pools = curve[n]
        batches.append(Curve.batch(*[[p[j] for p in pools] for j in range(5)]))
    return tokens, batches


def snapshot_delta(old, new, ladders=False):
    """What moved between two snapshots of the SAME pool set: `old` and `new` are `load_snapshot` results (or their batch
    lists).  -> {position: new state} for the pools whose state differs, in the form `update_pools_(router, changes)` takes
    for a router built from these batches: position = the pool's index in the concatenated batches; state = a reserve vector,
    `(R, α, β)` for Curve, the price for concentrated-liquidity pools.  Anything else that differs -- the pool set, a pool's
    family, tokens, fee, weights or tick ladder -- is a structural change (a re-upload): ArgumentError naming the pool.
    ladders=True: a concentrated-liquidity pool whose tick ladder differs (a mint, a burn) is a change like any other; its
    state is `(price, lower_ticks, liquidity)`, the pool's whole new ladder (cfmm_pools_set_ticks)."""
    def batches_of(snap):
        if isinstance(snap, tuple) and len(snap) == 2 and not hasattr(snap[0], "kind"):
            return snap[0], list(snap[1])
        return None, list(snap)

    (tok_a, a), (tok_b, b) = batches_of(old), batches_of(new)
    if len(a) != len(b) or any(x.kind != y.kind or len(x) != len(y) or x.Ai.shape != y.Ai.shape for x, y in zip(a, b)):
        raise ArgumentError("the snapshots hold different pool sets (pools per family: "
                            f"{[len(x) for x in a]} vs {[len(y) for y in b]})")
    changes, base = {}, 0
    for x, y in zip(a, b):
        # tokens: by identifier when the snapshots carry them (the numbering follows first appearance and may shift), else by index
        if tok_a is not None and tok_b is not None:
            same_tok = np.asarray(tok_a, dtype=object)[x.Ai - 1] == np.asarray(tok_b, dtype=object)[y.Ai - 1]
        else:
            same_tok = x.Ai == y.Ai
        fixed = [("tokens", ~same_tok), ("fee", x.γ != y.γ)] + ([("weights", x.w != y.w)] if hasattr(x, "w") else [])
        for what, differs in fixed:
            bad = np.nonzero(np.any(np.asarray(differs).reshape(len(x), -1), axis=1))[0]
            if bad.size:
                raise ArgumentError(f"pool {base + int(bad[0])}: {what} changed between the snapshots (a structural change: re-upload)")
        if hasattr(x, "tick_off"):
            nt = np.diff(x.tick_off)
            same = np.diff(y.tick_off) == nt                        # per pool: the same tick count ...
            px, py = np.repeat(np.arange(len(x)), nt), np.repeat(np.arange(len(y)), np.diff(y.tick_off))
            kx, ky = same[px], same[py]                             # ... and, tick by tick, the same prices and liquidity
            diff = (x.lower_ticks[kx] != y.lower_ticks[ky]) | (x.liquidity[kx] != y.liquidity[ky])
            same &= np.bincount(px[kx][diff], minlength=len(x)) == 0
            if not same.all() and ladders:
                for i in np.nonzero(~same)[0]:
                    o, e = y.tick_off[i], y.tick_off[i + 1]
                    changes[base + int(i)] = (float(y.current_price[i]), y.lower_ticks[o:e].copy(), y.liquidity[o:e].copy())
            elif not same.all():
                raise ArgumentError(f"pool {base + int(np.nonzero(~same)[0][0])}: tick ladder changed between the snapshots "
                                    "(a mint / burn is a structural change: re-upload)")
            for i in np.nonzero((x.current_price != y.current_price) & same)[0]:
                changes[base + int(i)] = float(y.current_price[i])
        else:
            moved = np.any(x.R != y.R, axis=1)
            if hasattr(x, "α"):
                moved |= (x.α != y.α) | (x.β != y.β)
            for i in np.nonzero(moved)[0]:
                changes[base + int(i)] = (y.R[i].copy(), float(y.α[i]), float(y.β[i])) if hasattr(x, "α") else y.R[i].copy()
        base += len(x)
    return changes


def stableswap_D(x, A):
    """StableSwap's invariant D of balances x [..., n] at amplification A [...]: the root of
    A·nⁿ·Σx + D = A·D·nⁿ + D^{n+1}/(nⁿ·Πx), by the contracts' own Newton iteration in float64 (vectorised)."""
    x = np.asarray(x, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n = x.shape[-1]
    S = x.sum(axis=-1)
    Ann = A * n ** n
    D = S.copy()
    for _ in range(255):
        DP = D.copy()
        for k in range(n):
            DP = DP * D / (n * x[..., k])
        Dn = (Ann * S + DP * n) * D / ((Ann - 1.0) * D + (n + 1) * DP)
        done = np.all(np.abs(Dn - D) <= 4 * np.finfo(float).eps * Dn)
        D = Dn
        if done:
            break
    return D


def stableswap_params(x, A):
    """(α, β) of Curve for a StableSwap pool with balances x [..., n] and amplification A: α = A·nⁿ, β = D^{n+1}/nⁿ."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    D = stableswap_D(x, A)
    return np.asarray(A, dtype=np.float64) * n ** n, D ** (n + 1) / n ** n


def _curve(rec, toks, tid, where):
    """one "curve" record with 2..8 tokens -> (R, γ, Ai, α, β)"""
    if not isinstance(toks, (list, tuple)) or not 2 <= len(toks) <= MAX_COINS or len(set(toks)) != len(toks):
        raise ArgumentError(f"{where}: tokens must be 2..{MAX_COINS} distinct identifiers")
    n = len(toks)
    dec = rec.get("decimals", [18] * n)
    if len(dec) != n:
        raise ArgumentError(f"{where}: decimals must have {n} entries")
    r = rec.get("balances")
    if r is None or len(r) != n:
        raise ArgumentError(f"{where}: balances must have {n} entries")
    A = rec.get("A")
    if A is None or not np.isfinite(float(A)) or float(A) < 0:
        raise ArgumentError(f"{where}: the amplification A must be a finite number >= 0")
    g = _gamma(rec, where)
    R = [_amount(r[i], dec[i], where) for i in range(n)]
    al, be = stableswap_params(R, float(A))
    return R, g, [tid(t) for t in toks], float(al), float(be)


def _weighted_n(rec, toks, tid, where):
    """one weighted record with 3..8 tokens -> (R, w normalised, γ, Ai)"""
    n = len(toks)
    if len(set(toks)) != n:
        raise ArgumentError(f"{where}: tokens must be distinct identifiers")
    dec = rec.get("decimals", [18] * n)
    if len(dec) != n:
        raise ArgumentError(f"{where}: decimals must have {n} entries")
    r, w = rec.get("balances"), [float(x) for x in rec.get("weights", ())]
    if r is None or len(r) != n:
        raise ArgumentError(f"{where}: balances must have {n} entries")
    if len(w) != n or min(w) <= 0:
        raise ArgumentError(f"{where}: {n} positive weights are needed")
    g = _gamma(rec, where)
    tot = sum(w)
    return ([_amount(r[i], dec[i], where) for i in range(n)], [x / tot for x in w], g, [tid(t) for t in toks])
