"""Host-side mirror of the reference's pool types (src/cfmms.jl).

Same names, same constructor arguments, same error behaviour as the Julia structs, so code and
tests written against the reference read the same here:

    ProductTwoCoin(R, γ, idx)                src/cfmms.jl:101-111
    GeometricMeanTwoCoin(R, w, γ, idx)       src/cfmms.jl:152-165
    UniV3(current_price, lower_ticks, liquidity, γ, Ai)   src/cfmms.jl:226-245
    GeometricMean(R, w, γ, Ai), Product(R, γ, Ai)        src/cfmms.jl:57-64 (2..8 coins; the reference declares
                                                         them without a find_arb!, the device solves them exactly)
    Curve(R, γ, Ai, α, β)                    src/cfmms.jl:66-70 (2..8 coins, φ = α·ΣR − β·ΠR⁻¹: StableSwap at
                                             fixed D; no find_arb! in the reference either)
    SolidlyStableTwoCoin(R, γ, idx)          the Solidly family's stable pair, φ = R₁³R₂ + R₁R₂³ (not in the
                                             reference; ProductTwoCoin's constructor, closed-form find_arb!)

Token indices are 1-BASED, exactly as in the reference (`Ai[j]` is the global id of the pool's
j-th coin); they are converted to 0-based int32 once, when a Router packs the pools for the
device.  The objects here hold data only: all arithmetic of `find_arb!` happens on the GPU
through the C ABI (`find_arb_(Δ, Λ, cfmm, v)` below is a one-pool device sweep).

For large markets, building m Python objects is the slow part, so every family also has a
structure-of-arrays batch (`ProductTwoCoin.batch(R[m,2], γ[m], idx[m,2])` ...) that a Router
accepts directly; `batch[i]` materialises the i-th pool object on demand.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from ._lib import KIND_CURVE, KIND_GEOMEAN, KIND_PRODUCT, KIND_SOLIDLY, KIND_UNIV3, KIND_WEIGHTED, ArgumentError

MAX_COINS = 8   # sweep.h kMaxCoins


class CFMM:
    """abstract type CFMM{T} -- src/cfmms.jl:5"""

    kind = -1

    def __len__(self):  # Base.length(c::CFMM) = length(c.Ai), src/cfmms.jl:19
        return len(self.Ai)


class _FeePool(CFMM):
    """The built-in pool types (a user's own CFMM subclass names its fields as it likes): `gamma` reads the fee γ."""

    gamma = property(lambda self: self.γ)


def _two_coin_check_cast(R, γ, idx):
    """two_coin_check_cast -- src/cfmms.jl:76-90"""
    R = np.asarray(R)
    idx = np.asarray(idx)
    if R.size != 2:
        raise ArgumentError("length of R must be 2 for *TwoCoin constructors")
    if idx.size != 2:
        raise ArgumentError("length of idx must be 2 for *TwoCoin constructors")
    if np.any(idx < 0):  # convert.(UInt, idx) throws InexactError on negatives
        raise ArgumentError("idx must be non-negative")
    return np.array(R, dtype=np.float64).reshape(2), float(γ), np.array(idx, dtype=np.int64).reshape(2)


class ProductTwoCoin(_FeePool):
    """ProductTwoCoin(R, γ, idx): φ(R) = R₁R₂ -- src/cfmms.jl:92-111"""

    kind = KIND_PRODUCT

    def __init__(self, R, γ, idx):
        self.R, self.γ, self.Ai = _two_coin_check_cast(R, γ, idx)

    @staticmethod
    def batch(R, γ, idx):
        return PoolBatch(KIND_PRODUCT, R=R, γ=γ, Ai=idx)


SOLIDLY_EXP_RANGE = 150   # sweep.h kFastExp: reserves of a Solidly stable pair lie within [2^-150, 2^150]


def _solidly_check(R, γ):
    """The upload's own checks of a Solidly stable pair (cfmm_pools_add_solidly): γ <= 1 and the reserve range."""
    R, γ = np.asarray(R, dtype=np.float64), np.asarray(γ, dtype=np.float64)
    if np.any(~(γ > 0)) or np.any(γ > 1):
        raise ArgumentError("fee γ must lie in (0, 1] (γ > 1 makes the arbitrage problem unbounded)")
    lo, hi = 2.0 ** -SOLIDLY_EXP_RANGE, 2.0 ** SOLIDLY_EXP_RANGE
    if R.size and not np.all((R >= lo) & (R < 2 * hi)):   # (the exponent test of the upload: [2^-150, 2^151))
        raise ArgumentError(f"reserves of a Solidly stable pair must lie within [2^-{SOLIDLY_EXP_RANGE}, 2^{SOLIDLY_EXP_RANGE}]")


class SolidlyStableTwoCoin(_FeePool):
    """SolidlyStableTwoCoin(R, γ, idx): φ(R) = R₁³R₂ + R₁R₂³, the "stable" pair of the Solidly family (Velodrome,
    Aerodrome and forks) on decimal-normalised balances.  Not in the reference; constructor of ProductTwoCoin
    (src/cfmms.jl:76-111) plus 0 < γ <= 1 and the upload's reserve range."""

    kind = KIND_SOLIDLY

    def __init__(self, R, γ, idx):
        self.R, self.γ, self.Ai = _two_coin_check_cast(R, γ, idx)
        _solidly_check(self.R, self.γ)

    @staticmethod
    def batch(R, γ, idx):
        return PoolBatch(KIND_SOLIDLY, R=R, γ=γ, Ai=idx)


class GeometricMeanTwoCoin(_FeePool):
    """GeometricMeanTwoCoin(R, w, γ, idx): φ(R) = R₁^w₁ R₂^w₂ -- src/cfmms.jl:142-165"""

    kind = KIND_GEOMEAN

    def __init__(self, R, w, γ, idx):
        self.R, self.γ, self.Ai = _two_coin_check_cast(R, γ, idx)
        w = np.array(w, dtype=np.float64)
        if w.size != 2:
            raise ArgumentError("length of w must be 2")  # SVector{2,T}(w) would throw
        self.w = w.reshape(2)

    @staticmethod
    def batch(R, w, γ, idx):
        return PoolBatch(KIND_GEOMEAN, R=R, w=w, γ=γ, Ai=idx)


def _n_coin_check_cast(R, γ, Ai, w=None, family="weighted"):
    R = np.array(R, dtype=np.float64).reshape(-1)
    Ai = np.array(Ai).reshape(-1)
    n = R.size
    if Ai.size != n:
        raise ArgumentError("length of Ai must equal length of R")
    if not 2 <= n <= MAX_COINS:
        raise ArgumentError(f"{family} pools have 2..{MAX_COINS} coins, got {n}")
    if np.any(Ai < 0):
        raise ArgumentError("Ai must be non-negative")
    if np.unique(Ai).size != n:
        raise ArgumentError("the token indices of a pool must be distinct")
    if not np.all(np.isfinite(R)) or np.any(R <= 0):
        raise ArgumentError("reserves must be finite and > 0")
    γ = float(γ)
    if not (0.0 < γ <= 1.0):
        raise ArgumentError("fee γ must lie in (0, 1] (γ > 1 makes the N-coin arbitrage problem unbounded)")
    if w is None:
        w = np.full(n, 1.0 / n)
    else:
        w = np.array(w, dtype=np.float64).reshape(-1)
        if w.size != n:
            raise ArgumentError("length of w must equal length of R")
        if not np.all(np.isfinite(w)) or np.any(w <= 0):
            raise ArgumentError("weights must be finite and > 0")
    return R, γ, Ai.astype(np.int64), w


class GeometricMean(_FeePool):
    """GeometricMean(R, w, γ, Ai): φ(R) = Π R_i^{w_i}, 2..8 coins -- src/cfmms.jl:60-63.  Argument order of
    GeometricMeanTwoCoin; the device normalises w to sum to 1 (same level sets, same trades)."""

    kind = KIND_WEIGHTED

    def __init__(self, R, w, γ, Ai):
        self.R, self.γ, self.Ai, self.w = _n_coin_check_cast(R, γ, Ai, w)

    @staticmethod
    def batch(R, w, γ, Ai):
        return PoolBatch(KIND_WEIGHTED, R=R, w=w, γ=γ, Ai=Ai)


class Product(GeometricMean):
    """Product(R, γ, Ai): φ(R) = Π R_i, 2..8 coins -- src/cfmms.jl:56-58.  The equal-weight GeometricMean: Π R_i has the
    level sets of Π R_i^{1/n}, so the trades are the same."""

    def __init__(self, R, γ, Ai):
        self.R, self.γ, self.Ai, self.w = _n_coin_check_cast(R, γ, Ai)

    @staticmethod
    def batch(R, γ, Ai):
        R = np.asarray(R, dtype=np.float64)
        return PoolBatch(KIND_WEIGHTED, R=R, w=np.full(R.shape, 1.0 / R.shape[-1]), γ=γ, Ai=Ai)


def _curve_check_cast(α, β):
    α, β = float(α), float(β)
    if not (np.isfinite(α) and α >= 0.0):
        raise ArgumentError("α must be finite and >= 0")
    if not (np.isfinite(β) and β > 0.0):
        raise ArgumentError("β must be finite and > 0")
    return α, β


CURVE_LOG_RANGE = 600.0   # curve_pool.h kCurveLogRange


def _curve_range_check(R, α, β):
    """The upload's range check (cfmm_pools_add_curve): at α > 0 every log(P₀/R_k) = log β − Σ log R − log R_k must lie
    within ±CURVE_LOG_RANGE.  R [m, n]; α, β [m]."""
    R = np.asarray(R, dtype=np.float64).reshape(np.size(β), -1)
    lr = np.log(R)
    x = (np.log(np.asarray(β, dtype=np.float64).reshape(-1)) - lr.sum(axis=1))[:, None] - lr
    if np.any((np.asarray(α).reshape(-1) > 0) & ~np.all(np.abs(x) <= CURVE_LOG_RANGE, axis=1)):
        raise ArgumentError(f"log(P₀/R_k) = log β − Σ log R − log R_k must lie within ±{CURVE_LOG_RANGE:g} when α > 0")


class Curve(_FeePool):
    """Curve(R, γ, Ai, α, β): φ(R) = α·Σ R_i − β·Π R_i⁻¹, 2..8 coins -- src/cfmms.jl:66-70 (the fields of Curve{T}, in
    the order of its default constructor).  Curve's StableSwap invariant with D held fixed: α = A·nⁿ, β = D^{n+1}/nⁿ
    (chain.stableswap_params).  α = 0 trades exactly like Product."""

    kind = KIND_CURVE

    def __init__(self, R, γ, Ai, α, β):
        self.R, self.γ, self.Ai, _ = _n_coin_check_cast(R, γ, Ai, family="Curve")
        self.α, self.β = _curve_check_cast(α, β)
        _curve_range_check(self.R[None], [self.α], [self.β])

    alpha = property(lambda self: self.α)
    beta = property(lambda self: self.β)

    @staticmethod
    def batch(R, γ, Ai, α, β):
        return PoolBatch(KIND_CURVE, R=R, γ=γ, Ai=Ai, α=α, β=β)


def ϕ(cfmm, R=None):
    """ϕ(c::CFMM; R=nothing): the trading function -- src/cfmms.jl:36-42, :113-116 (ProductTwoCoin:
    R₁R₂), :167-171 (GeometricMeanTwoCoin: R₁^w₁ R₂^w₂).  The reference defines no method for UniV3.
    Host-side definition (O(1) per pool, used by the optimality tests, not by the sweep)."""
    if not isinstance(cfmm, (ProductTwoCoin, GeometricMeanTwoCoin, GeometricMean, Curve, SolidlyStableTwoCoin)):
        raise ArgumentError("ϕ has no method for this pool type (as in the reference)")
    R = cfmm.R if R is None else np.asarray(R, dtype=np.float64)
    if isinstance(cfmm, SolidlyStableTwoCoin):
        return R[0] * R[1] * (R[0] * R[0] + R[1] * R[1])
    if isinstance(cfmm, Curve):
        return float(cfmm.α * np.sum(R) - cfmm.β / np.prod(R))
    if isinstance(cfmm, Product):
        return float(np.prod(R))
    if isinstance(cfmm, GeometricMean):
        return float(np.prod(R ** cfmm.w))
    if isinstance(cfmm, ProductTwoCoin):
        return R[0] * R[1]
    if isinstance(cfmm, GeometricMeanTwoCoin):
        return R[0] ** cfmm.w[0] * R[1] ** cfmm.w[1]
    raise ArgumentError("ϕ has no method for this pool type (as in the reference)")


def ϕ_grad_(out, cfmm, R=None):
    """∇ϕ!(x, c::CFMM; R=nothing): gradient of the trading function, stored in `out` --
    src/cfmms.jl:44-50, :117-122, :172-178."""
    if not isinstance(cfmm, (ProductTwoCoin, GeometricMeanTwoCoin, GeometricMean, Curve, SolidlyStableTwoCoin)):
        raise ArgumentError("∇ϕ! has no method for this pool type (as in the reference)")
    R = cfmm.R if R is None else np.asarray(R, dtype=np.float64)
    if isinstance(cfmm, SolidlyStableTwoCoin):
        x, y = R[0], R[1]
        out[0], out[1] = y * (3.0 * x * x + y * y), x * (x * x + 3.0 * y * y)
        return None
    if isinstance(cfmm, Curve):
        out[:] = cfmm.α + cfmm.β / np.prod(R) / R
        return None
    if isinstance(cfmm, Product):
        p = np.prod(R)
        out[:] = p / R
        return None
    if isinstance(cfmm, GeometricMean):
        out[:] = cfmm.w * np.prod(R ** cfmm.w) / R
        return None
    if isinstance(cfmm, ProductTwoCoin):
        out[0], out[1] = R[1], R[0]
        return None
    if isinstance(cfmm, GeometricMeanTwoCoin):
        w = cfmm.w
        out[0] = w[0] * (R[1] / R[0]) ** w[1]
        out[1] = w[1] * (R[0] / R[1]) ** w[0]
        return None
    raise ArgumentError("∇ϕ! has no method for this pool type (as in the reference)")


phi, grad_phi_ = ϕ, ϕ_grad_   # ASCII spellings ("∇" is not a valid Python identifier character, hence ϕ_grad_ for ∇ϕ!)


class UniV3(_FeePool):
    """UniV3(current_price, lower_ticks, liquidity, γ, Ai) -- src/cfmms.jl:206-245.

    `lower_ticks` is in decreasing order; `current_tick` is
    searchsortedlast(lower_ticks, current_price, rev=true) (:235), 1-based."""

    kind = KIND_UNIV3

    def __init__(self, current_price, lower_ticks, liquidity, γ, Ai):
        self.current_price = float(current_price)
        self.lower_ticks = np.array(lower_ticks, dtype=np.float64).reshape(-1)
        self.liquidity = np.array(liquidity, dtype=np.float64).reshape(-1)
        if self.lower_ticks.size != self.liquidity.size:
            raise ArgumentError("lower_ticks and liquidity must have the same length")
        self.γ = float(γ)
        self.Ai = np.array(Ai, dtype=np.int64).reshape(-1)
        if self.Ai.size != 2:
            raise ArgumentError("length of Ai must be 2")
        self._retick()

    def _retick(self):
        """current_tick: the number of ticks >= current_price in the descending vector (== searchsortedlast, rev=true)"""
        self.current_tick = int(np.count_nonzero(self.lower_ticks >= self.current_price))

    @staticmethod
    def batch(current_price, tick_off, lower_ticks, liquidity, γ, Ai):
        return PoolBatch(KIND_UNIV3, current_price=current_price, tick_off=tick_off,
                         lower_ticks=lower_ticks, liquidity=liquidity, γ=γ, Ai=Ai)


def BoundedProduct(current_price, p_lower, p_upper, liquidity, γ, Ai):
    """A stand-alone bounded-liquidity pool φ(R) = (R₁+α)(R₂+β) (src/cfmms.jl:261-289) on the
    price interval [p_lower, p_upper].  The reference's BoundedProduct struct is not a CFMM
    subtype and cannot enter a Router; the routable form is a UniV3 with two ticks whose second
    interval is empty (cf. the trailing 0.0 of the fixture at test/cfmms.jl:118-119)."""
    return UniV3(current_price, [p_upper, p_lower], [liquidity, 0.0], γ, Ai)


# What the host mirror knows about one pool family, a row of KINDS:
#   pool    the pool type PoolBatch[i] builds;  ctor: a pool's fields in the argument order of that type
#   family  None: two coins; else N coins (2..MAX_COINS, one batch per coin count), the family's name in error texts
#   add     the Context method that uploads a batch; its arrays are the batch's fields in ctor order, then the tick CSR
#   door    the sparse update a segment accepts: "reserves" (R), "curve" ((R, α, β)) or "prices" (a price or a new ladder)
#   state   the fields that door moves;  check: further value checks of a whole batch (raises ArgumentError)
Kind = namedtuple("Kind", "pool ctor family add door state check", defaults=(None,))
_LADDER = ("lower_ticks", "liquidity")     # per-pool vectors of any length: a batch holds them as a CSR behind tick_off [m + 1]
_COIN_FIELDS = ("R", "w", "Ai")            # [m, n_coins] in a batch; every other field [m]
# One row per kind with a device kernel, in the order a Router packs a pool list: the two-coin kinds (Solidly last: it never
# joins a fused launch), then the N-coin kinds.  THE place to edit when a family is added (with PoolLayout, if it changes
# where pools live).
KINDS = {
    KIND_PRODUCT: Kind(ProductTwoCoin, ("R", "γ", "Ai"), None, "add_product", "reserves", ("R",)),
    KIND_GEOMEAN: Kind(GeometricMeanTwoCoin, ("R", "w", "γ", "Ai"), None, "add_geomean", "reserves", ("R",)),
    KIND_UNIV3: Kind(UniV3, ("current_price",) + _LADDER + ("γ", "Ai"), None, "add_univ3", "prices", ("current_price",)),
    KIND_SOLIDLY: Kind(SolidlyStableTwoCoin, ("R", "γ", "Ai"), None, "add_solidly", "reserves", ("R",),
                       lambda b: _solidly_check(b.R, b.γ)),
    KIND_WEIGHTED: Kind(GeometricMean, ("R", "w", "γ", "Ai"), "weighted", "add_weighted", "reserves", ("R",)),
    KIND_CURVE: Kind(Curve, ("R", "γ", "Ai", "α", "β"), "Curve", "add_curve", "curve", ("R", "α", "β"),
                     lambda b: _curve_range_check(b.R, b.α, b.β) if len(b) else None),
}


def _fields(kind):
    """the per-pool array fields of a batch, in the argument order of the kind's pool type"""
    return tuple(f for f in KINDS[kind].ctor if f not in _LADDER)


def _has_ladder(kind):
    return _LADDER[0] in KINDS[kind].ctor


# value checks of N-coin batches, in order: field, zero allowed, message
_NCOIN_CHECKS = (("R", False, "reserves must be finite and > 0"), ("w", False, "weights must be finite and > 0"),
                 ("α", True, "α must be finite and >= 0"), ("β", False, "β must be finite and > 0"))


def _and(names):
    return names[0] if len(names) == 1 else ", ".join(names[:-1]) + " and " + names[-1]


class PoolBatch:
    """m pools of one family, structure-of-arrays (the HBM layout, on the host).

    Ai is 1-based [m, 2] like the reference's per-pool `Ai` ([m, n_coins] for KIND_WEIGHTED and KIND_CURVE: R, w and Ai of
    one batch have one coin count; pools with different coin counts go in different batches)."""

    def __init__(self, kind, **a):
        self.kind = kind
        self.γ = np.ascontiguousarray(a["γ"], dtype=np.float64).reshape(-1)
        m = self.γ.size
        if KINDS[kind].family is not None:
            self._init_ncoin(m, a)
        else:
            for f in _fields(kind):
                if f != "γ":
                    self._set(f, a, m, 2)
        if KINDS[kind].check is not None:
            KINDS[kind].check(self)
        if _has_ladder(kind):
            self.tick_off = np.ascontiguousarray(a["tick_off"], dtype=np.int64).reshape(m + 1)
            self.lower_ticks = np.ascontiguousarray(a["lower_ticks"], dtype=np.float64).reshape(-1)
            self.liquidity = np.ascontiguousarray(a["liquidity"], dtype=np.float64).reshape(-1)

    def _set(self, f, a, m, n):
        """self.f <- a[f] as [m, n] (per-coin fields) or [m]"""
        x = np.ascontiguousarray(a[f], dtype=np.int64 if f == "Ai" else np.float64)
        setattr(self, f, x.reshape((m, n) if f in _COIN_FIELDS else m))

    def _init_ncoin(self, m, a):
        """KIND_WEIGHTED (R, w, Ai [m, n]) and KIND_CURVE (R, Ai [m, n]; α, β [m])"""
        fam = KINDS[self.kind].family
        fields = [f for f in _fields(self.kind) if f != "γ"]
        R = np.asarray(a["R"], dtype=np.float64)
        n = R.shape[-1] if R.ndim == 2 else (R.size // m if m else 2)
        if not 2 <= n <= MAX_COINS:
            raise ArgumentError(f"{fam} pools have 2..{MAX_COINS} coins, got {n}")
        try:
            for f in fields:
                self._set(f, a, m, n)
        except ValueError:
            per_pool = [f for f in fields if f not in _COIN_FIELDS]
            raise ArgumentError(f"{_and([f for f in fields if f in _COIN_FIELDS])} of a {fam} batch must have shape [m, n_coins]"
                                + (f", {_and(per_pool)} shape [m]" if per_pool else "")) from None
        for f, zero_ok, msg in _NCOIN_CHECKS:
            x = getattr(self, f) if f in fields else None
            if x is not None and (not np.all(np.isfinite(x)) or np.any(x < 0 if zero_ok else x <= 0)):
                raise ArgumentError(msg)
        if np.any(~(self.γ > 0)) or np.any(self.γ > 1):
            raise ArgumentError("fee γ must lie in (0, 1] (γ > 1 makes the N-coin arbitrage problem unbounded)")
        if m and np.any(np.sort(self.Ai, axis=1)[:, 1:] == np.sort(self.Ai, axis=1)[:, :-1]):
            raise ArgumentError("the token indices of a pool must be distinct")

    n_coins = property(lambda self: self.Ai.shape[1])

    def __len__(self):
        return self.γ.size

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.slice(*i.indices(len(self))[:2])
        i = int(i)
        if i < 0:
            i += len(self)
        K = KINDS[self.kind]
        o, e = (self.tick_off[i], self.tick_off[i + 1]) if _has_ladder(self.kind) else (i, i)
        return K.pool(*(getattr(self, f)[o:e] if f in _LADDER else getattr(self, f)[i] for f in K.ctor))

    def slice(self, lo, hi):
        """Pools [lo, hi) as a new batch (used to shard a market across GPUs)."""
        part = {f: getattr(self, f)[lo:hi] for f in _fields(self.kind)}
        if _has_ladder(self.kind):
            o, e = self.tick_off[lo], self.tick_off[hi]
            part.update(tick_off=self.tick_off[lo:hi + 1] - o, lower_ticks=self.lower_ticks[o:e], liquidity=self.liquidity[o:e])
        return PoolBatch(self.kind, **part)

    @staticmethod
    def concat(batches):
        """One batch holding the pools of several same-family batches, in order."""
        batches = list(batches)
        kind = batches[0].kind
        if any(b.kind != kind for b in batches):
            raise ArgumentError("concat needs batches of one pool family")
        if KINDS[kind].family is not None and len({b.n_coins for b in batches}) > 1:
            raise ArgumentError("concat needs weighted / Curve batches of one coin count")
        cat = lambda name: np.concatenate([getattr(b, name) for b in batches])
        whole = {f: cat(f) for f in _fields(kind)}
        if _has_ladder(kind):
            off, base = [np.zeros(1, dtype=np.int64)], 0
            for b in batches:
                off.append(b.tick_off[1:] + base)
                base += int(b.tick_off[-1])
            whole.update(tick_off=np.concatenate(off), lower_ticks=cat("lower_ticks"), liquidity=cat("liquidity"))
        return PoolBatch(kind, **whole)

    @staticmethod
    def from_pools(kind, pools):
        if KINDS[kind].family is not None and len({len(p.Ai) for p in pools}) > 1:
            raise ArgumentError(f"one {KINDS[kind].family} batch holds pools of one coin count (group them by len(Ai))")
        fields = {f: [getattr(p, f) for p in pools] for f in _fields(kind)}
        if _has_ladder(kind):
            off = np.zeros(len(pools) + 1, dtype=np.int64)
            np.cumsum([p.lower_ticks.size for p in pools], out=off[1:])
            fields.update(tick_off=off, lower_ticks=np.concatenate([p.lower_ticks for p in pools]) if pools else [],
                          liquidity=np.concatenate([p.liquidity for p in pools]) if pools else [])
        return PoolBatch(kind, **fields)


def _set_pool_state(ctx, seg, batch: PoolBatch, rows, states):
    """New state of pools `rows` of `batch` (device segment `seg`; ctx None: host mirror only): a reserve vector per pool,
    (R, α, β) for Curve, a price for UniV3 -- or (price, lower_ticks, liquidity), a mint / burn.  The device call
    (cfmm_pools_set_*) checks every row before anything changes; the batch's arrays follow only when it accepted."""
    rows, door, n = np.asarray(rows, dtype=np.int64), KINDS[batch.kind].door, batch.n_coins
    reserves = lambda Rs: np.array([np.asarray(R, dtype=np.float64).reshape(n) for R in Rs]).reshape(len(rows), n)
    try:
        if door == "prices" and any(_is_ladder_state(s) for s in states):
            _set_univ3_ladders(ctx, seg, batch, rows, states)
        elif door == "prices":
            p = np.array([float(s) for s in states], dtype=np.float64)
            if ctx is not None:
                ctx.set_prices(seg, rows, p)
            batch.current_price[rows] = p
        elif door == "curve":
            R = reserves(s[0] for s in states)
            α = np.array([float(s[1]) for s in states], dtype=np.float64)
            β = np.array([float(s[2]) for s in states], dtype=np.float64)
            if ctx is not None:
                ctx.set_curve(seg, rows, R, α, β)
            batch.R[rows], batch.α[rows], batch.β[rows] = R, α, β
        else:
            R = reserves(states)
            if ctx is not None:
                ctx.set_reserves(seg, rows, R)
            batch.R[rows] = R
    except (TypeError, ValueError, IndexError) as e:
        if isinstance(e, ArgumentError):
            raise
        raise ArgumentError(f"new state of a {type(batch[0]).__name__ if len(batch) else 'pool'}: an R vector per pool, (R, α, β) "
                            f"for Curve, a price or (price, lower_ticks, liquidity) for UniV3 ({e})") from None


def _is_ladder_state(s):
    return isinstance(s, (tuple, list)) and len(s) == 3 and np.ndim(s[0]) == 0 and np.ndim(s[1]) == 1


def _set_univ3_ladders(ctx, seg, batch, rows, states):
    """UniV3 rows of which some bring a new ladder: ALL of them go through one cfmm_pools_set_ticks call (a bare price with
    the pool's own ladder), so the segment's rows are still checked together; then the batch's CSR arrays are rebuilt."""
    if ctx is None:
        raise NotImplementedError("this backend cannot change a UniV3 pool's tick ladder (the device context does: "
                                  "cfmm_pools_set_ticks)")
    p, lts, lqs = [], [], []
    for r, s in zip(rows, states):
        if _is_ladder_state(s):
            lt, lq = np.asarray(s[1], dtype=np.float64).reshape(-1), np.asarray(s[2], dtype=np.float64).reshape(-1)
            if lt.size != lq.size:
                raise ValueError("lower_ticks and liquidity must have the same length")
            p.append(float(s[0]))
        else:
            o, e = batch.tick_off[r], batch.tick_off[r + 1]
            lt, lq = batch.lower_ticks[o:e], batch.liquidity[o:e]
            p.append(float(s))
        lts.append(lt)
        lqs.append(lq)
    p = np.array(p, dtype=np.float64)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([a.size for a in lts], out=off[1:])
    ctx.set_ticks(seg, rows, p, off, np.concatenate(lts), np.concatenate(lqs))
    # the host mirror: untouched ladders keep their order, the rows' ladders take their new lengths
    m, old_len = len(batch), np.diff(batch.tick_off)
    new_len, keep = old_len.copy(), np.ones(m, dtype=bool)
    new_len[rows] = np.diff(off)
    keep[rows] = False
    new_off = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(new_len, out=new_off[1:])
    lt, lq = np.empty(new_off[-1]), np.empty(new_off[-1])
    src, dst = np.repeat(keep, old_len), np.repeat(keep, new_len)
    lt[dst], lq[dst] = batch.lower_ticks[src], batch.liquidity[src]
    for r, a, b in zip(rows, lts, lqs):
        lt[new_off[r]:new_off[r + 1]], lq[new_off[r]:new_off[r + 1]] = a, b
    batch.tick_off, batch.lower_ticks, batch.liquidity = new_off, lt, lq
    batch.current_price[rows] = p


def zerotrade(c):
    """zerotrade(c) -- src/cfmms.jl:73,248"""
    return np.zeros(2)


def find_arb_(Δ, Λ, cfmm, v, device=0):
    """find_arb!(Δ, Λ, cfmm, v) -- src/cfmms.jl:35 and the methods at :130, :185, :339.

    Solves one pool's arbitrage problem at local prices `v` (length len(cfmm.Ai)) ON THE DEVICE and
    overwrites Δ and Λ.  Convenience for tests and examples; routers sweep all pools at once."""
    from ._lib import Context

    n = len(cfmm.Ai)
    v = np.asarray(v, dtype=np.float64).reshape(n)
    ctx = Context(n, device)
    try:
        _upload(ctx, PoolBatch.from_pools(cfmm.kind, [_with_local_idx(cfmm)]))
        ctx.find_arb(v)
        D, Lm = ctx.trades()
    finally:
        ctx.close()
    Δ[:] = np.ravel(D)[:n]
    Λ[:] = np.ravel(Lm)[:n]
    return None


def forward_trade(Δ, cfmm, coin_out=None, device=0):
    """forward_trade(Δ, cfmm) -- src/cfmms.jl:436-449, there for UniV3 only; here for every device kind.

    Δ (length len(cfmm.Ai)) has exactly one positive entry: the amount tendered, at the position of its coin.  Returns the
    amount of the other coin -- of coin `coin_out` (0-based position; required on pools of more than two coins) -- that
    comes out, fee on the input: the largest λ with φ(R + γΔ − λ·e_out) = φ(R).  Δ == 0 returns 0.0 (:440-442).  One
    pool through the device (cfmm_quote), the way find_arb_(Δ, Λ, cfmm, v) works."""
    from ._lib import Context

    if not hasattr(cfmm, "kind") or cfmm.kind not in KINDS:
        raise ArgumentError(f"{type(cfmm).__name__} has no device quote")
    n = len(cfmm.Ai)
    Δ = np.asarray(Δ, dtype=np.float64).reshape(-1)
    if Δ.size != n:
        raise ArgumentError(f"Δ must have {n} entries")
    if not np.all(np.isfinite(Δ)) or np.any(Δ < 0):
        raise ArgumentError("Δ must be finite and >= 0")
    pos = np.flatnonzero(Δ > 0)
    if pos.size > 1:
        raise ArgumentError("Δ must have exactly one positive entry (one coin in)")
    if coin_out is None and n > 2:
        raise ArgumentError(f"coin_out= is required on a pool of {n} coins")
    if coin_out is not None and not 0 <= int(coin_out) < n:
        raise ArgumentError(f"coin_out {coin_out} out of range 0:{n - 1}")
    if pos.size == 0:
        return 0.0
    cin = int(pos[0])
    if coin_out is not None and int(coin_out) == cin:
        raise ArgumentError("coin_out is the tendered coin")
    ctx = Context(n, device)
    try:
        _upload(ctx, PoolBatch.from_pools(cfmm.kind, [_with_local_idx(cfmm)]))
        out = ctx.quote(0, [Δ[cin]], cin, None if coin_out is None else int(coin_out))
    finally:
        ctx.close()
    return float(out[0])


def backward_trade(Λ, cfmm, coin_in=None, device=0):
    """backward_trade(Λ, cfmm) -- the mirror of forward_trade (the reference has none): the exact-output quote of one pool.

    Λ (length len(cfmm.Ai)) has exactly one positive entry: the amount wanted, at the position of its coin.  Returns the
    amount of the other coin -- of coin `coin_in` (0-based position; required on pools of more than two coins) -- that must
    be tendered, fee on the input: the smallest δ with φ(R + γδ·e_in − Λ) = φ(R); +inf where the pool cannot give Λ.
    Λ == 0 returns 0.0.  One pool through the device (cfmm_quote_out)."""
    from ._lib import Context

    if not hasattr(cfmm, "kind") or cfmm.kind not in KINDS:
        raise ArgumentError(f"{type(cfmm).__name__} has no device quote")
    n = len(cfmm.Ai)
    Λ = np.asarray(Λ, dtype=np.float64).reshape(-1)
    if Λ.size != n:
        raise ArgumentError(f"Λ must have {n} entries")
    if not np.all(np.isfinite(Λ)) or np.any(Λ < 0):
        raise ArgumentError("Λ must be finite and >= 0")
    pos = np.flatnonzero(Λ > 0)
    if pos.size > 1:
        raise ArgumentError("Λ must have exactly one positive entry (one coin out)")
    if coin_in is None and n > 2:
        raise ArgumentError(f"coin_in= is required on a pool of {n} coins")
    if coin_in is not None and not 0 <= int(coin_in) < n:
        raise ArgumentError(f"coin_in {coin_in} out of range 0:{n - 1}")
    if pos.size == 0:
        return 0.0
    cout = int(pos[0])
    if coin_in is not None and int(coin_in) == cout:
        raise ArgumentError("coin_in is the wanted coin")
    cin = 1 - cout if coin_in is None else int(coin_in)
    ctx = Context(n, device)
    try:
        _upload(ctx, PoolBatch.from_pools(cfmm.kind, [_with_local_idx(cfmm)]))
        out = ctx.quote_out(0, [Λ[cout]], cin, cout)
    finally:
        ctx.close()
    return float(out[0])


def _with_local_idx(c):
    """the pool with token indices 1..n (a one-pool market)"""
    K = KINDS[c.kind]
    return K.pool(*(np.arange(1, len(c.Ai) + 1) if f == "Ai" else getattr(c, f) for f in K.ctor))


def _upload(ctx, batch: PoolBatch):
    """Append one homogeneous batch to the device pool store (1-based -> 0-based here)."""
    Ai0 = (batch.Ai - 1).astype(np.int32)
    if np.any(batch.Ai < 1) or np.any(batch.Ai > ctx.n_tokens):
        raise ArgumentError(f"token index out of range 1:{ctx.n_tokens}")
    if batch.kind not in KINDS:
        raise ArgumentError("unknown pool family")
    arrays = _fields(batch.kind) + (("tick_off",) + _LADDER if _has_ladder(batch.kind) else ())
    getattr(ctx, KINDS[batch.kind].add)(*(Ai0 if f == "Ai" else getattr(batch, f) for f in arrays))


def _download_state(ctx, seg, batch: PoolBatch):
    """The state update_reserves! moved, device segment `seg` -> batch: current prices (UniV3) or reserves."""
    if KINDS[batch.kind].door == "prices":
        batch.current_price[:] = ctx.prices(seg, len(batch))
    else:
        batch.R[:] = ctx.reserves(seg, len(batch), batch.R.shape[1])


def _sync_pool(pool, batch: PoolBatch, row, full):
    """pool <- row `row` of its batch.  full: everything update_pools_ can move (R; α, β; current_price and the ladder);
    else what update_reserves! moves (R or current_price).  current_tick follows."""
    state = KINDS[batch.kind].state
    for f in state if full else state[:1]:
        x = getattr(batch, f)[row]
        if np.ndim(x):
            getattr(pool, f)[:] = x
        else:
            setattr(pool, f, float(x))
    if _has_ladder(batch.kind):
        if full:
            o, e = batch.tick_off[row], batch.tick_off[row + 1]
            pool.lower_ticks, pool.liquidity = batch.lower_ticks[o:e].copy(), batch.liquidity[o:e].copy()
        pool._retick()
