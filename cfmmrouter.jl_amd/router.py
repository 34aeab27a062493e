"""Host-side mirror of the reference's Router / route! (src/router.jl).

    Router(objective, cfmms, n_tokens)      src/router.jl:4-36
    find_arb_(r, v)   (Julia find_arb!)     src/router.jl:38-42   -> one device sweep
    route_(r; ...)    (Julia route!)        src/router.jl:58-108
    netflows_(ψ, r), netflows(r)            src/router.jl:111-125
    update_reserves_(r)                     src/router.jl:127-132 (unimplemented upstream)

Julia's `!` cannot appear in a Python identifier; mutating verbs carry a trailing underscore.
`r.Δs` / `r.Λs` / `r.v` / `r.cfmms` / `r.objective` are the reference's fields.

What runs where: pools are packed once into the device pool store (type-partitioned segments,
SoA-of-pairs); every evaluation of the dual function is ONE call through the C ABI which sweeps
all pools on the GPU and returns Ψ (n_tokens doubles) and the dual scalar.  The outer L-BFGS-B
iteration stays on the host, as in the reference (LBFGSB.jl there, SciPy's translation of the same
L-BFGS-B 3.0 here); its cost is O(n_tokens) per step.
"""
from __future__ import annotations

import math

import numpy as np

from . import objectives as _obj
from ._lib import FOUND_REPEATS, MAX_PATH_HOPS, MAX_SPLIT_PATHS, ORDER_REFUSED, SPLIT_NONE, SPLIT_OK, SPLIT_SATURATED, SPLIT_UNOBTAINABLE, OBJ_BASKET_LIQUIDATION, OBJ_LINEAR_NONNEGATIVE, ArgumentError, CFMMDeviceError, Context
from .layout import PoolLayout
from .cfmms import CFMM, KINDS, MAX_COINS, PoolBatch, _download_state, _has_ladder, _set_pool_state, _upload


_BOXED_INF = 1e100   # stands in for the reference's u = Inf under nbd = 2 (see route_)


class DeviceBackend:
    """The pool store + sweeps of one GPU, behind the C ABI (include/cfmm_amd.h)."""

    def __init__(self, n_tokens, batches, device=0):
        self.ctx = Context(n_tokens, device)
        self.n_tokens = int(n_tokens)
        self._load(batches)

    def _load(self, batches):
        self.layout = PoolLayout(batches)      # of THIS pool store, packed order only (a Router's own layout also knows its order)
        for _, _, b in self.layout.segments():
            _upload(self.ctx, b)

    def eval(self, v):
        """fn/g! evaluation without trade write-back -> (Ψ, acc)."""
        return self.ctx.eval(v)

    def find_arb(self, v):
        """find_arb!(r, v): trades materialised on the device -> (Ψ, acc)."""
        self.ctx.find_arb(v)
        return self.ctx.netflows(), self.ctx.dual_value()

    def trades(self, out=None):
        return self.ctx.trades(out)

    def active_trades(self, min_value=0.0):
        """The pools that trade in the latest find_arb! and are worth at least min_value, selected on the device segment by
        segment (cfmm_select_trades) -> a list of blocks (idx, Δ, Λ, value): idx = positions in packed (segment) order,
        ascending; Δ, Λ = [count, coins] rows."""
        blocks = []
        for seg, first, _ in self.layout.segments():
            idx, D, Lm, val = self.ctx.select_trades(seg, min_value, n_coins=self.layout.coins[seg])
            blocks.append((idx + first, D, Lm, val))
        return blocks

    def reload(self, batches):
        """Replace the device pool store (used after update_reserves_)."""
        self.ctx.clear()
        self._load(batches)

    def close(self):
        peer = getattr(self, "peer", None)
        if peer is not None and hasattr(peer, "close"):
            peer.close()       # unmap / free the IPC peer buffers while the context still exists
            self.peer = None
        self.ctx.close()


def _segments_of(cfmms):
    """Pack a pool container into homogeneous batches.

    Returns (batches, order, host) where `order[k]` is the router index of the k-th packed pool (None when packing
    preserved the router order) and `host` lists the router indices of pools whose TYPE has no device kernel -- any
    other CFMM subclass with its own `find_arb_(Δ, Λ, v)` method, the reference's plugin seam (src/cfmms.jl:35,56:
    `find_arb!(Δ, Λ, cfmm::CFMM, v)` is dispatched on the pool's type, so a user's own CFMM subtype enters a Router
    by defining that one method).  They are evaluated on the host every evaluation (HostSegment)."""
    if isinstance(cfmms, PoolBatch):
        return [cfmms], None, []
    cfmms = list(cfmms)
    if cfmms and all(isinstance(c, PoolBatch) for c in cfmms):
        return cfmms, None, []
    for c in cfmms:
        if not isinstance(c, CFMM):
            raise ArgumentError("cfmms must hold CFMM objects or PoolBatch containers")
    batches, order = [], []
    for kind, K in KINDS.items():   # the table's order; N-coin kinds: one batch (one device segment) per coin count
        for n in (None,) if K.family is None else range(2, MAX_COINS + 1):
            idx = [i for i, c in enumerate(cfmms) if c.kind == kind and (n is None or len(c.Ai) == n)]
            if idx:
                batches.append(PoolBatch.from_pools(kind, [cfmms[i] for i in idx]))
                order.extend(idx)
    host = [i for i, c in enumerate(cfmms) if c.kind not in KINDS]
    for i in host:
        if not callable(getattr(cfmms[i], "find_arb_", None)) or not hasattr(cfmms[i], "Ai"):
            raise ArgumentError(f"cfmms[{i}] ({type(cfmms[i]).__name__}): a pool type without a device kernel needs its own "
                                f"find_arb_(Δ, Λ, v) method and an `Ai` field (src/cfmms.jl:35,56)")
    order = np.array(order, dtype=np.int64)
    if not host and np.array_equal(order, np.arange(len(cfmms))):
        order = None
    return batches, order, host


class HostSegment:
    """Pools whose type has no device kernel: the CALLER's own `find_arb_(Δ, Λ, v_local)` (Julia: the user's
    `find_arb!(Δ, Λ, cfmm, v)` method, src/cfmms.jl:35) runs on the host at every evaluation, exactly as
    `find_arb!(r::Router, v)` would call it (src/router.jl:40: `find_arb!(r.Δs[i], r.Λs[i], r.cfmms[i], v[r.cfmms[i].Ai])`),
    and their part of Ψ (src/router.jl:98-100, :114-115) and of the dual scalar (:82) is added to what the device returns.
    Any number of coins per pool (`len(pool.Ai)`)."""

    def __init__(self, pools, n_tokens):
        self.pools = list(pools)
        self.n_tokens = int(n_tokens)
        self.Ai0 = []
        for c in self.pools:
            ai = np.asarray(c.Ai, dtype=np.int64).reshape(-1) - 1
            if ai.size == 0 or np.any(ai < 0) or np.any(ai >= n_tokens):
                raise ArgumentError(f"token index out of range 1:{n_tokens}")
            self.Ai0.append(ai)
        self.Δs = [np.zeros(ai.size) for ai in self.Ai0]      # zerotrade(c), src/router.jl:23-26
        self.Λs = [np.zeros(ai.size) for ai in self.Ai0]

        self._sΔ = [np.zeros(ai.size) for ai in self.Ai0]     # scratch trades of non-materialising evaluations
        self._sΛ = [np.zeros(ai.size) for ai in self.Ai0]

    def sweep(self, v, materialize=True):
        """materialize=False (a bare evaluation: the device half writes no trades either): the pools' find_arb_ runs into
        scratch vectors, so self.Δs / self.Λs stay those of the latest find_arb -- the same price vector as the device
        pools' trades (the reference overwrites ALL pools' trades in every evaluation; here NONE move between find_arb!s)."""
        psi, acc = np.zeros(self.n_tokens), 0.0
        Ds, Ls = (self.Δs, self.Λs) if materialize else (self._sΔ, self._sΛ)
        if materialize:
            self.v = np.array(v, dtype=np.float64)       # the prices self.Δs / self.Λs belong to (active_trades)
        for c, ai, D, L in zip(self.pools, self.Ai0, Ds, Ls):
            vl = v[ai]                                   # v[r.cfmms[i].Ai]
            c.find_arb_(D, L, vl)                        # the user's method: overwrites Δ, Λ
            acc += float(np.dot(L, vl) - np.dot(D, vl))  # src/router.jl:82
            np.add.at(psi, ai, L - D)                    # src/router.jl:99
        return psi, acc

    def active_trades(self, min_value=0.0):
        """The host-evaluated pools that trade in the latest materialising sweep and are worth at least min_value, by the
        rule and the arithmetic of cfmm_select_trades: some entry of Δ or Λ compares != 0.0, value = Σ_k (Λ_k − Δ_k)·v[A_k]
        summed in coin order from +0.0, selected unless value < min_value -> (idx, Δ rows, Λ rows, value), idx = positions
        among the host pools."""
        idx, Ds, Ls, vals = [], [], [], []
        v = getattr(self, "v", None)
        for j, (ai, D, L) in enumerate(zip(self.Ai0, self.Δs, self.Λs)):
            if not (np.any(D != 0.0) or np.any(L != 0.0)):
                continue
            value = np.float64(0.0)
            for k in range(ai.size):
                value = value + (L[k] - D[k]) * v[ai[k]]
            if value < min_value:
                continue
            idx.append(j)
            Ds.append(D.copy())
            Ls.append(L.copy())
            vals.append(value)
        return np.array(idx, dtype=np.int64), Ds, Ls, np.array(vals, dtype=np.float64)


class MixedBackend:
    """A device (or any other) backend plus a HostSegment: one evaluation = the backend's sweep + the host pools' own
    find_arb_, their Ψ and dual parts summed -- what L-BFGS-B sees is the dual of the WHOLE router."""

    def __init__(self, inner, host: HostSegment):
        self.inner, self.host = inner, host
        self.n_tokens = host.n_tokens
        self.inner_pools = 0      # pools of the inner backend (set by the Router: host positions are numbered behind them)

    def _add(self, res, v, materialize):
        psi, acc = res
        ph, ah = self.host.sweep(np.asarray(v, dtype=np.float64), materialize)
        return psi + ph, acc + ah

    def eval(self, v):
        return self._add(self.inner.eval(v), v, False)

    def find_arb(self, v):
        return self._add(self.inner.find_arb(v), v, True)

    def trades(self, out=None):
        return self.inner.trades() if out is None else self.inner.trades(out)

    def active_trades(self, min_value=0.0):
        """The inner backend's blocks, then the host pools' (their positions follow the inner backend's pools)."""
        if hasattr(self.inner, "active_trades"):
            blocks = list(self.inner.active_trades(min_value))
        elif self.inner_pools == 0:                # every pool of the router is host-evaluated
            blocks = []
        else:
            raise NotImplementedError(f"{type(self.inner).__name__} has no active_trades")
        idx, Ds, Ls, vals = self.host.active_trades(min_value)
        return blocks + [(idx + self.inner_pools, Ds, Ls, vals)]

    def reload(self, batches):
        self.inner.reload(batches)

    ctx = property(lambda self: self.inner.ctx)     # library options / introspection of the device half

    def close(self):
        if hasattr(self.inner, "close"):
            self.inner.close()


class _PoolView:
    """`r.cfmms` for batch-built routers: indexable / iterable pool objects, built on demand."""

    def __init__(self, batches):
        self._batches = batches
        self._offsets = np.cumsum([0] + [len(b) for b in batches])

    def __len__(self):
        return int(self._offsets[-1])

    def __getitem__(self, i):
        i = int(i)
        if i < 0:
            i += len(self)
        s = int(np.searchsorted(self._offsets, i, side="right") - 1)
        return self._batches[s][i - int(self._offsets[s])]

    def __iter__(self):
        for b in self._batches:
            for i in range(len(b)):
                yield b[i]


class Router:
    """Router(objective, cfmms, n_tokens) -- src/router.jl:4-36."""

    def __init__(self, objective, cfmms, n_tokens, device=0, _backend=None):
        if not isinstance(objective, _obj.Objective):
            raise ArgumentError("objective must be an Objective")
        self.objective = objective
        self.n_tokens = int(n_tokens)
        if not isinstance(cfmms, PoolBatch):
            cfmms = list(cfmms)
        batches, order, host = _segments_of(cfmms)
        self._layout = PoolLayout(batches, order, host)
        self._batches = batches
        from_batches = isinstance(cfmms, PoolBatch) or (len(batches) > 0 and all(isinstance(c, PoolBatch) for c in cfmms))
        self.cfmms = _PoolView(batches) if from_batches else list(cfmms)
        self.v = np.zeros(self.n_tokens)  # :33
        self._backend = _backend if _backend is not None else DeviceBackend(self.n_tokens, batches, device)
        # the plugin seam: pools of any other CFMM subclass are evaluated by their own find_arb_ on the host
        self._host = HostSegment([cfmms[i] for i in host], self.n_tokens) if host else None
        if self._host is not None:
            self._backend = MixedBackend(self._backend, self._host)
            self._backend.inner_pools = self._layout.m
        self._reset_trades()
        self.n_sweeps = 0
        self.info = None

    def _reset_trades(self):
        """zerotrade per pool (src/router.jl:23-26), the host-evaluated pools' included; no sweep's Ψ and dual value"""
        self._trades = [self._layout.zero_trades(), self._layout.zero_trades()]      # Δ, Λ in packed order
        if self._host is not None:
            for x in self._host.Δs + self._host.Λs:
                x[:] = 0.0
        self._psi, self._acc, self._trades_stale = np.zeros(self.n_tokens), 0.0, False

    def _fetch(self):
        """The trades of the latest find_arb!, once: per-pool vectors for a ragged router, the backend's packed arrays for
        one with host pools, permuted into the router's arrays for a reordered one -- and an in-order DeviceBackend fills the
        router's own arrays: find_arb! overwrites r.Δs / r.Λs in place (src/router.jl:40)."""
        if not self._trades_stale:
            return
        L, own = self._layout, self._trades
        if not L.per_pool and L.order is None and isinstance(self._backend, DeviceBackend):
            self._backend.trades(out=tuple(own))
        else:
            got = self._backend.trades()
            for k in (0, 1):
                if L.ragged:
                    own[k] = L.split(got[k])
                elif L.per_pool or L.order is None:      # (host pools; test-injected backends)
                    own[k] = got[k]
                else:
                    own[k][L.order] = got[k]
        self._trades_stale = False

    def _router_trades(self, k):
        """r.Δs (k = 0) / r.Λs (k = 1): [m, 2] arrays in router order (rows are the reference's per-pool vectors); ragged
        routers and routers with host-evaluated pools: a list of per-pool vectors in router order (the reference's
        Vector{Vector}), host pools' vectors included"""
        self._fetch()
        if not self._layout.per_pool:
            return self._trades[k]
        return self._layout.to_router(self._trades[k], () if self._host is None else (self._host.Δs, self._host.Λs)[k])

    Δs = property(lambda self: self._router_trades(0))
    Λs = property(lambda self: self._router_trades(1))
    Deltas = Δs
    Lambdas = Λs

    def close(self):
        if hasattr(self._backend, "close"):
            self._backend.close()


def find_arb_(r: Router, v):
    """find_arb!(r::Router, v) -- src/router.jl:38-42: every pool's arbitrage at prices v."""
    v = np.asarray(v, dtype=np.float64)
    r._psi, r._acc = r._backend.find_arb(v)
    r._trades_stale = True
    r.n_sweeps += 1
    return None


def route_(r: Router, v=None, verbose=False, m=5, factr=1e1, pgtol=1e-5, maxfun=15_000, maxiter=15_000,
           solver="scipy"):
    """route!(r; v, verbose, m, factr, pgtol, maxfun, maxiter) -- src/router.jl:58-108.

    Overwrites r.Δs, r.Λs and r.v.  The dual function g(ν) = f(ν) + Σᵢ arbᵢ(Aᵢᵀν) is minimised
    with L-BFGS-B over the objective's box; each evaluation is one device sweep.

    solver="scipy"  (default): SciPy's translation of the Fortran L-BFGS-B 3.0 the reference calls
                    through LBFGSB.jl drives the loop from Python, one C-ABI call per evaluation.
    solver="native": the library's own L-BFGS-B (csrc/lbfgsb.cpp).  On a single-GPU router the whole
                    of route! then runs inside ONE C-ABI call (cfmm_route): no interpreter between
                    two device sweeps."""
    if solver == "native":
        return _route_native(r, v, m, factr, pgtol, maxfun, maxiter)
    if solver != "scipy":
        raise ArgumentError("solver must be 'scipy' or 'native'")
    from scipy.optimize import fmin_l_bfgs_b

    n = r.v.size
    if v is None:
        r.v[:] = np.ones(n) / n  # :62
    else:
        r.v[:] = v  # :64
    lo = _obj.lower_limit(r.objective)  # :67-70 (nbd = 2 with an infinite upper bound)
    up = _obj.upper_limit(r.objective)
    # nbd = 2 with u = Inf makes the Fortran code take its "boxed" unit first step; SciPy would turn an
    # infinite bound into "no bound" (first step min(1/|d|, 1)), so the reference's call shape is kept
    # with a finite upper bound no iterate can reach (solver="native" emulates the same thing directly).
    bounds = [(lo[j], _BOXED_INF if math.isinf(up[j]) else up[j]) for j in range(n)]

    sweep, fg = _dual_fg(r)
    sweep(r.v)  # :104
    kw = dict(bounds=bounds, m=m, factr=factr, pgtol=pgtol, maxfun=maxfun, maxiter=maxiter)
    if verbose:
        kw["iprint"] = 1
    x, fmin, info = fmin_l_bfgs_b(fg, r.v.copy(), **kw)  # :105
    r.v[:] = x  # :106
    r.info = {"f": fmin, **{k: info[k] for k in ("warnflag", "task", "funcalls", "nit") if k in info}}
    find_arb_(r, r.v)  # :107
    return None


def _dual_fg(r: Router):
    """The dual function both solvers minimise -> (sweep, fg): sweep(x) evaluates the pools at x; fg(x) -> (g(x), ∇g(x))
    = (f(x) + Σᵢ arbᵢ, ∇f(x) + Ψ), with one sweep unless x is where the latest one was."""
    n = r.v.size

    def sweep(x):
        r._psi, r._acc = r._backend.eval(x)
        r.n_sweeps += 1

    def fg(x):
        if not np.all(x == r.v):  # :74-77 / :92-95: one sweep per evaluation
            sweep(x)
            r.v[:] = x
        fval = _obj.f(r.objective, x) + r._acc  # :79-85
        G = np.zeros(n)  # :90
        _obj.grad_(G, r.objective, x)  # :96
        G += r._psi  # :98-100
        return fval, G

    return sweep, fg


def _objective_args(obj):
    """objective -> (kind, vector, index) as cfmm_route / cfmm_polish take it"""
    if isinstance(obj, _obj.LinearNonnegative):
        return OBJ_LINEAR_NONNEGATIVE, obj.c, 0
    if isinstance(obj, _obj.BasketLiquidation):
        return OBJ_BASKET_LIQUIDATION, obj.Δin, obj.i - 1
    raise ArgumentError("solver='native' knows LinearNonnegative and BasketLiquidation objectives")


def _native_info(info, **timing):
    return {"f": info["f"], "funcalls": info["evaluations"], "nit": info["iterations"],
            "warnflag": 0 if info["status"] in (0, 1) else 2, "task": info["status"], "solver": "native", **timing}


def _call_in_lockstep(guard, ctx, call):
    """A sharded router's (cfmm_set_peers) ranks run `call` in lockstep.  If ANY rank's call fails -- a lost pre-armed
    hand-over, a peer that did not publish within the time limit -- every rank learns it through one vote, the exchange is
    re-aligned, pre-arming goes off and the call is repeated launch-when-ready on all ranks -> (result, retried)."""
    def attempt():
        try:
            return call(), None
        except RuntimeError as e:      # CFMM_ERR_STATE (RuntimeError) or a HIP failure (CFMMDeviceError, its subclass)
            return None, e

    res, err = attempt()
    if guard.vote(res is not None):
        return res, False
    guard.resync()
    ctx.set_option("armed", 0)
    res, err = attempt()
    if not guard.vote(res is not None):
        raise err if err is not None else CFMMDeviceError("sharded route! failed on another rank")
    return res, True


def _route_native(r: Router, v, m, factr, pgtol, maxfun, maxiter):
    from ._lib import lbfgsb_minimize

    if isinstance(r._backend, DeviceBackend):   # everything in one library call
        kind, vec, idx = _objective_args(r.objective)
        ctx, guard = r._backend.ctx, getattr(r, "_guard", None)
        call = lambda: ctx.route(kind, vec, idx, v0=v, m=m, factr=factr, pgtol=pgtol, maxfun=maxfun, maxiter=maxiter)
        if guard is None:
            vout, psi, info = call()
        else:
            (vout, psi, info), retried = _call_in_lockstep(guard, ctx, call)
            if retried:
                r.collective_retries = getattr(r, "collective_retries", 0) + 1
        r.v[:] = vout
        r._psi, r._acc = psi, r._backend.ctx.dual_value()
        r._trades_stale = True
        r.n_sweeps += info["sweeps"]
        r.info = _native_info(info, sweep_seconds=info["sweep_seconds"], total_seconds=info["total_seconds"])
        return None
    # any other backend (sharded, test-injected): same solver, Python callback per evaluation
    n = r.v.size
    r.v[:] = np.ones(n) / n if v is None else v
    lo, up = _obj.lower_limit(r.objective), _obj.upper_limit(r.objective)
    bounds = [(lo[j], None if math.isinf(up[j]) else up[j]) for j in range(n)]
    sweep, fg = _dual_fg(r)
    sweep(r.v)
    x, info = lbfgsb_minimize(fg, r.v.copy(), bounds, m=m, factr=factr, pgtol=pgtol, maxfun=maxfun, maxiter=maxiter,
                              reference_boxed=True)   # nbd = 2 with u = Inf, as src/router.jl:67-70
    r.v[:] = x
    r.info = _native_info(info)
    find_arb_(r, r.v)
    return None


def _dual_gradient(r: Router, x):
    """G(ν) = ∇f(obj, ν) + Ψ(ν) of g! (src/router.jl:89-102) at ν = x: one fused sweep."""
    psi, acc = r._backend.eval(x)
    r.n_sweeps += 1
    G = np.zeros(x.size)
    _obj.grad_(G, r.objective, x)
    return G + psi, psi, acc


def dual_jacobian(r: Router, v=None, rel_step=1e-7):
    """Forward-difference Jacobian of the dual gradient G(ν) = ∇f(obj, ν) + Ψ(ν) (src/router.jl:89-102) at ν = v
    (default r.v): column j = (G(ν + hⱼeⱼ) − G(ν)) / hⱼ with hⱼ = rel_step·νⱼ -- n_tokens + 1 fused sweeps.  It is the
    Hessian of the dual where that exists (the dual is C¹ and piecewise C²: pools enter and leave their no-trade band).
    `polish_` uses it as the matrix of a chord-Newton iteration, where only its rough accuracy matters."""
    x = np.array(r.v if v is None else v, dtype=np.float64)
    G0, _, _ = _dual_gradient(r, x)
    J = np.empty((x.size, x.size))
    for j in range(x.size):
        xj = x.copy()
        xj[j] = x[j] * (1.0 + rel_step)
        J[:, j] = (_dual_gradient(r, xj)[0] - G0) / (xj[j] - x[j])
    return J


def polish_(r: Router, iters=8, jacobian=None, rel_step=1e-7, native=None):
    """Tighten a route!'s result beyond what L-BFGS-B's stopping rules can: a projected chord-Newton iteration on the
    optimality conditions of the dual problem route! solves (src/router.jl:58-108),

        Gⱼ(ν) = 0 for lⱼ < νⱼ,    Gⱼ(ν) ≥ 0 for νⱼ = lⱼ,    G(ν) = ∇f(obj, ν) + Ψ(ν),  l = lower_limit(obj),

    starting from r.v.  NOT part of the reference (its route! ends where L-BFGS-B ends); it exists because L-BFGS-B's
    line search works on the dual VALUE, whose rounding noise (a sum over 10⁶ pools) hides decreases below ~1e-15
    relative -- on interior optima that leaves a stationarity residual of ~1e-6·max|Ψ| -- while the GRADIENT Ψ is
    resolved to ~1e-12·max|Ψ|.  The iteration uses gradients only:

        free set F = {j : not (νⱼ = lⱼ and Gⱼ > 0)},   ν_F ← max(l_F, ν_F − J_FF⁻¹ G_F),

    J = `jacobian` (any reasonable approximation of the dual's Hessian: the limit point is where THIS backend's G
    satisfies the conditions, whatever J is; only the rate depends on it) or `dual_jacobian(r)` at the start
    (n_tokens + 1 sweeps).  Steps that do not reduce the residual are halved; the best iterate is kept.  Ends with
    find_arb!(r, ν) like route! does (:106-107), so r.v / r.Δs / r.Λs / netflows(r) describe the polished point.
    r.info["polish"] = {"residual0", "residual", "iterations", "sweeps"} (residual = max |G_F|, and −Gⱼ where a
    variable on its bound has Gⱼ < 0).

    native (default: True on an unsharded single-device router when no `jacobian` is given): the same iteration inside
    the library (cfmm_polish, one C-ABI call: what a Julia or C caller uses)."""
    if native is None:
        native = jacobian is None and isinstance(r._backend, DeviceBackend) and getattr(r, "_guard", None) is None
    if native:
        if jacobian is not None or not isinstance(r._backend, DeviceBackend):
            raise ArgumentError("native polish computes its own Jacobian on a DeviceBackend")
        kind, vec, idx = _objective_args(r.objective)
        vout, psi, pinfo = r._backend.ctx.polish(kind, vec, idx, r.v, max_iters=iters, rel_step=rel_step)
        r.v[:] = vout
        r._psi, r._acc = psi, r._backend.ctx.dual_value()
        r._trades_stale = True
        r.n_sweeps += pinfo["sweeps"]
        info = dict(r.info) if isinstance(r.info, dict) else {}
        info["polish"] = {k: pinfo[k] for k in ("residual0", "residual", "iterations", "sweeps")}
        info["polish"]["native_seconds"] = pinfo["total_seconds"]
        r.info = info
        return None
    n = r.v.size
    lo = _obj.lower_limit(r.objective)
    sweeps0 = r.n_sweeps
    x = np.maximum(np.array(r.v, dtype=np.float64), lo)
    J = dual_jacobian(r, x, rel_step) if jacobian is None else np.asarray(jacobian, dtype=np.float64)

    def residual(x, G):
        free = ~((x <= lo) & (G > 0.0))
        return free, (float(np.max(np.abs(G[free]))) if free.any() else 0.0)

    G, _, _ = _dual_gradient(r, x)
    free, res = residual(x, G)
    res0, done = res, 0
    for _ in range(int(iters)):
        if res == 0.0:
            break
        step = np.zeros(n)
        step[free] = np.linalg.lstsq(J[np.ix_(free, free)], -G[free], rcond=1e-13)[0]
        t, improved = 1.0, False
        while t >= 1.0 / 64:
            xt = np.maximum(x + t * step, lo)
            Gt, _, _ = _dual_gradient(r, xt)
            freet, rest = residual(xt, Gt)
            if rest < res:
                x, G, free, res, improved = xt, Gt, freet, rest, True
                break
            t *= 0.5
        done += 1
        if not improved:   # the rounding-noise floor of Ψ (or a kink the chord matrix cannot cross): keep the best iterate
            break
    r.v[:] = x
    find_arb_(r, r.v)
    info = dict(r.info) if isinstance(r.info, dict) else {}
    info["polish"] = {"residual0": res0, "residual": res, "iterations": done, "sweeps": r.n_sweeps - sweeps0}
    r.info = info
    return None


def active_trades(r: Router, min_value=0.0):
    """The short list a router that follows a chain executes: the pools that trade in the latest find_arb! / route! and are
    worth at least min_value, without fetching r.Δs / r.Λs -> (idx, Δ, Λ, value).

    A pool trades iff some entry of its Δ or Λ compares != 0.0 (−0.0 does not count, NaN does); its value is its term of the
    dual, Σ_k (Λ_k − Δ_k)·v[A_k] at the prices of that find_arb!, summed in coin order from +0.0 with every operation rounded on
    its own; it is selected unless value < min_value (min_value = -inf: every trading pool).  The device pools are selected on
    the device (cfmm_select_trades: three small launches per segment, then only the selected rows cross PCIe); host-evaluated
    plugin pools are filtered on the host by the same rule and the same arithmetic.

    idx: positions in r.cfmms, ascending.  Δ, Λ: their trade rows -- [count, 2] arrays for routers of two-coin device pools,
    a list of per-pool vectors otherwise (weighted / Curve pools, host-evaluated pools), as r.Δs is.  value: [count]."""
    if not hasattr(r._backend, "active_trades"):
        raise NotImplementedError(f"{type(r._backend).__name__} has no active_trades")
    blocks = r._backend.active_trades(min_value)
    # backend position -> position in r.cfmms
    idx = r._layout.place[np.concatenate([b[0] for b in blocks])] if blocks else np.zeros(0, dtype=np.int64)
    value = np.concatenate([b[3] for b in blocks]) if blocks else np.zeros(0)
    per_pool = r._layout.per_pool
    if per_pool:                                   # per-pool vectors, as PoolLayout.split makes them
        Ds = [np.array(row) for b in blocks for row in b[1]]
        Ls = [np.array(row) for b in blocks for row in b[2]]
    else:
        Ds = np.concatenate([b[1] for b in blocks]) if blocks else np.zeros((0, 2))
        Ls = np.concatenate([b[2] for b in blocks]) if blocks else np.zeros((0, 2))
    if idx.size and np.any(np.diff(idx) < 0):      # packed (family-grouped) order -> r.cfmms order
        perm = np.argsort(idx, kind="stable")
        idx, value = idx[perm], value[perm]
        if per_pool:
            Ds, Ls = [Ds[k] for k in perm], [Ls[k] for k in perm]
        else:
            Ds, Ls = Ds[perm], Ls[perm]
    return idx, Ds, Ls, value


def netflows_(ψ, r: Router, exact=False):
    """netflows!(ψ, r) -- src/router.jl:111-119: ψ = Σᵢ Aᵢ(Λᵢ − Δᵢ) for the latest sweep.

    exact=False (default): the device's reduction of the sweep that produced r.Δs / r.Λs (per-wavefront LDS bins, fixed-order
    folds): within 1e-12·max|ψ| of the reference's value, no per-pool data moved.
    exact=True: the reference's OWN loop -- `ψ[c.Ai] .+= Λ - Δ` pool after pool in router order (src/router.jl:113-116) --
    over the fetched trade rows, i.e. bit for bit what `netflows(r)` returns upstream, so that the reference's router test
    `all_flows .== netflows(r)` (test/arb.jl:16) holds unedited.  O(m) on the host (as upstream), and it fetches r.Δs / r.Λs."""
    if not exact:
        ψ[:] = r._psi
        return None
    Δs, Λs = r.Δs, r.Λs
    ψ[:] = 0.0
    if r._layout.per_pool:                       # per-pool vectors of any length, router order
        for Δ, Λ, c in zip(Δs, Λs, r.cfmms):
            ai = np.asarray(c.Ai, dtype=np.int64).reshape(-1) - 1
            for k in range(ai.size):             # broadcast assignment, element after element
                ψ[ai[k]] += Λ[k] - Δ[k]
        return None
    Ai = r._layout.Ai_router_order()
    # np.bincount adds its weights to each bin one after another in input order: pool 1 coin 1, pool 1 coin 2, pool 2 coin 1, ...
    # -- the reference's loop, starting from zeros
    ψ[:] = np.bincount((Ai.astype(np.int64) - 1).ravel(), weights=(Λs - Δs).ravel(), minlength=r.n_tokens)[:r.n_tokens]
    return None


def netflows(r: Router, exact=False):
    """netflows(r) -- src/router.jl:121-125 (exact: see netflows_)"""
    ψ = np.zeros_like(r.v)
    netflows_(ψ, r, exact)
    return ψ


def update_reserves_(r: Router, sync_host=True):
    """update_reserves!(r) -- src/router.jl:127-132.

    The reference's router method calls `update_reserves!(c, Δ, Λ, v)` per pool, a method that is
    defined nowhere (its own test marks it "borked", test/arb.jl:30-39), so there is no reference
    behaviour to match.  What is implemented is the update the routing problem itself prescribes
    (find_arb! docstring, src/cfmms.jl:26-31: the pool ends at R + γΔ − Λ), applied in place on the
    device from the trades of the latest find_arb!/route! (cfmm_update_reserves): one kernel for the
    two-coin families; UniV3 pools move to the price the arbitrage left them at.  The trades are
    consumed.  sync_host=True (default) also refreshes the host mirror (`r.cfmms[i].R`, batch.R,
    batch.current_price: 16 / 8 bytes per pool device-to-host); sequential routing that never reads
    them can pass sync_host=False and moves no per-pool data at all."""
    if r._host is not None:
        # host-evaluated pools: the pool type's own update_reserves_(Δ, Λ, v) -- the per-pool method the reference's
        # router calls (src/router.jl:129: update_reserves!(c, Δ, Λ, r.v[c.Ai])) -- then zero trades
        for c in r._host.pools:
            if not callable(getattr(c, "update_reserves_", None)):
                raise ArgumentError(f"{type(c).__name__} has no update_reserves_(Δ, Λ, v) method (src/router.jl:129)")
    ctx = getattr(r._backend, "ctx", None)
    if ctx is None:   # test-injected / sharded backends: host-side update of the two-coin families
        _update_reserves_host(r)
    else:
        ctx.update_reserves()
    if r._host is not None:
        # AFTER the device half (which can still refuse: no trades, a UniV3 segment without host prices) -- a refused
        # update then leaves every pool, host-evaluated ones included, as it was
        for c, ai, D, L in zip(r._host.pools, r._host.Ai0, r._host.Δs, r._host.Λs):
            c.update_reserves_(D, L, r.v[ai])
    if ctx is not None and sync_host:
        for seg, _, b in r._layout.segments():
            _download_state(ctx, seg, b)
        r._layout.sync_pools(r.cfmms)
    r._reset_trades()
    return None


def update_pools_(r: Router, changes):
    """New state for a few pools of a router, on the host mirror AND on the device, without re-uploading the market -- the
    reference's `r.cfmms[i].R .= ...` followed by another route! (there the pools ARE the router's state).

    `changes` maps positions in `r.cfmms` to new state: a reserve vector (ProductTwoCoin, GeometricMeanTwoCoin, Solidly,
    weighted pools), `(R, α, β)` (Curve), a price (UniV3; ticks and liquidity stay) or `(price, lower_ticks, liquidity)` (UniV3:
    a mint / burn, the pool's new ladder; cfmm_pools_set_ticks).  The pools are grouped by device segment;
    each segment's rows go through one cfmm_pools_set_* call, which checks all of them before anything changes (a refused
    segment is left as it was, and so are the segments after it).  Host-evaluated plugin pools (their own find_arb_) are
    updated on the host only: `pool.set_state_(state)` if the type defines it, else `pool.R[:] = state`.  The router's trades
    are those of the old market: they are zeroed, as by update_reserves_."""
    L = r._layout
    per_batch, host = {}, []
    for i, state in changes.items():
        where = L.locate(i)
        if where[0] == "host":
            host.append((r._host.pools[where[1]], state))
            continue
        rows, states = per_batch.setdefault(where[1], ([], []))
        rows.append(where[2])
        states.append(state)
    ctx = getattr(r._backend, "ctx", None)
    for b in sorted(per_batch):
        rows, states = per_batch[b]
        _set_pool_state(ctx, L.seg_of[b], L.batches[b], rows, states)
        L.sync_pools(r.cfmms, b, rows)
    if ctx is None and per_batch:   # test-injected backends: the only door is a reload
        getattr(r._backend, "inner", r._backend).reload(r._batches)
    for pool, state in host:
        if callable(getattr(pool, "set_state_", None)):
            pool.set_state_(state)
        elif hasattr(pool, "R"):
            pool.R[:] = np.asarray(state, dtype=np.float64)
        else:
            raise ArgumentError(f"{type(pool).__name__} has neither set_state_(state) nor an R field")
    r._reset_trades()
    return None


def quote(r: Router, pools, coin_in, amount_in, coin_out=None):
    """Exact-input swap quotes on the pools as they stand on the device (cfmm_quote; forward_trade, src/cfmms.jl:436-449,
    for every device kind): what comes out of pool `pools[q]` for `amount_in[q]` of its coin `coin_in[q]`.

    `pools` are positions in `r.cfmms` (any order, repeats allowed: a ladder of sizes is the same pool many times);
    coin_in / coin_out are 0-based positions in the pool's own coin order (scalars serve every query); coin_out=None means
    the other coin of a two-coin or UniV3 pool.  The pools map to (segment, row) the way update_pools_ maps its changes,
    each segment's queries go through one call, and the results come back in the caller's order.  Read-only: the router's
    trades, prices and pools stay as they are.  A host-evaluated plugin pool has no device state to quote: ArgumentError."""
    return _quote(r, "quote", pools, coin_in, amount_in, coin_out)


def quote_out(r: Router, pools, coin_in, amount_out, coin_out=None):
    """Exact-output swap quotes, the inverse of `quote` (cfmm_quote_out): how much of its coin `coin_in[q]` pool `pools[q]`
    must be tendered so that exactly `amount_out[q]` of the coin out comes from it as it stands on the device.  Arguments,
    mapping of pool numbers to (segment, row), order of the results and the refusal of a host-evaluated pool are those of
    `quote`.  The answer is +inf where the pool cannot give that much."""
    return _quote(r, "quote_out", pools, coin_in, amount_out, coin_out)


def quote_rate(r: Router, pools, coin_in, amount_in, coin_out=None):
    """`quote` and the MARGINAL RATE of every query (cfmm_quote_rate): returns (amount_out, rate).  amount_out is `quote`'s
    answer bit for bit; rate[q] is the right derivative of the quote at amount_in[q] -- units of the coin out per unit of the
    coin in for the NEXT unit tendered, fee included; at amount 0 the pool's spot rate.  On UniV3 it is the rate of the tick
    the amount lands in (at an exact tick boundary the next tick's) and 0.0 once the ladder is exhausted.  Arguments, mapping
    of pool numbers to (segment, row), order of the results and the refusal of a host-evaluated pool are `quote`'s."""
    n = np.asarray(pools).size
    res = _quote(r, "quote_rate", pools, coin_in, amount_in, coin_out, answers=2)
    return res[:n], res[n:]


def spot_price(r: Router, pools=None, coin_in=0, coin_out=None):
    """The SPOT RATE of pools as they stand on the device, fee included: `quote_rate`'s rate at amount 0, without tendering
    anything (cfmm_quote_rate with no amounts).  pools=None: every device pool of the router, in `r.cfmms` order with NaN at
    host-evaluated pools, one dense coalesced call per segment; else positions in `r.cfmms` as `quote` takes them."""
    if pools is not None:
        n = np.asarray(pools).size
        return _quote(r, "quote_rate", pools, coin_in, None, coin_out, answers=2)[n:]
    ctx = _path_context(r)
    L = r._layout
    out = np.full(L.n_pools, np.nan)
    for seg, first, batch in L.segments():   # (packed position first + row is router position place[first + row])
        _, rate = ctx.quote_rate(seg, None, coin_in, coin_out, None, count=len(batch), want_out=False)
        out[L.place[first:first + len(batch)]] = rate
    return out


def price_impact(r: Router, pools, coin_in, amount_in, coin_out=None):
    """The PRICE IMPACT of every query: 1 − amount_out/(amount_in·spot), the share of the spot value the order loses to its own
    size -- 0.0 where amount_in is 0, NaN where the spot rate is 0 (no liquidity in the direction), rising with the amount.
    ONE device call of 2·count queries: the orders themselves and the same pools at amount 0.  `quote`'s arguments."""
    pools = np.asarray(pools, dtype=np.int64).reshape(-1)
    n = pools.size
    try:
        amt = np.ascontiguousarray(np.broadcast_to(np.asarray(amount_in, dtype=np.float64), (n,)))
        ci = np.broadcast_to(np.asarray(coin_in, dtype=np.int32), (n,))
        co = None if coin_out is None else np.broadcast_to(np.asarray(coin_out, dtype=np.int32), (n,))
    except ValueError:
        raise ArgumentError("amount_in, coin_in and coin_out must be scalars or have one entry per pool") from None
    out, rate = quote_rate(r, np.tile(pools, 2), np.tile(ci, 2), np.concatenate([amt, np.zeros(n)]),
                           None if co is None else np.tile(co, 2))
    return _impact(amt, out[:n], rate[n:])


def _impact(amt, out, spot):
    with np.errstate(all="ignore"):
        imp = 1.0 - out / (amt * spot)
    imp = np.where(amt == 0.0, 0.0, imp)
    return np.where(spot == 0.0, np.nan, imp)


def quote_path_rate(r: Router, pools, tokens, amount_in, hops=False):
    """`quote_path` and the MARGINAL RATE of every path (cfmm_quote_path_rate): returns (amount_out, rate[, hop_out, hop_rate]).
    amount_out / hop_out are `quote_path`'s bit for bit; hop_rate[k, p] is `quote_rate` of hop k at the amount entering it and
    rate[p] their product ((r_0·r_1)·r_2)... -- the chain rule: units of the last token per unit of the first for the next
    unit tendered.  A hop through an exhausted UniV3 ladder makes the path's rate 0.0.  Arguments and refusals are
    `quote_path`'s."""
    n_hops, seg, row, ci, co, amt, _ = _path_hops(r, "quote_path_rate", pools, tokens, amount_in)
    return _path_context(r).quote_path_rate(n_hops, seg, row, ci, co, amt, hops)


def path_price_impact(r: Router, pools, tokens, amount_in):
    """`price_impact` for paths: 1 − amount_out/(amount_in·spot) with spot the path's rate at amount 0, from ONE device call of
    2·count paths.  `quote_path`'s arguments."""
    pools, tokens = list(pools), list(tokens)
    n = len(pools)
    try:
        amt = np.ascontiguousarray(np.broadcast_to(np.asarray(amount_in, dtype=np.float64), (n,)))
    except ValueError:
        raise ArgumentError("amount_in must be a scalar or have one entry per path") from None
    out, rate = quote_path_rate(r, pools + pools, tokens + tokens, np.concatenate([amt, np.zeros(n)]))
    return _impact(amt, out[:n], rate[n:])


def swap_(r: Router, pools, coin_in, amount_in, coin_out=None, sync_host=True):
    """Exact-input swaps APPLIED to the pools on the device (cfmm_swap): `quote`'s arguments and mapping of pool numbers to
    (segment, row), but every swap moves its pool to R + γΔ − Λ (UniV3: to the price it rests at) and the next swap of the
    same pool starts from there -- "apply this pending swap, then route_ for the back-run".

    Each segment's swaps go through one call, in the caller's order within the segment, so a pool named k times is swapped
    k times in the order given; the amounts that came out return in the caller's order.  A swap that would leave an invalid
    pool (a reserve driven to 0, say) is not applied and answers NaN.  A host-evaluated plugin pool has no device state:
    ArgumentError, before anything moves.  sync_host=True (default) also refreshes the host mirror of the touched segments
    (`r.cfmms[i].R`, `current_price`).  The router's trades are those of the old market: they are zeroed, as by
    update_pools_."""
    try:
        return _quote(r, "swap", pools, coin_in, amount_in, coin_out, sync_host=sync_host)
    finally:
        r._reset_trades()


def swap_out_(r: Router, pools, coin_in, amount_out, coin_out=None, max_in=None, sync_host=True):
    """Exact-output swaps APPLIED to the pools on the device (cfmm_swap_out): `quote_out`'s arguments and mapping, but every
    swap moves its pool -- "I must receive exactly this much; take what it costs, unless it costs more than max_in".  The
    pool gives exactly `amount_out[q]` and takes what `quote_out` answers on the pool as the earlier swaps left it.

    Returns (amount_in, status) in the caller's order: status[q] is SWAP_APPLIED, SWAP_UNOBTAINABLE (the pool cannot give
    that much: +inf), SWAP_REFUSED (the swap would leave an invalid pool: NaN) or SWAP_OVER_LIMIT (amount_in[q] >
    max_in[q]: the quote it would have cost); in the last three the pool stays as it was.  max_in: None (no limit), a scalar
    or one limit per swap.  Order within a segment, the refusal of a host-evaluated pool, sync_host and the zeroing of the
    router's trades are `swap_`'s."""
    n = np.asarray(pools).size
    if max_in is not None:
        try:
            max_in = np.ascontiguousarray(np.broadcast_to(np.asarray(max_in, dtype=np.float64), (n,)))
        except ValueError:
            raise ArgumentError("max_in must be a scalar or have one entry per pool") from None
    status = np.empty(n, dtype=np.int32)
    try:
        return _quote(r, "swap_out", pools, coin_in, amount_out, coin_out, sync_host=sync_host, max_in=max_in, status=status), status
    finally:
        r._reset_trades()


def _limit_queries(r: Router, pools, token_in, token_out, *columns):
    """the single-pool limit calls' arguments: positions in `r.cfmms` and 1-based token ids (as in `Ai`) mapped to (batch, row,
    coin positions) with the refusals of `quote` and of the path calls; columns: (name, values) broadcast to one entry per pool.
    -> (n, {batch: (queries, rows)}, coin_in, coin_out, the columns)"""
    L = r._layout
    pools = np.asarray(pools, dtype=np.int64).reshape(-1)
    n = pools.size
    try:
        ti = np.broadcast_to(np.asarray(token_in, dtype=np.int64), (n,))
        to = np.broadcast_to(np.asarray(token_out, dtype=np.int64), (n,))
        cols = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for _, v in columns]
    except ValueError:
        names = ", ".join(name for name, _ in columns)
        raise ArgumentError(f"token_in, token_out, {names} must be scalars or have one entry per pool") from None
    ci, co = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    per_batch = {}
    for q, i in enumerate(pools.tolist()):
        where = L.locate(i)
        if where[0] == "host":
            raise ArgumentError(f"pool {i}: {type(r._host.pools[where[1]]).__name__} is evaluated on the host by its own "
                                f"find_arb_ and has no device state to quote")
        Ai = L.batches[where[1]].Ai[where[2]]
        pos = []
        for t in (int(ti[q]), int(to[q])):
            at = np.flatnonzero(Ai == t)
            if at.size == 0:
                raise ArgumentError(f"query {q}: token {t} is not a coin of pool {i} (its coins: {Ai.tolist()})")
            pos.append(int(at[0]))
        if pos[0] == pos[1]:
            raise ArgumentError(f"query {q}: token {int(ti[q])} on both sides of pool {i}")
        ci[q], co[q] = pos
        qs, rows = per_batch.setdefault(where[1], ([], []))
        qs.append(q)
        rows.append(where[2])
    if getattr(r._backend, "ctx", None) is None and per_batch:
        raise NotImplementedError(f"{type(r._backend).__name__} has no device context to quote on")
    return n, per_batch, ci, co, cols


def amount_to_rate(r: Router, pools, token_in, token_out, rate):
    """The inverse of `quote_rate` (cfmm_quote_to_rate): how much of token `token_in[q]` pool `pools[q]` takes before its
    marginal rate -- units of `token_out[q]` per unit tendered, fee included -- has fallen to `rate[q]`, on the pools as they
    stand on the device.  Returns (amount_in, amount_out): amount_in is exactly 0.0 where the spot rate is already at or
    below the limit; amount_out is what `quote` answers for amount_in, bit for bit.  The rate the pool would rest at is the
    limit to rounding and may lie an ulp-scale amount below it: a strict caller passes a margin.

    `pools` are positions in `r.cfmms` (any order, repeats allowed); token_in / token_out are token ids, 1-based as in `Ai`
    (scalars serve every query); rate must be finite and > 0.  ArgumentError for a token that is not one of the pool's coins or
    is the same on both sides, and for a host-evaluated plugin pool.  Read-only, like `quote`."""
    n, per_batch, ci, co, (lim,) = _limit_queries(r, pools, token_in, token_out, ("rate", rate))
    ctx, L = r._backend.ctx if per_batch else None, r._layout
    amt, out = np.empty(n), np.empty(n)
    for b in sorted(per_batch):
        qs, rows = per_batch[b]
        amt[qs], out[qs] = ctx.quote_to_rate(L.seg_of[b], lim[qs], ci[qs], co[qs], rows)
    return amt, out


def swap_limit_(r: Router, pools, token_in, token_out, amount_in, rate_limit, sync_host=True):
    """Price-limited swaps APPLIED to the pools on the device (cfmm_swap_limit): "sell up to amount_in[q] of token_in[q] into
    pool pools[q], but stop where its marginal rate reaches rate_limit[q]".  Swap q tenders min(amount_in[q], what
    `amount_to_rate` answers on the pool as the earlier swaps left it); the amount out and the pool's new state are `swap_`'s
    for the amount used.  rate_limit 0.0 means no limit (the swap is `swap_`'s); amount_in may be inf -- "as much as it
    takes" -- where the limit is > 0: that moves the pool to an outside price.

    Returns (amount_used, amount_out, status) in the caller's order: LIMIT_FILLED (all of amount_in), LIMIT_PARTIAL (the pool
    rests at the limit, to rounding), LIMIT_NONE (the spot rate is already at or below the limit, or amount_in is 0: nothing
    moved) or LIMIT_REFUSED (the swap would leave an invalid pool: NaN, nothing moved).  Pools and tokens as `amount_to_rate`
    takes them; order within a segment, sync_host and the zeroing of the router's trades are `swap_`'s."""
    try:
        n, per_batch, ci, co, (amt, lim) = _limit_queries(r, pools, token_in, token_out, ("amount_in", amount_in), ("rate_limit", rate_limit))
        ctx, L = r._backend.ctx if per_batch else None, r._layout
        used, out, status = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        for b in sorted(per_batch):
            qs, rows = per_batch[b]
            used[qs], out[qs], status[qs] = ctx.swap_limit(L.seg_of[b], amt[qs], lim[qs], ci[qs], co[qs], rows)
            if sync_host:
                _download_state(ctx, L.seg_of[b], L.batches[b])
                L.sync_pools(r.cfmms, b, sorted(set(rows)))
        return used, out, status
    finally:
        r._reset_trades()


def _quote(r: Router, verb, pools, coin_in, amount, coin_out, sync_host=False, max_in=None, status=None, answers=1):
    """answers=2 (quote_rate): the context returns (amount_out, rate) and the result is [2n], the rates behind the amounts;
    amount=None there: no amounts (the spot rate), the first half stays NaN"""
    L = r._layout
    pools = np.asarray(pools, dtype=np.int64).reshape(-1)
    n = pools.size
    try:
        amt = None if amount is None else np.ascontiguousarray(np.broadcast_to(np.asarray(amount, dtype=np.float64), (n,)))
        ci = np.ascontiguousarray(np.broadcast_to(np.asarray(coin_in, dtype=np.int32), (n,)))
        co = None if coin_out is None else np.ascontiguousarray(np.broadcast_to(np.asarray(coin_out, dtype=np.int32), (n,)))
    except ValueError:
        raise ArgumentError(f"{'amount_out' if verb in ('quote_out', 'swap_out') else 'amount_in'}, coin_in and coin_out must be scalars or have one entry per pool") from None
    per_batch = {}
    for q, i in enumerate(pools):
        where = L.locate(i)
        if where[0] == "host":
            raise ArgumentError(f"pool {int(i)}: {type(r._host.pools[where[1]]).__name__} is evaluated on the host by its own "
                                f"find_arb_ and has no device state to quote")
        qs, rows = per_batch.setdefault(where[1], ([], []))
        qs.append(q)
        rows.append(where[2])
    ctx = getattr(r._backend, "ctx", None)
    if ctx is None and per_batch:
        raise NotImplementedError(f"{type(r._backend).__name__} has no device context to quote on")
    out = np.empty(n) if answers == 1 else np.full(2 * n, np.nan)
    for b in sorted(per_batch):
        qs, rows = per_batch[b]
        if answers == 2:   # quote_rate / spot_price
            a_out, rate = ctx.quote_rate(L.seg_of[b], None if amt is None else amt[qs], ci[qs], None if co is None else co[qs], rows,
                                         count=len(qs), want_out=amt is not None)
            if a_out is not None:
                out[qs] = a_out
            out[n + np.asarray(qs, dtype=np.int64)] = rate
        elif status is not None:   # swap_out_
            out[qs], status[qs] = ctx.swap_out(L.seg_of[b], amt[qs], ci[qs], None if co is None else co[qs], rows,
                                               None if max_in is None else max_in[qs], True)
        else:
            out[qs] = getattr(ctx, verb)(L.seg_of[b], amt[qs], ci[qs], None if co is None else co[qs], rows)
        if sync_host:   # (swap_: the host mirror of the segment follows the device)
            _download_state(ctx, L.seg_of[b], L.batches[b])
            L.sync_pools(r.cfmms, b, sorted(set(rows)))
    return out


def quote_path(r: Router, pools, tokens, amount_in, hops=False):
    """Exact-input quotes of swap PATHS on the pools as they stand on the device (cfmm_quote_path): `amount_in[p]` of token
    `tokens[p][0]` goes into pool `pools[p][0]`, what comes out goes into `pools[p][1]`, ... and the result is what leaves
    the path's last pool, in one launch for all paths whatever kinds the pools are.

    `pools[p]` is a sequence of 1 .. 8 positions in `r.cfmms`; `tokens[p]` the token ids along the path (1-based as in
    `Ai`), one more than the pools: hop k trades `tokens[p][k]` for `tokens[p][k+1]`.  Paths may differ in length.
    EVERY HOP IS QUOTED AGAINST THE POOL AS IT STANDS -- no state advances between hops -- which is why a pool may appear
    only once in a path.  ArgumentError (naming path and hop) for a token that is not one of the pool's coins or is the same
    on both sides, a repeated pool, a host-evaluated pool, or more than 8 pools.  hops=True: also the [max_hops, count]
    amounts leaving each hop (NaN where a path has no such hop).  Read-only, like `quote`."""
    return _quote_path(r, "quote_path", pools, tokens, amount_in, hops)


def quote_path_out(r: Router, pools, tokens, amount_out, hops=False):
    """Exact-output quotes of swap paths, the inverse of `quote_path` (cfmm_quote_path_out): how much of `tokens[p][0]`
    must be tendered to `pools[p][0]` so that exactly `amount_out[p]` of `tokens[p][-1]` leaves the path's last pool, walked
    from the last hop backwards.  +inf where a pool on the way cannot give that much.  Arguments and refusals are those of
    `quote_path`; hops=True: also the [max_hops, count] amounts to tender to each hop."""
    return _quote_path(r, "quote_path_out", pools, tokens, amount_out, hops)


def swap_path_(r: Router, pools, tokens, amount_in, min_out=None, hops=False, sync_host=True):
    """Swap PATHS APPLIED to the pools on the device (cfmm_swap_path): `quote_path`'s arguments, mapping and refusals, but the
    paths are executed in the order given, each ALL OR NOTHING -- "make this cycle, but only if at least this much comes out".
    Path p sees the market as the applied paths before it left it; an applied path's amounts are what `quote_path` answers on
    that market, and each of its pools moves as `swap_` moves it.

    Returns (amount_out, status[, hop_out]): status[p] is PATH_APPLIED, PATH_BELOW_LIMIT (amount_out[p] < min_out[p]: the
    quote it would have given; nothing moved) or PATH_REFUSED (a hop would leave an invalid pool: NaN; nothing moved).
    min_out: None (no limit), a scalar or one limit per path.  Unlike a chain of `swap_` calls, paths that share pools need no
    ordering by hand and a path refused at its third hop has nothing to unwind.  sync_host=True (default) also refreshes the
    host mirror of the touched segments (`r.cfmms[i].R`, `current_price`).  The router's trades are those of the old market:
    they are zeroed, as by swap_."""
    return _swap_path(r, "swap_path", "min_out", pools, tokens, amount_in, min_out, hops, sync_host)


def swap_path_out_(r: Router, pools, tokens, amount_out, max_in=None, hops=False, sync_host=True):
    """Exact-output swap PATHS APPLIED to the pools on the device (cfmm_swap_path_out): `quote_path_out`'s arguments, mapping
    and refusals, but the paths are executed in the order given, each ALL OR NOTHING -- "buy exactly this much through
    A -> B -> C, but only if it costs at most max_in".  Path p sees the market as the applied paths before it left it; its
    amounts are what `quote_path_out` answers on that market, and each pool of an applied path moves as `swap_out_` moves it.

    Returns (amount_in, status[, hop_in]): status[p] is SWAP_APPLIED, SWAP_UNOBTAINABLE (a pool on the way cannot give that
    much: +inf), SWAP_REFUSED (a hop would leave an invalid pool: NaN) or SWAP_OVER_LIMIT (amount_in[p] > max_in[p]: the
    quote it would have cost); in the last three nothing moved.  max_in: None (no limit), a scalar or one limit per path.
    sync_host and the zeroing of the router's trades are `swap_path_`'s."""
    return _swap_path(r, "swap_path_out", "max_in", pools, tokens, amount_out, max_in, hops, sync_host)


def find_path(r: Router, token_in, token_out, amount_in, max_hops=3):
    """The best swap path from `token_in[q]` to `token_out[q]` (token ids 1-based as in `Ai`) for `amount_in[q]`, of at most
    `max_hops` (1 .. 8) pools, FOUND on the device among the pools as they stand there (cfmm_find_path) -- "I have 1000 of A and
    want C: through which pools, and how much do I get?".  Scalars broadcast.

    Returns (amount_out, pools, tokens, status): `pools[q]` / `tokens[q]` are in the form `quote_path` / `swap_path_` accept
    (positions in `r.cfmms`; the token ids along the path, one more than the pools), empty where nothing was found.
    The contract is the layered search: layer h holds per token the largest quote over every pool and ordered coin pair from
    layer h-1, every hop quoted AGAINST THE POOL AS IT STANDS; the answer is the largest layer entry of token_out with the
    fewest hops, ties broken towards the smallest (segment, row, coin_in, coin_out) -- `quote_path(r, pools, tokens, amount_in)`
    answers `amount_out` bit for bit.  What is found is a walk: status[q] is FOUND, FOUND_NONE (token_out not reached within
    max_hops, or amount 0: amount_out 0.0) or FOUND_REPEATS (the walk visits a pool twice; `quote_path` and `swap_path_` refuse
    it as one path).  Host-evaluated plugin pools have no device state and are NOT searched.  Read-only, like `quote`."""
    return _find_path(r, "find_path", "amount_in", token_in, token_out, amount_in, max_hops)


def find_path_out(r: Router, token_in, token_out, amount_out, max_hops=3):
    """The CHEAPEST swap path that buys exactly `amount_out[q]` of `token_out[q]`, paid in `token_in[q]` (token ids 1-based as in
    `Ai`), of at most `max_hops` (1 .. 8) pools, FOUND on the device among the pools as they stand there (cfmm_find_path_out) --
    "buy exactly 1000 of C, pay in A: through which pools, and what does it cost?".  Scalars broadcast.  The best path for an
    input amount is not the cheapest path for an output amount; this is `find_path`'s search run backwards from the output.

    Returns (amount_in, pools, tokens, status): `pools[q]` / `tokens[q]` are in the form `quote_path_out` / `swap_path_out_`
    accept (positions in `r.cfmms`; the token ids along the path from token_in to token_out, one more than the pools), empty
    where nothing was found.  The contract is the layered search: layer h holds per token the smallest `quote_out` over every
    pool and ordered coin pair into layer h-1, every hop quoted AGAINST THE POOL AS IT STANDS; the answer is the smallest layer
    entry of token_in with the fewest hops, ties broken towards the smallest (segment, row, coin_in, coin_out) walking forward
    -- `quote_path_out(r, pools, tokens, amount_out)` answers `amount_in` bit for bit, and `swap_path_out_` with
    `max_in=amount_in` executes it.  status[q] is FOUND, FOUND_REPEATS (the walk visits a pool twice; `quote_path_out` and
    `swap_path_out_` refuse it as one path) or FOUND_NONE, with amount_in +inf (token_in not reached within max_hops: no pool
    can give that much) or 0.0 (amount_out 0: nothing to buy).  Host-evaluated plugin pools have no device state: they are
    NOT searched.  Read-only, like `quote_out`."""
    return _find_path(r, "find_path_out", "amount_out", token_in, token_out, amount_out, max_hops)


def size_path(r: Router, pools, tokens, max_in, value_in=None, value_out=None, rounds=5):
    """HOW MUCH to put into swap paths, on the pools as they stand on the device (cfmm_size_path): `quote_path`'s `pools` and
    `tokens`, mapping and refusals (a token break, a repeated pool, a host-evaluated pool), and per path the largest input
    `max_in[p]` to consider.  Returns (amount_in, amount_out, gain, status): the input of each path that maximises
    gain(x) = value_out[p] * quote_path(x) - value_in[p] * x, what `quote_path` answers for it bit for bit, and that gain.
    value_in / value_out: None (1.0: "out minus in", the profit of a cycle), a scalar or one value per path -- what a unit of
    the path's first and last token is worth elsewhere, for a path that is no cycle.

    The contract is the bracketing search: `rounds` (1 .. 16) rounds of 64 trial sizes spread evenly over a bracket that starts
    as [0, max_in] and becomes the two neighbours of the best trial size.  A path's gain is concave, so the bracket shrinks by
    2/63 per round around the maximiser; the default 5 rounds reach the closed-form optimum of two-pool cycles to about 1e-12 of
    its gain.  status[p] is SIZED, SIZED_AT_LIMIT (gain > 0 at amount_in == max_in: the limit binds), SIZED_NONE (no size gains:
    three 0.0) or SIZED_NAN.  It sizes ONE path on the STANDING market: it does not split an amount over several paths
    (`split_paths` does).
    `swap_path_(r, pools, tokens, amount_in, min_out=...)` executes the answer.  Read-only, like `quote`."""
    n_hops, seg, row, ci, co, lim, _ = _path_hops(r, "size_path", pools, tokens, max_in, "max_in")
    return _path_context(r).size_path(n_hops, seg, row, ci, co, lim, value_in, value_out, rounds)


def split_paths(r: Router, pools, tokens, amount_in, rounds=5):
    """HOW MUCH OF AN ORDER GOES DOWN EACH PATH, on the pools as they stand on the device (cfmm_split_paths) -- "I have A of X and
    these K routes to Y; how much goes down each?".  `pools[g]` is a list of 1 .. 8 paths, each a list of positions in `r.cfmms`;
    `tokens[g][k]` the token ids along path k (1-based as in `Ai`, one more than the pools); `amount_in[g]` the amount of
    order g (a scalar broadcasts).  The mapping and the refusals are `quote_path`'s (a token break, a repeated pool, a
    host-evaluated pool, named by the path's number in the whole call), and two more: every path of an order must start at
    the same token and end at the same token, and no pool may occur twice in an order -- the paths are quoted independently
    against the standing market, so a shared pool would be counted twice.

    Returns (path_amount_in, path_amount_out, total_out, status): the first two are lists shaped like `pools` (one array per
    order), the last two arrays with one entry per order.  The contract is the greedy search with scaling: `rounds` (1 .. 16)
    rounds of 64 grid points per path; a round hands out 63 slices of what is left, each to the path whose next slice buys the
    most, then steps every share back one slice and refines.  The shares sum to the amount; `quote_path` at a share answers
    its output bit for bit.  On 4000 random orders of product chains the default 5 rounds were within 8e-12 of the
    closed-form optimum for 99 % of the orders and within 1.6e-7 for all.  status[g] is SPLIT_OK, SPLIT_SATURATED (part of the
    amount buys nothing: the paths cannot absorb it), SPLIT_NONE (amount 0, or nothing comes out: zeros) or SPLIT_NAN.
    `swap_path_(r, pools[g], tokens[g], path_amount_in[g])` executes order g's split.  Read-only, like `quote`."""
    return _split_paths(r, "split_paths", "amount_in", pools, tokens, amount_in, rounds)


def split_paths_out(r: Router, pools, tokens, amount_out, rounds=5):
    """HOW MUCH OF A WANTED AMOUNT COMES OUT OF EACH PATH, on the pools as they stand on the device (cfmm_split_paths_out) -- "I
    want B of Y and have these K routes from X; how much do I buy through each?".  `pools`, `tokens`, the mapping and every
    refusal are `split_paths`'; `amount_out[g]` is the amount of the paths' common last token that order g buys (a scalar
    broadcasts).

    Returns (path_amount_out, path_amount_in, total_in, status): the first two are lists shaped like `pools` (the share of
    `amount_out[g]` bought through each path, and what `quote_path_out` answers for it bit for bit), the last two arrays with
    one entry per order.  The contract is `split_paths`' greedy search laid over the output: a round hands out 63 slices of what
    is left, each to the path whose next slice COSTS the least (+inf where a path cannot give that much), then steps every share
    back one slice and refines.  status[g] is SPLIT_OK; SPLIT_UNOBTAINABLE (a step found no path that can give another slice:
    costs and total +inf, shares 0.0 -- the search's verdict on its grid: paths that jointly give less than
    amount_out * (1 + K/63) may be refused though a finer split exists); SPLIT_NONE (amount 0: zeros) or SPLIT_NAN.  Three paths
    that can each give half of B fill an order that `quote_path_out` answers +inf for on every one of them.
    `swap_path_out_(r, pools[g], tokens[g], path_amount_out[g], max_in=path_amount_in[g])` executes order g's split.  Read-only,
    like `quote`."""
    return _split_paths(r, "split_paths_out", "amount_out", pools, tokens, amount_out, rounds)


def _split_paths(r: Router, verb, amount_name, pools, tokens, amount_in, rounds):
    pools, tokens = [list(o) for o in pools], [list(o) for o in tokens]
    if len(tokens) != len(pools):
        raise ArgumentError("tokens must have one list of paths per order")
    try:
        amt = np.ascontiguousarray(np.broadcast_to(np.asarray(amount_in, dtype=np.float64), (len(pools),)))
    except ValueError:
        raise ArgumentError(f"{amount_name} must be a scalar or have one entry per order") from None
    first, (n_hops, seg, row, ci, co, _, _) = _order_hops(r, verb, pools, tokens, 0.0)
    x, y, total, status = getattr(_path_context(r), verb)(first, amt, n_hops, seg, row, ci, co, rounds)
    cut = lambda v: [v[first[g]:first[g + 1]] for g in range(len(pools))]
    return cut(x), cut(y), total, status


def _order_hops(r: Router, verb, pools, tokens, path_amount):
    """(pools, tokens) of the order calls -- per order a list of paths -- as `order_first` and `_path_hops`' answer for the flat
    paths, with every refusal the router makes of an order; path_amount: a scalar or one entry per path of the whole call"""
    for g, (pl, tk) in enumerate(zip(pools, tokens)):
        if not 1 <= len(pl) <= MAX_SPLIT_PATHS:
            raise ArgumentError(f"order {g}: {len(pl)} paths (an order has 1 to {MAX_SPLIT_PATHS})")
        if len(tk) != len(pl):
            raise ArgumentError(f"order {g}: {len(tk)} token sequences for {len(pl)} paths")
    first = np.concatenate(([0], np.cumsum([len(pl) for pl in pools]))).astype(np.int64)
    flat_pools, flat_tokens = [p for pl in pools for p in pl], [t for tk in tokens for t in tk]
    hops = _path_hops(r, verb, flat_pools, flat_tokens, path_amount)
    for g, (pl, tk) in enumerate(zip(pools, tokens)):
        ends = {(int(np.asarray(t).reshape(-1)[0]), int(np.asarray(t).reshape(-1)[-1])) for t in tk}
        if len(ends) != 1:
            raise ArgumentError(f"order {g}: its paths must all start at the same token and end at the same token (got {sorted(ends)})")
        seen = {}
        for k, path in enumerate(pl):
            for i in np.asarray(path, dtype=np.int64).reshape(-1).tolist():
                if i in seen:
                    raise ArgumentError(f"order {g}: paths {seen[i]} and {k} share pool {i} (the paths are quoted independently "
                                        f"against the standing market, so a shared pool would be counted twice)")
                seen[i] = k
    return first, hops


def swap_order_(r: Router, pools, tokens, path_amount_in, min_total_out=None, hops=False, sync_host=True):
    """ORDERS APPLIED to the pools on the device, each ALL OR NOTHING ACROSS ITS PATHS (cfmm_swap_order) -- "send this order down
    these K routes, but only if at least this much comes out in total".  `pools[g]` and `tokens[g]` are lists of paths exactly as
    `split_paths` takes (and answers) them, with its refusals and `swap_path_`'s; `path_amount_in[g]` the amount going down each
    path of order g, as `split_paths` returns it.  The orders are executed in the order given; order g sees the market as the
    applied orders before it left it, every path is walked as `swap_path_` walks it, and only when no path refuses and the
    total clears the limit does anything move -- then every pool moves as `swap_path_` moves it.

    Returns (path_amount_out, total_out, status, path_status[, hop_out]): the first and `path_status` are lists shaped like
    `pools`.  total_out[g] is the paths' outputs added in path order (on an unmoved market `split_paths`' total_out bit for
    bit).  status[g] is ORDER_APPLIED, ORDER_LIMIT (total_out[g] < min_total_out[g]: nothing moved) or ORDER_REFUSED (some path
    has a refusing hop: NaN, nothing moved); path_status is PATH_APPLIED, PATH_REFUSED or ORDER_PATH_HELD (the path passes, its
    order was not applied).  min_total_out: None (no limit), a scalar or one limit per order.  Unlike `swap_path_` on the
    order's paths, a later order that an earlier one has moved out of its limit leaves NO path executed.  sync_host and the
    zeroing of the router's trades are `swap_path_`'s."""
    return _swap_order(r, "swap_order", "min_total_out", pools, tokens, path_amount_in, min_total_out, hops, sync_host)


def swap_order_out_(r: Router, pools, tokens, path_amount_out, max_total_in=None, hops=False, sync_host=True):
    """The exact-output twin of `swap_order_` (cfmm_swap_order_out): `path_amount_out[g]` is what each path of order g is to
    give, as `split_paths_out` returns it; every path is walked as `swap_path_out_` walks it.  Returns (path_amount_in, total_in,
    status, path_status[, hop_in]); status[g] may also be ORDER_UNOBTAINABLE (some path cannot give its amount: total_in +inf,
    that path's path_status SWAP_UNOBTAINABLE; nothing moved), and ORDER_LIMIT is total_in[g] > max_total_in[g]."""
    return _swap_order(r, "swap_order_out", "max_total_in", pools, tokens, path_amount_out, max_total_in, hops, sync_host)


def _swap_order(r: Router, verb, limit_name, pools, tokens, path_amount, limit, hops, sync_host):
    pools, tokens = [list(o) for o in pools], [list(o) for o in tokens]
    if len(tokens) != len(pools):
        raise ArgumentError("tokens must have one list of paths per order")
    amount_name = "path_amount_out" if verb.endswith("_out") else "path_amount_in"
    if np.isscalar(path_amount) or isinstance(path_amount, np.ndarray) and path_amount.ndim == 0:
        flat = float(path_amount)
    else:
        per_order = list(path_amount)
        if len(per_order) != len(pools) or any(np.size(a) != len(pl) for a, pl in zip(per_order, pools)):
            raise ArgumentError(f"{amount_name} must be a scalar or have one entry per path, shaped like pools")
        flat = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in per_order]) if per_order else np.empty(0)
    first, (n_hops, seg, row, ci, co, amt, touched) = _order_hops(r, verb, pools, tokens, flat)
    if limit is not None:
        try:
            limit = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, dtype=np.float64), (len(pools),)))
        except ValueError:
            raise ArgumentError(f"{limit_name} must be a scalar or have one entry per order") from None
    ctx = _path_context(r)
    L = r._layout
    cut = lambda v: [v[first[g]:first[g + 1]] for g in range(len(pools))]
    try:
        res = getattr(ctx, verb)(first, n_hops, seg, row, ci, co, amt, limit, hops)
        if sync_host:
            for b in sorted(touched):
                _download_state(ctx, L.seg_of[b], L.batches[b])
                L.sync_pools(r.cfmms, b, sorted(touched[b]))
        return (cut(res[0]), res[1], res[2], cut(res[3])) + tuple(res[4:])
    finally:
        r._reset_trades()


def route_order_(r: Router, token_in, token_out, amount_in, max_slippage=0.0, max_paths=4, max_hops=3, rounds=5, probe=None, sync_host=True):
    """find -> split -> EXECUTE in one call: `route_order`, then `swap_order_` on what it answered with
    min_total_out = total_out * (1 - max_slippage).  Orders for which nothing was found (or whose split is not SPLIT_OK /
    SPLIT_SATURATED) are not sent to the device: their executed total is 0.0, their status ORDER_REFUSED and their lists empty.
    Returns `route_order`'s six answers, then (path_amount_out, total_out, status, path_status) as executed."""
    if not 0.0 <= float(max_slippage) < 1.0:
        raise ArgumentError("max_slippage must be in [0, 1)")
    pools, tokens, x, y, total, split_status = route_order(r, token_in, token_out, amount_in, max_paths, max_hops, rounds, probe)
    limit = total * (1.0 - float(max_slippage))
    return (pools, tokens, x, y, total, split_status) + _execute_routed(r, swap_order_, pools, tokens, x, limit, split_status, sync_host)


def route_order_out_(r: Router, token_in, token_out, amount_out, max_slippage=0.0, max_paths=4, max_hops=3, rounds=5, probe=None, sync_host=True):
    """The exact-output twin of `route_order_`: `route_order_out`, then `swap_order_out_` with
    max_total_in = total_in * (1 + max_slippage).  Returns `route_order_out`'s six answers, then (path_amount_in, total_in,
    status, path_status) as executed."""
    if not float(max_slippage) >= 0.0:
        raise ArgumentError("max_slippage must be >= 0")
    pools, tokens, x, y, total, split_status = route_order_out(r, token_in, token_out, amount_out, max_paths, max_hops, rounds, probe)
    limit = total * (1.0 + float(max_slippage))
    return (pools, tokens, x, y, total, split_status) + _execute_routed(r, swap_order_out_, pools, tokens, x, limit, split_status, sync_host)


def _execute_routed(r: Router, execute, pools, tokens, shares, limit, split_status, sync_host):
    n = len(pools)
    send = [g for g in range(n) if pools[g] and split_status[g] in (SPLIT_OK, SPLIT_SATURATED)]
    out, pst = [np.empty(0) for _ in range(n)], [np.empty(0, dtype=np.int32) for _ in range(n)]
    total, status = np.zeros(n), np.full(n, ORDER_REFUSED, dtype=np.int32)
    if send:
        o, total[send], status[send], ps = execute(r, [pools[g] for g in send], [tokens[g] for g in send], [shares[g] for g in send],
                                                   limit[send], sync_host=sync_host)
        for g, og, pg in zip(send, o, ps):
            out[g], pst[g] = og, pg
    return out, total, status, pst


def _find_path(r: Router, verb, amount_name, token_in, token_out, amount, max_hops):
    L = r._layout
    try:
        tin, tout, amt = np.broadcast_arrays(np.asarray(token_in, dtype=np.int64).reshape(-1), np.asarray(token_out, dtype=np.int64).reshape(-1),
                                             np.asarray(amount, dtype=np.float64).reshape(-1))
    except ValueError:
        raise ArgumentError(f"token_in, token_out and {amount_name} must be scalars or have one entry per query") from None
    for name, t in (("token_in", tin), ("token_out", tout)):
        bad = np.flatnonzero((t < 1) | (t > r.n_tokens))
        if bad.size:
            raise ArgumentError(f"query {int(bad[0])}: {name} {int(t[bad[0]])} out of range 1:{r.n_tokens}")
    out, n_hops, seg, row, ci, co, status = getattr(_path_context(r), verb)(tin - 1, tout - 1, amt, max_hops)
    batch_of = {s: b for b, s in L.seg_of.items()}
    pools, tokens = [], []
    for q in range(len(out)):
        pl, tk = _found_path(L, batch_of, int(tin[q]), int(n_hops[q]), seg[q], row[q], co[q])
        pools.append(pl)
        tokens.append(tk)
    return out, pools, tokens, status


def _found_path(L, batch_of, token_in, n_hops, seg, row, co):
    """a found path's hops (segment, row, coin_out) as positions in r.cfmms and the 1-based token ids along it; two empty lists
    where nothing was found"""
    pl, tk = [], [token_in] if n_hops else []
    for k in range(n_hops):
        b = batch_of[int(seg[k])]
        pl.append(int(L.place[int(L.offsets[b]) + int(row[k])]))
        tk.append(int(L.batches[b].Ai[int(row[k]), int(co[k])]))
    return pl, tk


def find_disjoint_paths(r: Router, token_in, token_out, amount_in, max_paths=4, max_hops=3, usable_only=True):
    """SEVERAL swap paths per order that share no pool, FOUND on the device (cfmm_find_disjoint_paths) -- "I have A of X and want
    Y: which routes are there?", the link between `find_path` (one path) and `split_paths` (an order spread over the paths it is
    given).  For every query up to `max_paths` (1 .. 8) paths from `token_in[q]` to `token_out[q]` (1-based as in `Ai`) of at most
    `max_hops` pools.  Scalars broadcast.

    Returns (amount_out, pools, tokens, status): `pools[q]` / `tokens[q]` are LISTS OF PATHS, exactly the `pools[g]` / `tokens[g]`
    that `split_paths` takes (and each path what `quote_path` / `swap_path_` take); `amount_out[q]` and `status[q]` are arrays with
    one entry per listed path.  The contract is successive search: path r is `find_path`'s answer for `amount_in[q]` on the market
    without every pool of the query's paths before it -- the best path, the best one that avoids it, and so on; greedy, not "the K
    best overall".  The first path is `find_path`'s, the amounts do not increase along the list, and `quote_path` at `amount_in[q]`
    answers each bit for bit.  The same amount probes every round: to split A over K paths, A / K may be the better probe.
    usable_only=True (the default) leaves out paths whose status is FOUND_REPEATS (a walk that visits a pool twice: `split_paths`
    would refuse it; its pools stay banned for the paths after it); with False they are listed with their status.  A query for
    which nothing is found has empty lists.  Host-evaluated plugin pools are NOT searched.  Read-only, like `quote`."""
    return _find_disjoint(r, "find_disjoint_paths", "amount_in", token_in, token_out, amount_in, max_paths, max_hops, usable_only)


def find_disjoint_paths_out(r: Router, token_in, token_out, amount_out, max_paths=4, max_hops=3, usable_only=True):
    """SEVERAL swap paths per order that share no pool, FOUND on the device FOR A WANTED OUTPUT (cfmm_find_disjoint_paths_out) -- "I
    want B of Y and pay in X: which routes are there?", the link between `find_path_out` (one path) and `split_paths_out`.
    `find_disjoint_paths`' arguments and answer with the direction turned: returns (amount_in, pools, tokens, status), `pools[q]` /
    `tokens[q]` lists of paths as `split_paths_out` takes them, `amount_in[q]` what each listed path asks for `amount_out[q]`.
    Path r is `find_path_out`'s answer on the market without every pool of the query's paths before it: the first path is
    `find_path_out`'s, the amounts do not decrease along the list, and `quote_path_out` at `amount_out[q]` answers each bit for
    bit.  The same amount probes every round, and A PATH THAT CANNOT GIVE IT ALONE IS NEVER FOUND: to buy B through K paths probe
    with about B / K (`route_order_out` does).  usable_only as in `find_disjoint_paths`.  Read-only, like `quote`."""
    return _find_disjoint(r, "find_disjoint_paths_out", "amount_out", token_in, token_out, amount_out, max_paths, max_hops, usable_only)


def _find_disjoint(r: Router, verb, amount_name, token_in, token_out, amount_in, max_paths, max_hops, usable_only):
    L = r._layout
    try:
        tin, tout, amt = np.broadcast_arrays(np.asarray(token_in, dtype=np.int64).reshape(-1), np.asarray(token_out, dtype=np.int64).reshape(-1),
                                             np.asarray(amount_in, dtype=np.float64).reshape(-1))
    except ValueError:
        raise ArgumentError(f"token_in, token_out and {amount_name} must be scalars or have one entry per query") from None
    for name, t in (("token_in", tin), ("token_out", tout)):
        bad = np.flatnonzero((t < 1) | (t > r.n_tokens))
        if bad.size:
            raise ArgumentError(f"query {int(bad[0])}: {name} {int(t[bad[0]])} out of range 1:{r.n_tokens}")
    n_paths, out, n_hops, seg, row, ci, co, status = getattr(_path_context(r), verb)(tin - 1, tout - 1, amt, max_paths, max_hops)
    batch_of = {s: b for b, s in L.seg_of.items()}
    amounts, pools, tokens, statuses = [], [], [], []
    for q in range(len(n_paths)):
        keep = [k for k in range(int(n_paths[q])) if not (usable_only and status[q, k] == FOUND_REPEATS)]
        found = [_found_path(L, batch_of, int(tin[q]), int(n_hops[q, k]), seg[q, k], row[q, k], co[q, k]) for k in keep]
        pools.append([pl for pl, _ in found])
        tokens.append([tk for _, tk in found])
        amounts.append(out[q, keep])
        statuses.append(status[q, keep])
    return amounts, pools, tokens, statuses


def route_order(r: Router, token_in, token_out, amount_in, max_paths=4, max_hops=3, rounds=5, probe=None):
    """find -> split in one call: `find_disjoint_paths` (probed with `probe`, by default the order's amount) and `split_paths` on
    what it found.  Returns (pools, tokens, path_amount_in, path_amount_out, total_out, status): per order the list of paths and
    the share and output of each, then the total and the SPLIT_* status, as `split_paths` answers them.  An order for which
    nothing is found has empty lists, total 0.0 and SPLIT_NONE, and is not sent to `split_paths`.  Nothing is executed:
    `swap_path_(r, pools[g], tokens[g], path_amount_in[g])` executes order g.  Scalars broadcast."""
    try:
        tin, tout, amt = np.broadcast_arrays(np.asarray(token_in).reshape(-1), np.asarray(token_out).reshape(-1),
                                             np.asarray(amount_in, dtype=np.float64).reshape(-1))
        look = amt if probe is None else np.broadcast_to(np.asarray(probe, dtype=np.float64).reshape(-1), amt.shape)
    except ValueError:
        raise ArgumentError("token_in, token_out, amount_in and probe must be scalars or have one entry per order") from None
    _, pools, tokens, _ = find_disjoint_paths(r, tin, tout, look, max_paths, max_hops, usable_only=True)
    n = len(pools)
    have = [g for g in range(n) if pools[g]]
    x, y = [np.empty(0) for _ in range(n)], [np.empty(0) for _ in range(n)]
    total, status = np.zeros(n), np.full(n, SPLIT_NONE, dtype=np.int32)
    if have:
        xs, ys, total[have], status[have] = split_paths(r, [pools[g] for g in have], [tokens[g] for g in have], amt[have], rounds)
        for g, xg, yg in zip(have, xs, ys):
            x[g], y[g] = xg, yg
    return pools, tokens, x, y, total, status


def route_order_out(r: Router, token_in, token_out, amount_out, max_paths=4, max_hops=3, rounds=5, probe=None):
    """find -> split in one call for an order that BUYS an exact amount: `find_disjoint_paths_out` (probed with `probe`) and
    `split_paths_out` on what it found.  Returns (pools, tokens, path_amount_out, path_amount_in, total_in, status): per order
    the list of paths, the share of `amount_out[g]` bought through each and what it costs, then the total cost and the SPLIT_*
    status, as `split_paths_out` answers them.

    THE DEFAULT PROBE IS `amount_out / max_paths`, NOT THE AMOUNT.  The search finds only paths that can give the probe alone
    (a path that cannot answers +inf and is no path).  Probed with the whole amount, an order that is large against the pools
    -- one that no single path can fill, the very order that needs splitting -- would find nothing; probed with the size a
    share will have, it finds the paths that can each carry one.  Pass `probe=amount_out` for the paths that are best for the
    whole amount (`route_order`'s default), or any other size.

    An order for which nothing is found has empty lists, total +inf and SPLIT_UNOBTAINABLE (with `amount_out` 0: 0.0 and
    SPLIT_NONE), and is not sent to `split_paths_out`.  Nothing is executed:
    `swap_path_out_(r, pools[g], tokens[g], path_amount_out[g], max_in=path_amount_in[g])` executes order g.  Scalars broadcast."""
    try:
        tin, tout, amt = np.broadcast_arrays(np.asarray(token_in).reshape(-1), np.asarray(token_out).reshape(-1),
                                             np.asarray(amount_out, dtype=np.float64).reshape(-1))
        look = amt / float(max_paths) if probe is None else np.broadcast_to(np.asarray(probe, dtype=np.float64).reshape(-1), amt.shape)
    except ValueError:
        raise ArgumentError("token_in, token_out, amount_out and probe must be scalars or have one entry per order") from None
    _, pools, tokens, _ = find_disjoint_paths_out(r, tin, tout, look, max_paths, max_hops, usable_only=True)
    n = len(pools)
    have = [g for g in range(n) if pools[g]]
    x, y = [np.empty(0) for _ in range(n)], [np.empty(0) for _ in range(n)]
    total = np.where(amt == 0.0, 0.0, np.inf)
    status = np.where(amt == 0.0, SPLIT_NONE, SPLIT_UNOBTAINABLE).astype(np.int32)
    if have:
        xs, ys, total[have], status[have] = split_paths_out(r, [pools[g] for g in have], [tokens[g] for g in have], amt[have], rounds)
        for g, xg, yg in zip(have, xs, ys):
            x[g], y[g] = xg, yg
    return pools, tokens, x, y, total, status


def _swap_path(r: Router, verb, limit_name, pools, tokens, amount, limit, hops, sync_host):
    n_hops, seg, row, ci, co, amt, touched = _path_hops(r, verb, pools, tokens, amount)
    if limit is not None:
        try:
            limit = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, dtype=np.float64), amt.shape))
        except ValueError:
            raise ArgumentError(f"{limit_name} must be a scalar or have one entry per path") from None
    ctx = _path_context(r)
    L = r._layout
    try:
        res = getattr(ctx, verb)(n_hops, seg, row, ci, co, amt, limit, hops)
        if sync_host:
            for b in sorted(touched):
                _download_state(ctx, L.seg_of[b], L.batches[b])
                L.sync_pools(r.cfmms, b, sorted(touched[b]))
        return res
    finally:
        r._reset_trades()


def _quote_path(r: Router, verb, pools, tokens, amount, hops):
    n_hops, seg, row, ci, co, amt, _ = _path_hops(r, verb, pools, tokens, amount)
    return getattr(_path_context(r), verb)(n_hops, seg, row, ci, co, amt, hops)


def _path_context(r: Router):
    ctx = getattr(r._backend, "ctx", None)
    if ctx is None:
        raise NotImplementedError(f"{type(r._backend).__name__} has no device context to quote on")
    return ctx


def _path_hops(r: Router, verb, pools, tokens, amount, amount_name=None):
    """(pools, tokens) of the path calls as the context's hop arrays, with every refusal the router makes; also the rows the
    paths touch, per batch"""
    L = r._layout
    pools, tokens = list(pools), list(tokens)
    n = len(pools)
    if len(tokens) != n:
        raise ArgumentError("tokens must have one sequence per path")
    try:
        amt = np.ascontiguousarray(np.broadcast_to(np.asarray(amount, dtype=np.float64), (n,)))
    except ValueError:
        raise ArgumentError(f"{amount_name or ('amount_out' if verb.endswith('_out') else 'amount_in')} must be a scalar or have one entry per path") from None
    paths = [(np.asarray(pl, dtype=np.int64).reshape(-1), np.asarray(tk, dtype=np.int64).reshape(-1)) for pl, tk in zip(pools, tokens)]
    for p, (pl, tk) in enumerate(paths):
        if not 1 <= pl.size <= MAX_PATH_HOPS:
            raise ArgumentError(f"path {p}: {pl.size} pools (a path has 1 to {MAX_PATH_HOPS})")
        if tk.size != pl.size + 1:
            raise ArgumentError(f"path {p}: {tk.size} tokens for {pl.size} pools (one more than the pools)")
    H = max((pl.size for pl, _ in paths), default=1)
    n_hops = np.array([pl.size for pl, _ in paths], dtype=np.int32)
    seg, ci, co = (np.zeros((n, H), dtype=np.int32) for _ in range(3))
    row = np.zeros((n, H), dtype=np.int64)
    touched = {}
    for p, (pl, tk) in enumerate(paths):
        seen = set()
        for k, i in enumerate(pl.tolist()):
            where = L.locate(i)
            if where[0] == "host":
                raise ArgumentError(f"path {p}, hop {k}: pool {i}: {type(r._host.pools[where[1]]).__name__} is evaluated on the "
                                    f"host by its own find_arb_ and has no device state to quote")
            if i in seen:
                raise ArgumentError(f"path {p}, hop {k}: pool {i} appears twice (every hop is quoted against the pool as it "
                                    f"stands, so a second visit would ignore the first)")
            seen.add(i)
            Ai = L.batches[where[1]].Ai[where[2]]
            pos = []
            for t in (int(tk[k]), int(tk[k + 1])):
                at = np.flatnonzero(Ai == t)
                if at.size == 0:
                    raise ArgumentError(f"path {p}, hop {k}: token {t} is not a coin of pool {i} (its coins: {Ai.tolist()})")
                pos.append(int(at[0]))
            if pos[0] == pos[1]:
                raise ArgumentError(f"path {p}, hop {k}: token {int(tk[k])} on both sides of pool {i}")
            seg[p, k], row[p, k], ci[p, k], co[p, k] = L.seg_of[where[1]], where[2], pos[0], pos[1]
            touched.setdefault(where[1], set()).add(where[2])
    return n_hops, seg, row, ci, co, amt, touched


def _update_reserves_host(r: Router):
    if any(_has_ladder(b.kind) for b in r._batches):
        raise NotImplementedError("update_reserves! is not defined for UniV3 pools (nor in the reference)")
    if r._layout.ragged:
        raise NotImplementedError("this backend cannot update weighted or Curve pools (the device context does: "
                                  "cfmm_update_reserves)")
    if not hasattr(getattr(r._backend, "inner", r._backend), "reload"):    # (MixedBackend forwards to its inner backend)
        raise NotImplementedError("this backend cannot reload pools")
    D, Lm = r._backend.trades()                       # packed (segment) order
    for b, first in zip(r._batches, r._layout.offsets):
        b.R[:] = b.R + b.γ[:, None] * D[first:first + len(b)] - Lm[first:first + len(b)]
    r._backend.reload(r._batches)
    r._layout.sync_pools(r.cfmms)
