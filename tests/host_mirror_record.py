"""What the Python host mirror (router.py, cfmms.py) does, recorded without a device: the sequence of `Context` calls it
makes and the arrays it hands the caller, for a few small routers.  Shared by tests/golden/make_host_mirror_golden.py
(which writes the record of one commit to tests/golden/host_mirror_parent.json) and tests/test_host_mirror_cpu.py (which
records the current tree and compares).  Only the package's public API is used, plus one patch: the name `Context` that
`DeviceBackend` resolves is replaced by `RecordingContext`, so the shared library is never loaded."""
import contextlib
import hashlib
import json

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd import _lib, router

SEED = 20260301
N_TOKENS = 6


def digest(x):
    """A JSON value that pins x: arrays by dtype, shape and a hash of their bytes; containers element by element."""
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return f"{a.dtype.str}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()[:16]}"
    if isinstance(x, dict):
        return {str(k): digest(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        if len(x) > 3 and all(isinstance(a, np.ndarray) for a in x):       # per-pool vectors: one entry for all of them
            return {"sizes": [int(a.size) for a in x], "all": digest(np.concatenate([np.ravel(a) for a in x]))}
        return [digest(a) for a in x]
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return f"<{type(x).__name__}>"


class RecordingContext:
    """The methods of _lib.Context the host mirror calls.  Every call is appended to `RecordingContext.log` as
    [method, digest of each argument]; results are numbers drawn from (SEED, index of the call), except `eval`, a fixed
    smooth convex function of v so that a solver driven through it behaves like one."""

    log, calls = [], 0

    def __init__(self, n_tokens, device=0):
        self.n_tokens, self.device = int(n_tokens), device
        self.seg = []                                    # (pools, coins) per segment
        self.options = {}
        self._say("Context", n_tokens, device)

    def _say(self, name, *args):
        self.log.append([name] + [digest(a) for a in args])
        RecordingContext.calls += 1
        return np.random.default_rng([SEED, RecordingContext.calls])

    def _add(self, name, gamma, Ai0, *args):
        self._say(name, *args)
        m = int(np.size(gamma))
        self.seg.append((m, int(np.size(Ai0)) // m))

    def add_product(self, R, gamma, Ai0):
        self._add("add_product", gamma, Ai0, R, gamma, Ai0)

    def add_solidly(self, R, gamma, Ai0):
        self._add("add_solidly", gamma, Ai0, R, gamma, Ai0)

    def add_geomean(self, R, w, gamma, Ai0):
        self._add("add_geomean", gamma, Ai0, R, w, gamma, Ai0)

    def add_weighted(self, R, w, gamma, Ai0):
        self._add("add_weighted", gamma, Ai0, R, w, gamma, Ai0)

    def add_curve(self, R, gamma, Ai0, alpha, beta):
        self._add("add_curve", gamma, Ai0, R, gamma, Ai0, alpha, beta)

    def add_univ3(self, current_price, gamma, Ai0, tick_off, lower_ticks, liquidity):
        self._add("add_univ3", gamma, Ai0, current_price, gamma, Ai0, tick_off, lower_ticks, liquidity)

    def clear(self):
        self._say("clear")
        self.seg = []

    pool_count = property(lambda self: sum(m for m, _ in self.seg))
    trades_len = property(lambda self: sum(m * c for m, c in self.seg))

    def segments(self):
        self._say("segments")
        return [{"kind": -1, "m": m, "block": 0, "grid": 0} for m, _ in self.seg]

    def set_option(self, key, value):
        self._say("set_option", key, value)
        self.options[key] = int(value)

    def get_option(self, key):
        self._say("get_option", key)
        return self.options.get(key, 0)

    def find_arb(self, v):
        self._say("find_arb", np.asarray(v, dtype=np.float64))

    def eval(self, v):
        v = np.asarray(v, dtype=np.float64)
        self._say("eval", v)
        t = 1.0 + 0.25 * np.cos(np.arange(self.n_tokens))
        s = 1.0 + 0.5 * np.sin(np.arange(self.n_tokens)) ** 2
        return s * (v - t), float(0.5 * np.sum(s * (v - t) ** 2))

    def netflows(self):
        return self._say("netflows").standard_normal(self.n_tokens)

    def dual_value(self):
        return float(self._say("dual_value").standard_normal())

    def trades(self, out=None):
        rng = self._say("trades", "out" if out is not None else None)
        m, tl = self.pool_count, self.trades_len
        if tl != 2 * m:
            if out is not None:
                raise cr.ArgumentError("out arrays are not supported for ragged trades")
            return rng.standard_normal(tl), rng.standard_normal(tl)
        D, Lm = (np.empty((m, 2)), np.empty((m, 2))) if out is None else out
        D[:], Lm[:] = rng.standard_normal((m, 2)), rng.standard_normal((m, 2))
        return D, Lm

    def select_trades(self, seg, min_value=0.0, v=None, capacity=None, n_coins=2):
        rng = self._say("select_trades", seg, min_value, v, capacity, n_coins)
        m, coins = self.seg[int(seg)]
        assert coins == int(n_coins)
        idx = np.nonzero(rng.random(m) < 0.7)[0].astype(np.int64)
        return idx, rng.standard_normal((idx.size, coins)), rng.standard_normal((idx.size, coins)), rng.standard_normal(idx.size)

    def update_reserves(self):
        self._say("update_reserves")

    def reserves(self, seg, m, n_coins=2):
        rng = self._say("reserves", seg, m, n_coins)
        assert (int(m), int(n_coins)) == self.seg[int(seg)]
        return 100.0 + rng.random((int(m), int(n_coins)))

    def prices(self, seg, m):
        rng = self._say("prices", seg, m)
        assert int(m) == self.seg[int(seg)][0]
        return 0.5 + rng.random(int(m))

    def _refuse(self, *arrays):
        """as the device entries do: every row is checked before anything changes"""
        for a in arrays:
            if not np.all(np.isfinite(a)) or np.any(np.asarray(a) <= 0):
                raise cr.ArgumentError("recording context: new state must be finite and > 0")

    def set_reserves(self, seg, idx, R):
        self._say("set_reserves", seg, np.asarray(idx), np.asarray(R))
        self._refuse(R)

    def set_curve(self, seg, idx, R, alpha, beta):
        self._say("set_curve", seg, np.asarray(idx), np.asarray(R), np.asarray(alpha), np.asarray(beta))
        self._refuse(R, beta)

    def set_prices(self, seg, idx, current_price):
        self._say("set_prices", seg, np.asarray(idx), np.asarray(current_price))
        self._refuse(current_price)

    def set_ticks(self, seg, idx, current_price, tick_off, lower_ticks, liquidity):
        self._say("set_ticks", seg, np.asarray(idx), np.asarray(current_price), np.asarray(tick_off), np.asarray(lower_ticks),
                  np.asarray(liquidity))
        self._refuse(current_price)

    def route(self, objective_kind, objective_vec, objective_index=0, v0=None, m=5, factr=1e1, pgtol=1e-5, maxfun=15_000,
              maxiter=15_000):
        rng = self._say("route", objective_kind, np.asarray(objective_vec), objective_index, v0, m, factr, pgtol, maxfun, maxiter)
        info = {"f": float(rng.standard_normal()), "proj_grad": 1e-7, "iterations": 7, "evaluations": 9, "sweeps": 10,
                "status": int(rng.integers(0, 4)), "sweep_seconds": 0.25, "total_seconds": 0.5}
        return 1.0 + rng.random(self.n_tokens), rng.standard_normal(self.n_tokens), info

    def polish(self, objective_kind, objective_vec, objective_index, v, max_iters=8, rel_step=1e-7):
        rng = self._say("polish", objective_kind, np.asarray(objective_vec), objective_index, np.asarray(v), max_iters, rel_step)
        info = {"residual0": 1e-3, "residual": float(rng.random()) * 1e-9, "iterations": 3, "sweeps": 11, "total_seconds": 0.125}
        return 1.0 + rng.random(self.n_tokens), rng.standard_normal(self.n_tokens), info

    def close(self):
        self._say("close")


def recording_minimize(fun, x0, bounds, **kw):
    """Stands in for _lib.lbfgsb_minimize (the library's solver): evaluates `fun` at three fixed points, one of them
    twice in a row, and records what it was given and what came back."""
    log = RecordingContext.log
    log.append(["lbfgsb_minimize", digest(np.asarray(x0)), [list(map(digest, b)) for b in bounds], digest(kw)])
    x = np.array(x0, dtype=np.float64)
    for step in (0.0, 0.125, 0.125, -0.0625):
        f, g = fun(x * (1.0 + step))
        log.append(["fg", float(f), digest(np.asarray(g))])
    return x * 0.9375, {"f": float(f), "evaluations": 4, "iterations": 2, "status": 1, "sweeps": 0}


@contextlib.contextmanager
def recording():
    """Within the block every DeviceBackend talks to a RecordingContext; yields the log (emptied first)."""
    saved = router.Context, _lib.lbfgsb_minimize
    RecordingContext.log, RecordingContext.calls = [], 0
    router.Context, _lib.lbfgsb_minimize = RecordingContext, recording_minimize
    try:
        yield RecordingContext.log
    finally:
        router.Context, _lib.lbfgsb_minimize = saved


# ---- the pools ---------------------------------------------------------------------------------------------------------
class PluginPool(cr.CFMM):
    """A pool type without a device kernel: its own find_arb_ / update_reserves_ (deterministic, of no economic meaning)."""

    def __init__(self, R, Ai):
        self.R, self.Ai = np.array(R, dtype=np.float64), np.array(Ai, dtype=np.int64)
        self.gamma = 0.997           # a plugin type names its fields as it likes: CFMM itself defines none of them

    def find_arb_(self, Δ, Λ, v):
        Δ[:] = 0.01 * self.R                 # (constant trades: a linear term of the dual, its gradient constant)
        Λ[:] = 0.02 * self.R[::-1]

    def update_reserves_(self, Δ, Λ, v):
        self.R[:] = self.R + Δ - Λ


class PluginPoolWithState(PluginPool):
    def set_state_(self, state):
        self.R[:] = np.asarray(state, dtype=np.float64) * 2.0


def univ3(price, ticks, liq, Ai):
    return cr.UniV3(price, ticks, liq, 0.997, Ai)


def mixed_pools():
    """All six kinds interleaved (packing reorders them), weighted pools of 3 and 4 coins, Curve pools of 2 and 3, two
    plugin pools: at the start and in the middle."""
    return [
        PluginPool([5.0, 7.0, 9.0], [1, 3, 5]),                                               # 0  host
        cr.Curve([100.0, 101.0, 99.0], 0.9996, [1, 2, 3], 27.0 * 50, 100.0 ** 4 / 27.0),      # 1
        cr.ProductTwoCoin([100.0, 200.0], 0.997, [1, 2]),                                     # 2
        cr.GeometricMean([50.0, 60.0, 70.0, 80.0], [0.1, 0.2, 0.3, 0.4], 0.998, [2, 3, 4, 6]),  # 3
        univ3(1.05, [2.0, 1.5, 1.0, 0.5], [10.0, 20.0, 30.0, 0.0], [3, 4]),                   # 4
        cr.SolidlyStableTwoCoin([1000.0, 1001.0], 0.9995, [5, 6]),                            # 5
        cr.GeometricMeanTwoCoin([30.0, 40.0], [0.4, 0.6], 0.997, [2, 5]),                     # 6
        PluginPoolWithState([3.0, 4.0], [6, 2]),                                              # 7  host
        cr.Curve([500.0, 505.0], 0.9996, [4, 5], 4.0 * 100, 500.0 ** 3 / 4.0),                # 8
        cr.GeometricMean([10.0, 20.0, 30.0], [0.5, 0.25, 0.25], 0.997, [1, 4, 6]),            # 9
        cr.ProductTwoCoin([300.0, 150.0], 0.997, [3, 6]),                                     # 10
        univ3(0.8, [1.2, 0.9, 0.6], [5.0, 6.0, 0.0], [1, 6]),                                 # 11
        cr.Product([11.0, 12.0, 13.0], 0.997, [2, 4, 5]),                                     # 12
        cr.GeometricMeanTwoCoin([70.0, 20.0], [0.5, 0.5], 0.997, [1, 3]),                     # 13
        cr.SolidlyStableTwoCoin([2000.0, 1990.0], 0.9995, [1, 4]),                            # 14
    ]


def batch_list():
    """A list of PoolBatches with an EMPTY batch between two non-empty ones."""
    return [
        cr.ProductTwoCoin.batch([[100.0, 200.0], [300.0, 150.0], [10.0, 20.0]], [0.997] * 3, [[1, 2], [3, 6], [2, 5]]),
        cr.GeometricMeanTwoCoin.batch(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.zeros((0, 2), dtype=np.int64)),
        cr.UniV3.batch([1.05, 0.8], [0, 4, 7], [2.0, 1.5, 1.0, 0.5, 1.2, 0.9, 0.6], [10.0, 20.0, 30.0, 0.0, 5.0, 6.0, 0.0],
                       [0.997, 0.997], [[3, 4], [1, 6]]),
        cr.Curve.batch([[100.0, 101.0, 99.0], [50.0, 51.0, 52.0]], [0.9996] * 2, [[1, 2, 3], [4, 5, 6]], [1350.0, 1350.0],
                       [100.0 ** 4 / 27.0, 50.0 ** 4 / 27.0]),
    ]


def single_batch():
    return cr.SolidlyStableTwoCoin.batch([[1000.0, 1001.0], [2000.0, 1990.0]], [0.9995] * 2, [[5, 6], [1, 4]])


def two_coin_in_order():
    """Two-coin pools whose packing keeps the router order: trades are fetched into the router's own arrays."""
    return [cr.ProductTwoCoin([100.0, 200.0], 0.997, [1, 2]), cr.ProductTwoCoin([300.0, 150.0], 0.997, [3, 6]),
            cr.GeometricMeanTwoCoin([30.0, 40.0], [0.4, 0.6], 0.997, [2, 5]), univ3(1.05, [2.0, 1.5, 1.0, 0.5], [10.0, 20.0, 30.0, 0.0], [3, 4]),
            cr.SolidlyStableTwoCoin([1000.0, 1001.0], 0.9995, [5, 6])]


def all_host():
    return [PluginPool([5.0, 7.0, 9.0], [1, 3, 5]), PluginPoolWithState([3.0, 4.0], [6, 2]), PluginPool([1.0, 2.0], [4, 1])]


LADDER = (0.95, np.array([1.4, 1.1, 0.7, 0.3, 0.2]), np.array([1.0, 2.0, 3.0, 4.0, 0.0]))

# scenario -> (pools, a change per kind, a change the host refuses before any call, a change the context refuses)
SCENARIOS = {
    "mixed": (mixed_pools,
              {2: [101.0, 202.0], 6: [31.0, 41.0], 5: [1002.0, 1003.0], 3: [51.0, 61.0, 71.0, 81.0], 12: [11.5, 12.5, 13.5],
               1: ([102.0, 103.0, 98.0], 1400.0, 3.8e6), 8: ([510.0, 495.0], 410.0, 3.1e7), 11: 0.85, 4: LADDER, 0: [6.0, 8.0, 10.0],
               7: [1.5, 2.5]},
              {10: [1.0, 2.0, 3.0]},
              {2: [102.0, 203.0], 13: [-1.0, 21.0], 14: [2001.0, 1991.0]}),
    "batches": (batch_list, {0: [101.0, 202.0], 2: [11.0, 21.0], 3: 1.1, 4: LADDER, 6: ([51.0, 52.0, 53.0], 1300.0, 2.4e5)},
                {5: [1.0, 2.0]}, {1: [301.0, 151.0], 3: -1.0, 5: ([100.0, 100.0, 100.0], 1350.0, 3.7e6)}),
    "single_batch": (single_batch, {1: [2001.0, 1991.0]}, {0: [1.0, 2.0, 3.0]}, {0: [0.0, 1.0]}),
    "two_coin_in_order": (two_coin_in_order, {0: [101.0, 202.0], 2: [31.0, 41.0], 3: 1.1, 4: [1002.0, 1003.0]},
                          {3: "high"}, {1: [301.0, 151.0], 3: -2.0, 4: [1002.5, 1003.5]}),
    "all_host": (all_host, {0: [6.0, 8.0, 10.0], 1: [1.5, 2.5]}, None, None),
}


def pool_fields(p):
    return {f: (np.array(getattr(p, f)) if np.ndim(getattr(p, f)) else getattr(p, f))
            for f in ("R", "α", "β", "current_price", "current_tick", "lower_ticks", "liquidity") if hasattr(p, f)}


def state(r):
    """The host mirror's own state: batch arrays, per-pool objects, trades, Ψ and the dual value."""
    batches = [{f: np.array(getattr(b, f)) for f in ("R", "α", "β", "current_price", "tick_off", "lower_ticks", "liquidity")
                if hasattr(b, f)} for b in r._batches]
    short = lambda fields: hashlib.sha256(json.dumps(digest(fields), sort_keys=True).encode()).hexdigest()[:12]     # one per batch / pool
    return digest({"batches": [short(b) for b in batches], "pools": [short(pool_fields(p)) for p in r.cfmms], "Δs": trades(r.Δs),
                   "Λs": trades(r.Λs), "psi": np.array(r._psi), "acc": float(r._acc), "n_sweeps": r.n_sweeps})


def trades(x):
    return np.array(x) if isinstance(x, np.ndarray) else [np.array(a) for a in x]


def attempt(fn):
    try:
        fn()
        return None
    except Exception as e:       # the text is part of the record
        return f"{type(e).__name__}: {e}"


def record_scenario(name):
    """Every step of one scenario -> a list of {"step", "calls" (what reached the context during it), results}."""
    make, changes, host_refused, ctx_refused = SCENARIOS[name]
    steps = []
    with recording() as log:
        last = [None]

        def step(label, **results):
            results = {k: digest(v) for k, v in results.items()}
            if "state" in results:                   # the whole state once; "unchanged" where a step left all of it as it was
                results["state"], last[0] = ("unchanged" if results["state"] == last[0] else results["state"]), results["state"]
            steps.append({"step": label, "calls": list(log), **results})
            del log[:]

        v = 1.0 + 0.1 * np.arange(N_TOKENS)
        r = cr.Router(cr.LinearNonnegative(np.ones(N_TOKENS)), make(), N_TOKENS)
        step("upload", state=state(r))
        cr.find_arb_(r, v)
        step("find_arb", psi=np.array(r._psi), acc=r._acc)
        step("trades", Δs=trades(r.Δs), Λs=trades(r.Λs), again=trades(r.Δs))
        for min_value in (-np.inf, 0.25):
            idx, Ds, Ls, val = cr.active_trades(r, min_value)
            step(f"active_trades {min_value}", idx=idx, Δ=trades(Ds), Λ=trades(Ls), value=val)
        step("netflows", device=cr.netflows(r), exact=cr.netflows(r, exact=True))
        step("update_pools", error=attempt(lambda: cr.update_pools_(r, changes)), state=state(r))
        cr.find_arb_(r, v * 1.01)
        step("find_arb again")
        step("update_pools out of range", error=attempt(lambda: cr.update_pools_(r, {len(r.cfmms): [1.0, 1.0]})),
             negative=attempt(lambda: cr.update_pools_(r, {-1: [1.0, 1.0]})), state=state(r))
        if host_refused is not None:
            step("update_pools refused on the host", error=attempt(lambda: cr.update_pools_(r, host_refused)), state=state(r))
            step("update_pools refused by the context", error=attempt(lambda: cr.update_pools_(r, ctx_refused)), state=state(r))
        for sync_host in (True, False):
            cr.find_arb_(r, v * 1.02)
            step(f"update_reserves sync_host={sync_host}", error=attempt(lambda: cr.update_reserves_(r, sync_host=sync_host)), state=state(r))
        r.objective = cr.BasketLiquidation(2, np.array([0.0, 0.0, 3.0, 1.0, 0.0, 2.0]))
        for solver in ("scipy", "native"):
            for obj in (cr.LinearNonnegative(1.0 + 0.5 * np.arange(N_TOKENS)), r.objective):
                r.objective, r.info = obj, None
                step(f"route {solver} {type(obj).__name__}",
                     error=attempt(lambda: cr.route_(r, v=None if solver == "scipy" else v + 3.0, solver=solver, maxiter=6)),
                     info=r.info, v=np.array(r.v), psi=np.array(r._psi), acc=r._acc, n_sweeps=r.n_sweeps)
        step("polish native", error=attempt(lambda: cr.polish_(r, iters=5, native=True)), info=r.info, v=np.array(r.v),
             psi=np.array(r._psi), acc=r._acc, n_sweeps=r.n_sweeps)
        step("trades after route", Δs=trades(r.Δs), Λs=trades(r.Λs))
        r.close()
        step("close")
    return steps


def record_all():
    return {name: record_scenario(name) for name in SCENARIOS}
