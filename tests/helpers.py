"""Shared test helpers: bridge between the host mirror's PoolBatch containers and the CPU oracle."""
import ctypes
import math

import numpy as np

import cfmmrouter_amd as cr
from cfmmrouter_amd._lib import KIND_GEOMEAN, KIND_PRODUCT, KIND_UNIV3
from oracle import cfmm_oracle as orc
from reduction_ref import assert_reduction_exact


def oracle_poolset(batches, n_tokens):
    segs = []
    for b in batches:
        Ai0 = (b.Ai - 1).astype(np.int32)
        if b.kind == KIND_PRODUCT:
            segs.append(("product", dict(R=b.R, gamma=b.γ, Ai=Ai0)))
        elif b.kind == KIND_GEOMEAN:
            segs.append(("geomean", dict(R=b.R, w=b.w, gamma=b.γ, Ai=Ai0)))
        else:
            segs.append(("univ3", dict(current_price=b.current_price, gamma=b.γ, Ai=Ai0, tick_off=b.tick_off,
                                       lower_ticks=b.lower_ticks, liquidity=b.liquidity)))
    return orc.PoolSet(segs, n_tokens)


def oracle_objective(obj):
    if isinstance(obj, cr.LinearNonnegative):
        return orc.LinearNonnegative(obj.c)
    return orc.BasketLiquidation(obj.i - 1, obj.Δin)


def oracle_sweep(batches, n_tokens, v, nthreads=1):
    ps = oracle_poolset(batches, n_tokens)
    D, L = ps.sweep(np.asarray(v, dtype=np.float64), nthreads)
    psi = orc.netflows(D, L, ps.Ai, n_tokens)
    acc = orc.dual_acc(D, L, ps.Ai, v)
    return D, L, psi, acc


def rel_to_max(a, b):
    """max|a-b| / max|b| : the netflow parity measure (component-wise relative error is
    unattainable on constraint-active ~0 components)."""
    scale = max(np.max(np.abs(b)), np.finfo(float).tiny)
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / scale)


def device_sweep(n, batches, v, device=0):
    """One materialising sweep of `batches` on the device: flat Δ, flat Λ, Ψ, acc."""
    be = cr.DeviceBackend(n, batches, device=device)
    try:
        psi, acc = be.find_arb(v)
        D, L = be.trades()
    finally:
        be.close()
    return np.ravel(D), np.ravel(L), psi, acc


def coin_scale(b):
    """Per-pool trade scale of an N-coin batch: its largest reserve, [m, 1]."""
    return b.R.max(axis=1, keepdims=True)


class OracleBackend:
    """TEST-ONLY stand-in for DeviceBackend so the host logic (route loop, packing order, sharded
    reduction) can be exercised on a box with no GPU.  Lives in tests/, never in the package."""

    def __init__(self, n_tokens, batches, nthreads=1):
        self.ps = oracle_poolset(batches, n_tokens)
        self.n_tokens = n_tokens
        self.nthreads = nthreads

    def eval(self, v):
        self.D, self.L = self.ps.sweep(np.asarray(v, dtype=np.float64), self.nthreads)
        return orc.netflows(self.D, self.L, self.ps.Ai, self.n_tokens), orc.dual_acc(self.D, self.L, self.ps.Ai, v)

    find_arb = eval

    def trades(self):
        return self.D, self.L

    def reload(self, batches):
        self.ps = oracle_poolset(batches, self.n_tokens)


def route_converged(obj, market, n, v0=None, nthreads=1, solver="native", router=None):
    """Route-level parity BY CONVERGENCE.  Device side: route! (`solver`) on the HIP path, then
    polish_ with the device's own finite-difference Jacobian.  CPU side: route_oracle (SciPy L-BFGS-B on the CPU
    restatement), then the SAME polish_ code driven through the OracleBackend -- with the device's Jacobian as the chord
    matrix, which only sets the rate: the point it converges to is where the RESTATEMENT's gradient satisfies the
    optimality conditions (tests/test_polish_cpu.py::test_polish_with_a_foreign_chord_matrix...).  Returns the default-
    tolerance distance, the converged distance (both max|ΔΨ| / max|Ψ|) and the polish records."""
    r = router if router is not None else cr.Router(obj, market, n)
    try:
        cr.route_(r, v=v0, solver=solver)
        psi_default, v_default, evals = cr.netflows(r).copy(), r.v.copy(), r.info["funcalls"]
        J = cr.dual_jacobian(r)
        cr.polish_(r, jacobian=J)
        psi_dev, v_dev, pol_dev = cr.netflows(r).copy(), r.v.copy(), dict(r.info["polish"])
    finally:
        if router is None:
            r.close()
    ref = orc.route_oracle(oracle_objective(obj), oracle_poolset(market, n), v0=v0, nthreads=nthreads)
    ro = cr.Router(obj, market, n, _backend=OracleBackend(n, market, nthreads))
    ro.v[:] = ref["v"]
    cr.polish_(ro, jacobian=J)
    psi_ref = cr.netflows(ro)
    return {"default": rel_to_max(psi_default, ref["psi"]), "converged": rel_to_max(psi_dev, psi_ref),
            "v_converged": float(np.max(np.abs(v_dev - ro.v) / ro.v)),
            "device_moved": rel_to_max(psi_default, psi_dev), "oracle_moved": rel_to_max(ref["psi"], psi_ref),
            "evaluations_device": int(evals), "evaluations_oracle": int(ref["info"]["funcalls"]),
            "polish_device": pol_dev, "polish_oracle": dict(ro.info["polish"]), "psi_scale": float(np.max(np.abs(psi_ref)))}


def reduction_checks(c, rows, D, L, psi, acc, kk, bD, bL, check_self=True):
    """Ψ / acc of a 60-digit fixture case (dict: v, Ai, truth D / L) against the device's own trades (reduction_ref.
    assert_reduction_exact: the LDS scatter and the folds, (c + 2)·u·Σ|terms| for c nonzero terms, exact for c <= 1) and
    against the truth (the per-pool bounds K·(bD + bL) summed, plus that reduction bound).  rows: the case's rows that were
    swept; D, L: the device's trades, or None."""
    U = 2.0 ** -53
    Ai0 = (c["Ai"][rows] - 1).ravel()
    n = len(c["v"])
    vl = c["v"][Ai0]
    Dt, Lt = c["D"][rows].ravel(), c["L"][rows].ravel()
    if check_self:
        assert_reduction_exact(D, L, Ai0, c["v"], n, psi, acc)
    ft = Lt - Dt
    per = (kk[:, None] * (bD + bL)).ravel()
    for j in range(n):
        sel = Ai0 == j
        t = ft[sel]
        red = (np.count_nonzero(t) + 2) * U * np.sum(np.abs(t))
        assert abs(psi[j] - math.fsum(t)) <= np.sum(per[sel]) + red, j
    terms = np.concatenate([Lt * vl, -(Dt * vl)])
    red = (np.count_nonzero(terms) + 2) * U * np.sum(np.abs(terms))
    assert abs(acc - math.fsum(terms)) <= np.sum(per * vl) + red


def hip_runtime():
    """The HIP runtime the library already loaded, for tests that hand the library device pointers."""
    import cfmmrouter_amd._lib as lib
    lib.lib()
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                path = line.split()[-1]
                break
    assert path, "libamdhip64 is not loaded"
    h = ctypes.CDLL(path)
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


def dev_sweep(be, v, materialize=True):
    """One device-pointer sweep (cfmm_sweep_dev) of the backend's pools at prices v -> (Ψ, acc)."""
    h = hip_runtime()
    n = len(v)
    dv, dout = ctypes.c_void_p(), ctypes.c_void_p()
    assert h.hipMalloc(ctypes.byref(dv), 8 * n) == 0 and h.hipMalloc(ctypes.byref(dout), 8 * (n + 1)) == 0
    try:
        vh = np.ascontiguousarray(v, dtype=np.float64)
        out = np.empty(n + 1)
        assert h.hipMemcpy(dv, vh.ctypes.data, 8 * n, 1) == 0
        be.ctx.sweep_dev(dv.value, dout.value, materialize)
        assert h.hipDeviceSynchronize() == 0
        assert h.hipMemcpy(out.ctypes.data, dout, 8 * (n + 1), 2) == 0
        return out[:n], float(out[n])
    finally:
        h.hipFree(dv)
        h.hipFree(dout)
