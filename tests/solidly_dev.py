"""Device-pointer plumbing shared by the Solidly GPU tests: hipMalloc / hipMemcpy through the HIP runtime the library has
loaded, a cfmm_sweep_dev call, and a read of the cfmm_trades_dev views."""
import ctypes

import numpy as np


def hip():
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
    """cfmm_sweep_dev at prices v (uploaded here) -> (Ψ, acc)."""
    h = hip()
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


def read_trades_dev(be, m):
    """The [m][2] device views of cfmm_trades_dev, copied to the host -> (Δ, Λ)."""
    h = hip()
    pd, pl = be.ctx.trades_dev()
    D, L = np.empty((m, 2)), np.empty((m, 2))
    assert h.hipDeviceSynchronize() == 0
    assert h.hipMemcpy(D.ctypes.data, ctypes.c_void_p(pd), 16 * m, 2) == 0
    assert h.hipMemcpy(L.ctypes.data, ctypes.c_void_p(pl), 16 * m, 2) == 0
    return D, L
