"""ctypes binding of libcfmm_amd.so (include/cfmm_amd.h).

This is the only door from the Python host mirror into the device code.  There is NO fallback:
if the shared library is missing or no gfx950 device is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFMM_AMD_LIB") or os.path.join(_HERE, "libcfmm_amd.so")   # override: A/B builds in scripts/
CSRC = os.path.join(_HERE, "csrc")

OK = 0
ERR_INVALID_ARG = -1
ERR_HIP = -2
ERR_STATE = -3
ERR_UNSUPPORTED = -4
MAX_PATH_HOPS = 8          # CFMM_MAX_PATH_HOPS
PATH_APPLIED, PATH_BELOW_LIMIT, PATH_REFUSED = 0, 1, 2   # CFMM_PATH_*: Context.swap_path's status
LIMIT_FILLED, LIMIT_PARTIAL, LIMIT_NONE, LIMIT_REFUSED = 0, 1, 2, 3   # CFMM_LIMIT_*: Context.swap_limit's status
SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE = 0, 1, 2, 3   # CFMM_SWAP_*: Context.swap_out's / swap_path_out's status
FOUND, FOUND_NONE, FOUND_REPEATS = 0, 1, 2   # CFMM_FOUND*: Context.find_path's status
SIZED, SIZED_NONE, SIZED_AT_LIMIT, SIZED_NAN = 0, 1, 2, 3   # CFMM_SIZED*: Context.size_path's status
MAX_SIZE_ROUNDS = 16       # CFMM_MAX_SIZE_ROUNDS
SPLIT_OK, SPLIT_NONE, SPLIT_NAN, SPLIT_SATURATED = 0, 1, 2, 3   # CFMM_SPLIT_*: Context.split_paths' status
SPLIT_UNOBTAINABLE = 4     # CFMM_SPLIT_UNOBTAINABLE: Context.split_paths_out's "no path can give another slice"
ORDER_APPLIED, ORDER_LIMIT, ORDER_REFUSED, ORDER_UNOBTAINABLE = 0, 1, 2, 3   # CFMM_ORDER_*: Context.swap_order's / swap_order_out's status
ORDER_PATH_HELD = 4        # CFMM_ORDER_PATH_HELD: their path_status of a path that passes in an order that was not applied
MAX_SPLIT_PATHS = 8        # CFMM_MAX_SPLIT_PATHS
MAX_SPLIT_ROUNDS = 16      # CFMM_MAX_SPLIT_ROUNDS

KIND_PRODUCT, KIND_GEOMEAN, KIND_UNIV3, KIND_WEIGHTED, KIND_CURVE, KIND_SOLIDLY = 0, 1, 2, 3, 4, 5

_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_ctx = C.c_void_p

OBJ_LINEAR_NONNEGATIVE, OBJ_BASKET_LIQUIDATION = 0, 1


class RouteInfo(C.Structure):
    _fields_ = [("f", C.c_double), ("proj_grad", C.c_double), ("iterations", C.c_int32),
                ("evaluations", C.c_int32), ("sweeps", C.c_int32), ("status", C.c_int32),
                ("sweep_seconds", C.c_double), ("total_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PolishInfo(C.Structure):
    _fields_ = [("residual0", C.c_double), ("residual", C.c_double), ("iterations", C.c_int32), ("sweeps", C.c_int32),
                ("total_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


FG_CALLBACK = C.CFUNCTYPE(C.c_double, C.c_void_p, _f64p, _f64p)


class ArgumentError(ValueError):
    """The reference's ArgumentError (src/cfmms.jl:77-78, src/objectives.jl:54,97)."""


class CFMMDeviceError(RuntimeError):
    """A HIP runtime failure or a missing device/extension."""


def build(force: bool = False) -> str:
    """Compile libcfmm_amd.so for gfx950 with hipcc (csrc/Makefile)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs += [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("cfmm_amd.h", "cfmm_amd_path_out.h", "cfmm_amd_find_out.h", "cfmm_amd_size_path.h", "cfmm_amd_split.h", "cfmm_amd_split_out.h", "cfmm_amd_find_disjoint.h", "cfmm_amd_find_disjoint_out.h")]
    stale = not os.path.exists(LIB_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.run(["make", "-C", CSRC] + (["-B"] if force else []), check=True)
    return LIB_PATH


_lib = None


def lib():
    """Load the extension (once).  Raises CFMMDeviceError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CFMMDeviceError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C cfmmrouter.jl_amd/csrc`).  There is no CPU fallback.")
    # One HIP runtime per process: if torch is going to be used (streams, torch.distributed), its
    # bundled libamdhip64 must be the one that is loaded, so import it before our library.
    if "torch" not in sys.modules and os.environ.get("CFMM_AMD_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    L.cfmm_ctx_create.argtypes = [C.c_int, C.c_int32, C.POINTER(_ctx)]
    L.cfmm_ctx_create_multi.argtypes = [C.c_int32, _i32p, C.c_int32, C.POINTER(_ctx)]
    L.cfmm_device_count.argtypes = [_ctx]
    L.cfmm_device_count.restype = C.c_int32
    L.cfmm_ctx_destroy.argtypes = [_ctx]
    L.cfmm_ctx_destroy.restype = None
    L.cfmm_last_error.argtypes = [_ctx]
    L.cfmm_last_error.restype = C.c_char_p
    L.cfmm_version.restype = C.c_char_p
    L.cfmm_set_stream.argtypes = [_ctx, C.c_void_p]
    L.cfmm_reset_stream.argtypes = [_ctx]
    L.cfmm_set_option.argtypes = [_ctx, C.c_char_p, C.c_int64]
    L.cfmm_get_option.argtypes = [_ctx, C.c_char_p, _i64p]
    L.cfmm_pools_add_product.argtypes = [_ctx, C.c_int64, _f64p, _f64p, _i32p]
    L.cfmm_pools_add_solidly.argtypes = [_ctx, C.c_int64, _f64p, _f64p, _i32p]
    L.cfmm_pools_add_geomean.argtypes = [_ctx, C.c_int64, _f64p, _f64p, _f64p, _i32p]
    L.cfmm_pools_add_univ3.argtypes = [_ctx, C.c_int64, _f64p, _f64p, _i32p, _i64p, _f64p, _f64p]
    L.cfmm_pools_add_weighted.argtypes = [_ctx, C.c_int64, C.c_int32, _f64p, _f64p, _f64p, _i32p]
    L.cfmm_pools_add_curve.argtypes = [_ctx, C.c_int64, C.c_int32, _f64p, _f64p, _i32p, _f64p, _f64p]
    L.cfmm_trades_len.argtypes = [_ctx]
    L.cfmm_trades_len.restype = C.c_int64
    L.cfmm_pools_clear.argtypes = [_ctx]
    L.cfmm_pools_count.argtypes = [_ctx]
    L.cfmm_pools_count.restype = C.c_int64
    L.cfmm_n_tokens.argtypes = [_ctx]
    L.cfmm_n_tokens.restype = C.c_int32
    L.cfmm_find_arb.argtypes = [_ctx, _f64p]
    L.cfmm_eval.argtypes = [_ctx, _f64p, _f64p, _f64p]
    L.cfmm_get_trades.argtypes = [_ctx, _f64p, _f64p]
    L.cfmm_get_trades_range.argtypes = [_ctx, C.c_int32, C.c_int64, C.c_int64, _f64p, _f64p]
    L.cfmm_select_trades.argtypes = [_ctx, C.c_int32, _f64p, C.c_double, C.c_int64, _i64p, _i64p, _f64p, _f64p, _f64p]
    L.cfmm_netflows.argtypes = [_ctx, _f64p]
    L.cfmm_dual_value.argtypes = [_ctx, _f64p]
    L.cfmm_update_reserves.argtypes = [_ctx]
    L.cfmm_get_reserves.argtypes = [_ctx, C.c_int32, _f64p]
    L.cfmm_get_prices.argtypes = [_ctx, C.c_int32, _f64p]
    L.cfmm_pools_set_reserves.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _f64p]
    L.cfmm_pools_set_curve.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _f64p, _f64p, _f64p]
    L.cfmm_pools_set_prices.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _f64p]
    L.cfmm_pools_set_ticks.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _f64p, _i64p, _f64p, _f64p]
    L.cfmm_quote.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p]
    L.cfmm_quote_dev.argtypes = [_ctx, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cfmm_quote_out.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p]
    L.cfmm_quote_out_dev.argtypes = [_ctx, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cfmm_swap.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p]
    L.cfmm_swap_path.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _i32p]
    L.cfmm_swap_out.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, _i32p]
    L.cfmm_swap_path_out.argtypes = L.cfmm_swap_path.argtypes
    L.cfmm_quote_path.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p]
    L.cfmm_quote_path_out.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p]
    L.cfmm_quote_path_dev.argtypes = [_ctx, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cfmm_quote_path_out_dev.argtypes = [_ctx, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.cfmm_quote_rate.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p]
    L.cfmm_quote_rate_dev.argtypes = [_ctx, C.c_int32, C.c_int64] + [C.c_void_p] * 6
    L.cfmm_quote_to_rate.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p]
    L.cfmm_quote_to_rate_dev.argtypes = [_ctx, C.c_int32, C.c_int64] + [C.c_void_p] * 6
    L.cfmm_swap_limit.argtypes = [_ctx, C.c_int32, C.c_int64, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _i32p]
    L.cfmm_quote_path_rate.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p]
    L.cfmm_quote_path_rate_dev.argtypes = [_ctx, C.c_int64, C.c_int32] + [C.c_void_p] * 10
    L.cfmm_find_path.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _f64p, _f64p, _i32p, _i32p, _i64p, _i32p, _i32p, _i32p]
    L.cfmm_find_path_out.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _f64p, _f64p, _i32p, _i32p, _i64p, _i32p, _i32p, _i32p]
    L.cfmm_find_disjoint_paths.argtypes = [_ctx, C.c_int64, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _i32p, _f64p, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p]
    L.cfmm_find_disjoint_paths_out.argtypes = L.cfmm_find_disjoint_paths.argtypes
    L.cfmm_size_path.argtypes = [_ctx, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, C.c_int32,
                                 _f64p, _f64p, _f64p, _i32p]
    L.cfmm_size_path_dev.argtypes = [_ctx, C.c_int64, C.c_int32] + [C.c_void_p] * 8 + [C.c_int32] + [C.c_void_p] * 4
    L.cfmm_split_paths.argtypes = [_ctx, C.c_int64, _i64p, _f64p, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, C.c_int32,
                                   _f64p, _f64p, _f64p, _i32p]
    L.cfmm_split_paths_dev.argtypes = [_ctx, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 4
    L.cfmm_split_paths_out.argtypes = L.cfmm_split_paths.argtypes
    L.cfmm_swap_order.argtypes = [_ctx, C.c_int64, _i64p, C.c_int64, C.c_int32, _i32p, _i32p, _i64p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p]
    L.cfmm_swap_order_out.argtypes = L.cfmm_swap_order.argtypes
    L.cfmm_split_paths_out_dev.argtypes = L.cfmm_split_paths_dev.argtypes
    L.cfmm_sweep_dev.argtypes = [_ctx, C.c_void_p, C.c_void_p, C.c_int]
    L.cfmm_trades_dev.argtypes = [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.cfmm_kernel_times.argtypes = [_ctx, _i64p, _f64p, _i64p, _f64p]
    L.cfmm_route.argtypes = [_ctx, C.c_int32, _f64p, C.c_int32, _f64p, C.c_int32, C.c_double, C.c_double,
                             C.c_int32, C.c_int32, _f64p, _f64p, C.POINTER(RouteInfo)]
    L.cfmm_polish.argtypes = [_ctx, C.c_int32, _f64p, C.c_int32, _f64p, C.c_int32, C.c_double, _f64p, C.POINTER(PolishInfo)]
    L.cfmm_lbfgsb_minimize.argtypes = [C.c_int32, _f64p, _f64p, _f64p, _i32p, FG_CALLBACK, C.c_void_p, C.c_int32,
                                       C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RouteInfo)]
    L.cfmm_set_peers.argtypes = [_ctx, C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.c_uint64]
    L.cfmm_peer_buffer_bytes.argtypes = [C.c_int32]
    L.cfmm_peer_buffer_bytes.restype = C.c_int64
    L.cfmm_peer_buffer_alloc.argtypes = [_ctx, C.POINTER(C.c_uint64), C.c_char_p]
    L.cfmm_peer_buffer_open.argtypes = [_ctx, C.c_char_p, C.POINTER(C.c_uint64)]
    L.cfmm_peer_buffer_close.argtypes = [_ctx, C.c_uint64]
    L.cfmm_peer_buffer_free.argtypes = [_ctx, C.c_uint64]
    L.cfmm_rccl_unique_id.argtypes = [C.c_char_p]
    L.cfmm_rccl_init_rank.argtypes = [_ctx, C.c_char_p, C.c_int32, C.c_int32]
    L.cfmm_set_rccl_comm.argtypes = [_ctx, C.c_void_p]
    L.cfmm_segment_count.argtypes = [_ctx]
    L.cfmm_segment_count.restype = C.c_int32
    L.cfmm_segment_info.argtypes = [_ctx, C.c_int32, _i32p, _i64p, _i32p, _i32p]
    _lib = L
    return L


def f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def _ncoin_arrays(R, gamma, Ai0, coins, pools, shape_error):
    """The arrays of m N-coin pools (Context.add_weighted, add_curve): R, Ai0 and `coins` [m, n]; gamma and `pools` [m].
    Returns m, n, R, gamma, Ai0 (int32), coins, pools, all contiguous."""
    gamma = f64(gamma)
    m = gamma.size
    R = f64(R)
    n = R.shape[1] if R.ndim == 2 else (R.size // m if m else 0)
    Ai0 = np.ascontiguousarray(Ai0, dtype=np.int32)
    coins, pools = [f64(a) for a in coins], [f64(a) for a in pools]
    if any(a.size != n * m for a in (R, Ai0, *coins)) or any(a.size != m for a in pools):
        raise ArgumentError(shape_error)
    return m, int(n), R, gamma, Ai0, coins, pools


def ptr(a):
    if a is None:
        return None
    if a.dtype == np.float64:
        return a.ctypes.data_as(_f64p)
    if a.dtype == np.int32:
        return a.ctypes.data_as(_i32p)
    if a.dtype == np.int64:
        return a.ctypes.data_as(_i64p)
    raise TypeError(a.dtype)


class Context:
    """RAII wrapper of a cfmm_ctx: one device and its pool store, or -- `device` a list of HIP
    ordinals -- the single-process multi-device context of cfmm_ctx_create_multi (pools split in
    contiguous blocks over the devices, {Ψ, acc} summed on the host)."""

    def __init__(self, n_tokens: int, device=0):
        self._L = lib()
        h = _ctx()
        if isinstance(device, (list, tuple, np.ndarray)):
            ids = np.ascontiguousarray(device, dtype=np.int32)
            rc = self._L.cfmm_ctx_create_multi(int(ids.size), ptr(ids), int(n_tokens), C.byref(h))
            self.device = [int(d) for d in ids]
        else:
            rc = self._L.cfmm_ctx_create(int(device), int(n_tokens), C.byref(h))
            self.device = int(device)
        if rc != OK:
            self._h = None
            self._raise(rc, None)
        self._h = h
        self.n_tokens = int(n_tokens)

    @property
    def device_count(self) -> int:
        return int(self._L.cfmm_device_count(self._h))

    # -- errors --------------------------------------------------------------------------------
    def _raise(self, rc, h):
        msg = self._L.cfmm_last_error(h).decode()
        if rc == ERR_INVALID_ARG:
            raise ArgumentError(msg)
        if rc == ERR_STATE:
            raise RuntimeError(msg)
        if rc == ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise CFMMDeviceError(msg)

    def _check(self, rc):
        if rc != OK:
            self._raise(rc, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.cfmm_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        """Launch on exactly this hipStream_t handle (0 / None = HIP's default stream)."""
        self._check(self._L.cfmm_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def reset_stream(self):
        self._check(self._L.cfmm_reset_stream(self._h))

    def set_option(self, key: str, value: int):
        self._check(self._L.cfmm_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_int64()
        self._check(self._L.cfmm_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    # -- pools ---------------------------------------------------------------------------------
    def _add_pairs(self, entry, R, gamma, Ai0):
        R, gamma = f64(R), f64(gamma)
        Ai0 = np.ascontiguousarray(Ai0, dtype=np.int32)
        m = gamma.size
        if R.size != 2 * m or Ai0.size != 2 * m:
            raise ArgumentError("R and Ai must have shape [m, 2]")
        self._check(entry(self._h, m, ptr(R), ptr(gamma), ptr(Ai0)))

    def add_product(self, R, gamma, Ai0):
        self._add_pairs(self._L.cfmm_pools_add_product, R, gamma, Ai0)

    def add_solidly(self, R, gamma, Ai0):
        """m Solidly-style stable pairs (φ = x³y + xy³): the arrays of add_product (cfmm_pools_add_solidly)."""
        self._add_pairs(self._L.cfmm_pools_add_solidly, R, gamma, Ai0)

    def add_geomean(self, R, w, gamma, Ai0):
        R, w, gamma = f64(R), f64(w), f64(gamma)
        Ai0 = np.ascontiguousarray(Ai0, dtype=np.int32)
        m = gamma.size
        if R.size != 2 * m or w.size != 2 * m or Ai0.size != 2 * m:
            raise ArgumentError("R, w and Ai must have shape [m, 2]")
        self._check(self._L.cfmm_pools_add_geomean(self._h, m, ptr(R), ptr(w), ptr(gamma), ptr(Ai0)))

    def add_univ3(self, current_price, gamma, Ai0, tick_off, lower_ticks, liquidity):
        current_price, gamma = f64(current_price), f64(gamma)
        lower_ticks, liquidity = f64(lower_ticks), f64(liquidity)
        Ai0 = np.ascontiguousarray(Ai0, dtype=np.int32)
        tick_off = np.ascontiguousarray(tick_off, dtype=np.int64)
        m = gamma.size
        if current_price.size != m or Ai0.size != 2 * m or tick_off.size != m + 1:
            raise ArgumentError("inconsistent UniV3 array sizes")
        if m and (lower_ticks.size != tick_off[-1] or liquidity.size != tick_off[-1]):
            raise ArgumentError("tick arrays must have tick_off[-1] entries")
        self._check(self._L.cfmm_pools_add_univ3(self._h, m, ptr(current_price), ptr(gamma), ptr(Ai0),
                                                 ptr(tick_off), ptr(lower_ticks), ptr(liquidity)))

    def add_weighted(self, R, w, gamma, Ai0):
        """m weighted pools of n coins each: R, w, Ai0 [m, n] (cfmm_pools_add_weighted)."""
        m, n, R, gamma, Ai0, (w,), _ = _ncoin_arrays(R, gamma, Ai0, [w], [], "R, w and Ai must have shape [m, n_coins]")
        self._check(self._L.cfmm_pools_add_weighted(self._h, m, n, ptr(R), ptr(w), ptr(gamma), ptr(Ai0)))

    def add_curve(self, R, gamma, Ai0, alpha, beta):
        """m Curve pools of n coins each: R, Ai0 [m, n]; gamma, alpha, beta [m] (cfmm_pools_add_curve)."""
        m, n, R, gamma, Ai0, _, (alpha, beta) = _ncoin_arrays(
            R, gamma, Ai0, [], [alpha, beta], "R and Ai must have shape [m, n_coins], gamma, alpha and beta shape [m]")
        self._check(self._L.cfmm_pools_add_curve(self._h, m, n, ptr(R), ptr(gamma), ptr(Ai0), ptr(alpha), ptr(beta)))

    def clear(self):
        self._check(self._L.cfmm_pools_clear(self._h))

    @property
    def pool_count(self) -> int:
        return int(self._L.cfmm_pools_count(self._h))

    # -- hot path ------------------------------------------------------------------------------
    def _check_v(self, v):
        """A price vector as the contiguous float64 array the entries take; it must have n_tokens entries."""
        v = f64(v)
        if v.size != self.n_tokens:
            raise ArgumentError("v must have n_tokens entries")
        return v

    def find_arb(self, v):
        v = self._check_v(v)
        self._check(self._L.cfmm_find_arb(self._h, ptr(v)))

    def eval(self, v):
        v = self._check_v(v)
        psi = np.empty(self.n_tokens)
        acc = C.c_double()
        self._check(self._L.cfmm_eval(self._h, ptr(v), ptr(psi), C.byref(acc)))
        return psi, acc.value

    @property
    def trades_len(self) -> int:
        """Doubles per trade array: Σ over pools of their coin counts (cfmm_trades_len)."""
        return int(self._L.cfmm_trades_len(self._h))

    def trades(self, out=None):
        """r.Δs / r.Λs of the latest materialising sweep as [m, 2] arrays (cfmm_get_trades).  `out` = (Δ, Λ): fill
        caller-owned C-contiguous float64 arrays instead of allocating (what a binding that owns r.Δs / r.Λs does).
        A market with weighted pools of more than two coins has ragged trades: two flat arrays of trades_len doubles
        (segment order, each pool's coins in Ai order)."""
        m = self.pool_count
        tl = self.trades_len
        if tl != 2 * m:
            if out is not None:
                raise ArgumentError("out arrays are not supported for ragged trades")
            D, Lm = np.empty(tl), np.empty(tl)
            self._check(self._L.cfmm_get_trades(self._h, ptr(D), ptr(Lm)))
            return D, Lm
        if out is None:
            D, Lm = np.empty((m, 2)), np.empty((m, 2))
        else:
            D, Lm = out
            for a in (D, Lm):
                if a.dtype != np.float64 or a.shape != (m, 2) or not a.flags.c_contiguous:
                    raise ArgumentError("out arrays must be C-contiguous float64 of shape [m, 2]")
        self._check(self._L.cfmm_get_trades(self._h, ptr(D), ptr(Lm)))
        return D, Lm

    def trades_range(self, seg, first, count, n_coins=2):
        D, Lm = np.empty((count, n_coins)), np.empty((count, n_coins))
        self._check(self._L.cfmm_get_trades_range(self._h, int(seg), int(first), int(count), ptr(D), ptr(Lm)))
        return D, Lm

    def select_trades(self, seg, min_value=0.0, v=None, capacity=None, n_coins=2):
        """The rows of segment `seg` that trade in the latest materialising sweep and are worth at least min_value, compacted
        on the device (cfmm_select_trades) -> (idx, Δ, Λ, value): rows within the segment in ascending order, their
        [count, n_coins] trade rows and value = Σ_k (Λ_k − Δ_k)·v[A_k].  v=None: the prices of that sweep.  capacity=None
        starts at min(m, 65536) rows and repeats the call once with the returned count if that was too small; an explicit
        capacity returns the first min(count, capacity) rows (the count itself: select_count)."""
        if capacity is not None and int(capacity) < 0:
            raise ArgumentError("capacity must be >= 0")
        v = None if v is None else self._check_v(v)
        n_coins = int(n_coins)
        cap = min(int(self.segments()[int(seg)]["m"]), 65536) if capacity is None else int(capacity)
        while True:
            idx, val = np.empty(cap, dtype=np.int64), np.empty(cap)
            D, Lm = np.empty((cap, n_coins)), np.empty((cap, n_coins))
            count = C.c_int64()
            self._check(self._L.cfmm_select_trades(self._h, int(seg), ptr(v), float(min_value), cap, C.byref(count),
                                                   ptr(idx), ptr(D), ptr(Lm), ptr(val)))
            if count.value <= cap or capacity is not None:
                k = min(count.value, cap)
                return idx[:k], D[:k], Lm[:k], val[:k]
            cap = count.value

    def select_count(self, seg, min_value=0.0, v=None) -> int:
        """How many rows select_trades would return (cfmm_select_trades with capacity 0: nothing is copied)."""
        v = None if v is None else self._check_v(v)
        count = C.c_int64()
        self._check(self._L.cfmm_select_trades(self._h, int(seg), ptr(v), float(min_value), 0, C.byref(count), None, None, None, None))
        return count.value

    def netflows(self):
        psi = np.empty(self.n_tokens)
        self._check(self._L.cfmm_netflows(self._h, ptr(psi)))
        return psi

    def dual_value(self) -> float:
        acc = C.c_double()
        self._check(self._L.cfmm_dual_value(self._h, C.byref(acc)))
        return acc.value

    def route(self, objective_kind, objective_vec, objective_index=0, v0=None, m=5, factr=1e1, pgtol=1e-5,
              maxfun=15_000, maxiter=15_000):
        """cfmm_route: route! entirely inside the library (own L-BFGS-B).  -> (v, psi, info dict)."""
        ov = f64(objective_vec)
        if ov.size != self.n_tokens:
            raise ArgumentError("objective vector must have n_tokens entries")
        v0a = None if v0 is None else f64(v0)
        v, psi, info = np.empty(self.n_tokens), np.empty(self.n_tokens), RouteInfo()
        self._check(self._L.cfmm_route(self._h, int(objective_kind), ptr(ov), int(objective_index), ptr(v0a),
                                       int(m), float(factr), float(pgtol), int(maxfun), int(maxiter), ptr(v),
                                       ptr(psi), C.byref(info)))
        return v, psi, info.as_dict()

    def polish(self, objective_kind, objective_vec, objective_index, v, max_iters=8, rel_step=1e-7):
        """cfmm_polish: the gradient-only projected chord-Newton polish inside the library.  -> (v, psi, info dict)."""
        ov = f64(objective_vec)
        if ov.size != self.n_tokens:
            raise ArgumentError("objective vector must have n_tokens entries")
        vv, psi, info = f64(np.array(v, dtype=np.float64).copy()), np.empty(self.n_tokens), PolishInfo()
        self._check(self._L.cfmm_polish(self._h, int(objective_kind), ptr(ov), int(objective_index), ptr(vv), int(max_iters),
                                        float(rel_step), ptr(psi), C.byref(info)))
        return vv, psi, info.as_dict()

    def update_reserves(self):
        """update_reserves!(r) on the device (cfmm_update_reserves): consumes the latest materialised trades."""
        self._check(self._L.cfmm_update_reserves(self._h))

    def reserves(self, seg: int, m: int, n_coins: int = 2):
        R = np.empty((int(m), int(n_coins)))
        self._check(self._L.cfmm_get_reserves(self._h, int(seg), ptr(R)))
        return R

    def prices(self, seg: int, m: int):
        p = np.empty(int(m))
        self._check(self._L.cfmm_get_prices(self._h, int(seg), ptr(p)))
        return p

    # -- sparse pool-state updates (cfmm_pools_set_*): rows `idx` of segment `seg`, nothing re-uploaded ----------------
    def set_reserves(self, seg: int, idx, R):
        """New reserves R [count, n_coins] of pools idx of a Product / GeoMean / Solidly / weighted segment."""
        idx, R = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1), f64(R)
        if idx.size == 0 or R.size % idx.size:
            if idx.size == 0 and R.size == 0:
                return self._check(self._L.cfmm_pools_set_reserves(self._h, int(seg), 0, ptr(idx), ptr(R)))
            raise ArgumentError("R must have shape [len(idx), n_coins]")
        self._check(self._L.cfmm_pools_set_reserves(self._h, int(seg), idx.size, ptr(idx), ptr(R)))

    def set_curve(self, seg: int, idx, R, alpha, beta):
        """New reserves R [count, n_coins] and parameters alpha, beta [count] of pools idx of a Curve segment."""
        idx, R = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1), f64(R)
        alpha, beta = f64(alpha).reshape(-1), f64(beta).reshape(-1)
        if alpha.size != idx.size or beta.size != idx.size or (idx.size and R.size % idx.size) or (not idx.size and R.size):
            raise ArgumentError("R must have shape [len(idx), n_coins], alpha and beta shape [len(idx)]")
        self._check(self._L.cfmm_pools_set_curve(self._h, int(seg), idx.size, ptr(idx), ptr(R), ptr(alpha), ptr(beta)))

    def set_prices(self, seg: int, idx, current_price):
        """New current prices [count] of pools idx of a UniV3 segment (ticks and liquidity unchanged)."""
        idx, p = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1), f64(current_price).reshape(-1)
        if p.size != idx.size:
            raise ArgumentError("current_price must have len(idx) entries")
        self._check(self._L.cfmm_pools_set_prices(self._h, int(seg), idx.size, ptr(idx), ptr(p)))

    def set_ticks(self, seg: int, idx, current_price, tick_off, lower_ticks, liquidity):
        """A mint / burn: new tick ladders of pools idx of a UniV3 segment, in CSR form over the rows (tick_off [count + 1],
        lower_ticks and liquidity [tick_off[-1]], as add_univ3 takes them), and a current price per row (cfmm_pools_set_ticks)."""
        idx, p = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1), f64(current_price).reshape(-1)
        off = np.ascontiguousarray(tick_off, dtype=np.int64).reshape(-1)
        lt, lq = f64(lower_ticks).reshape(-1), f64(liquidity).reshape(-1)
        if p.size != idx.size or off.size != idx.size + 1:
            raise ArgumentError("current_price must have len(idx) entries, tick_off len(idx) + 1")
        if lt.size != off[-1] or lq.size != off[-1]:
            raise ArgumentError("tick arrays must have tick_off[-1] entries")
        self._check(self._L.cfmm_pools_set_ticks(self._h, int(seg), idx.size, ptr(idx), ptr(p), ptr(off), ptr(lt), ptr(lq)))

    # -- exact-input swap quotes (cfmm_quote): read-only, on the pools as they stand on the device ---------------------
    def quote(self, seg: int, amount_in, coin_in, coin_out=None, idx=None):
        """amount_out [count] of tendering amount_in [count] of coin_in (positions in the pool's own coin order; a scalar
        serves every query) to rows idx of segment `seg` (None: rows 0 .. count-1; any order, repeats allowed).
        coin_out=None means 1 - coin_in on two-coin and UniV3 segments; weighted / Curve segments need it.  Everything is
        checked before anything runs (ArgumentError names the query)."""
        return self._quote("cfmm_quote", seg, amount_in, coin_in, coin_out, idx)

    def quote_out(self, seg: int, amount_out, coin_in, coin_out=None, idx=None):
        """The inverse of quote (cfmm_quote_out): amount_in [count] of coin_in to tender so that exactly amount_out [count]
        of coin_out comes out; same arguments and checks.  +inf where the pool cannot give that much (not an error)."""
        return self._quote("cfmm_quote_out", seg, amount_out, coin_in, coin_out, idx)

    def swap(self, seg: int, amount_in, coin_in, coin_out=None, idx=None):
        """quote's arguments, but the swaps are APPLIED (cfmm_swap), in query order: amount_out[q] is what quote answers on the
        pool as swaps 0 .. q-1 left it, and the pool then moves to R + γΔ − Λ (UniV3: to the price the swap rests at).  A row
        named k times is swapped k times.  A swap that would leave an invalid pool is not applied and answers NaN
        (get_option("swap_refused") counts them).  A state change: earlier trades and outputs are invalidated."""
        return self._quote("cfmm_swap", seg, amount_in, coin_in, coin_out, idx)

    def swap_out(self, seg: int, amount_out, coin_in, coin_out=None, idx=None, max_in=None, status=False):
        """quote_out's arguments, but the swaps are APPLIED (cfmm_swap_out), in query order: amount_in[q] is what quote_out
        answers on the pool as swaps 0 .. q-1 left it, and the pool then gives exactly amount_out[q]: it moves to
        R_in + γ·amount_in, R_out − amount_out (UniV3: to the price `swap` of amount_in rests at).  max_in: None, a scalar or
        one limit per swap.  A swap is not applied when the pool cannot give that much (+inf, SWAP_UNOBTAINABLE), when it
        would leave an invalid pool (NaN, SWAP_REFUSED) or when it costs more than max_in (the would-be quote,
        SWAP_OVER_LIMIT); get_option("swap_refused") counts them.  status=True: returns (amount_in, status).  A state
        change: earlier trades and outputs are invalidated."""
        lim = None
        if max_in is not None:
            try:
                lim = np.ascontiguousarray(np.broadcast_to(np.asarray(max_in, dtype=np.float64), (f64(amount_out).size,)))
            except ValueError:
                raise ArgumentError("max_in must be a scalar or have one entry per amount") from None
        st = np.empty(f64(amount_out).size, dtype=np.int32)
        out = self._quote("cfmm_swap_out", seg, amount_out, coin_in, coin_out, idx, lim, st)
        return (out, st) if status else out

    def _quote(self, entry, seg, given, coin_in, coin_out, idx, *swap_out_args):
        amt = f64(given).reshape(-1)
        n = amt.size
        bcast = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32).reshape(-1) if np.ndim(a) else
                                                               np.int32(a), (n,)), dtype=np.int32)
        try:
            ci = bcast(coin_in)
            co = None if coin_out is None else bcast(coin_out)
        except ValueError:
            raise ArgumentError("coin_in and coin_out must be scalars or have one entry per amount") from None
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if ix is not None and ix.size != n:
            raise ArgumentError("idx must have one entry per amount")
        out = np.empty(n)
        if swap_out_args:   # cfmm_swap_out: the limits go in front of the answers, the statuses behind them
            lim, st = swap_out_args
            self._check(getattr(self._L, entry)(self._h, int(seg), n, ptr(ix), ptr(ci), ptr(co), ptr(amt), ptr(lim), ptr(out), ptr(st)))
        else:
            self._check(getattr(self._L, entry)(self._h, int(seg), n, ptr(ix), ptr(ci), ptr(co), ptr(amt), ptr(out)))
        return out

    def quote_dev(self, seg: int, count: int, d_amount_in: int, d_coin_in: int, d_amount_out: int, d_coin_out: int = 0,
                  d_idx: int = 0):
        """cfmm_quote_dev on device addresses (float64 amounts, int32 coins, int64 idx; 0 = NULL): asynchronous on the
        context's stream, unchecked -- a bad query gets NaN, nothing is read out of bounds."""
        self._check(self._L.cfmm_quote_dev(self._h, int(seg), int(count), C.c_void_p(d_idx or None), C.c_void_p(d_coin_in or None),
                                           C.c_void_p(d_coin_out or None), C.c_void_p(d_amount_in or None),
                                           C.c_void_p(d_amount_out or None)))

    def quote_out_dev(self, seg: int, count: int, d_amount_out: int, d_coin_in: int, d_amount_in: int, d_coin_out: int = 0,
                      d_idx: int = 0):
        """cfmm_quote_out_dev on device addresses, as quote_dev: d_amount_out [count] is read (the wanted outputs),
        d_amount_in [count] is written (the inputs to tender; NaN for a bad query)."""
        self._check(self._L.cfmm_quote_out_dev(self._h, int(seg), int(count), C.c_void_p(d_idx or None), C.c_void_p(d_coin_in or None),
                                               C.c_void_p(d_coin_out or None), C.c_void_p(d_amount_out or None),
                                               C.c_void_p(d_amount_in or None)))

    # -- marginal rates (cfmm_quote_rate / cfmm_quote_path_rate, include/cfmm_amd_rate.h): the quote and its derivative --------
    def quote_rate(self, seg: int, amount_in, coin_in, coin_out=None, idx=None, count=None, want_out=True):
        """(amount_out, rate) [count]: quote's answer bit for bit, and the right derivative of the quote at amount_in -- at
        0 the pool's spot rate, fee included.  quote's arguments and checks.  amount_in=None means 0 for every query (a
        spot-price table; `count` gives the number of queries when neither coin_in nor idx is an array, and idx=None is then
        the dense pass over rows 0 .. count-1); want_out=False is allowed exactly then and returns (None, rate)."""
        if amount_in is None:
            n = int(count) if count is not None else max(np.size(coin_in), 0 if idx is None else np.size(idx))
            amt = None
        else:
            amt = f64(amount_in).reshape(-1)
            n = amt.size
            want_out = True
        bcast = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32).reshape(-1) if np.ndim(a) else
                                                               np.int32(a), (n,)), dtype=np.int32)
        try:
            ci = bcast(coin_in)
            co = None if coin_out is None else bcast(coin_out)
        except ValueError:
            raise ArgumentError("coin_in and coin_out must be scalars or have one entry per query") from None
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if ix is not None and ix.size != n:
            raise ArgumentError("idx must have one entry per query")
        out, rate = (np.empty(n) if want_out else None), np.empty(n)
        self._check(self._L.cfmm_quote_rate(self._h, int(seg), n, ptr(ix), ptr(ci), ptr(co), ptr(amt), ptr(out), ptr(rate)))
        return out, rate

    def quote_rate_dev(self, seg: int, count: int, d_amount_in: int, d_coin_in: int, d_amount_out: int, d_rate: int,
                       d_coin_out: int = 0, d_idx: int = 0):
        """cfmm_quote_rate_dev on device addresses, as quote_dev (0 = NULL; d_amount_in 0: every amount is 0, and d_amount_out
        may be 0 exactly then): asynchronous, unchecked -- a bad query gets NaN in both outputs."""
        self._check(self._L.cfmm_quote_rate_dev(self._h, int(seg), int(count), *(C.c_void_p(p or None) for p in (
            d_idx, d_coin_in, d_coin_out, d_amount_in, d_amount_out, d_rate))))

    # -- price limits (cfmm_quote_to_rate / cfmm_swap_limit, include/cfmm_amd_limit.h): the inverse of quote_rate -------------
    def quote_to_rate(self, seg: int, rate_limit, coin_in, coin_out=None, idx=None, want_out=True):
        """(amount_in, amount_out) [count]: the amount of coin_in that brings the pool's marginal rate (quote_rate's) down to
        rate_limit -- exactly +0.0 where the spot rate is already at or below it -- and what quote answers for that amount,
        bit for bit.  quote's arguments and checks with the limit (finite, > 0) in the place of the amount.  Read-only.
        want_out=False returns (amount_in, None)."""
        lim = f64(rate_limit).reshape(-1)
        n = lim.size
        ci, co, ix = self._query_columns(coin_in, coin_out, idx, n)
        amt, out = np.empty(n), (np.empty(n) if want_out else None)
        self._check(self._L.cfmm_quote_to_rate(self._h, int(seg), n, ptr(ix), ptr(ci), ptr(co), ptr(lim), ptr(amt), ptr(out)))
        return amt, out

    def quote_to_rate_dev(self, seg: int, count: int, d_rate_limit: int, d_coin_in: int, d_amount_in: int, d_amount_out: int = 0,
                          d_coin_out: int = 0, d_idx: int = 0):
        """cfmm_quote_to_rate_dev on device addresses, as quote_rate_dev (0 = NULL; d_amount_out may be 0): asynchronous,
        unchecked -- a query with a bad row, coin or limit gets NaN in both outputs."""
        self._check(self._L.cfmm_quote_to_rate_dev(self._h, int(seg), int(count), *(C.c_void_p(p or None) for p in (
            d_idx, d_coin_in, d_coin_out, d_rate_limit, d_amount_in, d_amount_out))))

    def swap_limit(self, seg: int, amount_in, rate_limit, coin_in, coin_out=None, idx=None):
        """(amount_used, amount_out, status) [count]: swap's arguments and a limit on the marginal rate per swap (a scalar or
        one per swap; 0.0: no limit).  The swaps are APPLIED in query order; swap q tenders min(amount_in, quote_to_rate's
        answer on the pool as swaps 0 .. q-1 left it), and the answer and the new state are swap's for that amount.
        amount_in may be +inf where the limit is > 0.  status: LIMIT_FILLED / LIMIT_PARTIAL / LIMIT_NONE / LIMIT_REFUSED.
        A state change: earlier trades and outputs are invalidated."""
        amt = f64(amount_in).reshape(-1)
        n = amt.size
        try:
            lim = np.ascontiguousarray(np.broadcast_to(np.asarray(rate_limit, dtype=np.float64), (n,)))
        except ValueError:
            raise ArgumentError("rate_limit must be a scalar or have one entry per amount") from None
        ci, co, ix = self._query_columns(coin_in, coin_out, idx, n)
        used, out, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        self._check(self._L.cfmm_swap_limit(self._h, int(seg), n, ptr(ix), ptr(ci), ptr(co), ptr(amt), ptr(lim), ptr(used), ptr(out), ptr(st)))
        return used, out, st

    @staticmethod
    def _query_columns(coin_in, coin_out, idx, n):
        bcast = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int32).reshape(-1) if np.ndim(a) else
                                                               np.int32(a), (n,)), dtype=np.int32)
        try:
            ci = bcast(coin_in)
            co = None if coin_out is None else bcast(coin_out)
        except ValueError:
            raise ArgumentError("coin_in and coin_out must be scalars or have one entry per query") from None
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if ix is not None and ix.size != n:
            raise ArgumentError("idx must have one entry per query")
        return ci, co, ix

    def quote_path_rate(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, hops=False):
        """(amount_out, rate[, hop_out, hop_rate]): quote_path's answers bit for bit, every hop's rate at the amount entering
        it ([max_hops, count], NaN in the unused slots) and their left-fold product ((r_0·r_1)·r_2)..., the path's marginal
        rate.  quote_path's arguments and checks."""
        amt = f64(amount_in).reshape(-1)
        n = amt.size
        nh, seg, row, ci, co = self._path_columns(n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        max_hops = max(1, int(seg.shape[0]))
        out, rate = np.empty(n), np.empty(n)
        hv, hr = (np.empty((max_hops, n)), np.empty((max_hops, n))) if hops else (None, None)
        if n:
            self._check(self._L.cfmm_quote_path_rate(self._h, n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(amt),
                                                     ptr(out), ptr(rate), ptr(hv), ptr(hr)))
        return (out, rate, hv, hr) if hops else (out, rate)

    def quote_path_rate_dev(self, count: int, max_hops: int, d_n_hops: int, d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int,
                            d_hop_coin_out: int, d_amount_in: int, d_amount_out: int, d_rate: int, d_hop_out: int = 0,
                            d_hop_rate: int = 0):
        """cfmm_quote_path_rate_dev on device addresses, as quote_path_dev (the hop arrays hop-major [max_hops, count])."""
        self._check(self._L.cfmm_quote_path_rate_dev(self._h, int(count), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_in, d_amount_out, d_rate, d_hop_out, d_hop_rate))))

    # -- multi-hop path quotes (cfmm_quote_path / cfmm_quote_path_out): an amount through a path of pools of any segments ----
    def quote_path(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, hops=False):
        """amount_out [count] of carrying amount_in [count] through paths of n_hops[p] hops (1 .. MAX_PATH_HOPS): hop k of
        path p enters row hop_row[p, k] of segment hop_seg[p, k] with coin hop_coin_in[p, k] and leaves with hop_coin_out[p, k]
        (positions in the pool's own coin order).  The hop arguments are [count, max_hops] arrays (slots at k >= n_hops[p]
        are ignored).  Every hop is quoted against the pool as it stands: no state advances between hops.  hops=True: also
        the [max_hops, count] amounts leaving each hop (NaN in the unused slots).  Everything is checked before anything
        runs (ArgumentError names the path and the hop)."""
        return self._quote_path("cfmm_quote_path", n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, hops)

    def quote_path_out(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, hops=False):
        """The inverse of quote_path (cfmm_quote_path_out): amount_in [count] to tender to the first hop so that exactly
        amount_out [count] leaves the last, walked from the last hop backwards; +inf from the hop on (towards the first)
        where a pool cannot give that much.  hops=True: also the [max_hops, count] amounts to tender to each hop."""
        return self._quote_path("cfmm_quote_path_out", n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, hops)

    def _quote_path(self, entry, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, given, hops):
        amt = f64(given).reshape(-1)
        n = amt.size
        nh, seg, row, ci, co = self._path_columns(n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        if n == 0:
            return (np.empty(0), np.empty((max(1, seg.shape[0]), 0))) if hops else np.empty(0)
        max_hops = int(seg.shape[0])
        out = np.empty(n)
        hv = np.empty((max_hops, n)) if hops else None
        self._check(getattr(self._L, entry)(self._h, n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(amt), ptr(out),
                                            ptr(hv)))
        return (out, hv) if hops else out

    # -- multi-hop path execution (cfmm_swap_path / cfmm_swap_path_out): the paths applied in order, each all or nothing ----
    def swap_path(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, min_out=None, hops=False):
        """quote_path's arguments, but the paths are APPLIED (cfmm_swap_path), in query order, each all or nothing: returns
        (amount_out, status[, hop_out]).  status[p] is PATH_APPLIED (amount_out[p] is what quote_path answers on the market
        the applied paths before p left, and every hop's pool has moved as `swap` moves it), PATH_BELOW_LIMIT (amount_out[p]
        < min_out[p]: the quote it would have given, nothing moved) or PATH_REFUSED (a hop would leave an invalid pool:
        NaN, nothing moved).  min_out: None, a scalar or one limit per path.  A pool may appear only once in a path.  A
        state change: earlier trades and outputs are invalidated; get_option("swap_refused") counts the paths not applied."""
        return self._swap_path("cfmm_swap_path", "min_out", n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_in, min_out, hops)

    def swap_path_out(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, max_in=None, hops=False):
        """quote_path_out's arguments, but the paths are APPLIED (cfmm_swap_path_out), in query order, each all or nothing:
        returns (amount_in, status[, hop_in]).  amount_in[p] and hop_in are what quote_path_out answers on the market the
        applied paths before p left; status[p] is SWAP_APPLIED (every hop's pool has moved as `swap_out` moves it),
        SWAP_UNOBTAINABLE (a pool on the way cannot give that much: +inf), SWAP_REFUSED (a hop would leave an invalid pool:
        NaN) or SWAP_OVER_LIMIT (amount_in[p] > max_in[p]: the quote it would have cost); in the last three nothing moved.
        max_in: None, a scalar or one limit per path.  A pool may appear only once in a path.  A state change, as swap_path."""
        return self._swap_path("cfmm_swap_path_out", "max_in", n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, amount_out, max_in, hops)

    def _swap_path(self, entry, limit_name, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, given, limit, hops):
        amt = f64(given).reshape(-1)
        n = amt.size
        nh, seg, row, ci, co = self._path_columns(n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        lim = None
        if limit is not None:
            try:
                lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, dtype=np.float64), (n,)))
            except ValueError:
                raise ArgumentError(f"{limit_name} must be a scalar or have one entry per amount") from None
        max_hops = max(1, int(seg.shape[0]))
        out, st = np.empty(n), np.empty(n, dtype=np.int32)
        hv = np.empty((max_hops, n)) if hops else None
        self._check(getattr(self._L, entry)(self._h, n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(amt), ptr(lim),
                                            ptr(out), ptr(hv), ptr(st)))
        return (out, st, hv) if hops else (out, st)

    def _path_columns(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, n):
        """n_hops and the four [count, max_hops] hop arguments, checked and in the ABI's layout: hop-major, [max_hops][count]"""
        nh = np.ascontiguousarray(n_hops, dtype=np.int32).reshape(-1)
        if nh.size != n:
            raise ArgumentError("n_hops must have one entry per amount")
        cols = []
        for name, a, dt in (("hop_seg", hop_seg, np.int32), ("hop_row", hop_row, np.int64), ("hop_coin_in", hop_coin_in, np.int32),
                            ("hop_coin_out", hop_coin_out, np.int32)):
            a = np.asarray(a, dtype=dt)
            if a.ndim == 1:                                                   # one hop per path
                a = a.reshape(-1, 1)
            if a.ndim != 2 or a.shape[0] != n or (cols and a.shape != cols[0].shape):
                raise ArgumentError(f"{name} must be a [count, max_hops] array, like the other hop arguments")
            cols.append(a)
        return (nh, *(np.ascontiguousarray(a.T) for a in cols))

    # -- path search (cfmm_find_path / cfmm_find_path_out): the best walk of at most max_hops hops between two tokens, found on the device ----------
    def find_path(self, token_in, token_out, amount_in, max_hops=3):
        """The best swap walk from token_in[q] to token_out[q] (0-based token ids) for amount_in[q], of at most max_hops
        (1 .. MAX_PATH_HOPS) hops, on the pools as they stand on the device (cfmm_find_path): returns (amount_out, n_hops, seg,
        row, ci, co, status) -- amount_out, n_hops, status [count]; seg, row, ci, co [count, max_hops] hop arrays, exactly what
        quote_path / swap_path take (-1 in the slots at k >= n_hops[q]).  The contract is the layered search: layer h holds, per
        token, the largest quote over every pool and ordered coin pair from layer h-1; the answer is the largest layer entry of
        token_out, with the fewest hops, walked back through the smallest (segment, row, coin_in, coin_out) that attains each
        layer bit for bit -- so quote_path on the result answers amount_out bit for bit.  Every hop is quoted against the pool
        as it stands; the result is a WALK and may visit a pool twice: status[q] is FOUND, FOUND_NONE (not reached, or amount 0:
        amount_out 0.0, n_hops 0) or FOUND_REPEATS (swap_path would refuse it as one path).  Scalars broadcast.  Read-only.
        Everything is checked before anything runs (ArgumentError names the query)."""
        return self._find_path("cfmm_find_path", "amount_in", token_in, token_out, amount_in, max_hops)

    def find_path_out(self, token_in, token_out, amount_out, max_hops=3):
        """The CHEAPEST swap walk that buys exactly amount_out[q] of token_out[q], paid in token_in[q] (0-based token ids), of at
        most max_hops (1 .. MAX_PATH_HOPS) hops, on the pools as they stand on the device (cfmm_find_path_out): returns
        (amount_in, n_hops, seg, row, ci, co, status) -- amount_in, n_hops, status [count]; seg, row, ci, co [count, max_hops] hop
        arrays in path order, exactly what quote_path_out / swap_path_out take (-1 in the slots at k >= n_hops[q]).  The
        contract is find_path's layered search run backwards from the wanted output: layer h holds, per token, the SMALLEST
        quote_out over every pool and ordered coin pair into layer h-1; the answer is the smallest layer entry of token_in, with
        the fewest hops, walked forward through the smallest (segment, row, coin_in, coin_out) that attains each layer bit for
        bit -- so quote_path_out on the result answers amount_in bit for bit.  status[q] is FOUND, FOUND_REPEATS (a walk that
        visits a pool twice: swap_path_out would refuse it as one path) or FOUND_NONE with n_hops 0 and amount_in +inf (token_in
        not reached within max_hops: no pool can give that much) or +0.0 (amount_out 0: nothing to buy).  Scalars broadcast.
        Read-only.  Everything is checked before anything runs (ArgumentError names the query)."""
        return self._find_path("cfmm_find_path_out", "amount_out", token_in, token_out, amount_out, max_hops)

    def _find_path(self, entry, amount_name, token_in, token_out, amount, max_hops):
        try:
            tin, tout, amt = np.broadcast_arrays(np.asarray(token_in, dtype=np.int32).reshape(-1), np.asarray(token_out, dtype=np.int32).reshape(-1),
                                                 f64(amount).reshape(-1))
        except ValueError:
            raise ArgumentError(f"token_in, token_out and {amount_name} must be scalars or have one entry per query") from None
        tin, tout, amt = (np.ascontiguousarray(a) for a in (tin, tout, amt))
        n, H = amt.size, int(max_hops)
        out, nh, st = np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        seg, ci, co = (np.empty((max(H, 0), n), dtype=np.int32) for _ in range(3))
        row = np.empty((max(H, 0), n), dtype=np.int64)
        self._check(getattr(self._L, entry)(self._h, n, H, ptr(tin), ptr(tout), ptr(amt), ptr(out), ptr(nh), ptr(seg), ptr(row), ptr(ci),
                                            ptr(co), ptr(st)))
        return out, nh, seg.T.copy(), row.T.copy(), ci.T.copy(), co.T.copy(), st

    # -- several paths per order (cfmm_find_disjoint_paths): find_path's search run max_paths times, the found pools absent afterwards ----------
    def find_disjoint_paths(self, token_in, token_out, amount_in, max_paths=4, max_hops=3):
        """Up to max_paths (1 .. MAX_SPLIT_PATHS) swap paths from token_in[q] to token_out[q] (0-based token ids) that share NO
        POOL, on the pools as they stand on the device (cfmm_find_disjoint_paths): returns (n_paths [count], amount_out
        [count, K], n_hops [count, K], seg, row, ci, co [count, K, max_hops], status [count, K]) with K = max_paths.  The
        contract is successive search: path r of a query is find_path's answer for (token_in, token_out, amount_in, max_hops) on
        the market without every pool of the query's paths 0 .. r-1 -- greedy successive-best, not "the K best overall".  So
        slot 0 is find_path's answer, the amounts do not increase with r, quote_path on path r at amount_in[q] answers
        amount_out[q, r] bit for bit, and the found paths fill the slots 0 .. n_paths[q]-1; the others carry FOUND_NONE, 0 hops,
        0.0 and -1.  A walk that visits a pool twice keeps its slot as FOUND_REPEATS.  The same amount_in probes every round: to
        split A over K paths, probing with A / K may serve better.  Scalars broadcast.  Read-only.  Everything is checked before
        anything runs (ArgumentError names the query)."""
        return self._find_disjoint("cfmm_find_disjoint_paths", "amount_in", token_in, token_out, amount_in, max_paths, max_hops)

    def find_disjoint_paths_out(self, token_in, token_out, amount_out, max_paths=4, max_hops=3):
        """find_disjoint_paths for a wanted output (cfmm_find_disjoint_paths_out): up to max_paths paths from token_in[q] to
        token_out[q] that share NO POOL, path r being find_path_out's answer for (token_in, token_out, amount_out, max_hops) on
        the market without every pool of the query's paths 0 .. r-1.  Returns (n_paths [count], amount_in [count, K], n_hops
        [count, K], seg, row, ci, co [count, K, max_hops], status [count, K]).  Slot 0 is find_path_out's answer, the amounts do
        not decrease with r, quote_path_out on path r at amount_out[q] answers amount_in[q, r] bit for bit; empty slots carry
        FOUND_NONE, 0 hops, -1 and find_path_out's none value (+inf, or 0.0 where amount_out is 0).  The same amount_out probes
        every round, and a path that cannot give it alone is never found: to buy B through K paths probe with about B / K.
        Scalars broadcast.  Read-only.  Everything is checked before anything runs (ArgumentError names the query)."""
        return self._find_disjoint("cfmm_find_disjoint_paths_out", "amount_out", token_in, token_out, amount_out, max_paths, max_hops)

    def _find_disjoint(self, entry, amount_name, token_in, token_out, amount_in, max_paths, max_hops):
        try:
            tin, tout, amt = np.broadcast_arrays(np.asarray(token_in, dtype=np.int32).reshape(-1), np.asarray(token_out, dtype=np.int32).reshape(-1),
                                                 f64(amount_in).reshape(-1))
        except ValueError:
            raise ArgumentError(f"token_in, token_out and {amount_name} must be scalars or have one entry per query") from None
        tin, tout, amt = (np.ascontiguousarray(a) for a in (tin, tout, amt))
        n, H, K = amt.size, int(max_hops), int(max_paths)
        kk, hh = max(K, 0), max(H, 0)
        npaths, out = np.empty(n, dtype=np.int32), np.empty((kk, n))
        nh, st = (np.empty((kk, n), dtype=np.int32) for _ in range(2))
        seg, ci, co = (np.empty((kk, hh, n), dtype=np.int32) for _ in range(3))
        row = np.empty((kk, hh, n), dtype=np.int64)
        self._check(getattr(self._L, entry)(self._h, n, K, H, ptr(tin), ptr(tout), ptr(amt), ptr(npaths), ptr(out), ptr(nh), ptr(st),
                                            ptr(seg), ptr(row), ptr(ci), ptr(co)))
        hops = lambda a: np.ascontiguousarray(a.transpose(2, 0, 1))
        return npaths, out.T.copy(), nh.T.copy(), hops(seg), hops(row), hops(ci), hops(co), st.T.copy()

    # -- path sizing (cfmm_size_path): the input of a path, at most max_in, that maximises its gain ----------
    def size_path(self, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, max_in, value_in=None, value_out=None, rounds=5):
        """How much to put into each path (cfmm_size_path): quote_path's path arguments, and per path the largest input
        max_in[p] to consider.  Returns (amount_in, amount_out, gain, status), each [count]: the input that maximises
        gain(x) = value_out[p] * quote_path(p, x) - value_in[p] * x (None = 1.0: "out minus in", the profit of a cycle), what
        quote_path answers for it bit for bit, and that gain.  The contract is the bracketing search: `rounds` (1 ..
        MAX_SIZE_ROUNDS) rounds of 64 trial sizes spread evenly over the bracket, which starts as [0, max_in] and becomes the
        two neighbours of the best trial size (the smallest among equals; NaN loses).  For a concave gain -- every pool
        family's quote is concave -- the bracket shrinks by 2/63 per round around the maximiser; 5 rounds reach the closed-form
        optimum of two-pool cycles to about 1e-12 of its gain.  status[p] is SIZED, SIZED_AT_LIMIT (gain > 0 at amount_in == max_in
        bit for bit: the limit binds), SIZED_NONE (no trial size gains: three 0.0) or SIZED_NAN.  Every hop is quoted against the
        pool as it stands.  Scalars broadcast.  Read-only.  Everything is checked before anything runs (ArgumentError names
        the path and the hop)."""
        nh0 = np.ascontiguousarray(n_hops, dtype=np.int32).reshape(-1)
        n = nh0.size
        try:
            lim = np.ascontiguousarray(np.broadcast_to(f64(max_in).reshape(-1), (n,)))
            vi, vo = (None if v is None else np.ascontiguousarray(np.broadcast_to(f64(v).reshape(-1), (n,))) for v in (value_in, value_out))
        except ValueError:
            raise ArgumentError("max_in, value_in and value_out must be scalars or have one entry per path") from None
        nh, seg, row, ci, co = self._path_columns(nh0, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        max_hops = max(1, int(seg.shape[0]))
        x, y, g, st = np.empty(n), np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        self._check(self._L.cfmm_size_path(self._h, n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(lim), ptr(vi), ptr(vo),
                                           int(rounds), ptr(x), ptr(y), ptr(g), ptr(st)))
        return x, y, g, st

    def size_path_dev(self, count: int, max_hops: int, d_n_hops: int, d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int,
                      d_hop_coin_out: int, d_max_in: int, d_value_in: int, d_value_out: int, rounds: int, d_amount_in: int,
                      d_amount_out: int, d_gain: int, d_status: int):
        """cfmm_size_path_dev on device addresses (as quote_path_dev: the hop arrays hop-major [max_hops][count]; d_value_in /
        d_value_out 0 = NULL = 1.0; float64 amounts and gains, int32 status): asynchronous on the context's stream, unchecked
        -- a bad path, hop, limit or value gives that path SIZED_NAN and NaN outputs, nothing is read out of bounds."""
        self._check(self._L.cfmm_size_path_dev(self._h, int(count), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_max_in, d_value_in, d_value_out)), int(rounds),
            *(C.c_void_p(p or None) for p in (d_amount_in, d_amount_out, d_gain, d_status))))

    # -- order splitting (cfmm_split_paths): an order's amount spread over its 1 .. 8 paths ----------
    def split_paths(self, order_first, amount_in, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds=5):
        """How much of each order goes down each of its paths (cfmm_split_paths): quote_path's path arguments for all the
        paths, `order_first` [orders + 1] (order g owns the paths order_first[g] .. order_first[g+1] - 1, 1 .. MAX_SPLIT_PATHS of
        them) and the amount of each order.  Returns (path_amount_in [n_paths], path_amount_out [n_paths], total_out [orders],
        status [orders]).  The contract is the greedy search of include/cfmm_amd_split.h: `rounds` (1 .. MAX_SPLIT_ROUNDS) rounds
        of 64 grid points per path; each round hands out 63 slices of what is left, one by one, to the path whose next slice
        buys the most (the smallest path among equals; NaN loses), then steps every share back one slice and refines.  The
        shares sum to the amount (to its rounding); with one path the share is the amount bit for bit; quote_path at
        path_amount_in answers path_amount_out bit for bit.  On 4000 random orders of product chains the default 5 rounds
        were within 8e-12 of the closed-form optimum for 99 % of the orders and within 1.6e-7 for all (the worst orders have 8
        paths, one of which carries most of the amount: one step back is then not enough).  status[g] is SPLIT_OK,
        SPLIT_SATURATED (part of the amount buys nothing: the paths cannot absorb it), SPLIT_NONE (amount 0 or nothing
        comes out: zeros) or SPLIT_NAN.  No pool may occur twice among an order's paths.  Every hop is quoted against the
        pool as it stands.  Read-only.  Everything is checked before anything runs (ArgumentError names the order)."""
        first = np.ascontiguousarray(order_first, dtype=np.int64).reshape(-1)
        amt = np.ascontiguousarray(f64(amount_in).reshape(-1))
        if first.size != amt.size + 1:
            raise ArgumentError("order_first must have one entry more than amount_in")
        nh0 = np.ascontiguousarray(n_hops, dtype=np.int32).reshape(-1)
        n = nh0.size
        nh, seg, row, ci, co = self._path_columns(nh0, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        max_hops = max(1, int(seg.shape[0]))
        g = amt.size
        x, y, tot, st = np.empty(n), np.empty(n), np.empty(g), np.empty(g, dtype=np.int32)
        self._check(self._L.cfmm_split_paths(self._h, g, ptr(first), ptr(amt), n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co),
                                             int(rounds), ptr(x), ptr(y), ptr(tot), ptr(st)))
        return x, y, tot, st

    def split_paths_dev(self, count: int, d_order_first: int, d_amount_in: int, n_paths: int, max_hops: int, d_n_hops: int,
                        d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int, d_hop_coin_out: int, rounds: int, d_path_amount_in: int,
                        d_path_amount_out: int, d_total_out: int, d_status: int):
        """cfmm_split_paths_dev on device addresses (int64 order_first [count + 1], float64 amounts; the hop arrays hop-major
        [max_hops][n_paths] as quote_path_dev's; int32 status): asynchronous on the context's stream, unchecked -- a bad
        order, path, hop or amount gives that order SPLIT_NAN and NaN outputs, nothing is read out of bounds.  Pools shared
        between an order's paths are NOT looked for here."""
        self._check(self._L.cfmm_split_paths_dev(self._h, int(count), C.c_void_p(d_order_first or None), C.c_void_p(d_amount_in or None),
                                                 int(n_paths), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out)), int(rounds),
            *(C.c_void_p(p or None) for p in (d_path_amount_in, d_path_amount_out, d_total_out, d_status))))

    # -- order execution (cfmm_swap_order / cfmm_swap_order_out): orders applied in order, each all or nothing ACROSS its paths ----
    def swap_order(self, order_first, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, path_amount_in, min_total_out=None, hops=False):
        """split_paths' path arguments and `order_first`, with an amount per path, but the orders are APPLIED (cfmm_swap_order),
        in the caller's order, each all or nothing across its 1 .. MAX_SPLIT_PATHS paths: returns (path_amount_out [n_paths],
        total_out [orders], status [orders], path_status [n_paths][, hop_out]).  Every path is walked as swap_path walks it,
        on the market the applied orders before left; total_out[g] is the paths' outputs added in increasing path order
        (split_paths' total_out bit for bit on an unmoved market).  status[g] is ORDER_APPLIED (every path's pools moved as
        swap_path moves them), ORDER_LIMIT (total_out[g] < min_total_out[g]: the sum it would have given, nothing moved) or
        ORDER_REFUSED (some path has a refusing hop: NaN, nothing moved); path_status[p] is PATH_APPLIED, PATH_REFUSED or
        ORDER_PATH_HELD (the path passes, its order was not applied).  min_total_out: None, a scalar or one limit per order.
        No pool may occur twice among an order's paths.  A state change as swap_path; get_option("swap_refused") counts the
        orders not applied."""
        return self._swap_order("cfmm_swap_order", "min_total_out", order_first, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out,
                                path_amount_in, min_total_out, hops)

    def swap_order_out(self, order_first, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, path_amount_out, max_total_in=None, hops=False):
        """The exact-output twin (cfmm_swap_order_out): path_amount_out[p] is wanted from path p, every path is walked as
        swap_path_out walks it; returns (path_amount_in, total_in, status, path_status[, hop_in]).  status[g] may also be
        ORDER_UNOBTAINABLE (some path cannot give its amount: total_in +inf, nothing moved; that path's path_status is
        SWAP_UNOBTAINABLE); ORDER_LIMIT is total_in[g] > max_total_in[g]."""
        return self._swap_order("cfmm_swap_order_out", "max_total_in", order_first, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out,
                                path_amount_out, max_total_in, hops)

    def _swap_order(self, entry, limit_name, order_first, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, given, limit, hops):
        first = np.ascontiguousarray(order_first, dtype=np.int64).reshape(-1)
        amt = np.ascontiguousarray(f64(given).reshape(-1))
        n = amt.size
        nh, seg, row, ci, co = self._path_columns(n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        g = max(0, first.size - 1)
        if first.size == 0 and n:
            raise ArgumentError("order_first must have one entry more than there are orders")
        lim = None
        if limit is not None:
            try:
                lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, dtype=np.float64), (g,)))
            except ValueError:
                raise ArgumentError(f"{limit_name} must be a scalar or have one entry per order") from None
        max_hops = max(1, int(seg.shape[0]))
        out, pst = np.empty(n), np.empty(n, dtype=np.int32)
        tot, st = np.empty(g), np.empty(g, dtype=np.int32)
        hv = np.empty((max_hops, n)) if hops else None
        self._check(getattr(self._L, entry)(self._h, g, ptr(first), n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co), ptr(amt),
                                            ptr(lim), ptr(out), ptr(hv), ptr(tot), ptr(pst), ptr(st)))
        return (out, tot, st, pst, hv) if hops else (out, tot, st, pst)

    # -- buying through several paths (cfmm_split_paths_out): a wanted amount spread over an order's 1 .. 8 paths ----------
    def split_paths_out(self, order_first, amount_out, n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, rounds=5):
        """How much of each order's wanted amount is bought through each of its paths (cfmm_split_paths_out): split_paths'
        arguments with amount_out[g], the amount of the paths' common last token to buy.  Returns (path_amount_out [n_paths],
        path_amount_in [n_paths], total_in [orders], status [orders]).  The contract is the greedy search of
        include/cfmm_amd_split_out.h: split_paths' grid laid over the output; each round hands out 63 slices of what is left,
        one by one, to the path whose next slice COSTS the least (the smallest path among equals; +inf is a number, NaN
        loses), then steps every share back one slice and refines.  On a SPLIT_OK order the shares sum to the amount (to its
        rounding), with one path the share is the amount bit for bit, and quote_path_out at path_amount_out answers
        path_amount_in bit for bit.  status[g] is SPLIT_OK; SPLIT_UNOBTAINABLE (the first step that was not finite took +inf:
        no path can give another slice -- costs and total +inf, shares 0.0; the search's verdict on its grid: paths that
        jointly give less than amount * (1 + K/63) may be refused though a finer split exists); SPLIT_NONE (amount 0: zeros)
        or SPLIT_NAN.  No pool may occur twice among an order's paths.  Every hop is quoted against the pool as it stands.
        Read-only.  Everything is checked before anything runs (ArgumentError names the order)."""
        first = np.ascontiguousarray(order_first, dtype=np.int64).reshape(-1)
        amt = np.ascontiguousarray(f64(amount_out).reshape(-1))
        if first.size != amt.size + 1:
            raise ArgumentError("order_first must have one entry more than amount_out")
        nh0 = np.ascontiguousarray(n_hops, dtype=np.int32).reshape(-1)
        n = nh0.size
        nh, seg, row, ci, co = self._path_columns(nh0, hop_seg, hop_row, hop_coin_in, hop_coin_out, n)
        max_hops = max(1, int(seg.shape[0]))
        g = amt.size
        x, y, tot, st = np.empty(n), np.empty(n), np.empty(g), np.empty(g, dtype=np.int32)
        self._check(self._L.cfmm_split_paths_out(self._h, g, ptr(first), ptr(amt), n, max_hops, ptr(nh), ptr(seg), ptr(row), ptr(ci), ptr(co),
                                                 int(rounds), ptr(x), ptr(y), ptr(tot), ptr(st)))
        return x, y, tot, st

    def split_paths_out_dev(self, count: int, d_order_first: int, d_amount_out: int, n_paths: int, max_hops: int, d_n_hops: int,
                            d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int, d_hop_coin_out: int, rounds: int, d_path_amount_out: int,
                            d_path_amount_in: int, d_total_in: int, d_status: int):
        """cfmm_split_paths_out_dev on device addresses, as split_paths_dev: d_amount_out [count] is read (the wanted amounts),
        d_path_amount_out (the shares), d_path_amount_in (their costs), d_total_in and d_status are written."""
        self._check(self._L.cfmm_split_paths_out_dev(self._h, int(count), C.c_void_p(d_order_first or None), C.c_void_p(d_amount_out or None),
                                                     int(n_paths), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out)), int(rounds),
            *(C.c_void_p(p or None) for p in (d_path_amount_out, d_path_amount_in, d_total_in, d_status))))

    def quote_path_dev(self, count: int, max_hops: int, d_n_hops: int, d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int,
                       d_hop_coin_out: int, d_amount_in: int, d_amount_out: int, d_hop_out: int = 0):
        """cfmm_quote_path_dev on device addresses (int32 n_hops / segments / coins, int64 rows, float64 amounts; the hop
        arrays in the ABI's own hop-major [max_hops][count] layout; d_hop_out 0 = NULL): asynchronous on the context's
        stream, unchecked -- a bad path or hop gets NaN from there on, nothing is read out of bounds."""
        self._check(self._L.cfmm_quote_path_dev(self._h, int(count), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_in, d_amount_out, d_hop_out))))

    def quote_path_out_dev(self, count: int, max_hops: int, d_n_hops: int, d_hop_seg: int, d_hop_row: int, d_hop_coin_in: int,
                           d_hop_coin_out: int, d_amount_out: int, d_amount_in: int, d_hop_in: int = 0):
        """cfmm_quote_path_out_dev on device addresses, as quote_path_dev: d_amount_out [count] is read (the wanted outputs),
        d_amount_in [count] and d_hop_in (0 = NULL) are written."""
        self._check(self._L.cfmm_quote_path_out_dev(self._h, int(count), int(max_hops), *(C.c_void_p(p or None) for p in (
            d_n_hops, d_hop_seg, d_hop_row, d_hop_coin_in, d_hop_coin_out, d_amount_out, d_amount_in, d_hop_in))))

    def set_peers(self, peer_ptrs, world: int, rank: int, seq: int):
        """Sharded operation: every host-pointer sweep of this context ends with the one-shot peer
        all-reduce over the given symmetric buffers (cfmm_set_peers).  world=0 switches it off."""
        arr = (C.c_uint64 * max(world, 1))(*[int(p) for p in peer_ptrs][:max(world, 1)]) if world else None
        self._check(self._L.cfmm_set_peers(self._h, arr, int(world), int(rank), C.c_uint64(int(seq))))

    def peer_buffer_alloc(self):
        """This rank's symmetric buffer for cfmm_set_peers -> (device pointer, 64-byte IPC handle)."""
        p = C.c_uint64()
        h = C.create_string_buffer(64)
        self._check(self._L.cfmm_peer_buffer_alloc(self._h, C.byref(p), h))
        return p.value, h.raw

    def peer_buffer_open(self, handle: bytes) -> int:
        p = C.c_uint64()
        self._check(self._L.cfmm_peer_buffer_open(self._h, C.create_string_buffer(bytes(handle), 64), C.byref(p)))
        return p.value

    def peer_buffer_close(self, ptr_: int):
        self._check(self._L.cfmm_peer_buffer_close(self._h, C.c_uint64(int(ptr_))))

    def peer_buffer_free(self, ptr_: int):
        self._check(self._L.cfmm_peer_buffer_free(self._h, C.c_uint64(int(ptr_))))

    # sharded operation through RCCL (include/cfmm_amd.h): rank 0 makes the id, every rank joins with it
    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = lib().cfmm_rccl_unique_id(buf)
        if rc != OK:
            raise CFMMDeviceError(lib().cfmm_last_error(None).decode())
        return buf.raw

    def rccl_init_rank(self, uid: bytes, world: int, rank: int):
        self._check(lib().cfmm_rccl_init_rank(self._h, uid, int(world), int(rank)))

    def set_rccl_comm(self, comm_ptr):
        self._check(lib().cfmm_set_rccl_comm(self._h, comm_ptr))

    def sweep_dev(self, d_v_ptr: int, d_out_ptr: int, materialize: bool):
        self._check(self._L.cfmm_sweep_dev(self._h, C.c_void_p(d_v_ptr), C.c_void_p(d_out_ptr),
                                           1 if materialize else 0))

    def trades_dev(self):
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self._L.cfmm_trades_dev(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_times(self):
        sn, rn = C.c_int64(), C.c_int64()
        sm, rm = C.c_double(), C.c_double()
        self._check(self._L.cfmm_kernel_times(self._h, C.byref(sn), C.byref(sm), C.byref(rn), C.byref(rm)))
        return {"sweep_launches": sn.value, "sweep_ms": sm.value, "reduce_launches": rn.value,
                "reduce_ms": rm.value}

    def segments(self):
        out = []
        for s in range(self._L.cfmm_segment_count(self._h)):
            k, b, g = C.c_int32(), C.c_int32(), C.c_int32()
            m = C.c_int64()
            self._check(self._L.cfmm_segment_info(self._h, s, C.byref(k), C.byref(m), C.byref(b), C.byref(g)))
            out.append({"kind": k.value, "m": m.value, "block": b.value, "grid": g.value})
        return out


def lbfgsb_minimize(fun, x0, bounds, m=5, factr=1e1, pgtol=1e-5, maxfun=15_000, maxiter=15_000,
                    reference_boxed=False):
    """The library's own L-BFGS-B on a Python objective `fun(x) -> (f, g)` (host only; used by the
    CPU tests to compare the solver with SciPy's).  bounds: list of (lo, hi) with None = unbounded.
    reference_boxed=True passes nbd = 2 for every variable (infinite bounds included) and lets the
    solver take the Fortran code's "boxed" first step, as the reference's call does."""
    n = len(x0)
    x = f64(np.array(x0, dtype=np.float64).copy())
    lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
    hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
    nbd = np.array([(1 if np.isfinite(l) else 0) + (2 if np.isfinite(h) else 0) for l, h in zip(lo, hi)])
    nbd = np.array([{0: 0, 1: 1, 3: 2, 2: 3}[int(k)] for k in nbd], dtype=np.int32)
    if reference_boxed:
        nbd[:] = 2

    def cb(_user, xp, gp):
        xx = np.ctypeslib.as_array(xp, shape=(n,))
        fval, g = fun(xx.copy())
        np.ctypeslib.as_array(gp, shape=(n,))[:] = g
        return float(fval)

    info = RouteInfo()
    rc = lib().cfmm_lbfgsb_minimize(n, ptr(x), ptr(lo), ptr(hi), ptr(nbd), FG_CALLBACK(cb), None, int(m),
                                    float(factr), float(pgtol), int(maxfun), int(maxiter),
                                    1 if reference_boxed else 0, C.byref(info))
    if rc != OK:
        raise ArgumentError(lib().cfmm_last_error(None).decode())
    return x, info.as_dict()
