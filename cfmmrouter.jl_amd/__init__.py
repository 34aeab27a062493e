"""cfmmrouter.jl_amd -- MI355X-native drop-in for CFMMRouter.jl's arbitrage-sweep hot path.

Exports the reference's names (src/CFMMRouter.jl, src/cfmms.jl:1-3, src/objectives.jl:1,
src/router.jl:1-2).  Julia's `f!` is spelled `f_` here.  All pool arithmetic runs on the GPU
through libcfmm_amd.so (include/cfmm_amd.h); there is no CPU fallback in this package.
"""
from ._lib import FOUND, FOUND_NONE, FOUND_REPEATS, LIMIT_FILLED, LIMIT_NONE, LIMIT_PARTIAL, LIMIT_REFUSED, ORDER_APPLIED, ORDER_LIMIT, ORDER_PATH_HELD, ORDER_REFUSED, ORDER_UNOBTAINABLE, SIZED, SIZED_AT_LIMIT, SIZED_NAN, SIZED_NONE, SPLIT_NAN, SPLIT_NONE, SPLIT_OK, SPLIT_SATURATED, SPLIT_UNOBTAINABLE, ArgumentError, CFMMDeviceError, Context, build, lib
from .cfmms import (CFMM, BoundedProduct, Curve, GeometricMean, GeometricMeanTwoCoin, PoolBatch, Product, ProductTwoCoin,
                    SolidlyStableTwoCoin, UniV3, backward_trade, find_arb_ as _find_arb_pool, forward_trade,
                    grad_phi_, phi, zerotrade, ϕ, ϕ_grad_)
from .objectives import (BasketLiquidation, LinearNonnegative, Objective, Swap, f, grad_, lower_limit,
                         upper_limit)
from .router import (DeviceBackend, Router, active_trades, amount_to_rate, swap_limit_, dual_jacobian, find_arb_ as _find_arb_router, find_disjoint_paths, find_disjoint_paths_out, find_path, find_path_out, netflows, netflows_, path_price_impact, polish_, price_impact, quote, quote_out, quote_path, quote_path_out, quote_path_rate, quote_rate, route_, route_order, route_order_, route_order_out, route_order_out_, size_path, split_paths, split_paths_out, spot_price,
                     swap_, swap_order_, swap_order_out_, swap_out_, swap_path_, swap_path_out_, update_pools_, update_reserves_)


def find_arb_(*args, **kw):
    """find_arb!(r::Router, v)  or  find_arb!(Δ, Λ, cfmm, v)  (multiple dispatch on arity)."""
    if len(args) == 2:
        return _find_arb_router(*args, **kw)
    return _find_arb_pool(*args, **kw)


__all__ = [
    "CFMM", "ProductTwoCoin", "GeometricMeanTwoCoin", "UniV3", "BoundedProduct", "GeometricMean", "Product", "Curve",
    "SolidlyStableTwoCoin",
    "PoolBatch", "find_arb_",
    "update_reserves_", "update_pools_", "Objective", "LinearNonnegative", "BasketLiquidation", "Swap", "f", "grad_",
    "lower_limit", "upper_limit", "Router", "route_", "netflows_", "netflows", "ArgumentError",
    "CFMMDeviceError", "Context", "DeviceBackend", "build", "lib", "zerotrade", "ϕ", "ϕ_grad_", "phi", "grad_phi_",
    "polish_", "dual_jacobian", "active_trades", "forward_trade", "quote", "backward_trade", "quote_out",
    "quote_path", "quote_path_out", "swap_", "swap_path_", "swap_out_", "swap_path_out_",
    "find_path", "find_path_out", "FOUND", "FOUND_NONE", "FOUND_REPEATS",
    "size_path", "SIZED", "SIZED_NONE", "SIZED_AT_LIMIT", "SIZED_NAN",
    "find_disjoint_paths", "route_order",
    "split_paths", "SPLIT_OK", "SPLIT_NONE", "SPLIT_NAN", "SPLIT_SATURATED",
    "split_paths_out", "find_disjoint_paths_out", "route_order_out", "SPLIT_UNOBTAINABLE",
    "swap_order_", "swap_order_out_", "route_order_", "route_order_out_",
    "quote_rate", "spot_price", "price_impact", "quote_path_rate", "path_price_impact",
    "ORDER_APPLIED", "ORDER_LIMIT", "ORDER_REFUSED", "ORDER_UNOBTAINABLE", "ORDER_PATH_HELD",
    "amount_to_rate", "swap_limit_", "LIMIT_FILLED", "LIMIT_PARTIAL", "LIMIT_NONE", "LIMIT_REFUSED",
]
