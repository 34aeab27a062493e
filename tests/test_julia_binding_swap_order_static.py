"""The Julia binding of order execution, checked WITHOUT a Julia toolchain (there is none in the images this suite runs in) as
tests/test_julia_binding_split_out_static.py checks the splits: swap_orders! and swap_orders_out! exist in their own file, the
module includes the file and exports the verbs, each ccall names its entry with the argument count and types of
include/cfmm_amd_order.h, the five constants agree between the header, the Python binding and the Julia file, and the verbs' own
test file uses them."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read

NAMES = ("ORDER_APPLIED", "ORDER_LIMIT", "ORDER_REFUSED", "ORDER_UNOBTAINABLE", "ORDER_PATH_HELD")


def test_the_ccalls_match_the_header():
    decls = declarations(read("include", "cfmm_amd_order.h"))
    assert set(decls) == {"cfmm_swap_order", "cfmm_swap_order_out"}
    for other in ("cfmm_amd.h", "cfmm_amd_split.h", "cfmm_amd_split_out.h", "cfmm_amd_path_out.h"):
        assert not set(decls) & set(declarations(read("include", other)))        # the addition lives in its own header
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "swap_order.jl"))}
    assert list(calls) == ["cfmm_swap_order", "cfmm_swap_order_out"]
    for entry in calls:
        cret, cargs = decls[entry]
        ret, args = calls[entry]
        assert ret in C2J[cret]
        assert len(args) == len(cargs) == 17, f"{entry}: {len(args)} Julia arguments vs {len(cargs)} in the header"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert ja in C2J[ca], f"{entry} argument {k}: Julia {ja} vs C {ca}"
    assert decls["cfmm_swap_order_out"][1] == decls["cfmm_swap_order"][1]       # the twin takes the forward entry's list


def test_the_verbs_are_defined_exported_used_and_carry_the_headers_constants():
    module = read("julia", "src", "CFMMRouterAMD.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    src = read("julia", "src", "swap_order.jl")
    tests = read("julia", "test", "swap_order.jl")
    assert 'include("swap_order.jl")' in module and ":cfmm_swap_order" not in module
    assert module.index('include("split_paths_out.jl")') < module.index('include("swap_order.jl")')   # it uses split_paths.jl's limits
    defined = set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    for verb in ("swap_orders!", "swap_orders_out!"):
        assert verb in exported and verb in defined and f"{verb}(" in tests, verb
    header = read("include", "cfmm_amd_order.h")
    from cfmmrouter_amd import _lib
    for name in NAMES:
        value = re.search(r"#define CFMM_" + name + r" (\d+)", header).group(1)
        assert re.search(r"^const " + name + r" = Int32\((\d)\)", src, flags=re.M).group(1) == value, name
        assert getattr(_lib, name) == int(value), name
    assert '#include "cfmm_amd_split_out.h"' in header and "CFMM_MAX_SPLIT_PATHS" not in re.findall(r"#define (\w+)", header)   # the limits are the split header's
    body = src[src.index("function order_hop_arrays("):]
    assert "path_hop_arrays(r, flat_pools, flat_tokens" in body                 # quote_paths' mapping: 1-based tokens, every refusal
    assert "download_state!(r)" in body and "fill!(d, 0)" in body               # swap_paths!' host sync and trade reset
    assert "split_paths(r, [paths], [toks]" in tests and "swap_paths!(twin, paths, toks, x[1])" in tests
    assert "split_paths_out(r, [paths], [toks]" in tests and "swap_paths_out!(twin, paths, toks, x[1]; max_in=c[1])" in tests


def test_the_python_argtypes_are_shared():
    import inspect
    from cfmmrouter_amd import _lib
    assert "L.cfmm_swap_order_out.argtypes = L.cfmm_swap_order.argtypes" in inspect.getsource(_lib)
