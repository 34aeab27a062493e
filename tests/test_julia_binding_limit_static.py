"""The Julia binding of the price-limit entries, checked without a Julia toolchain as tests/test_julia_binding_rate_static.py
checks the marginal rates: amount_to_rate and swap_limit! exist in julia/src/quote_to_rate.jl, the module includes the file and
exports the verbs, and their ccalls name cfmm_quote_to_rate / cfmm_swap_limit with the argument counts and types of
include/cfmm_amd_limit.h."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccalls_match_the_header():
    decls = declarations(read("include", "cfmm_amd_limit.h"))
    assert set(decls) == {"cfmm_quote_to_rate", "cfmm_quote_to_rate_dev", "cfmm_swap_limit"}
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "quote_to_rate.jl"))}
    assert list(calls) == ["cfmm_quote_to_rate", "cfmm_swap_limit"]
    for name, nargs in (("cfmm_quote_to_rate", 9), ("cfmm_swap_limit", 11)):
        cret, cargs = decls[name]
        ret, args = calls[name]
        assert ret in C2J[cret]
        assert len(args) == len(cargs) == nargs, f"{name}: {len(args)} Julia arguments vs {len(cargs)} in the header"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert ja in C2J[ca], f"{name} argument {k}: Julia {ja} vs C {ca}"
    assert decls["cfmm_quote_to_rate_dev"][1] == decls["cfmm_quote_to_rate"][1]      # the device form takes the same list


def test_the_verbs_are_defined_exported_and_tested():
    module, src = read("julia", "src", "CFMMRouterAMD.jl"), read("julia", "src", "quote_to_rate.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    defined = set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    for verb in ("amount_to_rate", "swap_limit!"):
        assert verb in exported and verb in defined, verb
    assert 'include("quote_to_rate.jl")' in module
    assert module.index('include("quote_rate.jl")') < module.index('include("quote_to_rate.jl")')
    assert "segment_rows(r)" in src                                             # quote_swaps' mapping of pools to (segment, row)
    for k, name in enumerate(("FILLED", "PARTIAL", "NONE", "REFUSED")):
        assert f"const LIMIT_{name} = Int32({k})" in src
    tests = read("julia", "test", "quote_to_rate.jl")
    for needle in ("amount_to_rate(r,", "swap_limit!(r,", "== quote_swaps(r,", "LIMIT_PARTIAL", "LIMIT_NONE", "LIMIT_FILLED"):
        assert needle in tests, needle


def test_the_python_binding_declares_the_same_entries():
    from cfmmrouter_amd import _lib
    text = read("cfmmrouter.jl_amd", "_lib.py")
    for name in ("cfmm_quote_to_rate", "cfmm_quote_to_rate_dev", "cfmm_swap_limit"):
        assert f"L.{name}.argtypes" in text, name
    for verb in ("quote_to_rate", "quote_to_rate_dev", "swap_limit"):
        assert callable(getattr(_lib.Context, verb)), verb
