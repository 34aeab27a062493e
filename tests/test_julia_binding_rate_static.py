"""The Julia binding of the marginal-rate entries, checked without a Julia toolchain as
tests/test_julia_binding_size_path_static.py checks path sizing: quote_rate, spot_price and quote_path_rate exist in
julia/src/quote_rate.jl, the module includes the file and exports the verbs, and their ccalls name cfmm_quote_rate /
cfmm_quote_path_rate with the argument counts and types of include/cfmm_amd_rate.h."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccalls_match_the_header():
    decls = declarations(read("include", "cfmm_amd_rate.h"))
    assert set(decls) == {"cfmm_quote_rate", "cfmm_quote_rate_dev", "cfmm_quote_path_rate", "cfmm_quote_path_rate_dev"}
    main = declarations(read("include", "cfmm_amd.h"))
    assert not set(decls) & set(main)                                           # the addition lives in its own header
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "quote_rate.jl"))}
    assert list(calls) == ["cfmm_quote_rate", "cfmm_quote_path_rate"]
    for name, nargs in (("cfmm_quote_rate", 9), ("cfmm_quote_path_rate", 13)):
        cret, cargs = decls[name]
        ret, args = calls[name]
        assert ret in C2J[cret]
        assert len(args) == len(cargs) == nargs, f"{name}: {len(args)} Julia arguments vs {len(cargs)} in the header"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert ja in C2J[ca], f"{name} argument {k}: Julia {ja} vs C {ca}"
        assert decls[name + "_dev"][1] == cargs                                 # the device form takes the same list
    # cfmm_quote's list with one more output; cfmm_quote_path's with the rate before the hop amounts and the hop rates behind
    assert decls["cfmm_quote_rate"][1] == main["cfmm_quote"][1] + ["double*"]
    assert decls["cfmm_quote_path_rate"][1] == main["cfmm_quote_path"][1] + ["double*", "double*"]


def test_the_verbs_are_defined_exported_and_tested():
    module, src = read("julia", "src", "CFMMRouterAMD.jl"), read("julia", "src", "quote_rate.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    defined = set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    for verb in ("quote_rate", "spot_price", "quote_path_rate"):
        assert verb in exported and verb in defined, verb
    assert 'include("quote_rate.jl")' in module
    assert "path_hop_arrays(r, pools, tokens, amount_in)" in src                # quote_paths' mapping: 1-based tokens, every refusal
    assert "segment_rows(r)" in src                                             # quote_swaps' mapping of pools to (segment, row)
    tests = read("julia", "test", "quote_rate.jl")
    for needle in ("quote_rate(r,", "spot_price(r,", "quote_path_rate(r,", "== quote_swaps(r,", "== quote_paths(r,"):
        assert needle in tests, needle


def test_the_python_binding_declares_the_same_entries():
    from cfmmrouter_amd import _lib
    text = read("cfmmrouter.jl_amd", "_lib.py")
    for name in ("cfmm_quote_rate", "cfmm_quote_rate_dev", "cfmm_quote_path_rate", "cfmm_quote_path_rate_dev"):
        assert f"L.{name}.argtypes" in text, name
    for verb in ("quote_rate", "quote_rate_dev", "quote_path_rate", "quote_path_rate_dev"):
        assert callable(getattr(_lib.Context, verb)), verb
