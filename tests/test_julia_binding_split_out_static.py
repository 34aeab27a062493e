"""The Julia bindings of exact-output splitting and of the exact-output disjoint search, checked WITHOUT a Julia toolchain (there
is none in the images this suite runs in) as tests/test_julia_binding_split_paths_static.py checks the forward ones:
split_paths_out and find_disjoint_paths_out exist in their own files, the module includes the files and exports the verbs, each
ccall names its entry with the argument count and types of its header, CFMM_SPLIT_UNOBTAINABLE agrees between the header, the
Python binding, the numpy reference and the Julia constant, and each verb's own test file uses it."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccalls_match_the_headers():
    for header, entry, others, src, n_args in (("cfmm_amd_split_out.h", "cfmm_split_paths_out", {"cfmm_split_paths_out_dev"}, "split_paths_out.jl", 16),
                                               ("cfmm_amd_find_disjoint_out.h", "cfmm_find_disjoint_paths_out", set(), "find_disjoint_paths_out.jl", 15)):
        decls = declarations(read("include", header))
        assert set(decls) == {entry} | others
        assert entry not in declarations(read("include", "cfmm_amd.h"))     # the addition lives in its own header
        calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", src))}
        assert list(calls) == [entry]
        cret, cargs = decls[entry]
        ret, args = calls[entry]
        assert ret in C2J[cret]
        assert len(args) == len(cargs) == n_args, f"{entry}: {len(args)} Julia arguments vs {len(cargs)} in the header"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert ja in C2J[ca], f"{entry} argument {k}: Julia {ja} vs C {ca}"
        for other in others:
            assert decls[other][1] == cargs                                # the device form takes the same list
    # the twins take their forward entries' lists
    assert declarations(read("include", "cfmm_amd_split_out.h"))["cfmm_split_paths_out"][1] == \
        declarations(read("include", "cfmm_amd_split.h"))["cfmm_split_paths"][1]
    assert declarations(read("include", "cfmm_amd_find_disjoint_out.h"))["cfmm_find_disjoint_paths_out"][1] == \
        declarations(read("include", "cfmm_amd_find_disjoint.h"))["cfmm_find_disjoint_paths"][1]


def test_the_verbs_are_defined_exported_used_and_carry_the_headers_status_code():
    module = read("julia", "src", "CFMMRouterAMD.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    for verb, src_name, entry in (("split_paths_out", "split_paths_out.jl", "cfmm_split_paths_out"),
                                  ("find_disjoint_paths_out", "find_disjoint_paths_out.jl", "cfmm_find_disjoint_paths_out")):
        src = read("julia", "src", src_name)
        assert verb in exported and f'include("{src_name}")' in module and f":{entry}" not in module
        assert verb in set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
        assert f"{verb}(" in read("julia", "test", src_name)
    assert module.index('include("split_paths.jl")') < module.index('include("split_paths_out.jl")')   # it uses split_paths.jl's constants
    h = read("include", "cfmm_amd_split_out.h")
    assert re.search(r"#define CFMM_SPLIT_UNOBTAINABLE (\d+)", h).group(1) == "4"
    assert '#include "cfmm_amd_split.h"' in h and "CFMM_SPLIT_POINTS" not in re.findall(r"#define (\w+)", h)   # the limits are the forward header's
    src = read("julia", "src", "split_paths_out.jl")
    assert re.search(r"^const SPLIT_UNOBTAINABLE = Int32\((\d)\)", src, flags=re.M).group(1) == "4"
    from cfmmrouter_amd import _lib
    assert _lib.SPLIT_UNOBTAINABLE == 4 and _lib.SPLIT_UNOBTAINABLE not in (_lib.SPLIT_OK, _lib.SPLIT_NONE, _lib.SPLIT_NAN, _lib.SPLIT_SATURATED)
    import cfmmrouter_amd as cr
    for name in ("split_paths_out", "split_paths_out_dev", "find_disjoint_paths_out"):
        assert hasattr(_lib.Context, name)
    for name in ("split_paths_out", "find_disjoint_paths_out", "route_order_out", "SPLIT_UNOBTAINABLE"):
        assert name in cr.__all__ and hasattr(cr, name)
    import split_paths_out_ref
    assert split_paths_out_ref.SPLIT_UNOBTAINABLE == 4
    body = src[src.index("function split_paths_out("):]
    assert "path_hop_arrays(r, flat_pools, flat_tokens" in body             # quote_paths' mapping: 1-based tokens, every refusal
    tests = read("julia", "test", "split_paths_out.jl")
    assert "quote_paths_out(r, paths, toks, x[1]) == c[1]" in tests and "swap_paths_out!(r, paths, toks, x[1]; max_in=c[1])" in tests
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "split_paths_out" in read(doc) and "find_disjoint_paths_out" in read(doc), doc
    # what the two forward headers said was out of scope no longer is
    assert "exact-output splitting" not in read("include", "cfmm_amd_split.h")
    assert "the exact-output direction" not in read("include", "cfmm_amd_find_disjoint.h")


def test_the_python_argtypes_are_the_forward_entries():
    import ctypes as C
    import inspect
    from cfmmrouter_amd import _lib
    text = inspect.getsource(_lib)
    assert "L.cfmm_split_paths_out.argtypes = L.cfmm_split_paths.argtypes" in text
    assert "L.cfmm_split_paths_out_dev.argtypes = L.cfmm_split_paths_dev.argtypes" in text
    assert "L.cfmm_find_disjoint_paths_out.argtypes = L.cfmm_find_disjoint_paths.argtypes" in text
    assert C.sizeof(C.c_double) == 8
