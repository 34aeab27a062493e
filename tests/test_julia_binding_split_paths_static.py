"""The Julia binding of order splitting, checked without a Julia toolchain as tests/test_julia_binding_size_path_static.py checks
path sizing: split_paths exists in julia/src/split_paths.jl, the module includes the file and exports the verb, its ccall names
cfmm_split_paths with the argument count and types of include/cfmm_amd_split.h, the CFMM_SPLIT_* codes agree between the
header, the Python binding, the numpy reference and the Julia constants, and the verb's own test file uses it."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccall_matches_the_header():
    decls = declarations(read("include", "cfmm_amd_split.h"))
    assert set(decls) == {"cfmm_split_paths", "cfmm_split_paths_dev"}
    assert "cfmm_split_paths" not in declarations(read("include", "cfmm_amd.h"))   # the addition lives in its own header
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "split_paths.jl"))}
    assert list(calls) == ["cfmm_split_paths"]
    cret, cargs = decls["cfmm_split_paths"]
    ret, args = calls["cfmm_split_paths"]
    assert ret in C2J[cret]
    assert len(args) == len(cargs) == 16, f"{len(args)} Julia arguments vs {len(cargs)} in the header"
    for k, (ja, ca) in enumerate(zip(args, cargs)):
        assert ja in C2J[ca], f"cfmm_split_paths argument {k}: Julia {ja} vs C {ca}"
    assert decls["cfmm_split_paths_dev"][1] == cargs                                # the device form takes the same list


def test_the_verb_is_defined_exported_used_and_carries_the_headers_status_codes():
    module, src = read("julia", "src", "CFMMRouterAMD.jl"), read("julia", "src", "split_paths.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    assert "split_paths" in exported and 'include("split_paths.jl")' in module and ":cfmm_split_paths" not in module
    assert "split_paths" in set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    h = read("include", "cfmm_amd_split.h")
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFMM_SPLIT_(?:OK|NONE|NAN|SATURATED)) (\d+)", h)}
    assert codes == {"CFMM_SPLIT_OK": 0, "CFMM_SPLIT_NONE": 1, "CFMM_SPLIT_NAN": 2, "CFMM_SPLIT_SATURATED": 3}
    limits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFMM_SPLIT_POINTS|CFMM_MAX_SPLIT_PATHS|CFMM_MAX_SPLIT_ROUNDS) (\d+)", h)}
    assert limits == {"CFMM_SPLIT_POINTS": 64, "CFMM_MAX_SPLIT_PATHS": 8, "CFMM_MAX_SPLIT_ROUNDS": 16}
    line = re.search(r"^const SPLIT_OK, SPLIT_NONE, SPLIT_NAN, SPLIT_SATURATED = (.*?)#", src, flags=re.M).group(1)
    assert [int(x) for x in re.findall(r"Int32\((\d)\)", line)] == [0, 1, 2, 3]
    assert int(re.search(r"^const MAX_SPLIT_PATHS = (\d+)", src, flags=re.M).group(1)) == 8
    assert int(re.search(r"^const MAX_SPLIT_ROUNDS = (\d+)", src, flags=re.M).group(1)) == 16
    from cfmmrouter_amd import _lib
    assert (_lib.SPLIT_OK, _lib.SPLIT_NONE, _lib.SPLIT_NAN, _lib.SPLIT_SATURATED, _lib.MAX_SPLIT_PATHS, _lib.MAX_SPLIT_ROUNDS) == (0, 1, 2, 3, 8, 16)
    import cfmmrouter_amd as cr
    assert hasattr(_lib.Context, "split_paths") and hasattr(_lib.Context, "split_paths_dev") and callable(cr.split_paths)
    for name in ("split_paths", "SPLIT_OK", "SPLIT_NONE", "SPLIT_NAN", "SPLIT_SATURATED"):
        assert name in cr.__all__
    import split_paths_ref
    assert (split_paths_ref.SPLIT_OK, split_paths_ref.SPLIT_NONE, split_paths_ref.SPLIT_NAN, split_paths_ref.SPLIT_SATURATED) == (0, 1, 2, 3)
    assert (split_paths_ref.POINTS, split_paths_ref.MAX_PATHS, split_paths_ref.MAX_ROUNDS) == (64, 8, 16)
    body = src[src.index("function split_paths("):]
    body = body[:body.index("\nend\n")]
    assert "path_hop_arrays(r, flat_pools, flat_tokens" in body                     # quote_paths' mapping: 1-based tokens, every refusal
    tests = read("julia", "test", "split_paths.jl")
    assert "split_paths(" in tests and "quote_paths(r, paths, toks, x[1]) == y[1]" in tests and "swap_paths!(r, paths, toks, x[1])" in tests
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "cfmm_split_paths" in read(doc) or "split_paths" in read(doc), doc


def test_the_new_codes_stay_out_of_the_patterns_other_tests_read_the_main_header_with():
    h = read("include", "cfmm_amd_split.h")
    names = re.findall(r"#define (CFMM_\w+)", h)
    assert names and not any(re.match(r"CFMM_(FOUND|SWAP_|PATH_|SIZED|SIZE_)", n) for n in names if n != "CFMM_AMD_SPLIT_H")
