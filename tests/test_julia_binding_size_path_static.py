"""The Julia binding of path sizing, checked without a Julia toolchain as tests/test_julia_binding_find_path_static.py checks the path
search: size_paths exists in julia/src/size_paths.jl, the module includes the file and exports the verb, its ccall names
cfmm_size_path with the argument count and types of include/cfmm_amd_size_path.h, the CFMM_SIZED* codes agree between the header,
the Python binding and the Julia constants, and the package's tests use the verb."""
import re

from test_julia_binding_static import C2J
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccall_matches_the_header():
    decls = declarations(read("include", "cfmm_amd_size_path.h"))
    assert set(decls) == {"cfmm_size_path", "cfmm_size_path_dev"}
    assert "cfmm_size_path" not in declarations(read("include", "cfmm_amd.h"))     # the addition lives in its own header
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "size_paths.jl"))}
    assert list(calls) == ["cfmm_size_path"]
    cret, cargs = decls["cfmm_size_path"]
    ret, args = calls["cfmm_size_path"]
    assert ret in C2J[cret]
    assert len(args) == len(cargs) == 16, f"{len(args)} Julia arguments vs {len(cargs)} in the header"
    for k, (ja, ca) in enumerate(zip(args, cargs)):
        assert ja in C2J[ca], f"cfmm_size_path argument {k}: Julia {ja} vs C {ca}"
    assert decls["cfmm_size_path_dev"][1] == cargs                                  # the device form takes the same list


def test_the_verb_is_defined_exported_used_and_carries_the_headers_status_codes():
    module, src = read("julia", "src", "CFMMRouterAMD.jl"), read("julia", "src", "size_paths.jl")
    exported = set(re.search(r"^export (.*)$", module, flags=re.M).group(1).replace(" ", "").split(","))
    assert "size_paths" in exported and 'include("size_paths.jl")' in module
    assert "size_paths" in set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    h = read("include", "cfmm_amd_size_path.h")
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFMM_SIZED\w*) (\d+)", h)}
    assert codes == {"CFMM_SIZED": 0, "CFMM_SIZED_NONE": 1, "CFMM_SIZED_AT_LIMIT": 2, "CFMM_SIZED_NAN": 3}
    limits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFMM_SIZE_POINTS|CFMM_MAX_SIZE_ROUNDS) (\d+)", h)}
    assert limits == {"CFMM_SIZE_POINTS": 64, "CFMM_MAX_SIZE_ROUNDS": 16}
    line = re.search(r"^const SIZED, SIZED_NONE, SIZED_AT_LIMIT, SIZED_NAN = (.*?)#", src, flags=re.M).group(1)
    assert [int(x) for x in re.findall(r"Int32\((\d)\)", line)] == [0, 1, 2, 3]
    assert int(re.search(r"^const MAX_SIZE_ROUNDS = (\d+)", src, flags=re.M).group(1)) == 16
    from cfmmrouter_amd import _lib
    assert (_lib.SIZED, _lib.SIZED_NONE, _lib.SIZED_AT_LIMIT, _lib.SIZED_NAN, _lib.MAX_SIZE_ROUNDS) == (0, 1, 2, 3, 16)
    import size_path_ref
    assert (size_path_ref.SIZED, size_path_ref.SIZED_NONE, size_path_ref.SIZED_AT_LIMIT, size_path_ref.SIZED_NAN) == (0, 1, 2, 3)
    assert (size_path_ref.POINTS, size_path_ref.MAX_ROUNDS) == (64, 16)
    body = src[src.index("function size_paths("):]
    body = body[:body.index("\nend\n")]
    assert "path_hop_arrays(r, pools, tokens, max_in)" in body                      # quote_paths' mapping: 1-based tokens, every refusal
    tests = read("julia", "test", "runtests.jl")
    assert "size_paths(" in tests and "quote_paths(r, [cycle, cycle], [toks, toks], x) == y" in tests and "swap_paths!(r, [cycle]" in tests


def test_the_new_codes_stay_out_of_the_patterns_other_tests_read_the_main_header_with():
    h = read("include", "cfmm_amd_size_path.h")
    names = re.findall(r"#define (CFMM_\w+)", h)
    assert names and not any(re.match(r"CFMM_(FOUND|SWAP_|PATH_)", n) for n in names if n != "CFMM_AMD_SIZE_PATH_H")
