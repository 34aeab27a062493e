"""The Julia binding of the path search, checked without a Julia toolchain as tests/test_julia_binding_swap_out_static.py checks
the exact-output entries: find_paths exists, is exported, its ccall names cfmm_find_path with the argument count and types of
include/cfmm_amd.h, it carries the header's status codes, and the package's tests use it."""
import os
import re

from test_julia_binding_static import C2J, ROOT
from test_julia_binding_swap_out_static import ccalls, declarations, read


def test_the_ccall_matches_the_header():
    decls = declarations(read("include", "cfmm_amd.h"))
    calls = {name: (ret, args) for name, ret, args in ccalls(read("julia", "src", "CFMMRouterAMD.jl"))}
    assert "cfmm_find_path" in decls, "cfmm_find_path is not declared in include/cfmm_amd.h"
    assert "cfmm_find_path" in calls, "cfmm_find_path is not called from julia/src/CFMMRouterAMD.jl"
    cret, cargs = decls["cfmm_find_path"]
    ret, args = calls["cfmm_find_path"]
    assert ret in C2J[cret]
    assert len(args) == len(cargs) == 13, f"{len(args)} Julia arguments vs {len(cargs)} in the header"
    for k, (ja, ca) in enumerate(zip(args, cargs)):
        assert ja in C2J[ca], f"cfmm_find_path argument {k}: Julia {ja} vs C {ca}"


def test_the_verb_is_defined_exported_used_and_carries_the_headers_status_codes():
    src = read("julia", "src", "CFMMRouterAMD.jl")
    exported = set(re.search(r"^export (.*)$", src, flags=re.M).group(1).replace(" ", "").split(","))
    defined = set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    assert "find_paths" in defined and "find_paths" in exported
    h = read("include", "cfmm_amd.h")
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFMM_FOUND\w*) (\d+)", h)}
    assert codes == {"CFMM_FOUND": 0, "CFMM_FOUND_NONE": 1, "CFMM_FOUND_REPEATS": 2}
    line = re.search(r"^const FOUND, FOUND_NONE, FOUND_REPEATS = (.*?)#", src, flags=re.M).group(1)
    assert [int(x) for x in re.findall(r"Int32\((\d)\)", line)] == [0, 1, 2]
    from cfmmrouter_amd import _lib
    assert (_lib.FOUND, _lib.FOUND_NONE, _lib.FOUND_REPEATS) == (0, 1, 2)
    body = src[src.index("function find_paths("):]
    body = body[:body.index("\nend\n")]
    assert "token_in[q] - 1" in body and "token_out[q] - 1" in body        # 1-based token ids become the library's 0-based ones
    assert "segment_rows(r)" in body and "co[q, k] + 1" in body            # ... and the hops come back as pools and 1-based tokens
    tests = read("julia", "test", "runtests.jl")
    assert "find_paths(" in tests and "quote_paths(r, paths[found]" in tests and "swap_paths!(" in tests
    assert os.path.exists(os.path.join(ROOT, "julia", "test", "runtests.jl"))
