"""The Julia binding of the exact-output execution entries, checked without a Julia toolchain as
tests/test_julia_binding_static.py checks the others: swap_out! and swap_paths_out! exist, are exported, and their ccalls name
cfmm_swap_out / cfmm_swap_path_out with the argument count and types of include/cfmm_amd.h and include/cfmm_amd_path_out.h
(the path entry's header; its Julia verb is julia/src/swap_paths_out.jl, included by the module)."""
import os
import re

from test_julia_binding_static import C2J, ROOT, split_top


def read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def declarations(text):
    """{name: (return type, [parameter types])} of the cfmm_* functions a header text declares, const and names stripped"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(int|void)\s+(cfmm_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        types = []
        for p in [q.strip() for q in m.group(3).replace("\n", " ").split(",") if q.strip() and q.strip() != "void"]:
            p = re.sub(r"\bconst\b", "", p).strip()
            p = re.sub(r"^(.*?)(\w+)\s*\[[^\]]*\]$", r"\1* \2", p)      # `unsigned char id[N]` is `unsigned char* id`
            types.append(re.match(r"^(.*?)(\w+)?$", p).group(1).replace(" ", ""))
        decls[m.group(2)] = (m.group(1), types)
    return decls


def ccalls(text):
    """[(C name, return type, [argument types])] of the ccalls of a Julia source text"""
    text = re.sub(r"#[^\n]*", "", text)
    calls = []
    for m in re.finditer(r"ccall\(\(:(\w+),\s*LIB\),\s*(\w+),\s*\(", text):
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        calls.append((m.group(1), m.group(2), split_top(text[m.end():j - 1])))
    return calls


def c_declarations():
    a, b = declarations(read("include", "cfmm_amd.h")), declarations(read("include", "cfmm_amd_path_out.h"))
    assert "cfmm_swap_path_out" in b and "cfmm_swap_path_out" not in a and "cfmm_swap_out" in a and "cfmm_swap_path" in a
    return {**a, **b}


def julia_ccalls():
    a, b = ccalls(read("julia", "src", "CFMMRouterAMD.jl")), ccalls(read("julia", "src", "swap_paths_out.jl"))
    assert [c[0] for c in b] == ["cfmm_swap_path_out"]
    return a + b


def test_the_new_ccalls_match_the_header():
    decls = c_declarations()
    calls = {name: (ret, args) for name, ret, args in julia_ccalls()}
    for name, nargs in (("cfmm_swap_out", 10), ("cfmm_swap_path_out", 13)):
        assert name in decls, f"{name} is not declared in include/cfmm_amd.h"
        assert name in calls, f"{name} is not called from julia/src/CFMMRouterAMD.jl"
        cret, cargs = decls[name]
        ret, args = calls[name]
        assert ret in C2J[cret]
        assert len(args) == len(cargs) == nargs, f"{name}: {len(args)} Julia arguments vs {len(cargs)} in the header"
        for k, (ja, ca) in enumerate(zip(args, cargs)):
            assert ja in C2J[ca], f"{name} argument {k}: Julia {ja} vs C {ca}"
    # the path entry takes cfmm_swap_path's list, position by position
    assert decls["cfmm_swap_path_out"] == decls["cfmm_swap_path"]


def test_the_verbs_are_defined_exported_and_carry_the_headers_status_codes():
    src = open(os.path.join(ROOT, "julia", "src", "CFMMRouterAMD.jl")).read()
    assert 'include("swap_paths_out.jl")' in src
    src += open(os.path.join(ROOT, "julia", "src", "swap_paths_out.jl")).read()
    exported = set(re.search(r"^export (.*)$", src, flags=re.M).group(1).replace(" ", "").split(","))
    defined = set(re.findall(r"^function (\w+!?)\(", src, flags=re.M))
    for verb in ("swap_out!", "swap_paths_out!"):
        assert verb in defined and verb in exported, verb
    h = open(os.path.join(ROOT, "include", "cfmm_amd.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CFMM_SWAP_(\w+) (\d+)", h)}
    assert codes == {"APPLIED": 0, "OVER_LIMIT": 1, "REFUSED": 2, "UNOBTAINABLE": 3}
    line = re.search(r"^const SWAP_APPLIED, SWAP_OVER_LIMIT, SWAP_REFUSED, SWAP_UNOBTAINABLE = (.*?)#", src, flags=re.M).group(1)
    assert [int(x) for x in re.findall(r"Int32\((\d)\)", line)] == [0, 1, 2, 3]
    from cfmmrouter_amd import _lib
    assert (_lib.SWAP_APPLIED, _lib.SWAP_OVER_LIMIT, _lib.SWAP_REFUSED, _lib.SWAP_UNOBTAINABLE) == (0, 1, 2, 3)
    assert codes["APPLIED"] == _lib.PATH_APPLIED and codes["OVER_LIMIT"] == _lib.PATH_BELOW_LIMIT and codes["REFUSED"] == _lib.PATH_REFUSED
