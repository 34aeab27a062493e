"""What the query entries (cfmm_quote, cfmm_swap, cfmm_quote_path, cfmm_swap_path, cfmm_find_path) share on the host --
csrc/stage_layout.h (the staging layouts), shard_split.h (a parent's queries by shard), seg_view.h (a segment as the kernels and
the checks see it) and hostres.h EventPairs -- driven by tests/native/query_host.cpp: a stand-alone program over malloc / free,
built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_shard_split_and_segment_views_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "query_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "query_host.cpp"), "-o", exe, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "QUERY_HOST_OK" in r.stdout and r.stderr == ""
