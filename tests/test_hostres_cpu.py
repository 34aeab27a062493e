"""csrc/hostres.h (PinnedBuf, Event, Stream, TradeStaging: the owners of pinned memory, events and streams) and csrc/granule.h
(the output granule's codec), driven by tests/native/hostres_host.cpp: a stand-alone program over malloc / free with live
counts and an injectable k-th failure, built with the address and undefined-behaviour sanitizers and run as a program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_and_granule_codec_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "hostres_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "hostres_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr[-2000:])
    assert r.returncode == 0 and "HOSTRES_OK" in r.stdout and r.stderr == ""
