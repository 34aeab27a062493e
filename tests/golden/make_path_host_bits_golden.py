"""Records every answer of the order-level path entries (split_paths, split_paths_out and their _dev forms, swap_order,
swap_order_out, and the read-only path entries on a two-shard parent) on the market of tests/path_host_bits_record.py -- ONCE, on
the MI355X, with the library of the commit whose bits are to be kept -- for tests/test_gpu_path_host_bits.py to hold later builds
against, bit for bit.

    build the commit to record (make -C cfmmrouter.jl_amd/csrc), then on the GPU
    CFMM_AMD_LIB=<that build's libcfmm_amd.so> python tests/golden/make_path_host_bits_golden.py <commit>   # -> tests/golden/path_host_bits.npz

The scenario uses the public Python API only, so this file and tests/path_host_bits_record.py run unchanged on the recorded
commit and on every later tree.  The fixture is data this project's own build wrote."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import cfmmrouter_amd as cr  # noqa: E402
import path_host_bits_record as rec  # noqa: E402
from cfmmrouter_amd import synth  # noqa: E402

if __name__ == "__main__":
    commit = sys.argv[1]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), "give the full hash of the commit the library was built at"
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "path_host_bits.npz")
    res = rec.record_all(cr, synth)
    again = rec.record_all(cr, synth)                                   # the record is a function of the build alone
    assert res.keys() == again.keys() and all(np.array_equal(rec.as_words(res[k]), rec.as_words(again[k])) for k in res)
    np.savez_compressed(out, commit=np.array(commit), **res)
    print(out, os.path.getsize(out), "bytes,", len(res), "arrays")
    for k in sorted(res):
        if k.endswith("status") or k.endswith("launches"):
            print(k, np.bincount(res[k], minlength=5).tolist() if k.endswith("status") else res[k].tolist())
    assert os.path.getsize(out) < 1 << 20
