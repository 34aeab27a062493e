"""Records what the Python host mirror does -- its Context calls and the arrays it hands the caller -- at ONE commit, for
tests/test_host_mirror_cpu.py to hold later trees against.

    git stash / git worktree at the commit to record, with THIS file and tests/host_mirror_record.py copied in, then
    python tests/golden/make_host_mirror_golden.py <commit>       # -> tests/golden/host_mirror_parent.json

The scenarios and the recording context are tests/host_mirror_record.py's; they use the public API plus one patched name,
so the same two files run unchanged on the recorded commit and on every later tree.  No GPU, no shared library."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import host_mirror_record as rec  # noqa: E402

if __name__ == "__main__":
    commit = sys.argv[1]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), "give the full hash of the commit the package was checked out at"
    note = "recorded by tests/golden/make_host_mirror_golden.py with the package (cfmmrouter.jl_amd/*.py) of that commit"
    dumps = lambda x: json.dumps(x, ensure_ascii=False, separators=(",", ":"))
    scenarios = ",\n".join(f"{dumps(name)}:[\n" + ",\n".join(dumps(s) for s in steps) + "\n]"         # one step per line
                           for name, steps in rec.record_all().items())
    path = os.path.join(HERE, "host_mirror_parent.json")
    with open(path, "w") as f:
        f.write(f'{{"commit":{dumps(commit)},\n"note":{dumps(note)},\n"scenarios":{{\n{scenarios}\n}}}}\n')
    print(path, os.path.getsize(path), "bytes")
