"""Register / LDS / scratch footprint of every kernel in libcfmm_amd.so (hipcc -Rpass-analysis=kernel-resource-usage on
csrc/sweep_kernels.hip, cross-compiled for gfx950: no GPU needed) and the instruction mix of the ProductTwoCoin tile
loops (fast arithmetic vs the compiler's division / square-root sequences).
usage: python scripts/kernel_resources.py > profiles/rNN_kernel_resources.txt
       python scripts/kernel_resources.py --digest
--digest: from the same compile, one SHA-256 per kernel over its assembly (label to .Lfunc_end; comment text and every
line that mentions __hip_cuid_ dropped), sorted by symbol, then one over the rest of the file.  Two builds whose
digests agree run the same device code: how a change that only moves or renames device source proves it changed nothing."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cfmmrouter.jl_amd", "csrc", "sweep_kernels.hip")
tmp = tempfile.mkdtemp()
# the kernels' own flags (kernarg preload): what the Makefile's KFLAGS default says, so that the figures are the shipped build's
with open(os.path.join(os.path.dirname(SRC), "Makefile"), encoding="utf-8") as f:
    KFLAGS = re.search(r"^KFLAGS\s*\?=(.*)$", f.read(), re.M).group(1).split()
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"] + KFLAGS + [
       "-save-temps", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", os.path.join(tmp, "k.o")]
r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
asm = open(os.path.join(tmp, "sweep_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")).read()


def digest_report():
    lines = asm.split("\n")
    kernels = {b.split("\n")[0].split()[0] for b in blocks}
    sha = {None: hashlib.sha256()}   # per kernel; None: everything outside the kernels
    cur = None
    for l in lines:
        text = l.split(";")[0].rstrip()
        if cur is None and text.endswith(":") and text[:-1] in kernels:
            cur = text[:-1]
            sha[cur] = hashlib.sha256()
        if text and "__hip_cuid_" not in l:
            sha[cur].update(text.encode() + b"\n")
        if cur is not None and re.match(r"\.Lfunc_end\d+:", l):
            cur = None

    print("# hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off %s -save-temps -c csrc/sweep_kernels.hip" % " ".join(KFLAGS))
    print(f"# {len(kernels)} kernels in the code object")
    for sym in sorted(kernels):
        if sym not in sha:
            sys.exit(f"kernel_resources: no assembly found for kernel {sym}")
        print(f"{sha[sym].hexdigest()}  {sym}")
    print(f"{sha[None].hexdigest()}  (everything outside the kernels)")


if "--digest" in sys.argv[1:]:
    digest_report()
    sys.exit(0)

print("# hipcc --offload-arch=gfx950 -O3 -ffp-contract=off %s -Rpass-analysis=kernel-resource-usage csrc/sweep_kernels.hip" % " ".join(KFLAGS))
print(f"# {len(blocks)} kernels in the code object")
print(f"{'VGPR':>5} {'SGPR':>5} {'scratch':>8} {'LDS(static)':>12} {'waves/SIMD':>11}  kernel")
rows = []
mangled = {}
for b in blocks:
    name = b.split("\n")[0].split()[0]
    g = lambda k: int(re.search(k + r": (\d+)", b).group(1))
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("cfmm::", "").replace("void ", "")
    dem = re.sub(r"\(.*\)$", "", dem)
    mangled[dem] = name
    rows.append((dem, g("VGPRs"), g("SGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"LDS Size \[bytes/block\]"), g(r"Occupancy \[waves/SIMD\]")))
for dem, v, s_, sc, lds, occ in sorted(rows):
    print(f"{v:5d} {s_:5d} {sc:8d} {lds:12d} {occ:11d}  {dem}")

# instruction classes of the fused (not materialising) 1024-thread kernels that carry BOTH tile loops (kArithAuto = 2) --
# the one on the fast arithmetic and the one on the compiler's division / square-root sequences --, whole kernel: staging,
# the tile loops and the epilogue.  Looked up by demangled name (UniV3Ops is UniV3OpsT<true>).
print("\n# static instruction counts (whole kernel code)")
for label in ("sweep_kernel<ProductOps, false, 1024, false, 2>", "sweep_kernel<GeoMeanLogOps, false, 1024, false, 2>",
              "sweep_kernel<UniV3OpsT<true>, false, 1024, false, 2>"):
    m = label in mangled and re.search(r"^" + re.escape(mangled[label]) + r":.*?s_endpgm", asm, flags=re.S | re.M)
    if not m:
        sys.exit(f"kernel_resources: kernel {label} not found in the code object")
    ins = [l.split()[0] for l in m.group(0).split("\n") if l.startswith("\t") and not l.strip().startswith(";") and not l.strip().startswith(".")]
    cnt = lambda pat: sum(1 for i in ins if re.match(pat, i))
    print(f"  {label}: {len(ins)} instructions; f64 VALU {cnt(r'v_.*_f64')}, of them v_div_scale/fmas/fixup {cnt(r'v_div_')} and "
          f"v_rcp/v_rsq/v_sqrt {cnt(r'v_(rcp|rsq|sqrt)_f64')}; v_cndmask {cnt(r'v_cndmask')}, ds_* {cnt(r'ds_')}, global_* {cnt(r'global_')}, s_* {cnt(r's_')}")
