#!/usr/bin/env python
"""What stands between a sweep kernel's entry and its first pool-state load, read off the ISA (no GPU needed).

    make -C cfmmrouter.jl_amd/csrc asm          # or: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --cuda-device-only -S
    python scripts/sweep_entry_waits.py cfmmrouter.jl_amd/csrc/sweep_kernels-hip-amdgcn-amd-amdhsa-gfx950.s

Per sweep_kernel / sweep_multi instantiation, over the instructions from the kernel's label to its first pool load (the first
global_load_dword* in program text; the fused kernel's text begins with one family's branch), it counts
  waits     s_waitcnt on scalar or vector memory (every one is a dependent round trip through argument memory),
  arg_vmem  vector loads of single bytes (the pattern[] / rank[] lookups of the kernarg segment),
  spills    v_writelane (SGPRs parked in VGPR lanes),
  divs      reciprocal seeds of the integer-division expansions (v_rcp_iflag_f32, v_rcp_f32),
  instr     all instructions.
"""
import re
import sys


def kernels(path):
    name, body = None, []
    for line in open(path, encoding="utf-8", errors="replace"):
        m = re.match(r"^(_ZN4cfmm\w+):", line)
        if m:
            if name:
                yield name, body
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                yield name, body
                name, body = None, []
            else:
                body.append(line.strip())
    if name:
        yield name, body


def entry(body):
    c = dict(waits=0, arg_vmem=0, spills=0, divs=0, instr=0)
    for ins in body:
        if not ins or ins.startswith((";", ".")) or ins.endswith(":"):
            continue
        op = ins.split()[0]
        if re.match(r"global_load_dword", op):
            return c
        c["instr"] += 1
        if op == "s_waitcnt" and ("lgkmcnt" in ins or "vmcnt" in ins):
            c["waits"] += 1
        elif op == "global_load_ubyte":
            c["arg_vmem"] += 1
        elif op.startswith("v_writelane"):
            c["spills"] += 1
        elif op in ("v_rcp_iflag_f32_e32", "v_rcp_f32_e32"):
            c["divs"] += 1
    return None


def demangled(name):
    m = re.match(r"_ZN4cfmm(\d+)(sweep_kernel|sweep_multi)I(.*)EEv", name)
    return (m.group(2) + "<" + m.group(3) + ">") if m else name


def main():
    rows = []
    for name, body in kernels(sys.argv[1]):
        if "sweep_kernel" not in name and "sweep_multi" not in name:
            continue
        c = entry(body)
        if c:
            rows.append((demangled(name), c))
    print("%-64s %5s %8s %6s %4s %5s" % ("kernel (mangled template arguments)", "waits", "arg_vmem", "spills", "divs", "instr"))
    for n, c in sorted(rows):
        print("%-64s %5d %8d %6d %4d %5d" % (n[:64], c["waits"], c["arg_vmem"], c["spills"], c["divs"], c["instr"]))
    for k in ("waits", "spills", "divs", "instr"):
        v = [c[k] for _, c in rows]
        print("%s: min %d max %d over %d kernels" % (k, min(v), max(v), len(v)))


if __name__ == "__main__":
    main()
