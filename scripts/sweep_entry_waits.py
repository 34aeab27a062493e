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
A translation unit built with kernarg preload (csrc/Makefile KFLAGS) gives every kernel a 256-byte compatibility prologue --
the loads of the preloaded arguments and one wait, for a firmware that does not preload, closed by `s_branch` and
`.p2align 8`; a firmware that preloads enters behind it.  Counting starts behind that prologue (column `pro`: 1 = the kernel
has one), so the table says what a preloading firmware runs.  Vector loads in front of the first wait are the price requests
of the kernel's first instructions (sweep_core.h request_prices; column `prices`), not pool loads: counting goes on behind them.
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


def behind_prologue(body):
    """the body behind the kernarg-preload prologue, if it has one: [loads, s_waitcnt, s_branch, .p2align 8] at the very top"""
    code = [k for k, ins in enumerate(body) if ins and not ins.startswith(";") and not ins.endswith(":")]
    for pos, k in enumerate(code[:24]):
        if body[k].split()[0] == "s_branch" and pos + 1 < len(code) and body[code[pos + 1]].startswith(".p2align\t8"):
            if all(body[j].split()[0].startswith(("s_load_dword", "s_waitcnt", "s_nop")) for j in code[:pos]):
                return body[code[pos + 1] + 1:], 1
    return body, 0


def entry(body):
    body, pro = behind_prologue(body)
    c = dict(waits=0, arg_vmem=0, spills=0, divs=0, instr=0, pro=pro, prices=0)
    for ins in body:
        if not ins or ins.startswith((";", ".")) or ins.endswith(":"):
            continue
        op = ins.split()[0]
        if re.match(r"global_load_dword", op):
            if c["waits"] == 0 and pro:
                c["prices"] += 1       # requested before anything was waited for: a lane's first prices, not pool state
                c["instr"] += 1
                continue
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
    m = re.match(r"_ZN4cfmm(\d+)(sweep_kernel|sweep_multi)I(.*?)EEv", name)
    return (m.group(2) + "<" + m.group(3) + ">") if m else name


def main():
    rows = []
    for name, body in kernels(sys.argv[1]):
        if "sweep_kernel" not in name and "sweep_multi" not in name:
            continue
        c = entry(body)
        if c:
            rows.append((demangled(name), c))
    print("%-64s %5s %8s %6s %4s %5s %3s %6s" % ("kernel (mangled template arguments)", "waits", "arg_vmem", "spills", "divs", "instr", "pro", "prices"))
    for n, c in sorted(rows):
        print("%-64s %5d %8d %6d %4d %5d %3d %6d" % (n[:64], c["waits"], c["arg_vmem"], c["spills"], c["divs"], c["instr"], c["pro"], c["prices"]))
    for k in ("waits", "spills", "divs", "instr", "pro", "prices"):
        v = [c[k] for _, c in rows]
        print("%s: min %d max %d over %d kernels" % (k, min(v), max(v), len(v)))


if __name__ == "__main__":
    main()
