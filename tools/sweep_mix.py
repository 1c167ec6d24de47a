#!/usr/bin/env python3
"""Instruction mix of kernel 5's in-tile sweep loops, from the compiler's assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off \
          -mllvm -amdgpu-atomic-optimizer-strategy=None -Iinclude \
          -Iplanning-path_planning_amd/csrc --cuda-device-only -S \
          planning-path_planning_amd/csrc/fim_kernels.hip -o fim_kernels.s
    python tools/sweep_mix.py fim_kernels.s

(the flags of the Makefile's fim_kernels.o rule).  For the default pass kernel
k_fim_pass_dyn<16, true, false> and the exact_sqrt one <16, false, false> it
prints each sweep loop -- an innermost loop that reads the pass clock
(rb_sweeps4's deadline test) and writes LDS -- with its counts of LDS reads and
writes by form, flat loads, VALU instructions and waits.  One loop body is one
sweep pair: four half-sweeps, eight cell updates per lane.  The loops of a
kernel come in the order of the assembly; "general" is the loop for tiles with
some F < 2^-383 (rb_sweeps4<false>: sqrt() with its range scaling, v_ldexp_f64),
"fast" the one every other tile runs.  The two kernels share the general loop,
so there are three distinct loops.  A report, not a test.
"""
import re
import sys

KERNELS = {
    "_ZN4dymu14k_fim_pass_dynILi16ELb1ELb0EEEvNS_8PassArgsE": "k_fim_pass_dyn<16,true,false> (default)",
    "_ZN4dymu14k_fim_pass_dynILi16ELb0ELb0EEEvNS_8PassArgsE": "k_fim_pass_dyn<16,false,false> (exact_sqrt)",
}
COUNTS = [
    ("ds_read_b64", r"ds_read_b64\b"),
    ("ds_read2_b64", r"ds_read2(st64)?_b64\b"),
    ("ds_write_b64", r"ds_write_b64\b"),
    ("ds_write2_b64", r"ds_write2(st64)?_b64\b"),
    ("flat_load", r"flat_load_"),
    ("v_*", r"v_"),
    ("s_waitcnt", r"s_waitcnt\b"),
]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def body(lines, name):
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def loops(fn):
    """(first, last) line ranges of the innermost loops: label .. backward branch to it"""
    at = {}
    spans = []
    for i, l in enumerate(fn):
        m = LABEL.match(l)
        if m:
            at[m.group(1)] = i
        m = BRANCH.match(l)
        if m and m.group(1) in at:
            spans.append((at[m.group(1)], i))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    return sorted(set(inner))


def opcode(line):
    s = line.split(";")[0].strip()
    return s.split()[0] if s and not s.startswith(".") and not s.endswith(":") else ""


def main():
    lines = open(sys.argv[1]).read().splitlines()
    meta = "\n".join(lines)
    for sym, title in KERNELS.items():
        m = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % sym, meta)
        print("%s: %s VGPRs, %s VGPR spills" % (title, m.group(1), m.group(2)))
        fn = body(lines, sym)
        n = 0
        for a, b in loops(fn):
            ops = [opcode(l) for l in fn[a : b + 1]]
            if "s_memrealtime" not in ops or not any(o.startswith("ds_write") for o in ops):
                continue
            n += 1
            kind = "general" if any(o.startswith("v_ldexp_f64") for o in ops) else "fast"
            row = ", ".join("%s %d" % (k, sum(1 for o in ops if re.match(p, o))) for k, p in COUNTS)
            print("  sweep loop %d (%s, asm lines +%d..+%d): %s" % (n, kind, a, b, row))
        if n == 0:
            print("  no sweep loop found")


if __name__ == "__main__":
    main()
