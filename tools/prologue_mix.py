#!/usr/bin/env python3
"""What kernel 5's pass kernel runs once per wave before its first list entry,
from the compiler's assembly (built as tools/sweep_mix.py's docstring says).

    python tools/prologue_mix.py fim_kernels.s

For the default pass kernel k_fim_pass_dyn<16, true, false> and the exact_sqrt
one <16, false, false> it prints
  - the VALU instructions up to the prologue's s_barrier (every wave runs them,
    15 of 16 while waiting for wave 0's list scan),
  - the VALU instructions between that barrier and the entry loop's first LDS
    atomic (the draw from s_next), in the order of the assembly: the straight-
    line code on every wave's way to its first visit, with block 0's bookkeeping
    (which the other workgroups branch over) counted apart,
  - how many of them are v_writelane_b32 (SGPRs parked in a VGPR),
  - whether an f64 division (v_rcp_f64 / v_div_*_f64), an integer-division
    reciprocal (v_rcp_iflag_f32) or a ds_bpermute_b32 is left in the prologue,
  - VGPRs and VGPR spills.
A report, not a test.
"""
import re
import sys

from sweep_mix import KERNELS, body, opcode

ATOMIC = re.compile(r"ds_\w+_rtn_")
FLAGS = [
    ("f64 division", r"v_rcp_f64|v_div_(scale|fmas|fixup)_f64"),
    ("integer reciprocal", r"v_rcp_iflag_f32"),
    ("ds_bpermute", r"ds_bpermute_b32"),
]
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def block0_span(fn, bar, first):
    """Block 0's bookkeeping sits between the barrier and the entry loop; the other
    workgroups jump over it on a scalar condition (the workgroup id).  It is by far the
    longest stretch there that a scalar branch skips: returns the lines (branch, target
    label) of the longest forward s_branch / s_cbranch_scc jump, or (bar, bar)."""
    at = {LABEL.match(l).group(1): i for i, l in enumerate(fn) if LABEL.match(l)}
    best = (bar, bar)
    for i in range(bar, first):
        m = BRANCH.match(fn[i])
        if m and opcode(fn[i]) in ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1"):
            t = at.get(m.group(1), -1)
            if i < t < first and t - i > best[1] - best[0]:
                best = (i, t)
    return best


def main():
    lines = open(sys.argv[1]).read().splitlines()
    meta = "\n".join(lines)
    for sym, title in KERNELS.items():
        m = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % sym, meta)
        print("%s: %s VGPRs, %s VGPR spills" % (title, m.group(1), m.group(2)))
        fn = body(lines, sym)
        ops = [opcode(l) for l in fn]
        bar = ops.index("s_barrier")
        first = next(i for i in range(bar, len(ops)) if ATOMIC.match(ops[i]))
        valu = lambda a, b: sum(1 for o in ops[a:b] if o.startswith("v_"))
        b0, b1 = block0_span(fn, bar, first)
        print("  before the barrier: %d VALU" % valu(0, bar))
        print("  barrier to first LDS atomic (asm lines +%d..+%d): %d VALU, %d without block 0's "
              "bookkeeping (+%d..+%d), %d of those v_writelane_b32"
              % (bar, first, valu(bar, first), valu(bar, first) - valu(b0, b1), b0, b1,
                 sum(1 for i in range(bar, first) if ops[i] == "v_writelane_b32" and not b0 <= i < b1)))
        for name, pat in FLAGS:
            pre = sum(1 for o in ops[:bar] if re.match(pat, o))
            post = sum(1 for o in ops[bar:first] if re.match(pat, o))
            print("  %s: %d before the barrier, %d after" % (name, pre, post))


if __name__ == "__main__":
    main()
