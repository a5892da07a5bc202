#!/usr/bin/env python3
"""Vector instructions of the FIRST pass of a one-wave kernel, by stretch, from a cross-compile.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -S --cuda-device-only -o X.s g1_locomotion_amd/csrc/srbdqp.hip
    tools/pass_vector_counts.py X.s [mangled kernel symbol [multiply-adds of F]]      (default: srbdqp_wave_defer_kernel<10, 2, false>, 426)

Reads the .s file and nothing else.  Counted: every v_* mnemonic but v_mfma*, in the text of the kernel from its start to the first
v_fmac_f64_dpp (the front end), from there to the 480th (the four packed inversions and the panels: F), and from there to the header of
the first loop behind it that holds 40 or more v_fmac_f64_dpp (the ADMM iteration): I + the row gather.  The multiply-adds of F at N = 10: three
full tiles of 120 and the last one's twelve real pivots on its twelve real rows, 66 -- 426; 480 until round 33 (pass 480 for a listing of such a tree).
Since round 35 the first panel tile of a block row rides the inversion in a DPP row of the same multiply-adds: F still ends at the 426th.
The first pass is the first one in the text of these kernels (profiles/r23_wave_setup_diet.txt has the parent's 1918 / 1644 / 451)."""
import collections
import re
import sys

DEFAULT = "_ZN6srbdqp24srbdqp_wave_defer_kernelILi10ELi2ELb0EEEvNS_5KArgsE"


def body_of(path, sym):
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
    body = []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        s = ln.split(";")[0].strip()
        if s:
            body.append(s)
    return body


def main():
    path = sys.argv[1]
    sym = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    b = body_of(path, sym)
    dpp = [i for i, s in enumerate(b) if s.startswith("v_fmac_f64_dpp")]
    nf = int(sys.argv[3]) if len(sys.argv) > 3 else 426
    first, last = dpp[0], dpp[nf - 1]
    labels = {}
    for i, s in enumerate(b):
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = i
    header = None
    for i, s in enumerate(b):
        if i <= last:
            continue
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", s)
        if m and last < labels.get(m.group(1), len(b)) < i and sum(1 for x in dpp if labels[m.group(1)] < x < i) >= 40:
            header = labels[m.group(1)]
            break
    total = 0
    for name, lo, hi in (("front end", 0, first), ("F", first, last + 1), ("I + row gather", last + 1, header)):
        seg = b[lo:hi]
        c = collections.Counter(s.split()[0] for s in seg if s.startswith("v_") and not s.startswith("v_mfma"))
        n = sum(c.values())
        total += n
        print(f"{name}: {n} vector (+{sum(1 for s in seg if s.startswith('v_mfma'))} MFMA) of {len(seg)} instructions; " + ", ".join(f"{k} {v}" for k, v in c.most_common(14)))
    print("total", total)


if __name__ == "__main__":
    main()
