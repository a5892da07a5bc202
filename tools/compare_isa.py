#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -Iinclude -S --cuda-device-only -o X.s g1_locomotion_amd/csrc/srbdqp.hip
    tools/compare_isa.py parent.s this.s [--loose REGEX] [--rename REGEX=REPLACEMENT]...

Reads the two .s files and nothing else.  Every --rename is applied to the symbols of both files before kernels are
matched, so that a renamed kernel can be held against its predecessor.  Per kernel: the text between `<symbol>:` and
`.Lfunc_end` (comments and .loc / .file / .cfi lines dropped, `.LBB<n>_` label numbers normalised), the `.amdhsa_*` lines, and the counts of the
instruction classes below.  Kernels whose demangled-or-not symbol matches --loose (default: the general and the
compact kernel families) may differ in text as long as every `.amdhsa_*` line and every class count is equal;
every other kernel must be identical.  Exit status 0 when all of that holds."""
import re
import sys

CLASSES = [
    ("mfma", r"v_mfma"),
    ("lds", r"ds_"),
    ("scratch", r"scratch_"),
    ("vmem", r"(global_|flat_|buffer_)"),
    ("sload", r"(s_load|s_buffer_load)"),
    ("barrier", r"s_barrier"),
    ("branch", r"(s_cbranch|s_branch)"),
    ("lane", r"(v_readlane|v_readfirstlane|v_writelane)"),
    ("fparith", r"v_(pk_)?(fma|fmac|mul|add|rcp|rsq|div_)[a-z_]*_(f32|f64)"),
]
CLASSES = [(n, re.compile(p)) for n, p in CLASSES]


def parse(path, renames=()):
    text = open(path).read()
    for rx, to in renames:
        text = re.sub(rx, to, text)
    text = text.split("\n")
    kernels = {}
    hsa = {}
    names = set()
    for ln in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            names.add(m.group(1))
    cur = None
    body = None
    hcur = None
    for ln in text:
        s = ln.split(";", 1)[0].rstrip()
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            hcur = m.group(1)
            hsa[hcur] = []
            continue
        if hcur is not None:
            if s.strip() == ".end_amdhsa_kernel":
                hcur = None
            elif s.strip():
                hsa[hcur].append(" ".join(s.split()))
            continue
        if cur is None:
            m = re.match(r"^(\S+):\s*$", s)
            if m and m.group(1) in names:
                cur = m.group(1)
                body = []
            continue
        if s.startswith(".Lfunc_end"):
            kernels[cur] = body
            cur = None
            continue
        st = s.strip()
        if not st or st.startswith((".loc", ".file", ".cfi", ".p2align 0")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(st.split())))
    return kernels, hsa


def counts(body):
    c = {n: 0 for n, _ in CLASSES}
    tot = 0
    for ln in body:
        if ln.endswith(":") or ln.startswith("."):
            continue
        tot += 1
        mn = ln.split()[0]
        for n, rx in CLASSES:
            if rx.match(mn):
                c[n] += 1
    return tot, c


def main():
    args = sys.argv[1:]
    loose = r"(srbdqp_wrench_kernel|srbdqp_compact_kernel)"
    if "--loose" in args:
        k = args.index("--loose")
        loose = args[k + 1]
        del args[k:k + 2]
    renames = []
    while "--rename" in args:
        k = args.index("--rename")
        rx, to = args[k + 1].split("=", 1)
        renames.append((rx, to))
        del args[k:k + 2]
    ka, ha = parse(args[0], renames)
    kb, hb = parse(args[1], renames)
    bad = 0
    if set(ka) != set(kb):
        print("SYMBOLS DIFFER: only in A:", sorted(set(ka) - set(kb)), "only in B:", sorted(set(kb) - set(ka)))
        bad += 1
    print(f"# {len(ka)} kernels in {args[0]}, {len(kb)} in {args[1]}")
    print("# kernel | instructions A | B | delta % | text | amdhsa | classes that differ (A -> B)")
    same = 0
    for k in sorted(set(ka) & set(kb)):
        ta, ca = counts(ka[k])
        tb, cb = counts(kb[k])
        ident = ka[k] == kb[k]
        hs = ha.get(k) == hb.get(k)
        dc = [f"{n} {ca[n]}->{cb[n]}" for n, _ in CLASSES if ca[n] != cb[n]]
        same += ident
        ok = ident or (re.search(loose, k) and hs and not dc)
        if not hs or not ok:
            bad += 1
        if not hs:
            for x, y in zip(ha.get(k, []), hb.get(k, [])):
                if x != y:
                    dc.append(f"[{x} | {y}]")
        print(f"{k} | {ta} | {tb} | {100.0 * (tb - ta) / max(ta, 1):+.3f} | {'same' if ident else 'differs'} | {'same' if hs else 'DIFFERS'} | {', '.join(dc) if dc else '-'}{'' if ok else '   <-- FAIL'}")
    print(f"# identical text: {same} of {len(set(ka) & set(kb))}; failures: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
