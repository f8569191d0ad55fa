#!/usr/bin/env python3
"""Are the functions of two sets of AMDGPU assembly files the same code?

  hipcc <the Makefile's flags> --cuda-device-only -S -o a.s old.hip      (likewise b.s, c.s)
  tools/kernel_identity.py --a a.s --b b.s c.s [--out report.txt]

For every function symbol (kernels and the device functions left out of line) of side A and
of side B: the instruction stream (labels and instructions, comments dropped, the
per-file numbering of local labels removed) and, for kernels, the .amdhsa_* directives of
the kernel descriptor. A refactor that moves code between files without touching a body
leaves every stream and every directive equal. Prints one line per symbol and exits 1 on
any difference.
"""
import argparse
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp)(\d+)")


def functions(path):
    """{symbol: (instruction lines, amdhsa directives or None)}"""
    out, name, pending, body, desc, in_desc = {}, None, None, [], None, False
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            pending = m.group(1)
            continue
        if pending and line == pending + ":":
            name, pending, body, desc = line[:-1], None, [], None
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = (body, desc)
            name = None
        elif line.startswith(".amdhsa_kernel"):
            in_desc, desc = True, []
        elif line.startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            desc.append(" ".join(line.split()))
        elif not line.startswith(".") or line.startswith(".LBB"):
            body.append(LOCAL.sub(lambda k: ".L" + k.group(1), " ".join(line.split())))
    return out


def collect(paths):
    merged = {}
    for p in paths:
        for sym, f in functions(p).items():
            if sym in merged:
                sys.exit("%s: defined twice on one side" % sym)
            merged[sym] = f
    return merged


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--a", nargs="+", required=True, help="assembly files of the first side")
    ap.add_argument("--b", nargs="+", required=True, help="assembly files of the second side")
    ap.add_argument("--out", help="also write the report here")
    args = ap.parse_args()
    A, B = collect(args.a), collect(args.b)
    lines, bad = [], 0
    for sym in sorted(set(A) | set(B)):
        if sym not in A or sym not in B:
            verdict = "ONLY IN " + ("A" if sym in A else "B")
        else:
            (ia, da), (ib, db) = A[sym], B[sym]
            diffs = [w for w, x, y in (("instructions", ia, ib), ("descriptor", da, db)) if x != y]
            verdict = "DIFFERENT " + "+".join(diffs) if diffs else "identical"
        bad += verdict != "identical"
        ins, d = A.get(sym) or B.get(sym)
        kind = "kernel  " if d is not None else "function"
        lines.append("%-22s %s %6d lines  %s" % (verdict, kind, len(ins), sym))
    nk = sum(1 for f in A.values() if f[1] is not None)
    lines.append("A: %d symbols (%d kernels) in %d file(s); B: %d symbols in %d file(s); %d not identical"
                 % (len(A), nk, len(args.a), len(B), len(args.b), bad))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        open(args.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
