#!/usr/bin/env python3
"""tools/isa_diff.py A.s B.s [substring] -- compares the gfx950 ISA of every kernel two builds have in common.

A.s / B.s are `hipcc -save-temps` device assembly files (`make -C 3dscan_amd/csrc asm` writes /tmp/sl3d_*-gfx950.s; several
files per side may be given separated by commas).  For every kernel symbol present on both sides the instruction stream is
compared after normalising what a refactoring may legitimately change: comments, directives, local label numbers.
Prints one line per kernel that differs (first differing instruction + the instruction-histogram delta) and a summary.
With `--kernarg` the immediate offsets of scalar loads from the kernel-argument segment (s[0:1] / s[4:5] ...) are masked too
(a change of the KParams layout moves them and nothing else).  `--pair=OLD=NEW` (any number of them) also compares the kernel of A
whose name (demangled where llvm-cxxfilt is there, mangled otherwise) contains OLD -- OLD holds no `=` -- with the kernel of B whose
name contains NEW: a kernel that was renamed.  With `--scalar-equivalent` every kernel that differs gets a second line: the histogram delta
restricted to vector, memory and LDS instructions, scalar loads, waits and barriers (v_*, global_*, flat_*, buffer_*, ds_*, s_load_*,
s_buffer_load_*, s_waitcnt, s_barrier), the registers, scratch, LDS and occupancy lines of both sides, and the verdict: SCALAR-EQUIVALENT if that
delta is empty and those lines are all found and equal -- what is left is scalar ALU, compare, branch, move and s_nop -- or NOT EQUIVALENT; the summary then
counts them.  The default output is unchanged."""
import collections
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def kernels(paths, mask_kernarg):
    out = {}
    for path in paths.split(","):
        cur, body = None, []
        for line in open(path, errors="replace"):
            line = line.split(";", 1)[0].rstrip()
            if not line.strip():
                continue
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur, body = m.group(1), []
                continue
            if cur is None:
                continue
            s = line.strip()
            if s.startswith(".Lfunc_end"):
                out[cur] = body
                cur = None
                continue
            if s.startswith(".") and not s.startswith(".LBB"):
                continue
            body.append(s)
    norm = {}
    for k, body in out.items():
        labels = {}
        res = []
        for s in body:
            def lab(m):
                return labels.setdefault(m.group(0), f".L{len(labels)}")
            s = re.sub(r"\.LBB\d+_\d+", lab, s)
            if mask_kernarg:
                s = re.sub(r"(s_load_\w+ \S+ s\[\d+:\d+\], )0x[0-9a-f]+", r"\1OFF", s)
            res.append(s)
        norm[k] = res
    return norm


RESTRICTED = re.compile(r"^(v_|global_|flat_|buffer_|ds_|s_load_|s_buffer_load_|s_waitcnt|s_barrier)")
RESOURCES = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def resources(paths):
    """kernel symbol -> the resource lines of its `; Kernel info:` block"""
    out = {}
    for path in paths.split(","):
        cur = None
        for line in open(path, errors="replace"):
            m = re.match(r"^\s*\.size\s+(_Z\w+),", line)
            if m:
                cur = m.group(1)
                continue
            m = re.match(r"^; (\w+): (\d+)", line)
            if m and cur and m.group(1) in RESOURCES:
                out.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mask = "--kernarg" in sys.argv
    A, B = kernels(args[0], mask), kernels(args[1], mask)
    sub = args[2] if len(args) > 2 else ""
    names = demangle(sorted(set(A) | set(B)))
    pairs = [(k, k, names[k]) for k in sorted(set(A) & set(B)) if not sub or sub in names[k]]
    for old, new in (a[len("--pair="):].split("=", 1) for a in sys.argv[1:] if a.startswith("--pair=")):
        ka, kb = [k for k in A if old in names[k]], [k for k in B if new in names[k]]
        if len(ka) != 1 or len(kb) != 1:
            sys.exit(f"--pair={old}={new}: {len(ka)} kernels of A and {len(kb)} of B match")
        pairs.append((ka[0], kb[0], f"{names[ka[0]]} = {names[kb[0]]}"))
    scalar = "--scalar-equivalent" in sys.argv
    RA, RB = (resources(args[0]), resources(args[1])) if scalar else ({}, {})
    same = diff = equivalent = 0
    for ka, kb, name in pairs:
        a, b = A[ka], B[kb]
        if a == b:
            same += 1
            continue
        diff += 1
        ha = collections.Counter(s.split()[0] for s in a if not s.endswith(":"))
        hb = collections.Counter(s.split()[0] for s in b if not s.endswith(":"))
        delta = {op: hb[op] - ha[op] for op in set(ha) | set(hb) if hb[op] != ha[op]}
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"DIFF {name}: {len(a)} -> {len(b)} lines, first difference at {first}: "
              f"{a[first] if first < len(a) else '<end>'!r} vs {b[first] if first < len(b) else '<end>'!r}; histogram delta {delta or 'none (order only)'}")
        if scalar:
            restricted = {op: d for op, d in delta.items() if RESTRICTED.match(op)}
            ra, rb = RA.get(ka, {}), RB.get(kb, {})
            ok = not restricted and ra == rb and set(ra) == set(RESOURCES)  # (resource lines missing on a side: not shown equal)
            equivalent += ok
            print(f"  {'SCALAR-EQUIVALENT' if ok else 'NOT EQUIVALENT'}: restricted histogram delta {restricted or 'none'}; resources {ra} vs {rb}")
    print(f"{same} kernels identical, {diff} differ; {len(set(A) - set(B))} only in A, {len(set(B) - set(A))} only in B"
          + (f"; of the {diff}: {equivalent} scalar-equivalent, {diff - equivalent} not" if scalar else ""))


if __name__ == "__main__":
    main()
