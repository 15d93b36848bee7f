#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  tools/same_kernels.py BUILD_A BUILD_B

Compares every device assembly file (<stem>-hip-amdgcn-amd-amdhsa-gfx950.s, which ecc_ldpc_amd/build.py keeps next to the objects)
the two build directories share, KERNEL BY KERNEL: a change of host code moves the order in which templates are instantiated, so
the files differ as wholes even where every kernel is unchanged.  Per kernel it compares
  code      the lines from the kernel's label to its .Lfunc_end, the .amdhsa_kernel ... .end_amdhsa_kernel block among them;
  metadata  its entry under amdhsa.kernels (register counts, segment sizes, the argument list),
with comments stripped and the numbers of local labels normalised (.LBB<n>_ -> .LBB_, .Lfunc_begin<n> / .Lfunc_end<n> likewise):
those number a file's functions in emission order.  __hip_cuid_* (a hash of the translation unit) is ignored.
Prints per file the kernel count, whether the two sets of names are equal, and the names of kernels that differ or are missing;
exits non-zero on any difference, or if the directories share no such file."""
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def _clean(line):
    line = line.split(";", 1)[0].rstrip()
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def kernels(text):
    """{kernel name: (code lines, metadata lines)} of one device assembly text"""
    lines = text.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    code = {}
    cur = None
    for l in lines:
        head = l.split(";", 1)[0].strip()
        if cur is None and head.endswith(":") and head[:-1] in names:
            cur = head[:-1]
            code[cur] = []
        if cur is not None:
            c = _clean(l)
            if c.strip() and "__hip_cuid_" not in c:
                code[cur].append(c)
            if re.match(r"\.Lfunc_end\d+:", head):
                cur = None
    meta = {}
    entry = None
    inside = False
    for l in lines:
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and l.startswith("  - "):          # a new entry of the list
            entry = [l]
        elif inside and l.startswith("    ") and entry is not None:
            entry.append(l)
            m = re.match(r"\s+\.name:\s+(\S+)", l)
            if m:
                meta[m.group(1)] = entry
        elif inside:                                    # amdhsa.target, "...": the list is over
            inside = False
    return {n: (code.get(n, []), [_clean(l) for l in meta.get(n, [])]) for n in names}


def compare(text_a, text_b):
    """(kernels of a, kernels of b, names in one only, names whose code or metadata differ)"""
    a, b = kernels(text_a), kernels(text_b)
    missing = sorted(set(a) ^ set(b))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    return len(a), len(b), missing, differ


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    da, db = argv[1], argv[2]
    fa = {f for f in os.listdir(da) if f.endswith(SUFFIX)}
    fb = {f for f in os.listdir(db) if f.endswith(SUFFIX)}
    bad = 0
    for f in sorted(fa ^ fb):
        print(f"{f[:-len(SUFFIX)]}: only in {da if f in fa else db}")
        bad += 1
    total = 0
    for f in sorted(fa & fb):
        na, nb, missing, differ = compare(open(os.path.join(da, f)).read(), open(os.path.join(db, f)).read())
        total += na
        print(f"{f[:-len(SUFFIX)]}: {na} kernels / {nb} kernels, names {'equal' if not missing else 'DIFFER'}, {len(differ)} differing")
        for n in missing:
            print(f"    in one build only: {n}")
        for n in differ:
            print(f"    differs: {n}")
        bad += len(missing) + len(differ)
    if not fa & fb:
        print("no device assembly file in common")
        return 1
    print(f"{len(fa & fb)} files, {total} kernels: " + ("all the same" if not bad else f"{bad} differences"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
