"""Recipe for oracle/_ref/: the kernels of the reference's live GPU decoder `cuda-arraylet2` (cudabits/arraylet2.cu + common.h),
compiled as HIP source for gfx950 through oracle/ref_arraylet2_wrap.hip.  The reference is read where it lies (an include path at
build time); neither its text nor the code object is part of this repository: oracle/_ref/ is ignored by git.
TEST INFRASTRUCTURE ONLY, like the rest of oracle/ -- tests/ref_kernels.py launches what this builds.

cudabits/two_arrays.cu (its selfProduct also writes the transpose) is NOT built: its selfProduct computes
`offsets[(j*colCount) + blockI]` with j a row, not a block row (two_arrays.cu:83) -- a read far past the offsets table.  The value is
dead, but whether the read survives is the optimiser's choice, and a wrapper macro cannot take it out."""
from __future__ import annotations

import hashlib
import json
import os
import struct
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
CODE_OBJECT = os.path.join(REF_DIR, "arraylet2.co")
MANIFEST = os.path.join(REF_DIR, "MANIFEST.json")
WRAPPER = os.path.join(_HERE, "ref_arraylet2_wrap.hip")
REFERENCE_DIR = os.environ.get("LDPC_REFERENCE_DIR", "/root/reference")  # where a checkout of the reference lies, if anywhere
REFERENCE_FILES = ["cudabits/arraylet2.cu", "cudabits/common.h"]       # every file of the reference the compiler reads
# -O2 and nothing else special, as the reference's Makefile asks of nvcc; contraction off so that -(lam - v)/2 and the products stay
# the operations that are written
FLAGS = ["--offload-arch=gfx950", "--genco", "-O2", "-ffp-contract=off", "-fno-fast-math"]
KERNELS = ["tanhTransform", "setToOne", "makeNonzeroMat", "insertOnes", "atanhTransform", "updateLam", "parityRowResults",
           "checkParity", "selfProduct"]


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def kernel_names(blob: bytes):
    """names of the kernels in a gfx950 code object (the ELF itself or clang's offload bundle around it): the symbols `<name>.kd`
    (kernel descriptors) of its symbol tables"""
    if blob[:24] == b"__CLANG_OFFLOAD_BUNDLE__":
        n, p = struct.unpack_from("<Q", blob, 24)[0], 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24: p + 24 + tlen]
            p += 24 + tlen
            if triple.startswith(b"hip") and b"gfx950" in triple:
                blob = blob[off: off + size]
                break
        else:
            raise ValueError("no gfx950 entry in the offload bundle")
    if blob[:4] != b"\x7fELF" or blob[4] != 2 or blob[5] != 1:
        raise ValueError("not a little-endian ELF64 code object")
    shoff = struct.unpack_from("<Q", blob, 0x28)[0]
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + k * shentsize) for k in range(shnum)]
    names = set()
    for sh in sections:
        if sh[1] not in (2, 11):                                      # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff = sections[sh[6]][4]                                    # sh_link: its string table
        for q in range(sh[4], sh[4] + sh[5], sh[9] or 24):
            st_name = struct.unpack_from("<I", blob, q)[0]
            s = blob[stroff + st_name: blob.index(b"\0", stroff + st_name)].decode()
            if s.endswith(".kd"):
                names.add(s[:-3])
    return sorted(names)


def reference_present(reference_dir=REFERENCE_DIR):
    return all(os.path.isfile(os.path.join(reference_dir, f)) for f in REFERENCE_FILES)


def build_ref(reference_dir=REFERENCE_DIR, out_dir=None):
    """compile the reference's arraylet2.cu into <out_dir>/arraylet2.co and write <out_dir>/MANIFEST.json; -> the code object's path.
    Raises RuntimeError, with the compiler's log, when hipcc is missing or fails."""
    out_dir = out_dir or REF_DIR
    files = [os.path.join(reference_dir, f) for f in REFERENCE_FILES]
    for f in files:
        if not os.path.isfile(f):
            raise FileNotFoundError(f)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "arraylet2.co")
    hipcc = _hipcc()
    cmd = [hipcc] + FLAGS + ["-I", reference_dir, "-x", "hip", WRAPPER, "-o", out]
    try:
        version = subprocess.run([hipcc, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except (OSError, subprocess.CalledProcessError) as e:
        raise RuntimeError(f"cannot run {hipcc}: {e}") from e
    if p.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"{' '.join(cmd)} failed with status {p.returncode}:\n{p.stdout}")
    found = kernel_names(open(out, "rb").read())
    missing = [k for k in KERNELS if k not in found]
    if missing:
        raise RuntimeError(f"{out}: kernels {missing} are missing (found {found})")
    manifest = {
        "artefact": "arraylet2.co",
        "sha256": _sha256(out),
        "wrapper": {os.path.basename(WRAPPER): _sha256(WRAPPER)},
        "reference_files": {f: _sha256(p_) for f, p_ in zip(REFERENCE_FILES, files)},
        "hipcc_version": next((l for l in version.splitlines() if "version" in l.lower()), version.strip()),
        "flags": FLAGS,
        "kernels": found,
    }
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")
    return out


if __name__ == "__main__":
    print(build_ref())
