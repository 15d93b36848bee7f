"""The recipe that compiles the reference's cudabits/arraylet2.cu for gfx950 (oracle/ref_kernels.py): what it writes, what it records,
how it fails, and that nothing it makes is tracked by git.  Needs a checkout of the reference (and hipcc); skipped without one."""
import hashlib
import json
import os
import subprocess

import pytest

from oracle import ref_kernels as recipe
from tests.helpers import ROOT

REFERENCE = recipe.REFERENCE_DIR
pytestmark = pytest.mark.skipif(not recipe.reference_present(),
                                reason=f"no checkout of the reference at {REFERENCE}")


def tracked(path):
    """files under path that git tracks (none when this tree is not a git checkout)"""
    p = subprocess.run(["git", "-C", ROOT, "ls-files", "--", path], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    return p.stdout.split() if p.returncode == 0 else []


def test_build_ref_writes_a_code_object_and_a_manifest_that_describes_it(tmp_path):
    out = recipe.build_ref(REFERENCE, str(tmp_path))
    assert out == str(tmp_path / "arraylet2.co") and os.path.getsize(out) > 0
    blob = open(out, "rb").read()
    m = json.load(open(tmp_path / "MANIFEST.json"))
    assert sorted(m["kernels"]) == sorted(recipe.KERNELS) == recipe.kernel_names(blob) and len(m["kernels"]) == 9
    assert m["sha256"] == hashlib.sha256(blob).hexdigest()
    assert sorted(m["reference_files"]) == sorted(recipe.REFERENCE_FILES)
    for f, h in m["reference_files"].items():
        assert h == hashlib.sha256(open(os.path.join(REFERENCE, f), "rb").read()).hexdigest(), f
    assert m["wrapper"] == {"ref_arraylet2_wrap.hip": hashlib.sha256(open(recipe.WRAPPER, "rb").read()).hexdigest()}
    assert "version" in m["hipcc_version"].lower()
    assert m["flags"] == recipe.FLAGS and {"-O2", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950"} <= set(m["flags"])
    assert tracked(str(tmp_path)) == [] and tracked(os.path.join(ROOT, "oracle", "_ref")) == []


def test_a_missing_compiler_raises(tmp_path, monkeypatch):
    monkeypatch.setenv("HIPCC", str(tmp_path / "no-such-hipcc"))
    with pytest.raises(RuntimeError, match="no-such-hipcc"):
        recipe.build_ref(REFERENCE, str(tmp_path))
    assert not os.path.exists(tmp_path / "arraylet2.co") and not os.path.exists(tmp_path / "MANIFEST.json")


def test_a_compile_error_raises_with_the_compilers_log(tmp_path):
    """a directory that has the two file names but not their contents: the compiler's own message comes back in the exception"""
    bad = tmp_path / "ref" / "cudabits"
    bad.mkdir(parents=True)
    (bad / "common.h").write_text("typedef float float_ty;\n")
    (bad / "arraylet2.cu").write_text('#include "common.h"\nthis_is_not_a_declaration;\n')
    with pytest.raises(RuntimeError, match="this_is_not_a_declaration"):
        recipe.build_ref(str(tmp_path / "ref"), str(tmp_path / "out"))
    assert not os.path.exists(tmp_path / "out" / "MANIFEST.json")


def test_the_ignore_file_keeps_the_artefacts_out_of_git():
    lines = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "oracle/_ref/" in lines and "*.co" in lines
