"""(CPU) the graph layout of the on-chip layered kernel for any H (csrc/layered_csr_layout.cc: barrier steps, slabs, the column table, the
per-wave weights) under AddressSanitizer and UBSan, through its stand-alone driver tools/layered_csr_layout_main.cc -- which holds the
tables to the rows itself and exits non-zero on a violation -- on the graphs of tests/layered_shapes.py, and against that module's
restatement of the steps and slabs.  Thread counts: the default, 128 (a last slab with an idle wave) and 64 (steps of several slabs),
the situations tests/test_layered_shapes.py proves these graphs to hold."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import layered_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, layers): the declared layers of case(), and "w8" with one row per layer
GRAPHS = [("w8", "declared"), ("w20", "declared"), ("w27", "declared"), ("w8", "rows")]
DEFAULT_THREADS = {"w8": 256, "w20": 256, "w27": 192}        # (tests/test_layered_shapes.py THREADS)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("layout") / "layered_csr_layout_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "layered_csr_layout_main.cc"),
                           os.path.join(ROOT, "ecc_ldpc_amd", "csrc", "layered_csr_layout.cc"), "-o", str(exe)])
    return str(exe)


def _layers(name, layers):
    g = S.case(name)
    return g, (g.layer_ptr if layers == "declared" else np.arange(g.M + 1))


@pytest.mark.parametrize("threads", ["default", 128, 64])
@pytest.mark.parametrize("name,layers", GRAPHS)
def test_layout(driver, tmp_path, name, layers, threads):
    g, lp = _layers(name, layers)
    if threads == "default":
        T = S.default_threads(g, lp)
        if layers == "declared":
            assert T == DEFAULT_THREADS[name]
    else:
        T = threads
    path = tmp_path / "graph.txt"
    with open(path, "w") as f:
        f.write(f"{g.N} {g.M} {len(lp) - 1} {T}\n")
        for a in (lp, g.row_ptr, g.col_idx):
            f.write(" ".join(map(str, np.asarray(a).tolist())) + "\n")
    out = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("ok")
    # the step boundaries, the slab count and the last slab's rows of every step
    got = [tuple(map(int, m.groups())) for m in re.finditer(r"^step \d+ rows (\d+) lo (\d+) hi (\d+) slabs (\d+) last (\d+)$", out.stdout, re.M)]
    want = [(len(s), int(s[0]), int(s[-1])) + S.slabs(s, T) for s in S.steps_of(g, lp)]
    assert got == want
    head = re.match(r"graph N (\d+) M (\d+) layers (\d+) T (\d+): steps (\d+) rmax (\d+) nslab (\d+)\n", out.stdout)
    assert tuple(map(int, head.groups())) == (g.N, g.M, len(lp) - 1, T, len(want), max(w[0] for w in want), sum(w[3] for w in want))
    assert len(re.findall(r"^slab \d+ offset", out.stdout, re.M)) == sum(w[3] for w in want)
