"""tools/same_kernels.py on synthetic device assembly: two kernels, in opposite emission order and so with other local label numbers,
are the same code; one changed instruction, one changed register count in the metadata, or a missing kernel name that kernel."""
import importlib.util
import os

_TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "same_kernels.py")
_spec = importlib.util.spec_from_file_location("same_kernels", _TOOL)
same_kernels = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(same_kernels)


def _kernel(name, n, op="v_add_f32_e32 v1, v0, v0"):
    """the text of function number n of a file: label, a loop with a local label, the descriptor, the end label"""
    return f"""\t.protected\t{name} ; -- Begin function {name}
\t.globl\t{name}
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dword s4, s[0:1], 0x38
.LBB{n}_1: ; =>This Inner Loop Header: Depth=1
\t{op}
\ts_cbranch_scc1 .LBB{n}_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
                                        ; -- End function
"""


def _meta(name, vgprs=2):
    return f"""  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .name:           {name}
    .symbol:         {name}.kd
    .vgpr_count:     {vgprs}
"""


def _file(kernels, cuid="aaaa"):
    """kernels: (name, instruction, vgpr_count) in emission order"""
    body = "".join(_kernel(name, n, op) for n, (name, op, _) in enumerate(kernels))
    meta = "".join(_meta(name, v) for name, _, v in kernels)
    return (f'\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.text\n{body}\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n'
            f"\t.amdgpu_metadata\n---\namdhsa.kernels:\n{meta}amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


ADD, MUL = "v_add_f32_e32 v1, v0, v0", "v_mul_f32_e32 v1, v0, v0"
BASE = _file([("_Z1av", ADD, 2), ("_Z1bv", MUL, 2)], "aaaa")


def test_order_and_label_numbers_do_not_count():
    other = _file([("_Z1bv", MUL, 2), ("_Z1av", ADD, 2)], "bbbb")
    assert BASE != other
    assert same_kernels.compare(BASE, other) == (2, 2, [], [])


def test_changed_instruction_names_the_kernel():
    other = _file([("_Z1bv", ADD, 2), ("_Z1av", ADD, 2)])
    assert same_kernels.compare(BASE, other) == (2, 2, [], ["_Z1bv"])


def test_changed_vgpr_count_names_the_kernel():
    other = _file([("_Z1av", ADD, 3), ("_Z1bv", MUL, 2)])
    assert same_kernels.compare(BASE, other) == (2, 2, [], ["_Z1av"])


def test_missing_kernel_is_named():
    other = _file([("_Z1av", ADD, 2)])
    assert same_kernels.compare(BASE, other) == (2, 1, ["_Z1bv"], [])


def test_exit_status(tmp_path):
    for d, text in (("a", BASE), ("b", _file([("_Z1bv", MUL, 2), ("_Z1av", ADD, 2)])), ("c", _file([("_Z1av", MUL, 2), ("_Z1bv", MUL, 2)]))):
        os.makedirs(tmp_path / d)
        (tmp_path / d / ("x" + same_kernels.SUFFIX)).write_text(text)
    assert same_kernels.main(["same_kernels.py", str(tmp_path / "a"), str(tmp_path / "b")]) == 0
    assert same_kernels.main(["same_kernels.py", str(tmp_path / "a"), str(tmp_path / "c")]) == 1
