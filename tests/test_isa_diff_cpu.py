"""tools/isa_diff.py on two small synthetic listings: label numbers and comments are normalised away, a changed
line, a changed directive, a missing kernel and a renamed kernel are each reported as such."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_diff.py")


def _kernel(name, index, body, vgpr=8, kernarg=16, tmp=0):
    return f"""\t.globl\t{name}
\t.type\t{name},@function
{name}:                                  ; @{name}
; %bb.0:
\ts_load_dword s2, s[0:1], 0x0
.LBB{index}_1:                           ; =>This Inner Loop Header: Depth=1
{body}
\ts_cbranch_scc1 .LBB{index}_1
.Ltmp{tmp}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_kernarg_size {kernarg}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
"""


def _run(tmp_path, old, new, *args):
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    r = subprocess.run([sys.executable, TOOL, str(tmp_path / "old.s"), str(tmp_path / "new.s"), *args],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


def test_same_after_label_renumbering_and_gone(tmp_path):
    add = "\tv_add_u32_e32 v1, v1, v2"
    old = _kernel("_Z3fooPf", 0, add) + _kernel("_Z4gonePf", 1, add, tmp=1) + _kernel("_Z3barPf", 2, add, tmp=2)
    new = _kernel("_Z3fooPf", 0, add + "   ; another comment") + _kernel("_Z3barPf", 1, add, tmp=7)
    rc, out = _run(tmp_path, old, new)
    assert rc == 0, out
    assert "same  _Z3fooPf" in out and "same  _Z3barPf" in out and "GONE  _Z4gonePf" in out
    assert "DIFF" not in out and "NEW" not in out
    assert "next_free_vgpr=8" in out and "kernarg_size=16" in out


def test_changed_line_and_directive_are_diffs(tmp_path):
    old = _kernel("_Z3fooPf", 0, "\tv_add_u32_e32 v1, v1, v2") + _kernel("_Z3barPf", 1, "\tv_mov_b32_e32 v0, 0")
    new = _kernel("_Z3fooPf", 0, "\tv_add_u32_e32 v1, v1, v3") + _kernel("_Z3barPf", 1, "\tv_mov_b32_e32 v0, 0", vgpr=9)
    rc, out = _run(tmp_path, old, new)
    assert rc == 1
    assert "DIFF  _Z3fooPf" in out and "- v_add_u32_e32 v1, v1, v2" in out and "+ v_add_u32_e32 v1, v1, v3" in out
    assert "DIFF  _Z3barPf" in out and ".amdhsa_next_free_vgpr: 8 -> 9" in out


def test_name_map(tmp_path):
    body = "\tv_mov_b32_e32 v0, 0"
    old, new = _kernel("_Z3fooILb0EEvPf", 0, body), _kernel("_Z3fooPf", 0, body)
    rc, out = _run(tmp_path, old, new)
    assert "GONE  _Z3fooILb0EEvPf" in out and "NEW   _Z3fooPf" in out
    rc, out = _run(tmp_path, old, new, "--map", "_Z3fooILb0EEvPf=_Z3fooPf")
    assert rc == 0 and "same  _Z3fooILb0EEvPf -> _Z3fooPf" in out
