"""tools/kernel_code_diff.py on made-up assembly text: what it calls the same, what it calls different, and its exit status."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("c25519_kernel_code_diff", os.path.join(ROOT, "tools", "kernel_code_diff.py"))
kcd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kcd)


def kernel(sym, f, pc, reg="v1"):
    """one kernel the way `hipcc -S` prints it, as function number `f` of its file, with the file's getpc counter at `pc`"""
    return f"""\t.protected\t{sym}
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}:                                  ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_add_u32_e32 {reg}, v0, v0              ; a comment
\ts_cbranch_scc0 .LBB{f}_2
; %bb.1:
\ts_getpc_b64 s[2:3]
.Lpost_getpc{pc}:
\ts_add_u32 s2, s2, (.LBB{f}_3-.Lpost_getpc{pc})&4294967295
\ts_setpc_b64 s[2:3]
.LBB{f}_2:
\tv_mov_b32_e32 v2, 0
.LBB{f}_3:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_next_free_vgpr 3
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{f}:
\t.size\t{sym}, .Lfunc_end{f}-{sym}
"""


A, B = "_Z3k_aPj", "_Z3k_bPj"


def run(tmp_path, capsys, old, new, allow=()):
    (tmp_path / "old.s").write_text(old)
    (tmp_path / "new.s").write_text(new)
    rc = kcd.main(["--old", str(tmp_path / "old.s"), "--new", str(tmp_path / "new.s"), "--allow", *allow])
    lines = [l for l in capsys.readouterr().out.splitlines() if not l.startswith("#")]
    return rc, {l.split()[-1]: l.split()[0] for l in lines}, lines


def test_label_numbers_alone_are_the_same(tmp_path, capsys):
    rc, status, lines = run(tmp_path, capsys, kernel(A, 0, 0) + kernel(B, 1, 1), kernel(B, 0, 0) + kernel(A, 7, 12))
    assert rc == 0 and status == {A: "same", B: "same"}
    assert all(" 8 -> 8 " in l for l in lines), lines                          # eight instructions, labels not counted


def test_one_register_differs(tmp_path, capsys):
    rc, status, _ = run(tmp_path, capsys, kernel(A, 0, 0) + kernel(B, 1, 1), kernel(A, 0, 0) + kernel(B, 1, 1, reg="v3"))
    assert rc == 1 and status == {A: "same", B: "differs"}


def test_missing_kernel_is_reported(tmp_path, capsys):
    rc, status, _ = run(tmp_path, capsys, kernel(A, 0, 0) + kernel(B, 1, 1), kernel(A, 0, 0))
    assert rc == 1 and status == {A: "same", B: "only-old"}
    rc, status, _ = run(tmp_path, capsys, kernel(A, 0, 0), kernel(A, 0, 0) + kernel(B, 1, 1))
    assert rc == 1 and status == {A: "same", B: "only-new"}


def test_allow_lifts_the_status(tmp_path, capsys):
    old, new = kernel(A, 0, 0) + kernel(B, 1, 1), kernel(A, 0, 0, reg="v9")
    assert run(tmp_path, capsys, old, new)[0] == 1
    assert run(tmp_path, capsys, old, new, allow=["k_a"])[0] == 1              # k_b is still missing
    rc, status, _ = run(tmp_path, capsys, old, new, allow=["k_a", B])          # the plain name or the whole symbol
    assert rc == 0 and status == {A: "differs", B: "only-old"}
