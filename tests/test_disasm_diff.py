"""tools/disasm_diff.py: the per-symbol split and compare of two llvm-objdump listings, on hand-written text (no compiler, no GPU)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A = """
dev.co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001900 <_Z5firstPf>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001900: C0060002 00000000
\tv_mov_b32_e32 v1, 0                                        // 000000001908: 7E020280
\ts_endpgm                                                   // 00000000190C: BF810000

0000000000001a00 <_Z6secondPf>:
\tv_add_f32_e32 v0, v0, v1                                   // 000000001A00: 02000300
\ts_endpgm                                                   // 000000001A04: BF810000
"""
# the same code at other addresses: only the dropped columns differ
MOVED = A.replace("0000000000001900", "0000000000002900").replace("// 00000000190", "// 00000000290").replace("// 000000001A0", "// 000000002A0")


def test_disasm_diff_splits_and_compares_per_symbol():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import disasm_diff as dd
    syms = dd.split_symbols(A)
    assert list(syms) == ["_Z5firstPf", "_Z6secondPf"]
    assert syms["_Z5firstPf"] == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "s_endpgm"]
    # identical, at other addresses
    assert dd.compare(A, MOVED) == ([], 2, 2)
    # one changed line in one symbol
    assert dd.compare(A, A.replace("v_mov_b32_e32 v1, 0 ", "v_mov_b32_e32 v1, 1 ")) == ([("_Z5firstPf", 1, 3)], 1, 2)
    # a symbol missing on one side, whichever side
    cut = A[:A.index("0000000000001a00")]
    assert dd.compare(A, cut) == ([("_Z6secondPf", None, 2)], 1, 2)
    assert dd.compare(cut, A) == ([("_Z6secondPf", None, 2)], 1, 2)
