"""tools/kernel_isa_diff.py: the disassembly normaliser and the comparison, on
canned llvm-objdump text (no compiler, no GPU)."""
import importlib.util
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                     "kernel_isa_diff.py")
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", _PATH)
kid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kid)

OLD = """
a.out:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001800 <void (anonymous namespace)::k_assign<64, 2, false, false>((anonymous namespace)::Tbl, int*)>:
\ts_load_dwordx2 s[4:5], s[0:1], 0x0                         // 000000001800: C0060100 00000000
\tv_cmp_gt_i32_e32 vcc, s13, v0                              // 000000001808: 7D88000D
\ts_cbranch_execz 33                                         // 00000000180C: BF880021 <void (anonymous namespace)::k_assign<64, 2, false, false>((anonymous namespace)::Tbl, int*)+0xac>
\ts_endpgm                                                   // 000000001810: BF810000
\t...

0000000000001900 <k_plain(float const*, int)>:
\tv_mov_b32_e32 v1, 0                                        // 000000001900: 7E020280
\ts_endpgm                                                   // 000000001904: BF810000

0000000000001a00 <void (anonymous namespace)::k_gone<3>(int*)>:
\ts_endpgm                                                   // 000000001A00: BF810000
\ts_nop 0                                                    // 000000001A04: BF800000
\ts_nop 0                                                    // 000000001A08: BF800000
"""

# k_assign moved and lost a template argument, same instructions; k_plain lost
# an instruction; k_gone went; k_new came
NEW = """
Disassembly of section .text:

0000000000004000 <k_plain(float const*, int)>:
\ts_endpgm                                                   // 000000004000: BF810000

0000000000004100 <void (anonymous namespace)::k_assign<64, 2, false>((anonymous namespace)::Tbl, int*)>:
\ts_load_dwordx2 s[4:5], s[0:1], 0x0                         // 000000004100: C0060100 00000000
\tv_cmp_gt_i32_e32 vcc, s13, v0                              // 000000004108: 7D88000D
\ts_cbranch_execz 33                                         // 00000000410C: BF880021 <void (anonymous namespace)::k_assign<64, 2, false>((anonymous namespace)::Tbl, int*)+0xac>
\ts_endpgm                                                   // 000000004110: BF810000

0000000000004200 <void (anonymous namespace)::k_new<1>(int*)>:
\ts_endpgm                                                   // 000000004200: BF810000
"""


def test_normalise_strips_addresses_targets_and_padding():
    old = kid.normalise(OLD)
    assert sorted(old) == ["k_assign<64, 2, false, false>", "k_gone<3>", "k_plain"]
    assert old["k_assign<64, 2, false, false>"] == [
        "s_load_dwordx2 s[4:5], s[0:1], 0x0", "v_cmp_gt_i32_e32 vcc, s13, v0",
        "s_cbranch_execz 33", "s_endpgm"]
    assert old["k_plain"] == ["v_mov_b32_e32 v1, 0", "s_endpgm"]
    # the s_nop run that closes .text is padding of whichever kernel is last
    assert old["k_gone<3>"] == ["s_endpgm"]


def test_compare_pairs_renamed_kernels_and_honours_allow():
    old, new = kid.normalise(OLD), kid.normalise(NEW)
    rename = {"k_assign<64, 2, false, false>": "k_assign<64, 2, false>"}
    removed, added, diff, same, ok = kid.compare(old, new, rename, set())
    assert (removed, added, diff, same, ok) == (["k_gone<3>"], ["k_new<1>"], ["k_plain"], 1, False)
    assert kid.compare(old, new, rename, {"k_plain"})[4] is True
    # without the rename the moved kernel is a removal and an addition, not a match
    removed, added, diff, same, ok = kid.compare(old, new, {}, {"k_plain"})
    assert "k_assign<64, 2, false, false>" in removed and "k_assign<64, 2, false>" in added
    assert same == 0 and ok
