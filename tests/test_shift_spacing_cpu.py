"""Shift-spacing guard (CPU): in the pair-rule K1w main loop no half-rate
instruction (DPP move, funnel shift) follows another within G instructions
(isolated, a shift's half rate hides behind the fetch of the
8-byte LUTs around it; clustered, it does not), and the loop's instruction
counts are those of the rule itself.  Reads the emitted code of the built
libgolhip.so (no GPU); skipped when it is not built."""
import collections
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "game-of-life-distributed_amd", "golhip", "libgolhip.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not shutil.which("/opt/rocm/lib/llvm/bin/llvm-objdump"),
                                reason="libgolhip.so not built or no LLVM tools")

G = 3  # the smallest gap of the spaced schedule


@pytest.fixture(scope="module")
def disasm():
    import loop_parity
    return loop_parity.disassemble(LIB)


def test_issue_classes_and_crowding():
    import loop_parity
    cls = loop_parity.issue_classes(["v_bitop3_b32", "v_mov_b32_dpp", "v_alignbit_b32", "s_nop", "v_mov_b32_e32"])
    assert cls == "VHHOV"
    assert loop_parity.crowded_shifts("HVVVHVVHVVVV", 3) == (1, 3)   # only the 3-apart pair; the back edge is 5 apart
    assert loop_parity.crowded_shifts("HVVH", 3) == (2, 2)           # 3 apart, and 1 apart around the back edge
    assert loop_parity.crowded_shifts("VVVV", 3) == (0, 0)


@pytest.mark.parametrize("kernel", [
    "gol_skew_kernelILi18ELi2ELb0ELb1E",   # the headline: 65536^2
    "gol_skew_kernelILi18ELi2ELb1ELb1E",   # half-wave tiles: 16384^2
])
def test_pair_main_loop_shifts_are_spaced(disasm, kernel):
    import loop_parity
    mn = loop_parity.main_loop_mnemonics(disasm, kernel)
    cnt = collections.Counter(mn)
    # two 3-row groups of 18 stages at two words per lane: 8 LUTs, one DPP move
    # and one funnel shift a word-turn, nothing added or lost
    assert cnt["v_mov_b32_dpp"] == 216 and cnt["v_alignbit_b32"] == 216 and cnt["v_bitop3_b32"] == 1728, cnt
    # (4 before the spaced schedule: a hazard pad flips the code parity)
    assert cnt["s_nop"] <= 4, cnt["s_nop"]
    crowded, total = loop_parity.crowded_shifts(loop_parity.issue_classes(mn), G)
    assert total == 432
    assert crowded <= 0.05 * total, f"{kernel}: {crowded} of {total} half-rate instructions within {G} of the next"
