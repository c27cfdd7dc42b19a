"""The two-front chain kernels solve the middle link of the block-tridiagonal sweep from registers (ck_tri_mid_regs, cclqr_chain.h): the sixty LDS reads of
the one-lane middle solve (ck_tri_mid) are sixty DPP row broadcasts, and the first back step no longer reads dl of the middle link back.  What this file
checks in the ISA (CPU suite: one gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests): the broadcasts are there, the reads are gone, and the
8-lane kernels -- one front, which keep ck_tri_mid -- are what they were.  The counts "before" are the parent's, measured with this toolchain; today's are
recorded in DESIGN 8, round 13."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN5cclqr20rollout_chain_kernelILi%dELi%dELi%dELb%dELi%dELi%dEEEvNS_11RolloutArgsE"
# instantiation -> ds_read_b64 before the change
READS_BEFORE = {
    KERNEL % (32, 17, 0, 0, 1, 32): 511,       # the headline
    KERNEL % (16, 8, 0, 0, 1, 16): 358,        # Sawyer cfg4, bench.py --links 7
}
EIGHT_LANES = KERNEL % (8, 4, 0, 0, 3, 2)      # cartpole cfg2, bench.py --links 1
EIGHT_LANES_INSTRUCTIONS = 6600


@pytest.fixture(scope="module")
def asm_lines(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("isa") / "rollout_chain.s")
    src = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "rollout_chain.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=fast", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", asm, src],
                          stderr=subprocess.DEVNULL)
    return open(asm).read().splitlines()


def _body(lines, name):
    """instruction lines of the kernel"""
    start = [i for i, l in enumerate(lines) if l.startswith(name + ":")][0]
    end = [i for i in range(start, len(lines)) if "s_endpgm" in lines[i]][0]
    return [l for l in (x.strip() for x in lines[start:end]) if l and not l.startswith((";", ".")) and not l.endswith(":")]


def _broadcasts(body):
    return [l for l in body if l.split()[0] == "v_mov_b32_dpp" and "row_newbcast" in l]


@pytest.mark.parametrize("name", list(READS_BEFORE))
def test_middle_block_is_gathered_by_row_broadcasts(asm_lines, name):
    """five columns and the right-hand side, 30 doubles: 60 moves, each lane k's column to every lane of its row"""
    bc = _broadcasts(_body(asm_lines, name))
    print("v_mov_b32_dpp row_newbcast: %d" % len(bc))
    assert len(bc) >= 60, len(bc)
    assert {int(m.group(1)) for l in bc for m in [re.search(r"row_newbcast:(\d+)", l)]} == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("name", list(READS_BEFORE))
def test_middle_solve_reads_are_gone(asm_lines, name):
    """the sixty single reads of ck_tri_mid are gone; the six of the first back step's own operands come in (those of a chain without a sweep step
    are the same six, pointed elsewhere)"""
    n = sum(l.split()[0] == "ds_read_b64" for l in _body(asm_lines, name))
    print("ds_read_b64: %d (before %d)" % (n, READS_BEFORE[name]))
    assert n <= READS_BEFORE[name] - 50, n


def test_eight_lane_kernel_is_what_it_was(asm_lines):
    body = _body(asm_lines, EIGHT_LANES)
    print("instructions: %d" % len(body))
    assert not [l for l in body if "row_newbcast" in l]
    assert len(body) == EIGHT_LANES_INSTRUCTIONS, len(body)
