"""The two-front chain kernels solve the middle link of the block-tridiagonal sweep from registers (ck_tri_mid_regs, cclqr_chain.h): the sixty LDS reads of
the one-lane middle solve (ck_tri_mid) are sixty DPP row broadcasts, and the first back step no longer reads dl of the middle link back.  What this file
checks in the ISA (CPU suite: one gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests): the broadcasts are there, the reads are gone, and the
8-lane kernels -- one front, which keep ck_tri_mid -- are what they were.  The counts "before" are the parent's, measured with this toolchain; today's are
recorded in DESIGN 8, round 13."""
import re

import pytest

from build_common import chain_kernel, device_asm

# instantiation -> ds_read_b64 before the change
READS_BEFORE = {
    chain_kernel(32, 17, 0, 0, 1, 32): 511,       # the headline
    chain_kernel(16, 8, 0, 0, 1, 16): 358,        # Sawyer cfg4, bench.py --links 7
}
EIGHT_LANES = chain_kernel(8, 4, 0, 0, 3, 2)      # cartpole cfg2, bench.py --links 1
EIGHT_LANES_INSTRUCTIONS = 6600


@pytest.fixture(scope="module")
def asm_lines():
    """csrc/rollout_chain.hip cross-compiled for gfx950 (build_common.device_asm: once per test process)"""
    return device_asm("rollout_chain.hip")


def _body(asm, name):
    """instruction lines of the kernel"""
    return asm.kernel(name).body


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
