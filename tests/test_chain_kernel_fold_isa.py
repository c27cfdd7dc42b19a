"""ISA of the headline kernel rollout_chain_kernel<32, 17, 0, false, 1, 32> after the Newton loop's fold (CPU suite: one gfx950 cross-compile of
csrc/rollout_chain.hip, shared by the tests of this file).  Until the fold the kernel carried THREE inlined copies of chain_eval<G, true> (residual,
Jacobians, Schur rows: about 1.8 k instructions each): in front of the loop, as the full-step trial, and at the bottom of the loop body.  The first and
the third did the same job and are one call now."""
import pytest

from build_common import HEADLINE, device_asm



@pytest.fixture(scope="module")
def asm_lines():
    """csrc/rollout_chain.hip cross-compiled for gfx950 (build_common.device_asm: once per test process)"""
    return device_asm("rollout_chain.hip")


def _ops(asm, name):
    return asm.kernel(name).ops


def test_headline_kernel_has_two_copies_of_the_evaluation(asm_lines):
    """9 224 instructions today (10 789 with three copies; 9 031 right after the fold, the rest is the single LDS reads); the bound is today's count + 1 %,
    the margin of test_host.py's budget test.  A third copy of the evaluation (+ 1.8 k) cannot hide under it."""
    ops = _ops(asm_lines, HEADLINE)
    assert len(ops) <= 9316, len(ops)


def test_no_flat_instruction_in_any_chain_kernel(asm_lines):
    """the single-read accessor of the solve phases (cclqr_chain.h LDS_RD) is a volatile read through a pointer typed to the LDS address space; volatile on a
    generic pointer would make every such read a flat load (address-space test + the memory pipeline).  No chain instantiation has one."""
    names = asm_lines.kernel_names("_ZN5cclqr20rollout_chain_kernel")
    assert names and HEADLINE in names
    for n in names:
        flat = [o for o in _ops(asm_lines, n) if o.startswith("flat_")]
        assert not flat, (n, flat[:3])


def test_single_lds_reads_outnumber_the_paired_ones(asm_lines):
    """CDNA4 executes a ds_read2_b64 at half the rate of two ds_read_b64; the solve phases and the Schur rows' operands read through LDS_RD
    (cclqr_chain.h).  Headline kernel today: 465 ds_read_b64, 58 ds_read2_b64 (122 / 279 before)."""
    ops = _ops(asm_lines, HEADLINE)
    single, paired = sum(o == "ds_read_b64" for o in ops), sum(o == "ds_read2_b64" for o in ops)
    assert single > paired, (single, paired)
