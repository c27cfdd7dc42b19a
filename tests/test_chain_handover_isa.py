"""The chain kernel hands its LDS image from phase to phase with WAVE_HANDOVER (cclqr_rollout_step.h), not with __syncthreads(): every chain instantiation is a
workgroup of ONE wavefront, for which a barrier already lowered to a bare `s_waitcnt lgkmcnt(0)` -- a drain of the LDS queue in front of the next phase's
first read.  The hand-over is a wavefront-scope fence: no instruction, the reads queue behind the stores.  What this file checks in the ISA (CPU suite: one
gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests): the static count of full drains fell, no barrier came in, the headline kernel kept
its registers.  The counts "before" are the parent's, measured with this toolchain; the counts "today" are recorded in DESIGN 8, round 12."""
import re

import pytest

from build_common import HEADLINE, chain_kernel, device_asm

# instantiation -> (full drains before the hand-over, full drains today)
DRAINS = {
    HEADLINE: (81, 72),
    chain_kernel(16, 8, 0, 0, 1, 16): (60, 54),       # Sawyer cfg4, bench.py --links 7
    chain_kernel(8, 4, 0, 0, 3, 2): (68, 61),         # cartpole cfg2, bench.py --links 1
}


@pytest.fixture(scope="module")
def asm_lines():
    """csrc/rollout_chain.hip cross-compiled for gfx950 (build_common.device_asm: once per test process)"""
    return device_asm("rollout_chain.hip")


def _kernel(asm, name):
    """(instruction lines of the kernel, the resource comments behind it)"""
    k = asm.kernel(name)
    return k.body, k.tail


def _chain_kernels(asm):
    return asm.kernel_names("_ZN5cclqr20rollout_chain_kernel")


def _full_drains(body):
    """s_waitcnt instructions whose lgkmcnt operand is 0"""
    return sum(1 for l in body if l.split()[0] == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", l))


@pytest.mark.parametrize("name", list(DRAINS))
def test_fewer_full_drains_of_the_lds_queue(asm_lines, name):
    before, today = DRAINS[name]
    body, _ = _kernel(asm_lines, name)
    n = _full_drains(body)
    print("s_waitcnt lgkmcnt(0): %d (before %d)" % (n, before))
    assert n < before, n
    assert n <= today, n


def test_no_barrier_in_any_chain_kernel(asm_lines):
    names = _chain_kernels(asm_lines)
    assert names and all(k in names for k in DRAINS)
    for name in names:
        body, _ = _kernel(asm_lines, name)
        assert not [l for l in body if l.split()[0] == "s_barrier"], name


def test_headline_kernel_keeps_its_registers(asm_lines):
    """456 registers (256 + 200 accumulation registers), no scratch: one wavefront per SIMD either way, but a spill would put memory traffic in the solve"""
    _, tail = _kernel(asm_lines, HEADLINE)
    total = [int(m.group(1)) for l in tail for m in [re.search(r"TotalNumVgprs:\s*(\d+)", l)] if m]
    scratch = [int(m.group(1)) for l in tail for m in [re.search(r"ScratchSize:\s*(\d+)", l)] if m]
    print("registers %s, scratch %s" % (total, scratch))
    assert total and total[0] <= 456, total
    assert scratch and scratch[0] == 0, scratch
