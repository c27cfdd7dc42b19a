"""The chain kernel hands its LDS image from phase to phase with WAVE_HANDOVER (cclqr_rollout_step.h), not with __syncthreads(): every chain instantiation is a
workgroup of ONE wavefront, for which a barrier already lowered to a bare `s_waitcnt lgkmcnt(0)` -- a drain of the LDS queue in front of the next phase's
first read.  The hand-over is a wavefront-scope fence: no instruction, the reads queue behind the stores.  What this file checks in the ISA (CPU suite: one
gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests): the static count of full drains fell, no barrier came in, the headline kernel kept
its registers.  The counts "before" are the parent's, measured with this toolchain; the counts "today" are recorded in DESIGN 8, round 12."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN5cclqr20rollout_chain_kernelILi%dELi%dELi%dELb%dELi%dELi%dEEEvNS_11RolloutArgsE"
HEADLINE = KERNEL % (32, 17, 0, 0, 1, 32)
# instantiation -> (full drains before the hand-over, full drains today)
DRAINS = {
    HEADLINE: (81, 72),
    KERNEL % (16, 8, 0, 0, 1, 16): (60, 54),       # Sawyer cfg4, bench.py --links 7
    KERNEL % (8, 4, 0, 0, 3, 2): (68, 61),         # cartpole cfg2, bench.py --links 1
}


@pytest.fixture(scope="module")
def asm_lines(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("isa") / "rollout_chain.s")
    src = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "rollout_chain.hip")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=fast", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", asm, src],
                          stderr=subprocess.DEVNULL)
    return open(asm).read().splitlines()


def _kernel(lines, name):
    """(instruction lines of the kernel, the resource comments behind it)"""
    start = [i for i, l in enumerate(lines) if l.startswith(name + ":")][0]
    end = [i for i in range(start, len(lines)) if "s_endpgm" in lines[i]][0]
    body = [l for l in (x.strip() for x in lines[start:end]) if l and not l.startswith((";", ".")) and not l.endswith(":")]
    tail = []
    for l in lines[end:]:
        if l.startswith("_ZN5cclqr"):
            break
        tail.append(l)
    return body, tail


def _chain_kernels(lines):
    return [m.group(1) for l in lines for m in [re.match(r"(_ZN5cclqr20rollout_chain_kernel\w+):", l)] if m]


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
