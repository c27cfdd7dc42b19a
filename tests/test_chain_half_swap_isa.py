"""The 32-lane chain kernels that split the Schur rows exchange values between the two halves of the wavefront by v_permlane32_swap_b32 and form every
group sum a branch waits for by the row swap (rollout_chain.hip halves_pick, group_sum_rows32): the partner's search flag, the trial state of a lone
searcher, the helper's two norms, the step's norm and the two norms of a line-search pass no longer go through the LDS crossbar, where each of them
waited behind a full drain of the LDS queue.  What this file checks in the ISA (CPU suite: one gfx950 cross-compile of csrc/rollout_chain.hip, shared by
the tests): no ds_bpermute is left (the control law's sum, once per step, takes the row swap too), the half swaps are there -- 25 doubles of the trial and two
norms, two dwords each --, and the full drains fell with them.  The bounds are the counts of the build that shipped, recorded in DESIGN 8,
round 23; the parent had 63 ds_bpermute_b32, no half swap, and 71 / 70 drains."""
import re

import pytest

from build_common import HEADLINE, chain_kernel, device_asm

# instantiation -> (ds_bpermute_b32 at most, v_permlane32_swap_b32 at least, s_waitcnt lgkmcnt(0) at most)
SHIPPED = {
    HEADLINE: (0, 54, 59),
    chain_kernel(32, 16, 0, 0, 1, 32): (0, 54, 58),        # bench.py --links 15
}


@pytest.fixture(scope="module")
def asm_lines():
    """csrc/rollout_chain.hip cross-compiled for gfx950 (build_common.device_asm: once per test process)"""
    return device_asm("rollout_chain.hip")


@pytest.mark.parametrize("name", list(SHIPPED))
def test_half_exchanges_leave_the_lds_crossbar(asm_lines, name):
    bperm_max, swaps_min, drains_max = SHIPPED[name]
    body = asm_lines.kernel(name).body
    op = lambda l: l.split()[0]
    bperm = sum(1 for l in body if op(l).startswith("ds_bpermute_b32"))
    swaps = sum(1 for l in body if op(l).startswith("v_permlane32_swap_b32"))
    drains = sum(1 for l in body if op(l) == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", l))
    print("ds_bpermute_b32 %d, v_permlane32_swap_b32 %d, s_waitcnt lgkmcnt(0) %d" % (bperm, swaps, drains))
    assert bperm <= bperm_max, bperm
    assert swaps >= swaps_min, swaps
    assert drains <= drains_max, drains
