"""The ten fixed-plan chain kernels, rollout_chain_fixed_kernel<16 | 17, law, relax> (the kernel text of csrc/rollout_chain.hip compiled with CHAIN_PLAN_FIXED; the N-link
cartpoles of bench.py's headline and --links 15), in the ISA (CPU suite: the one gfx950 cross-compile of csrc/rollout_chain.hip that the other
tests/test_chain_*_isa.py files share).  Each of them

  * exists, next to its run-time-plan counterpart rollout_chain_kernel<32, NBP, law, relax, 1, 32>;
  * keeps the headline kernel's limits: at most 456 registers and no scratch (test_chain_handover_isa.py), at most 8 values the allocator parks after its
    first pass (test_host.py test_chain_rollout_kernel_resources), no s_barrier, no ds_bpermute_b32, at most 59 s_waitcnt lgkmcnt(0)
    (test_chain_half_swap_isa.py), no static LDS (the launch gives it the same dynamic size: four workgroups per CU);
  * has strictly fewer instructions, s_cselect_*, s_bfe_u32 and v_readlane_b32 than the counterpart: the plan is no longer derived from the plan word;
  * stays within the counts of the build that shipped, as upper bounds."""
import re

import pytest

from build_common import chain_kernel, device_asm

FIXED = "_ZN5cclqr26rollout_chain_fixed_kernelILi%dELi%dELb%dEEEvNS_11RolloutArgsE"
# (NBP, law, relax) -> (instructions, s_cselect_*, s_bfe_u32, v_readlane_b32) of the build that shipped
SHIPPED = {
    (16, 0, 1): (8550, 20, 0, 0), (16, 0, 0): (8547, 20, 0, 0), (16, 1, 0): (8735, 23, 0, 0), (16, 2, 0): (9025, 26, 0, 0), (16, 3, 0): (8750, 21, 0, 0),
    (17, 0, 1): (8673, 21, 0, 0), (17, 0, 0): (8670, 21, 0, 0), (17, 1, 0): (8873, 24, 0, 0), (17, 2, 0): (9150, 27, 0, 0), (17, 3, 0): (8874, 22, 0, 0),
}


@pytest.fixture(scope="module")
def asm():
    return device_asm("rollout_chain.hip")


def _counts(k):
    ops = k.ops
    return (len(k.body), sum(o.startswith("s_cselect_") for o in ops), ops.count("s_bfe_u32"), ops.count("v_readlane_b32"))


def test_the_ten_fixed_kernels_exist(asm):
    names = asm.kernel_names("_ZN5cclqr26rollout_chain_fixed_kernel")
    assert sorted(names) == sorted(FIXED % key for key in SHIPPED), names


@pytest.mark.parametrize("key", list(SHIPPED))
def test_fixed_kernel_keeps_the_headline_limits(asm, key):
    k = asm.kernel(FIXED % key)
    r = k.resources
    total = [int(m.group(1)) for l in k.tail for m in [re.search(r"TotalNumVgprs:\s*(\d+)", l)] if m]
    scratch = [int(m.group(1)) for l in k.tail for m in [re.search(r"ScratchSize:\s*(\d+)", l)] if m]
    drains = sum(1 for l in k.body if l.split()[0] == "s_waitcnt" and re.search(r"lgkmcnt\(0\)", l))
    print("registers %s (metadata %d), scratch %s, parked values %d, scalar spills %d, full drains %d" % (total, r["vgpr"], scratch, r["vgpr_spill"], r["sgpr_spill"], drains))
    assert total and total[0] <= 456 and r["vgpr"] <= 456, (total, r)
    assert scratch and scratch[0] == 0 and r["scratch"] == 0, (scratch, r)
    assert r["vgpr_spill"] <= 8, r
    assert r["lds"] == 0 and r["lds"] == asm.kernel(chain_kernel(32, key[0], key[1], key[2], 1, 32)).resources["lds"], r
    assert not [o for o in k.ops if o == "s_barrier" or o.startswith("ds_bpermute_b32")]
    assert drains <= 59, drains


@pytest.mark.parametrize("key", list(SHIPPED))
def test_fixed_kernel_derives_no_plan(asm, key):
    fixed = _counts(asm.kernel(FIXED % key))
    runtime = _counts(asm.kernel(chain_kernel(32, key[0], key[1], key[2], 1, 32)))
    print("instructions, s_cselect, s_bfe_u32, v_readlane_b32: fixed %s, run-time plan %s, shipped %s" % (fixed, runtime, SHIPPED[key]))
    for f, r, s in zip(fixed, runtime, SHIPPED[key]):
        assert f < r, (fixed, runtime)
        assert f <= s, (fixed, SHIPPED[key])
