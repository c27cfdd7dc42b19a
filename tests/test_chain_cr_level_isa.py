"""The solve of the ten fixed-plan chain kernels, rollout_chain_fixed_kernel<16 | 17, law, relax>, without its register detours, in the ISA (CPU suite: the one
gfx950 cross-compile of csrc/rollout_chain.hip that the other tests/test_chain_*_isa.py files share).

  * The reduction level (cclqr_chain.h cr_level_a / cr_level_b) no longer takes the 45 doubles of a pass through accumulation registers on their way to LDS:
    the kernels' v_accvgpr_read_b32 + v_accvgpr_write_b32 fell by 131 .. 184 (the headline kernel <17, 0, false>: 841 -> 710), their instructions by
    115 .. 155.  Pinned as upper bounds, per kernel, at the counts of the build that ships.
  * The middle block is gathered with one 64-bit DPP move per double (rollout_chain.hip ck_tri_mid_regs<true>): no v_mov_b32_dpp row_newbcast is left, and at
    least 30 v_mov_b64_dpp row_newbcast are there.  (The run-time-plan kernels keep the 32-bit form: test_chain_mid_registers_isa.py.)

The limits the fixed kernels share with the headline kernel -- registers, scratch, parked values, full drains -- are those of test_chain_fixed_plan_isa.py."""
import pytest

from build_common import device_asm

FIXED = "_ZN5cclqr26rollout_chain_fixed_kernelILi%dELi%dELb%dEEEvNS_11RolloutArgsE"
# (NBP, law, relax) -> (instructions, v_accvgpr_read_b32 + v_accvgpr_write_b32) of the build that ships
SHIPPED = {
    (16, 0, 1): (8424, 702), (16, 0, 0): (8421, 702), (16, 1, 0): (8607, 753), (16, 2, 0): (8895, 838), (16, 3, 0): (8595, 755),
    (17, 0, 1): (8555, 710), (17, 0, 0): (8552, 710), (17, 1, 0): (8735, 760), (17, 2, 0): (9007, 802), (17, 3, 0): (8759, 796),
}


@pytest.fixture(scope="module")
def asm():
    return device_asm("rollout_chain.hip")


def _bcast(k, op):
    return sum(1 for l in k.body if l.split()[0] == op and "row_newbcast" in l)


@pytest.mark.parametrize("key", list(SHIPPED))
def test_fixed_kernel_keeps_its_moves_down(asm, key):
    k = asm.kernel(FIXED % key)
    acc = k.ops.count("v_accvgpr_read_b32") + k.ops.count("v_accvgpr_write_b32")
    print("instructions %d, accumulation-register moves %d (shipped %s)" % (len(k.body), acc, SHIPPED[key]))
    assert len(k.body) <= SHIPPED[key][0], (len(k.body), SHIPPED[key])
    assert acc <= SHIPPED[key][1], (acc, SHIPPED[key])


@pytest.mark.parametrize("key", list(SHIPPED))
def test_fixed_kernel_gathers_the_middle_block_with_64_bit_broadcasts(asm, key):
    k = asm.kernel(FIXED % key)
    b32, b64 = _bcast(k, "v_mov_b32_dpp"), _bcast(k, "v_mov_b64_dpp")
    print("row_newbcast: v_mov_b32_dpp %d, v_mov_b64_dpp %d" % (b32, b64))
    assert b32 == 0, b32
    assert b64 >= 30, b64
