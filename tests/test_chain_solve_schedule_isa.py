"""Where the compiler puts the LDS reads of the block-tridiagonal solve in the headline kernel rollout_chain_kernel<32, 17, 0, false, 1, 32> (CPU suite: one
gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests of this file).  The solve is a chain of dependent 5 x 5 stages at one wavefront per SIMD:
thirty reads each behind a scalar branch of its own, on the one lane the whole wavefront waits for, were 1.6 % of the headline's time.
The sweep step's reads (tri_step) are where the compiler puts them: dealing them to the pivot stages was measured as no gain."""
import re

import pytest

from build_common import HEADLINE, device_asm



@pytest.fixture(scope="module")
def kernel():
    """(lines of the headline kernel's body, the resource comments that follow it)"""
    k = device_asm("rollout_chain.hip").kernel(HEADLINE)
    return k.raw, k.tail


def _is_op(l):
    l = l.strip()
    return bool(l) and not l.startswith((";", ".")) and not l.endswith(":")


def _ops(body):
    return [l.split()[0] for l in body if _is_op(l)]


def test_few_scalar_branches(kernel):
    """ck_tri_mid read each of its thirty scratch words behind `merge ? ... : 0`, a scalar branch around every read on the one lane the wavefront waits for:
    37 s_cbranch_vccnz in the kernel then, 7 with the unconditional reads and the select behind them.  Bound: today's count + 2 (the parent's - 25 at the most)."""
    body, _ = kernel
    n = sum(o == "s_cbranch_vccnz" for o in _ops(body))
    print("s_cbranch_vccnz:", n)
    assert n <= 9, n
    assert n <= 37 - 25


def test_no_larger_than_before(kernel):
    """the re-placed reads cost neither instructions nor registers: 9 224 instructions and 469 registers (256 + 213 accumulation registers) before, 9 183
    and 456 today"""
    body, tail = kernel
    n = len(_ops(body))
    total = [int(m.group(1)) for l in tail for m in [re.search(r"TotalNumVgprs:\s*(\d+)", l)] if m]
    print("instructions %d, registers %s" % (n, total))
    assert n <= 9224, n
    assert total and total[0] <= 469, total
