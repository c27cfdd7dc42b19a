"""The 32-lane chain kernels of at most 17 links build the Schur rows split by block between a link's lane and the idle lane sixteen above it
(ck_schur_rows_split, cclqr_chain.h; the transfer is rollout_chain.hip schur_split_take): one build issues 63 G_k operand reads and 55 stores where
ck_schur_rows issues 87 and 80, and the link's W reaches the helper lane by v_permlane16_swap_b32 -- a vector-ALU instruction, not a trip through the LDS
crossbar.  What this file checks in the ISA (CPU suite: one gfx950 cross-compile of csrc/rollout_chain.hip, shared by the tests): the reads and stores
fell, the swaps are there, no ds_bpermute came in, and every kernel that keeps ck_schur_rows -- 8 and 16 lanes, 32 lanes with the 32-link image, 64 lanes
-- is instruction for instruction what it was.  The counts and digests "before" are the parent's, measured with this toolchain; today's counts are
recorded in DESIGN 8, round 14."""
import hashlib
import re

import pytest

from build_common import HEADLINE, chain_kernel, device_asm

# instantiation -> (ds_read_b64, LDS store instructions, ds_bpermute_b32) before the split; two builds of the rows per kernel
BEFORE = {
    HEADLINE: (457, 217, 67),
    chain_kernel(32, 16, 0, 0, 1, 32): (454, 217, 67),        # bench.py --links 15: every link has a helper
}
# (lanes, image links, law, relaxed stop, lanes per link, links per sub-group) -> (instructions, first 16 hex digits of the SHA-1 of the instruction
# lines, blanks squeezed, the function number taken out of the branch labels) of the parent's kernel
UNCHANGED = {
    (8, 4, 0, 1, 3, 2): (6604, "e1f91d9ac0506732"), (8, 4, 0, 0, 3, 2): (6600, "cb2d514e43cabee0"), (8, 4, 1, 0, 3, 2): (6770, "7c41d97f5bbbaae6"),
    (8, 4, 2, 0, 3, 2): (7034, "8f7330b56f07ecb7"), (8, 4, 3, 0, 3, 2): (6778, "2cd12819a83c9df8"),
    (8, 4, 0, 1, 1, 8): (7565, "7857cb6ea6368dd5"), (8, 4, 0, 0, 1, 8): (7561, "bd03486206fa14a3"), (8, 4, 1, 0, 1, 8): (7724, "e5f2ff3a61d38f92"),
    (8, 4, 2, 0, 1, 8): (8024, "ba2a1b159755534b"), (8, 4, 3, 0, 1, 8): (7731, "cd85cefb24aaebae"),
    (16, 8, 0, 1, 1, 16): (7957, "9f3a61ee3b5bcef4"), (16, 8, 0, 0, 1, 16): (7946, "e4046621366e6d8c"), (16, 8, 1, 0, 1, 16): (8155, "97ef6b23d7c5b1fb"),
    (16, 8, 2, 0, 1, 16): (8446, "fbbc720e28ca7ce6"), (16, 8, 3, 0, 1, 16): (8124, "1102fb84553a0e68"),
    (32, 32, 0, 1, 1, 32): (7862, "cd2ab0e20c94b886"), (32, 32, 0, 0, 1, 32): (7859, "061c25cb3485d08c"), (32, 32, 1, 0, 1, 32): (8051, "560b1eb074984958"),
    (32, 32, 2, 0, 1, 32): (8359, "6ea92edc8550bf20"), (32, 32, 3, 0, 1, 32): (8065, "1be1caa118717858"),
    (64, 64, 0, 1, 1, 64): (7404, "da6df99766087f39"), (64, 64, 0, 0, 1, 64): (7400, "80756050ca6bf3b3"), (64, 64, 1, 0, 1, 64): (7568, "4760591e034f0924"),
    (64, 64, 2, 0, 1, 64): (7836, "c3d01c574476b422"), (64, 64, 3, 0, 1, 64): (7567, "278f75ac602c39d8"),
}


@pytest.fixture(scope="module")
def asm_lines():
    """csrc/rollout_chain.hip cross-compiled for gfx950 (build_common.device_asm: once per test process)"""
    return device_asm("rollout_chain.hip")


def _body(asm, name):
    """instruction lines of the kernel"""
    return asm.kernel(name).body


def _count(body, pattern):
    return sum(1 for l in body if re.match(pattern, l.split()[0]))


@pytest.mark.parametrize("name", list(BEFORE))
def test_fewer_lds_reads_and_stores(asm_lines, name):
    """24 operand reads fewer per build, two builds; 25 stores fewer per build (the compiler pairs some into ds_write2_b64, so fewer instructions than that)"""
    reads, stores, _ = BEFORE[name]
    body = _body(asm_lines, name)
    r, w = _count(body, r"ds_read_b64$"), _count(body, r"ds_write")
    print("ds_read_b64 %d (before %d), LDS stores %d (before %d)" % (r, reads, w, stores))
    assert r <= reads - 48, r
    assert w < stores, w
    assert _count(body, r"ds_read2") <= 36


@pytest.mark.parametrize("name", list(BEFORE))
def test_w_moves_by_row_swaps_not_through_the_lds_crossbar(asm_lines, name):
    """24 doubles per build, two builds, and the helper's scale once per launch: 98 swaps"""
    body = _body(asm_lines, name)
    swaps, bperm = _count(body, r"v_permlane16_swap_b32"), _count(body, r"ds_bpermute")
    print("v_permlane16_swap_b32 %d, ds_bpermute_b32 %d (before %d)" % (swaps, bperm, BEFORE[name][2]))
    assert swaps >= 96, swaps
    assert bperm <= BEFORE[name][2], bperm


@pytest.mark.parametrize("key", list(UNCHANGED), ids=["-".join(map(str, k)) for k in UNCHANGED])
def test_kernels_that_keep_ck_schur_rows_are_the_parents(asm_lines, key):
    kernel = asm_lines.kernel(chain_kernel(*key))
    body = kernel.body
    assert not [l for l in body if l.split()[0].startswith("v_permlane16_swap")]
    text = kernel.normalised()
    n, digest = UNCHANGED[key]
    assert len(body) == n, len(body)
    assert hashlib.sha1(text.encode()).hexdigest()[:16] == digest
