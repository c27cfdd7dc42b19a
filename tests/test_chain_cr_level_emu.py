"""The reduction level as the fixed-plan chain kernels run it (cclqr_chain.h cr_level_a / cr_level_b: columns of its own for each pass, no fence between a
pass's arithmetic and its stores, z of pass B read back from LDS through cr_phase_b<W, true>) must leave the LDS image of today's cr_phase_a / cr_store_a /
cr_phase_b / cr_store_b BIT FOR BIT: every change is a reload of a value just stored or a different home for a temporary, no sum changes its operands or
their order.  tests/emu/emu_cr_level.cpp runs both forms on the CPU, all 32 lanes, on the same random block-tridiagonal system in images poisoned with
signalling NaNs, and poisons the new form's K.z and pass-A columns between the passes; the two images must be the same words everywhere.  CPU suite."""
import ctypes as C

import numpy as np
import pytest

from build_common import host_library

# (links of the chain, links the image is laid out for)
CASES = {
    "chain17": (17, 17),      # every odd link has a next link
    "chain16": (16, 16),      # the last odd link has none: its Z+ slots are not in use, pass B sits out on its lanes
    "chain13": (13, 16),      # six odd links: lanes 24 .. 31 take no part
    "chain12": (12, 16),      # the shortest chain that takes the level
}


@pytest.fixture(scope="module")
def lib():
    return host_library("libemu_cr_level.so", ["emu/emu_cr_level.cpp"], compiler="/opt/rocm/lib/llvm/bin/clang++",
                        flags=("-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I/opt/rocm/include"))


def _run(lib, cn, nbp, seed, zeros, skip):
    lay = (C.c_int * 6)()
    lib.emu_cr_level_layout(C.c_int(nbp), lay)
    total = lay[5]
    ref, neu, start = np.zeros(total), np.zeros(total), np.zeros(total)
    dp = C.POINTER(C.c_double)
    n = lib.emu_cr_level_case(C.c_int(cn), C.c_int(nbp), C.c_uint64(seed), C.c_int(zeros), C.c_int(skip),
                              ref.ctypes.data_as(dp), neu.ctypes.data_as(dp), start.ctypes.data_as(dp), C.c_int(total))
    assert n == total, n
    return list(lay), ref, neu, start


@pytest.mark.parametrize("zeros", [0, 1], ids=["dense", "exact_zeros"])
@pytest.mark.parametrize("case", list(CASES))
def test_fixed_plan_level_leaves_the_image_of_todays_phases_bit_for_bit(lib, case, zeros):
    cn, nbp = CASES[case]
    for seed in range(1, 9):
        (SJJ, SJP, SPJ, R, DL, total), ref, neu, start = _run(lib, cn, nbp, seed, zeros, 0)
        a, b, s = ref.view(np.uint64), neu.view(np.uint64), start.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (case, seed, bad[:8], ref[bad[:8]], neu[bad[:8]])
        # the level did its work, from words that had been written: every odd link's solutions and every even link's updates are finite and new
        for l in range(1, cn, 2):
            has_n = l + 1 < cn
            for o, n in ((SJP + 25 * l, 25), (R + 5 * l, 5)) + (((SPJ + 25 * (l + 1), 25),) if has_n else ()):
                assert np.isfinite(neu[o:o + n]).all() and (b[o:o + n] != s[o:o + n]).any(), (case, seed, l, o)
            for p in (l - 1,) + ((l + 1,) if has_n else ()):
                assert np.isfinite(neu[SJJ + 25 * p:SJJ + 25 * p + 25]).all() and (b[SJJ + 25 * p:SJJ + 25 * p + 25] != s[SJJ + 25 * p:SJJ + 25 * p + 25]).any(), (case, seed, p)
                assert np.isfinite(neu[R + 5 * p:R + 5 * p + 5]).all(), (case, seed, p)
        # ... and nothing else: S_ll of the odd links, the multiplier step and the blocks of links that do not exist are what they were
        for l in range(1, cn, 2):
            assert (b[SJJ + 25 * l:SJJ + 25 * l + 25] == s[SJJ + 25 * l:SJJ + 25 * l + 25]).all(), (case, seed, l)
        assert (b[DL:DL + 5 * nbp] == s[DL:DL + 5 * nbp]).all()
        for j in range(cn, nbp):
            assert np.isnan(neu[SJJ + 25 * j:SJJ + 25 * j + 25]).all() and np.isnan(neu[R + 5 * j:R + 5 * j + 5]).all(), (case, seed, j)


@pytest.mark.parametrize("case", ["chain17", "chain16"])
def test_a_done_instance_touches_nothing(lib, case):
    """skip: the instance has converged and no lane takes part -- neither form reads or writes a word"""
    cn, nbp = CASES[case]
    for zeros in (0, 1):
        _, ref, neu, start = _run(lib, cn, nbp, 3, zeros, 1)
        assert (ref.view(np.uint64) == start.view(np.uint64)).all() and (neu.view(np.uint64) == start.view(np.uint64)).all()


def test_exact_zero_inputs_reach_the_stored_columns(lib):
    """with exact zeros among the inputs some stored words are exact zeros: the case in which a reload that dropped a sign or a fill column's 0 * old would show"""
    seen = 0
    for seed in range(1, 9):
        (SJJ, SJP, SPJ, R, DL, total), ref, neu, start = _run(lib, 17, 17, seed, 1, 0)
        seen += int(np.count_nonzero(neu[SJP:SJP + 25 * 17] == 0.0))
    assert seen > 0
