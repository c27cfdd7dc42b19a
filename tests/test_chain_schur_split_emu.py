"""The Schur rows split by block between a link's lane and the idle lane sixteen above it (cclqr_chain.h ck_schur_rows_split; the 32-lane chain kernels of at
most 17 links) must give the blocks of ck_schur_rows BIT FOR BIT: every sum keeps its order, the helper's - sxb and its - 0 addend are exact, lane 0 of a
17-link group builds its child-side block in the parent-side slot with wPB in wPA's place.  tests/emu/emu_schur_split.cpp runs both forms on the CPU, all 32
lanes, from the same random W and G_k into LDS images poisoned with signalling NaNs; the two images must be the same words everywhere -- so a block that one
form writes and the other does not, or a word read before it is written, shows.  CPU suite."""
import ctypes as C

import numpy as np
import pytest

from build_common import host_library

# (chains of the forest in link order, links the image is laid out for)
CASES = {
    "chain17": ([17], 17),                # link 0 without a helper, the leaf on lane 16
    "chain16": ([16], 16),                # every link has a helper
    "chain12": ([12], 16),                # lanes 12 .. 15 and their helpers idle
    "forest_1_11": ([1, 11], 16),         # a one-link chain: a root without a child, then a root with a helper
    "forest_9_8": ([9, 8], 17),           # 17 links in two chains: the second root (link 9) has a helper, link 0 none
    "forest_1_16": ([1, 16], 17),         # link 0 a one-link chain: lane 0 builds no child-side block
}


@pytest.fixture(scope="module")
def lib():
    return host_library("libemu_schur_split.so", ["emu/emu_schur_split.cpp"], compiler="/opt/rocm/lib/llvm/bin/clang++",
                        flags=("-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I/opt/rocm/include"))


def _run(lib, chains, nbp, seed, zeros):
    lay = (C.c_int * 6)()
    lib.emu_schur_split_layout(C.c_int(nbp), lay)
    total = lay[5]
    ref, split = np.zeros(total), np.zeros(total)
    dp = C.POINTER(C.c_double)
    n = lib.emu_schur_split_case((C.c_int * len(chains))(*chains), C.c_int(len(chains)), C.c_int(nbp), C.c_uint64(seed), C.c_int(zeros),
                                 ref.ctypes.data_as(dp), split.ctypes.data_as(dp), C.c_int(total))
    assert n == total, n
    return list(lay), ref, split


@pytest.mark.parametrize("zeros", [0, 1], ids=["dense", "exact_zeros"])
@pytest.mark.parametrize("case", list(CASES))
def test_split_rows_are_the_rows_of_ck_schur_rows_bit_for_bit(lib, case, zeros):
    chains, nbp = CASES[case]
    nb = sum(chains)
    for seed in range(1, 9):
        (SJJ, SJP, SPJ, R, GKA, total), ref, split = _run(lib, chains, nbp, seed, zeros)
        a, b = ref.view(np.uint64), split.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (case, seed, bad[:8], ref[bad[:8]], split[bad[:8]])
        # what must have been written has been, from words that were written: no NaN in a block that exists
        first = np.zeros(nb, dtype=bool)
        first[np.cumsum([0] + chains[:-1])] = True
        last = np.zeros(nb, dtype=bool)
        last[np.cumsum(chains) - 1] = True
        for j in range(nb):
            assert np.isfinite(split[SJJ + 25 * j:SJJ + 25 * j + 25]).all(), (case, seed, j)
            assert np.isfinite(split[R + 5 * j:R + 5 * j + 5]).all(), (case, seed, j)
            assert np.isfinite(split[SJP + 25 * j:SJP + 25 * j + 25]).all() == (not first[j]), (case, seed, j)
            if not last[j]:
                assert np.isfinite(split[SPJ + 25 * (j + 1):SPJ + 25 * (j + 1) + 25]).all(), (case, seed, j)
        # ... and nothing else: the blocks of links that do not exist are still the poison
        for j in range(nb, nbp):
            assert np.isnan(split[SJJ + 25 * j:SJJ + 25 * j + 25]).all() and np.isnan(split[SPJ + 25 * j:SPJ + 25 * j + 25]).all(), (case, seed, j)


def test_exact_zero_inputs_reach_the_signed_zero_sums(lib):
    """the case the - 0 addend exists for: with exact zeros among the inputs some child-side entries are - 0, which + 0.0 would turn into + 0"""
    seen = 0
    for seed in range(1, 9):
        (SJJ, SJP, SPJ, R, GKA, total), ref, split = _run(lib, [16], 16, seed, 1)
        blk = ref[SPJ + 25:SPJ + 25 * 16]
        seen += int(np.count_nonzero((blk == 0.0) & np.signbit(blk)))
    assert seen > 0
