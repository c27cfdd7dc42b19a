"""The fixed-plan chain kernels (the kernel text of csrc/rollout_chain.hip compiled with CHAIN_PLAN_FIXED: rollout_chain_fixed_kernel<16 | 17, law, relax>) take the chain of
the solve from the constants of PlanFixed<NBP> (cclqr_chain.h) where rollout_chain_kernel reads the plan word.  CPU checks (tests/emu/emu_chain_fixed_plan.cpp,
no GPU): for both kernels and every lane of a wavefront, the balanced two-front plan (TriPlanB), the lane's cursor (TriCur) and its part in the reduction level
(CrLane<4>) that the constants yield are, field for field, those of the run-time functions fed the word of one chain (0, NBP); and the rule that picks the
kernel (cclqr_tables.h rollout_shape_of -> RolloutShape::fixed_plan) says yes for the 15- and 16-link cartpoles only -- not for a 17-body forest of two chains,
a shorter or longer chain, or any tree."""
import ctypes as C

import numpy as np
import pytest

from build_common import host_library


@pytest.fixture(scope="module")
def twin():
    return host_library("libemu_chain_fixed_plan.so", ["emu/emu_chain_fixed_plan.cpp"])


@pytest.mark.parametrize("nbp", [16, 17])
def test_fixed_plan_is_the_runtime_plan_field_for_field(twin, nbp):
    n = twin.emu_plan_words()
    a, b = (C.c_int * n)(), (C.c_int * n)()
    for t in range(64):
        assert twin.emu_fixed_plan(nbp, t, a) == 1
        assert twin.emu_runtime_plan(nbp, 1, 0, nbp, t, b) == 1
        assert list(a) == list(b), (nbp, t, list(a), list(b))
    # the plan the issue's reasoning rests on: reduction level taken, 4 sweep steps, both fronts fold in the last step of 17 links (9 reduced links)
    twin.emu_fixed_plan(nbp, 0, a)
    cs, cn, nA, nB, mid, steps, merge, st = list(a)[:8]
    assert (cs, cn, st, steps) == (0, (nbp + 1) // 2, 2, 4) and a[n - 2] == 1, list(a)
    assert merge == (1 if nbp == 17 else 0) and nA + nB + 1 == cn
    # (a different chain gives a different plan: the comparison above is not vacuous)
    twin.emu_runtime_plan(nbp, 2, 0, 9, 0, b)
    assert list(a) != list(b)
    assert twin.emu_fixed_plan(32, 0, a) == -1


def _shape(twin, orc, t):
    out = (C.c_int * 3)()
    flag = twin.emu_shape_fixed_plan(C.byref(orc.mech_desc(t).desc), out)
    return flag, tuple(out)


def test_only_the_single_full_length_chains_take_the_fixed_kernels(twin, cclqr, orc):
    for n_links, want in ((15, 1), (16, 1), (14, 0), (17, 0), (7, 0), (1, 0)):
        flag, (family, G, nbp) = _shape(twin, orc, cclqr.examples.cartpole_n(n_links)["mech"].tables())
        assert family == 0 and flag == want, (n_links, flag, family, G, nbp)
        if want:
            assert (G, nbp) == (32, n_links + 1)
        # the launcher's choice: the fixed kernels by default and with the other flags, the general kernel with ROLLOUT_RUNTIME_PLAN
        desc = orc.mech_desc(cclqr.examples.cartpole_n(n_links)["mech"].tables())
        capi = cclqr._capi
        for flags in (0, capi.ROLLOUT_PACK_WAVEFRONTS | capi.ROLLOUT_CARRY_STATUS | capi.ROLLOUT_NO_ALLOC):
            assert twin.emu_launch_takes_fixed_plan(C.byref(desc.desc), flags) == want, (n_links, flags)
            assert twin.emu_launch_takes_fixed_plan(C.byref(desc.desc), flags | capi.ROLLOUT_RUNTIME_PLAN) == 0, (n_links, flags)
    # 17 and 16 bodies in TWO chains off the origin: the same kernels' images (32 lanes, 17 / 16 links), the run-time plan
    for sizes in ((9, 8), (8, 8), (16, 1)):
        parents = []
        for s in sizes:
            parents += [-1] + list(range(len(parents), len(parents) + s - 1))
        flag, (family, G, nbp) = _shape(twin, orc, cclqr.examples.tree_mechanism(parents, seed=3)["mech"].tables())
        assert (flag, family, G, nbp) == (0, 0, 32, sum(sizes)), (sizes, flag, family, G, nbp)
    # trees of 16 and 17 bodies (one body with two children)
    for nb in (16, 17):
        parents = [-1] + list(range(nb - 2)) + [3]
        flag, (family, G, nbp) = _shape(twin, orc, cclqr.examples.tree_mechanism(parents, seed=4)["mech"].tables())
        assert family == 1 and flag == 0, (nb, flag, family)
