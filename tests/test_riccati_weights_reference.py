"""The cases of the per-problem-weights Riccati (tests/riccati_weights_common.py) are well posed: what tests/test_gpu_riccati_weights.py asserts on the device
cannot pass vacuously.  CPU only."""
import numpy as np
import pytest

import dlqr_reference as ref
from riccati_weights_common import CASES, build_case


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_weight_cases_are_well_posed(c):
    """choose_tol placed the break (build_case asserts that no float64 or longdouble norm of any problem lies within 1e-6 of tol); the fp64 twins sit at the
    reference's floor; the problems of a case do not all break at one index; and every problem's gains under its NEIGHBOUR's weights differ from its own by more than
    1e-3 relative -- a kernel that read another problem's weights misses the gain bound (<= 1e-7) by four orders of magnitude at the least"""
    pr = build_case(c["name"])
    nprob, N = c["nprob"], c["N"]
    kbs = [r[1] for r in pr["ref"]]
    print(c["name"], "kbreak", kbs, "e64", [r[3] for r in pr["ref"]], "tol", pr["tol"])
    assert pr["tol"] > 0 and 1 < kbs[0] < N - 1
    assert len(set(kbs)) > 1, kbs
    for p, (Kref, kb, norms, e64) in enumerate(pr["ref"]):
        assert e64 < 1e-12 and ref.tolerance(e64) <= 1e-7
        if c["mu"] == 0:
            continue
        q = (p + 1) % nprob
        model = (pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p])
        own = ref.dlqr_projected64(*model, pr["Q"][p], pr["R"][p], N, pr["tol"])[0]
        swapped = ref.dlqr_projected64(*model, pr["Q"][q], pr["R"][q], N, pr["tol"])[0]
        sens = float(np.abs(swapped - own).max() / np.abs(own).max())
        print(c["name"], "problem", p, "swap sensitivity", sens)
        assert sens > 1e-3, (p, sens)


def test_weight_cases_reach_the_kernels_that_read_the_weights():
    """through the mirror of launch_riccati's choice (dlqr_reference.riccati_kernels): the register-fragment forms <1,3> <1,6> <7,21>, the generic register form
    <2,0>, the LDS-LU form <0,0> (mu 8 and mu 0), the tiled three-launch step with edge tiles, and -- one asymmetric Q in the batch -- the general <1,0>"""
    seen = set()
    for c in CASES:
        for path in c["paths"]:
            seen |= ref.riccati_kernels(c["mx"], c["mu"], c["ml"], c["nprob"], path, symmetric=not c["nonsym"])
    want = {"riccati_resident_kernel<1, 3, 0>", "riccati_resident_kernel<1, 6, 0>", "riccati_resident_kernel<7, 21, 0>", "riccati_resident_kernel<2, 0, 0>",
            "riccati_resident_kernel<0, 0, 0>", "riccati_resident_kernel<1, 0, 0>", "ric_project_kernel<true>", "ric_pa_kernel", "ric_gain_update_kernel",
            "ric_pn_kernel", "ric_backfill_kernel"}
    assert want <= seen, sorted(want - seen)
    tiled_only = [c for c in CASES if c["paths"] == (0, 2)]
    assert tiled_only and all(ref.ric_use_tiled(c["mx"], c["mu"], c["nprob"], 1) and c["mx"] % 32 for c in tiled_only)
    assert all(not ref.ric_use_tiled(c["mx"], c["mu"], c["nprob"], 1) for c in CASES if c["paths"] == (0, 1, 2))
    # the asymmetric problem is not the first one: the batch rule (ric_p_rows_batch) must look past problem 0
    assert [c["nonsym"] for c in CASES if c["nonsym"]] == [(1,)]
