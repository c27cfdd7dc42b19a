"""The cases of tests/policy_doubling_common.py cannot pass vacuously: the doubling schedule in plain numpy float64 meets the acceptance rule on every case against the
longdouble STEPPING references, in both modes, and makes no more mx^3 products than square-and-multiply allows.  No GPU."""
import numpy as np
import pytest

import dlqr_reference as ref
import policy_doubling_common as pdc


@pytest.mark.parametrize("name", [c["name"] for c in pdc.CASES])
def test_the_float64_doubling_twin_is_within_the_bound(name):
    pr = pdc.build_case(name)
    Q = np.asarray(pr["Q"], dtype=np.float64)
    for p in range(pr["nprob"]):
        Abar, Qbar = pdc.closed_loop(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"], pr["K"], np.float64, True)
        for n in pr["steps"]:
            P, levels, _, gM = pdc.doubling_fixed(Abar, Qbar, Q, n)
            pdc.check_fixed(P, levels, np.array([gM, np.nan]), np.array([np.nan, np.nan]), pr["fixed"][n][p], "%s problem %d, %d steps" % (name, p, n))
        P, levels, reason, incs, gs = pdc.doubling_converge(Abar, Qbar, Q, pr["tol"], pr["max_levels"])
        pdc.check_conv(P, levels, reason, pdc.last_two(incs), pdc.last_two(gs), pr["conv"][p], "%s problem %d to convergence" % (name, p))
        assert ref.tolerance(pr["conv"][p][5]) < 1e-7, "a float64 twin stopped elsewhere than the reference: the case decides nothing"


@pytest.mark.parametrize("n", sorted(set(pdc.ALL_STEPS) | {3, 255, 256, 4096, 2 ** 31 - 2}))
def test_the_schedule_makes_no_more_products_than_square_and_multiply(n):
    """at most 3 ceil(log2 n) + 3 popcount(n) + 2 products of mx^3 (a doubling and an accumulation are three each, the final M' Q M two), and the result is the
    stepping recursion's: checked on a 2 x 2 problem whose powers are exact in float64"""
    Abar = np.array([[0.5, 0.25], [0.0, 0.5]])
    Qbar, Q = np.array([[1.0, 0.5], [0.25, 2.0]]), np.array([[1.0, 0.0], [0.5, 1.0]])
    P, levels, products, _ = pdc.doubling_fixed(Abar, Qbar, Q, n)
    assert levels == max(n.bit_length() - 1, 0)
    assert products <= 3 * (0 if n < 2 else (n - 1).bit_length()) + 3 * bin(n).count("1") + 2
    if n <= 4096:
        S, M = np.zeros((2, 2)), np.eye(2)
        for _ in range(n):
            S, M = Qbar + Abar.T @ S @ Abar, M @ Abar
        assert np.allclose(P, S + M.T @ Q @ M, rtol=1e-13, atol=0.0)
