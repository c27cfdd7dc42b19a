"""The yardstick of the cost-to-go tests (tests/riccati_value_common.py) is well posed: what tests/test_gpu_riccati_value.py asserts on the device cannot pass
vacuously.  CPU only."""
import numpy as np
import pytest
import scipy.linalg as sl

import dlqr_reference as ref
from riccati_value_common import CASES, build_case, case_P, reference_P, sweep_P


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_cost_to_go_cases_are_well_posed(c):
    """per problem: the three runs (longdouble, the two float64 twins) break at one index -- the one the gain reference breaks at --, the twins sit at the
    longdouble run's floor so that the acceptance bound is the suite's rule at its 1e-12 floor, and no problem's P passes for its neighbour's"""
    pr = build_case(c["name"])
    refs = case_P(c["name"])
    print(c["name"], "e64P", [r[2] for r in refs], "max|P|", [float(np.abs(r[0]).max()) for r in refs])
    for p, (P, kb, e64) in enumerate(refs):
        assert kb == pr["ref"][p][1]
        assert e64 < 1e-13 and ref.tolerance(e64) == 1e-12, (p, e64)
        assert np.isfinite(P).all() and not np.array_equal(P, pr["Q"][p])
        q = (p + 1) % c["nprob"]
        assert np.abs(refs[q][0] - P).max() > 1e-3 * np.abs(P).max(), (p, q)


def test_a_nonsymmetric_weight_gives_a_nonsymmetric_cost_to_go():
    refs = case_P("w_nonsym_one")
    P = refs[1][0]
    assert np.abs(P - P.T).max() > 1e-3 * np.abs(P).max()


def test_kept_matrix_follows_the_loop_semantics_of_lqr_jl():
    """N = 1: no step runs, P = Q; tol = inf: the break fires on the first step, whose Pkp1 is kept; tol = 0: step 1's"""
    rng = np.random.default_rng(3)
    A, Bu, Bl, G = ref._model(rng, 8, 2, 3)
    Q, R = ref._spd(rng, 8), ref._spd(rng, 2)
    model = lambda k: (A, Bu, Bl, G)
    _, P, kb, _ = sweep_P(model, Q, R, 1, 1.0, np.float64, ref._step)
    assert kb == 0 and np.array_equal(P, Q)
    one = ref._step(A, Bu, Bl, G, Q, R, Q, np.float64)[1]
    _, P, kb, norms = sweep_P(model, Q, R, 6, np.inf, np.float64, ref._step)
    assert kb == 5 and len(norms) == 1 and np.array_equal(P, one)
    _, P, kb, norms = sweep_P(model, Q, R, 3, 0.0, np.float64, ref._step)
    assert kb == 1 and len(norms) == 2 and np.array_equal(P, ref._step(A, Bu, Bl, G, Q, R, one, np.float64)[1])


def test_yardstick_converges_to_scipy_dare():
    """unconstrained (ml = 0), a small tolerance and a long horizon: the kept Pkp1 is the DARE solution, to the margin of tests/test_oracle.py's DARE test"""
    rng = np.random.default_rng(1)
    n, m = 6, 2
    A = rng.normal(size=(n, n)) * 0.5
    B = rng.normal(size=(n, m))
    Q, R = np.eye(n), np.eye(m)
    P, kb, e64 = reference_P(A, B, np.zeros((n, 0)), np.zeros((0, n)), Q, R, 2000, 1e-13)
    Pd = sl.solve_discrete_are(A, B, Q, R)
    err = float(np.abs(P - Pd).max())
    print("kbreak %d, max|P - P_dare| = %.3g (max|P_dare| %.3g), e64P %.3g" % (kb, err, np.abs(Pd).max(), e64))
    assert 1 < kb < 1999 and err < 1e-10
