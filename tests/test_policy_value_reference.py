"""The cases of the policy evaluation (tests/policy_value_common.py) cannot pass vacuously.  CPU only:
  * the float64 twins of every case pass the acceptance rule;
  * with the Riccati cost-to-go of the SAME model substituted, every perturbed problem (p >= 1) fails it: a kernel that evaluated the wrong recursion would be seen;
  * on the model the table was designed on, with tol = 0, the evaluation of the time-varying table IS the Riccati cost-to-go (riccati_value_common.reference_P);
  * pv_unstable holds a problem whose norms grow and one whose norms decay."""
import numpy as np
import pytest

import dlqr_reference as ref
from policy_value_common import CASES, build_case, check, last_two, policy_sweep
from riccati_value_common import reference_P

IDS = [c["name"] for c in CASES]


def _args(pr, p):
    return pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"]


@pytest.mark.parametrize("name", IDS)
def test_float64_twins_pass_the_rule(name):
    pr = build_case(name)
    for p in range(pr["nprob"]):
        for projected in (False, True):
            P, kb, norms = policy_sweep(*_args(pr, p), pr["K"], pr["N"], pr["tol"], np.float64, projected)
            check(P, kb, last_two(norms), pr["ref"][p], "%s problem %d twin %d" % (name, p, projected))


@pytest.mark.parametrize("name", [n for n in IDS if n != "pv_mu0"])
def test_the_riccati_cost_to_go_of_the_same_model_fails_the_rule(name):
    """what predicted_cost used before: the Riccati P of the perturbed model is not the cost of the NOMINAL gains on it (>= 1e-4 relative here, bounds <= 1e-12);
    on problem 0 -- the table's own model -- the time-varying tables agree with it to rounding.  (pv_mu0 has no gain: both recursions are the same.)"""
    pr = build_case(name)
    for p in range(pr["nprob"]):
        Pref, kb, dn, e64, _ = pr["ref"][p]
        Pric = reference_P(*_args(pr, p), pr["N"], 0.0)[0]
        dev = float(np.abs(Pric - Pref).max() / np.abs(Pref).max())
        print("%s problem %d: Riccati P of the same model differs by %.3g relative (bound %.3g)" % (name, p, dev, ref.tolerance(e64)))
        if p >= 1:
            assert dev > 1e-4
            with pytest.raises(AssertionError):
                check(Pric, kb, None, pr["ref"][p], "%s problem %d, Riccati P substituted" % (name, p))


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["nK"] > 1])
def test_own_table_on_own_model_is_the_riccati_cost_to_go(name):
    pr = build_case(name)
    Pric, kbric, _ = reference_P(*_args(pr, 0), pr["N"], 0.0)
    P, kb, _ = policy_sweep(*_args(pr, 0), pr["Kfull"], pr["N"], 0.0, np.longdouble)
    dev = float(np.abs(P.astype(np.float64) - Pric).max() / np.abs(Pric).max())
    print("%s: policy evaluation of the own table vs Riccati P: %.3g relative" % (name, dev))
    assert kb == kbric == 1 and dev <= 1e-13      # (the table is a float64 dlqr: it is the longdouble run's gain to ~1e-15, and P is stationary in the gain to first order)


def test_unstable_case_has_a_growing_and_a_decaying_problem():
    pr = build_case("pv_unstable")
    n0, n2 = pr["ref"][0][4], pr["ref"][2][4]
    assert n0[-1] < pr["tol"] and all(b < a for a, b in zip(n0[-6:], n0[-5:])), n0[-6:]
    # problem 2: the nominal gain leaves a complex pair outside the unit circle, so the norms grow along an oscillation -- by thirds of the sweep, not step by step
    third = len(n2) // 3
    peaks = [max(n2[i * third:(i + 1) * third]) for i in range(3)]
    assert pr["ref"][2][1] == 1 and len(n2) == pr["N"] - 1 and peaks[0] < peaks[1] < peaks[2] and n2[-1] > 10 * n2[0], (peaks, n2[0], n2[-1])
    A, Bu, Bl, G = pr["A"][2], pr["Bu"][2], pr["Bl"][2], pr["G"][2]
    Abar = A - Bu @ pr["K"][0]
    Abar = Abar - Bl @ np.linalg.solve(G @ Bl, G @ Abar)
    rho = float(np.abs(np.linalg.eigvals(Abar)).max())
    print("pv_unstable problem 2: closed-loop spectral radius %.4f, contraction estimate of the last two norms %.4f" % (rho, float(np.sqrt(n2[-1] / n2[-2]))))
    assert rho > 1.0
    # problem 1 is stable but slow: it never meets the tolerance, which is an answer (kbreak 1, last norm above tol), not an error
    assert pr["ref"][1][1] == 1 and pr["ref"][1][4][-1] > pr["tol"]
