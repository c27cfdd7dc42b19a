"""The references of tests/tracking_policy_common.py without a GPU: the backward recursion and its prices are the adjoint of the forward covariance recursion of
tests/tracking_covariance_common.py -- in longdouble, tr(P_0 Σ_0) + sum_j price_j equals the tracked run's summed expected stage costs on every case, sharing and
horizon --, and with one model and one gain the recursion is policy_value_common's.  Neither can pass vacuously: the first ties two independently written
steppings, the second a third.  This file validates the REFERENCE the other tracking-policy tests hold the library to, not the library: it never calls the product
and does not depend on the feature being built (the host and gpu files of the feature do)."""
import numpy as np
import pytest

import policy_value_common as pv
import tracking_covariance_common as tc
import tracking_policy_common as tp

LD = np.longdouble


@pytest.mark.parametrize("name", tp.NAMES)
def test_cost_to_go_and_prices_are_the_adjoint_of_the_covariance(name):
    pr = tp.build_case(name)
    Q, R, S0, Wu = (None if pr[k] is None else np.asarray(pr[k], dtype=LD) for k in ("Q", "R", "Sigma0", "Wu"))
    worst = 0.0
    for tvA, tvK in tp.SHARINGS:
        for p in range(pr["nprob"]):
            S = tc.step_tracking(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["K"][p], Wu, S0, pr["nmax"], tvA, tvK)      # a horizon's Σ_j: the first N of these
            for N in pr["horizons"]:
                r = tp.reference(name, tvA, tvK, N)
                cost = LD(0.0)
                for j in range(N):
                    cost += np.sum(Q * S[j].T)                                                      # tr(Q Σ_j)
                    if j < N - 1:
                        Kj = np.asarray(pr["K"][p][j if tvK else 0], dtype=LD)
                        cost += np.sum(R * (Kj @ S[j] @ Kj.T).T)                                    # tr(R K_j Σ_j K_j')
                dual = np.sum(r["P"][p][0] * S0.T) + np.sum(r["price"][p])                           # tr(P_0 Σ_0) + sum_j price_j
                rel = float(abs(dual - cost) / abs(cost))
                worst = max(worst, rel)
                assert cost > 0 and rel <= 1e-15, (name, tvA, tvK, p, N, float(dual), float(cost), rel)
                assert r["price"][p][N - 1] == 0 and bool(np.all(r["price"][p][:N - 1] > 0)) == (pr["mu"] > 0 or N == 1)      # Wu, P are positive definite
    print("%s: tr(P_0 Σ_0) + sum price against the summed costs: off by at most %.3g relative" % (name, worst))


@pytest.mark.parametrize("name", tp.NAMES)
def test_one_model_and_one_gain_is_the_policy_recursion(name):
    pr = tp.build_case(name)
    for N in pr["horizons"]:
        r = tp.reference(name, False, False, N)
        for p in range(pr["nprob"]):
            P, _, _ = pv.policy_sweep(pr["A"][p][0], pr["Bu"][p][0], pr["Bl"][p][0], pr["G"][p][0], pr["Q"], pr["R"], pr["K"][p][:1], N, 0.0)
            rel = float(np.abs(np.asarray(P, dtype=LD) - r["P"][p][0]).max() / np.abs(r["P"][p][0]).max())
            assert rel <= 1e-17, (name, N, p, rel)


def test_the_cases_are_the_covariance_cases_and_the_mirror_agrees():
    assert tp.CASES is tc.CASES and tp.CASES == ((12, 1, 5), (36, 1, 15), (48, 1, 20), (84, 7, 35), (96, 7, 0), (24, 0, 4), (30, 2, 6), (100, 3, 10)) and tp.NPROB == 3
    assert [tp.horizons_of(n) for n in tp.NAMES] == [(1, 2, 3, 11, 38)] + [(1, 2, 3, 11)] * 7
    assert [tp.paths_of(n) for n in tp.NAMES] == [tc.paths_of(n) for n in tc.NAMES]
