"""The references of tests/tracking_covariance_common.py checked on the CPU, without the product: with one model and one gain the stepping is
covariance_common.step_covariance knot by knot; a rank-one start without noise stays the outer product of the propagated perturbation; total is the sum of the
knots' costs; the builder's asserts hold for every case; and the acceptance rule is met by a plain float64 implementation of the projected form and NOT by one
that applies the gain rows one knot late, so the GPU tests cannot pass vacuously."""
import numpy as np
import pytest

import covariance_common as cc
import tracking_covariance_common as tc

LD = np.longdouble


def _float64_outputs(pr, key, N, p, shift=0):
    """what a straightforward float64 implementation of the projected form returns for problem p; shift: gain row j + shift at knot j (a deliberate indexing error)"""
    run = pr["runs"][key]
    _, tvA, tvK = key
    wu = run["Wu"]
    wp = None if wu is None else (wu[p] if wu.ndim == 3 else wu)
    K = np.roll(pr["K"][p], -shift, axis=0)
    S = tc.step_tracking(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], K, wp, run["Sigma0"], N, tvA, tvK, dtype=np.float64, projected=True)
    mu = pr["mu"]
    cost, zstd, ustd = np.zeros((N, 2)), np.zeros((N, pr["mx"])), np.zeros((N, mu))
    for j in range(N):
        Kj = K[j if tvK and j < N - 1 else 0]
        V = Kj @ S[j] @ Kj.T
        cost[j, 0] = np.sum(pr["Q"] * S[j].T)
        zstd[j] = np.sqrt(np.maximum(np.diag(S[j]), 0.0))
        if j < N - 1:
            cost[j, 1] = np.sum(pr["R"] * V.T)
            ustd[j] = np.sqrt(np.maximum(np.diag(V), 0.0))
    total = [0.0, 0.0]
    for j in range(N):
        total = [total[0] + cost[j, 0], total[1] + cost[j, 1]]
    return S[N - 1], np.stack(S), cost, zstd, ustd, np.array(total)


@pytest.mark.parametrize("name", tc.NAMES)
def test_builder_asserts_hold_and_a_float64_twin_meets_the_rule(name):
    pr = tc.build_case(name)
    assert pr["A"].shape == (tc.NPROB, pr["nmax"] - 1, pr["mx"], pr["mx"]) and pr["K"].shape == (tc.NPROB, pr["nmax"] - 1, pr["mu"], pr["mx"])
    assert (1 in pr["paths"]) == (pr["mx"] % 4 == 0 and pr["mx"] <= 96) and 2 in pr["paths"]
    for key in pr["runs"]:
        for N in pr["horizons"]:
            if key[0] == "nostart" and N == 1:
                continue
            for p in range(pr["nprob"]):
                tc.check_horizon(pr, key, N, p, *_float64_outputs(pr, key, N, p), "%s %s N=%d problem %d" % (name, key, N, p))


def test_gain_rows_one_knot_late_do_not_pass():
    pr = tc.build_case(tc.NAMES[0])
    key = ("full", True, True)
    with pytest.raises(AssertionError):
        tc.check_horizon(pr, key, 11, 0, *_float64_outputs(pr, key, 11, 0, shift=1), "shifted")


@pytest.mark.parametrize("name", (tc.NAMES[0], tc.NAMES[6]))
def test_one_model_and_one_gain_is_the_stationary_stepping(name):
    pr = tc.build_case(name)
    run = pr["runs"][("full", False, False)]
    for p in range(pr["nprob"]):
        Abar, D = tc.closed_loop(pr["A"][p][0], pr["Bu"][p][0], pr["Bl"][p][0], pr["G"][p][0], pr["K"][p][0])
        want = cc.step_covariance(Abar, cc.noise(D, run["Wu"]), np.asarray(run["Sigma0"], dtype=LD), range(pr["nmax"]))
        for j in range(pr["nmax"]):
            assert np.array_equal(run["S"][p][j], want[j][0]), (p, j)


def test_a_rank_one_start_without_noise_stays_rank_one():
    """Σ_j = (M_j δ)(M_j δ)' with M_j = Abar_{j-1} .. Abar_0: two products of mx terms per step in longdouble (eps 1.1e-19), held to 1e-15 of max|Σ_j|"""
    pr = tc.build_case(tc.NAMES[1])
    mx, N = pr["mx"], pr["nmax"]
    d = np.asarray(np.random.default_rng(5).normal(size=mx), dtype=LD)
    for p in range(pr["nprob"]):
        S = tc.step_tracking(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["K"][p], None, np.outer(d, d), N, True, True)
        v = d
        for j in range(N):
            assert float(np.abs(S[j] - np.outer(v, v)).max()) <= 1e-15 * float(np.abs(S[j]).max()), (p, j)
            if j < N - 1:
                v = tc.closed_loop(pr["A"][p][j], pr["Bu"][p][j], pr["Bl"][p][j], pr["G"][p][j], pr["K"][p][j])[0] @ v


def test_total_is_the_sum_of_the_knots_costs_and_the_last_knot_has_no_input():
    pr = tc.build_case(tc.NAMES[0])
    for N in pr["horizons"]:
        recs, _ = tc.records(pr, ("full", True, True), N, 1)
        assert len(recs) == N and recs[-1]["cost"][1] == 0.0 and len(recs[-1]["uvar"]) == 0
        assert all(len(r["uvar"]) == pr["mu"] and r["cost"][1] > 0.0 for r in recs[:-1])
