"""cclqr_policy_value on the device: every case of tests/policy_value_common.py on every path its shape has against the extended-precision reference and the
acceptance rule stated there (the CPU twin tests/test_policy_value_reference.py shows that the cases cannot pass vacuously), and what the entry point promises besides:
shared and per-problem gains / weights give the same bits, N = 1 returns Q, a non-symmetric problem keeps a non-symmetric P, kbreak = dnorm = NULL changes nothing,
every CCLQR_EINVAL leaves the outputs untouched, and the Riccati's own gains fed back reproduce the Riccati's own cost-to-go, device against device."""
import numpy as np
import pytest

import dlqr_reference as ref
from policy_value_common import CASES, build_case, check, refusal_call, refusal_cases

pytestmark = pytest.mark.gpu

RUNS = [(c["name"], path) for c in CASES for path in c["paths"]]


def _models(pr):
    return pr["A"], pr["Bu"], pr["Bl"], pr["G"]


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_case_against_extended_precision(cclqr, name, path):
    pr = build_case(name)
    P, kb, dn = cclqr._capi.policy_value(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path)
    for p in range(pr["nprob"]):
        check(P[p], kb[p], dn[p], pr["ref"][p], "%s path %d problem %d" % (name, path, p))


@pytest.mark.parametrize("name,path", [("pv_frag_1_6", 1), ("pv_tiled_30", 2), ("pv_stationary", 1), ("pv_stationary", 2)])
def test_shared_and_per_problem_gains_and_weights_give_the_same_bits(cclqr, name, path):
    capi = cclqr._capi
    pr = build_case(name)
    n = pr["nprob"]
    args = dict(tol=pr["tol"], path=path)
    P, kb, dn = capi.policy_value(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["N"], **args)
    Pg, kbg, dng = capi.policy_value(*_models(pr), np.stack([pr["K"]] * n), pr["Q"], pr["R"], pr["N"], **args)
    assert np.array_equal(P, Pg) and np.array_equal(kb, kbg) and np.array_equal(dn, dng, equal_nan=True)
    Pw, kbw, dnw = capi.policy_value(*_models(pr), pr["K"], np.stack([pr["Q"]] * n), np.stack([pr["R"]] * n), pr["N"], **args)
    assert np.array_equal(P, Pw) and np.array_equal(kb, kbw) and np.array_equal(dn, dnw, equal_nan=True)
    # and per-problem arguments are read per problem: a table of zeros for problem 1 alone changes problem 1 alone
    Kz = np.stack([pr["K"]] * n)
    Kz[1] = 0.0
    Pz, _, _ = capi.policy_value(*_models(pr), Kz, pr["Q"], pr["R"], pr["N"], **args)
    assert np.array_equal(Pz[0], P[0]) and not np.array_equal(Pz[1], P[1])


@pytest.mark.parametrize("name,path", [("pv_frag_1_6", 1), ("pv_reg_mu2", 1), ("pv_tiled_30", 2), ("pv_nonsym", 1), ("pv_nonsym", 2)])
def test_a_horizon_of_one_returns_the_weights(cclqr, name, path):
    """N = 1: no backward step runs -- P = Q bitwise, kbreak 0, no norm"""
    pr = build_case(name)
    P, kb, dn = cclqr._capi.policy_value(*_models(pr), pr["K"][:1], pr["Q"], pr["R"], 1, tol=pr["tol"], path=path)
    assert (kb == 0).all() and np.isnan(dn).all() and all(np.array_equal(P[p], pr["Q"]) for p in range(pr["nprob"]))


@pytest.mark.parametrize("path", [1, 2])
def test_a_nonsymmetric_problem_keeps_a_nonsymmetric_cost_to_go(cclqr, path):
    pr = build_case("pv_nonsym")
    P, _, _ = cclqr._capi.policy_value(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path)
    assert all(np.abs(P[p] - P[p].T).max() > 1e-3 * np.abs(P[p]).max() for p in range(pr["nprob"]))


@pytest.mark.parametrize("name,path", [("pv_reg_mu2", 1), ("pv_tiled_30", 2)])
def test_null_kbreak_and_dnorm_give_the_same_cost_to_go(cclqr, name, path):
    pr = build_case(name)
    P, _, _ = cclqr._capi.policy_value(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path)
    P0, kb0, dn0 = cclqr._capi.policy_value(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path, want_diag=False)
    assert kb0 is None and dn0 is None and np.array_equal(P0, P)


def test_every_einval_leaves_the_outputs_untouched(cclqr):
    capi = cclqr._capi
    pr = build_case("pv_reg_mu2")
    call = refusal_call(capi, pr)
    assert call()[0] == capi.OK
    refused = {what: call(**kw) for what, kw in refusal_cases(pr).items()}
    for what, (rc, untouched, msg) in refused.items():
        assert rc == capi.EINVAL and untouched, (what, rc, untouched, msg)


@pytest.mark.parametrize("name,path", [("pv_frag_1_6", 1), ("pv_frag_7_21", 1), ("pv_tiled_30", 2), ("pv_nonsym", 1)])
def test_the_riccati_gains_fed_back_give_the_riccati_cost_to_go(cclqr, name, path):
    """device against device: cclqr_riccati_value on the case's base model with tol = 0, its K through cclqr_policy_value on the same model, weights and N -- the
    policy evaluation of a recursion's own gains is that recursion's cost-to-go, within the rule (the reference here is the Riccati's P, the bound the case's)"""
    capi = cclqr._capi
    pr = build_case(name)
    base = tuple(x[:1] for x in _models(pr))
    K, Pric, kbric = capi.riccati_value(*base, pr["Q"], pr["R"], pr["N"], tol=0.0, path=path)
    P, kb, dn = capi.policy_value(*base, K[0], pr["Q"], pr["R"], pr["N"], tol=0.0, path=path)
    bound = ref.tolerance(pr["ref"][0][3])
    dev = float(np.abs(P[0] - Pric[0]).max() / np.abs(Pric[0]).max())
    print("%s path %d: policy evaluation of the Riccati's own gains vs its P: %.3g relative, bound %.3g" % (name, path, dev, bound))
    assert int(kb[0]) == int(kbric[0]) == 1 and dev <= bound and dn[0, 0] > 0.0
