"""cclqr_riccati_value on the device: the cost-to-go of every Riccati kernel against the extended-precision reference (tests/riccati_value_common.py; the CPU twin
tests/test_riccati_value_reference.py shows that the cases cannot pass vacuously).  Each case of riccati_weights_common.CASES runs on every path its shape has:
  * per problem, max|P - Pref| <= tolerance(e64P) max|Pref|;
  * K and kbreak bitwise those of cclqr_riccati_weights on the same arguments -- emitting P changes nothing else -- also with keep_last, and with P = NULL;
  * N = 1 gives P = Q bitwise, a non-symmetric problem's P is not symmetric, the time-varying call is checked against dlqr_tv on a resident and a tiled shape,
    the bf16 measured-error mode gives a finite P and is compared only with itself."""
import numpy as np
import pytest

import dlqr_reference as ref
from riccati_value_common import CASES, build_case, case_P, check_P, reference_P

pytestmark = pytest.mark.gpu


def _models(pr):
    return pr["A"], pr["Bu"], pr["Bl"], pr["G"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_cost_to_go_against_extended_precision_and_gains_unchanged(cclqr, c):
    capi = cclqr._capi
    pr = build_case(c["name"])
    refs = case_P(c["name"])
    N, tol, nprob = pr["N"], pr["tol"], pr["nprob"]
    for path in c["paths"]:
        what = "%s path %d" % (c["name"], path)
        K, P, kb = capi.riccati_value(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path)
        Kw, kbw = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path)
        assert np.array_equal(kb, kbw) and np.array_equal(K, Kw), "%s: K / kbreak differ from cclqr_riccati_weights" % what
        for p in range(nprob):
            assert int(kb[p]) == refs[p][1], "%s problem %d: kbreak %d, reference %d" % (what, p, kb[p], refs[p][1])
            check_P(P[p], refs[p], "%s problem %d" % (what, p))
        Kl, Pl, kbl = capi.riccati_value(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path, keep_last=True)
        Kwl, kbwl = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path, keep_last=True)
        assert np.array_equal(kbl, kbwl) and np.array_equal(Kl, Kwl) and np.array_equal(Pl, P), "%s: keep_last" % what
        K0, P0, kb0 = capi.riccati_value(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path, want_P=False)
        assert P0 is None and np.array_equal(kb0, kbw) and np.array_equal(K0, Kw), "%s: P = NULL" % what


@pytest.mark.parametrize("name,path", [("w_frag_1_6", 1), ("w_reg_mu2", 1), ("w_tiled_30", 2), ("w_nonsym_one", 1), ("w_nonsym_one", 2)])
def test_a_horizon_of_one_returns_the_weights(cclqr, name, path):
    """N = 1: no backward step runs (kbreak 0, no gains) and the cost-to-go is Q_p, bitwise"""
    pr = build_case(name)
    K, P, kb = cclqr._capi.riccati_value(*_models(pr), pr["Q"], pr["R"], 1, tol=pr["tol"], path=path)
    assert K.shape[1] == 0 and (kb == 0).all() and np.array_equal(P, pr["Q"])


@pytest.mark.parametrize("path", [1, 2])
def test_a_nonsymmetric_problem_keeps_a_nonsymmetric_cost_to_go(cclqr, path):
    pr = build_case("w_nonsym_one")
    _, P, _ = cclqr._capi.riccati_value(*_models(pr), pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path)
    assert np.abs(P[1] - P[1].T).max() > 1e-3 * np.abs(P[1]).max()


@pytest.mark.parametrize("mx,mu,ml,path", [(24, 1, 10, 1), (30, 3, 10, 2)], ids=["resident", "tiled"])
def test_time_varying_cost_to_go_against_dlqr_tv(cclqr, mx, mu, ml, path):
    """per-knot models (lqr_tracking.jl:73-122) through cclqr_riccati_value: P against the wrapped dlqr_tv sweep, K and kbreak against the gain reference;
    on the automatic path K and kbreak are bitwise cclqr_riccati_tv's"""
    capi = cclqr._capi
    pr = ref.make_problem(np.random.default_rng(100 + mx), mx, mu, ml, N=10, tv=True)
    args = (pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"])
    Pref = reference_P(*args, pr["tol"], tv=True)
    K, P, kb = capi.riccati_value(*args, tol=pr["tol"], path=path, time_varying=True)
    Kref, kbref, _, e64 = pr["ref"][0]
    assert int(kb[0]) == kbref == Pref[1]
    assert np.abs(K[0] - Kref).max() <= ref.tolerance(e64) * np.abs(Kref).max()
    check_P(P[0], Pref, "tv mx %d path %d" % (mx, path))
    K0, P0, kb0 = capi.riccati_value(*args, tol=pr["tol"], time_varying=True)
    Kt, kbt = capi.riccati_tv(*args, tol=pr["tol"])
    assert int(kb0[0]) == kbt and np.array_equal(K0[0], Kt)
    check_P(P0[0], Pref, "tv mx %d automatic path" % mx)


@pytest.mark.parametrize("path", [1, 2])
def test_bf16_mode_emits_the_cost_to_go_it_computed(cclqr, path):
    """the measured-error mode (bf16_terms = 2) compared only with itself: P finite, each problem's own (problem p = the shared-weights call with its pair), and the
    gains bitwise those of the call without P"""
    capi = cclqr._capi
    pr = build_case("w_frag_1_6")
    K, P, kb = capi.riccati_value(*_models(pr), pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path, bf16_terms=2)
    Kw, kbw = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path, bf16_terms=2)
    assert np.isfinite(P).all() and np.array_equal(K, Kw) and np.array_equal(kb, kbw)
    for p in range(pr["nprob"]):
        _, Ps, _ = capi.riccati_value(*_models(pr), pr["Q"][p], pr["R"][p], pr["N"], tol=pr["tol"], path=path, bf16_terms=2)
        assert np.array_equal(Ps[p], P[p]), (path, p)
    assert not np.array_equal(P[0], P[1])
