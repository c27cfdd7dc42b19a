"""Shared by tests/test_riccati_value_reference.py (CPU), tests/test_gpu_riccati_value.py and tests/test_gpu_predicted_cost.py: the extended-precision reference of the
cost-to-go that cclqr_riccati_value returns -- the Pkp1 of lqr.jl:170 at the last backward step a problem executes.

The recursion is NOT restated here: the step function handed to dlqr_reference._sweep is wrapped so that it keeps the last Pkp1 it computed.  _sweep calls the step
once per executed backward step and breaks AFTER the call whose norm met the tolerance (lqr.jl:172), so the kept matrix is the Pkp1 of the step the test fired on,
of step 1 when it never fired, and nothing (-> Q) when N = 1.  The cases are those of the per-problem-weights Riccati (riccati_weights_common.CASES)."""
import numpy as np

import dlqr_reference as ref
from riccati_weights_common import CASES, build_case      # noqa: F401  (re-exported: the tests import the cases from here)

LD = np.longdouble


def sweep_P(model, Q, R, N, tol, dtype, step):
    """dlqr_reference._sweep with `step` wrapped: returns (K, P = the last Pkp1 in dtype, kbreak, norms)"""
    last = []

    def keeping(A, Bu, Bl, G, Q_, R_, Pk, dt):
        Kuk, Pkp1 = step(A, Bu, Bl, G, Q_, R_, Pk, dt)
        last[:] = [Pkp1]
        return Kuk, Pkp1

    K, kb, norms = ref._sweep(model, Q, R, N, tol, dtype, keeping)
    P = last[0] if last else np.asarray(Q, dtype=dtype)
    return K, np.asarray(P, dtype=dtype), kb, norms


def _model_of(A, Bu, Bl, G, tv):
    return (lambda k: (A[k - 1], Bu[k - 1], Bl[k - 1], G[k - 1])) if tv else (lambda k: (A, Bu, Bl, G))


def reference_P(A, Bu, Bl, G, Q, R, N, tol, tv=False):
    """(P as float64 from the longdouble run, kbreak, e64P): e64P is the larger relative deviation max|P64 - P_ld| / max|P_ld| of the two float64 twins
    (dlqr_reference._step, _step_projected64) from the longdouble run; a twin that breaks at another index counts as deviation 1"""
    model = _model_of(A, Bu, Bl, G, tv)
    _, P, kb, _ = sweep_P(model, Q, R, N, tol, LD, ref._step)
    scale = float(np.max(np.abs(P)))
    e64 = 0.0
    for step in (ref._step, ref._step_projected64):
        _, P64, kb64, _ = sweep_P(model, Q, R, N, tol, np.float64, step)
        e64 = max(e64, 1.0 if kb64 != kb else float(np.max(np.abs(P64.astype(LD) - P))) / scale)
    return P.astype(np.float64), kb, e64


_refs = {}


def case_P(name):
    """[(P, kbreak, e64P)] per problem of riccati_weights_common.build_case(name), built once per session"""
    if name not in _refs:
        pr = build_case(name)
        _refs[name] = [reference_P(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"][p], pr["R"][p], pr["N"], pr["tol"]) for p in range(pr["nprob"])]
    return _refs[name]


def check_P(P, refp, what):
    """the acceptance rule: max|P - Pref| <= dlqr_reference.tolerance(e64P) max|Pref|"""
    Pref, kb, e64 = refp
    scale = float(np.abs(Pref).max())
    err = float(np.abs(P - Pref).max())
    print("%s: max|P - Pref| = %.3g relative, bound %.3g (e64P %.3g, max|Pref| %.3g)" % (what, err / scale, ref.tolerance(e64), e64, scale))
    assert np.isfinite(P).all() and err <= ref.tolerance(e64) * scale, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, err / scale, ref.tolerance(e64))
