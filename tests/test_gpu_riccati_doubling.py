"""cclqr_riccati_doubling on the device: every case of tests/riccati_doubling_common.py against the extended-precision STEPPING references and the acceptance rule
stated there (the CPU twin tests/test_riccati_doubling_reference.py shows that the cases cannot pass vacuously).
  * fixed horizon: K and P within their bounds, levels exact, reason 0, dnorm NaN; and K, P within the same bound of the device's own cclqr_riccati_value(N, tol = 0,
    keep_last).
  * to convergence: levels and reason exact, K, P, dnorm and anorm within the rule; an unstable model without inputs stops with reason 2 and every output finite or
    NaN by contract; max_levels = 1 stops with reason 1 at the gain of N = 3.
  * bitwise: shared against replicated weights, a problem alone against inside a batch.
  * a zero pivot of I + G1 H2 (one state, q = -r / d^2) is reason 3 for that problem alone, in both modes: NaN gain and P for a fixed horizon, the triple of the
    level before kept in a run to convergence; its neighbour in the batch is untouched.
  * every CCLQR_EINVAL leaves the outputs untouched; a singular G Bλ is CCLQR_ESINGULAR."""
import numpy as np
import pytest

import dlqr_reference as ref
import riccati_doubling_common as rdc

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in rdc.CASES]


def _models(pr, sl=slice(None)):
    return pr["A"][sl], pr["Bu"][sl], pr["Bl"][sl], pr["G"][sl]


@pytest.mark.parametrize("name", NAMES)
def test_every_fixed_horizon_against_extended_precision_and_the_stepping_kernels(cclqr, name):
    capi = cclqr._capi
    pr = rdc.build_case(name)
    for n in pr["steps"]:
        K, P, lv, rs, dn, an = capi.riccati_doubling(*_models(pr), pr["Q"], pr["R"], n + 1)
        Ks, Ps, _ = capi.riccati_value(*_models(pr), pr["Q"], pr["R"], n + 1, tol=0.0, keep_last=True)
        for p in range(pr["nprob"]):
            what = "%s problem %d, %d steps" % (name, p, n)
            Kref, Pref, levels, e64K, e64P, _, _ = pr["fixed"][n][p]
            rdc.check(K[p], P[p], Kref, Pref, e64K, e64P, what)
            assert (lv[p], rs[p]) == (levels, 0) and np.isnan(dn[p]).all() and np.isfinite(an[p, 0]) and np.isnan(an[p, 1]), (what, lv[p], rs[p], dn[p], an[p])
            devK = float(np.abs(K[p] - Ks[p, 0]).max()) / float(np.abs(Kref).max()) if Kref.size else 0.0
            devP = float(np.abs(P[p] - Ps[p]).max()) / float(np.abs(Pref).max())
            print("%s: against the stepping kernels K %.3g, P %.3g relative" % (what, devK, devP))
            assert devK <= ref.tolerance(e64K) and devP <= ref.tolerance(e64P), what


@pytest.mark.parametrize("name", NAMES)
def test_every_run_to_convergence_against_extended_precision(cclqr, name):
    pr = rdc.build_case(name)
    K, P, lv, rs, dn, an = cclqr._capi.riccati_doubling(*_models(pr), pr["Q"], pr["R"], 0, tol=pr["tol"], max_levels=pr["max_levels"])
    for p in range(pr["nprob"]):
        what = "%s problem %d to convergence" % (name, p)
        Kref, Pref, levels, reason, dnref, anref, e64K, e64P, _, _ = pr["conv"][p]
        print("%s: levels %d reason %d (reference %d, %d), dnorm %s (reference %s), anorm %s (reference %s)" % (what, lv[p], rs[p], levels, reason, dn[p], dnref, an[p], anref))
        assert (lv[p], rs[p]) == (levels, reason), what
        rdc.check(K[p], P[p], Kref, Pref, e64K, e64P, what)
        bound, scale = ref.tolerance(max(e64K, e64P)), float(np.abs(Pref).max())
        rdc.check_norms(dn[p], dnref, bound, scale, "dnorm", what)
        rdc.check_norms(an[p], anref, bound, scale, "anorm", what)


def test_an_unstable_model_without_inputs_stops_for_growth(cclqr):
    A, Bu, Bl, G, Q, R, levels, reason = rdc.unstable_problem()
    K, P, lv, rs, dn, an = cclqr._capi.riccati_doubling(A, Bu, Bl, G, Q, R, 0, tol=1e-5, max_levels=40)
    print("unstable: levels %s reason %s dnorm %s anorm %s max|P| %.3g" % (lv, rs, dn, an, np.abs(P).max()))
    assert (lv[0], rs[0]) == (levels, 2) and K.shape == (1, 0, 12)
    assert np.isfinite(P).all() and np.isfinite(dn).all() and an[0, 0] > rdc.GROWTH > an[0, 1]


@pytest.mark.parametrize("name", ["rd_12", "rd_30", "rd_97"])
def test_max_levels_stops_with_reason_one(cclqr, name):
    """tol = 0 never converges: one level is two triples, and the result is the fixed horizon's of N = 3"""
    pr = rdc.build_case(name)
    K, P, lv, rs, dn, an = cclqr._capi.riccati_doubling(*_models(pr), pr["Q"], pr["R"], 0, tol=0.0, max_levels=1)
    assert (lv == 1).all() and (rs == 1).all() and np.isfinite(dn[:, 0]).all() and np.isnan(dn[:, 1]).all() and np.isfinite(an[:, 0]).all()
    for p in range(pr["nprob"]):
        Kref, Pref, _, e64K, e64P, _, _ = pr["fixed"][2][p] if 2 in pr["fixed"] else (None,) * 7
        if Kref is None:      # the horizon of two steps is not among the case's: its reference is built here
            m = (pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"])
            Kl, Pl = rdc.stepping(*m, 2)
            tw = [rdc.stepping(*m, 2, np.float64), rdc.stepping(*m, 2, np.float64, True)]
            e64K, e64P = max(rdc._rel(t[0], Kl) for t in tw), max(rdc._rel(t[1], Pl) for t in tw)
            Kref, Pref = Kl.astype(np.float64), Pl.astype(np.float64)
        rdc.check(K[p], P[p], Kref, Pref, e64K, e64P, "%s problem %d, max_levels 1" % (name, p))


@pytest.mark.parametrize("name,N", [("rd_24", 38), ("rd_24", 0), ("rd_30", 38), ("rd_30", 0), ("rd_84", 10), ("rd_97", 0), ("rd_mu0", 10)])
def test_shared_replicated_alone_and_batched_give_the_same_bits(cclqr, name, N):
    capi = cclqr._capi
    pr = rdc.build_case(name)
    n = pr["nprob"]
    kw = dict(tol=pr["tol"], max_levels=pr["max_levels"])
    same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    base = capi.riccati_doubling(*_models(pr), pr["Q"], pr["R"], N, **kw)
    assert same(base, capi.riccati_doubling(*_models(pr), np.stack([pr["Q"]] * n), np.stack([pr["R"]] * n), N, **kw))
    for p in range(n):
        alone = capi.riccati_doubling(*_models(pr, slice(p, p + 1)), pr["Q"], pr["R"], N, **kw)
        assert same([x[p:p + 1] for x in base], alone), p
    # per-problem weights are read per problem: another Q for problem 1 alone changes problem 1 alone
    Qs = np.stack([pr["Q"]] * n)
    Qs[1] = 2.0 * Qs[1]
    other = capi.riccati_doubling(*_models(pr), Qs, np.stack([pr["R"]] * n), N, **kw)
    assert np.array_equal(other[1][0], base[1][0]) and not np.array_equal(other[1][1], base[1][1])
    # NULL diagnostics and a NULL P change nothing
    K0, P0, lv, rs, dn, an = capi.riccati_doubling(*_models(pr), pr["Q"], pr["R"], N, want_P=False, want_diag=False, **kw)
    assert P0 is None and lv is None and rs is None and dn is None and an is None and np.array_equal(K0, base[0])


def test_a_zero_pivot_is_reason_three_for_that_problem_alone(cclqr):
    """one state, one input, A = a, Bu = d = 1, R = r = 1: G0 = d^2 / r = 1, and with Q = q = -r / d^2 = -1 (symmetric, not positive definite) the first composition's
    M = I + G0 Q is exactly 0.  Problem 1 (a = 0.5, q = 1 through its own weights) is healthy"""
    capi = cclqr._capi
    A = np.array([[[0.9]], [[0.5]]])
    Bu, Bl, G = np.ones((2, 1, 1)), np.zeros((2, 1, 0)), np.zeros((2, 0, 1))
    Q, R = np.array([[[-1.0]], [[1.0]]]), np.ones((2, 1, 1))
    sl = slice(1, 2)
    for N in (3, 10, 0):
        K, P, lv, rs, dn, an = capi.riccati_doubling(A, Bu, Bl, G, Q, R, N, tol=1e-12, max_levels=8)
        alone = capi.riccati_doubling(A[sl], Bu[sl], Bl[sl], G[sl], Q[sl], R[sl], N, tol=1e-12, max_levels=8)
        print("N = %d: K %s P %s levels %s reason %s dnorm %s anorm %s" % (N, K.ravel(), P.ravel(), lv, rs, dn.tolist(), an.tolist()))
        assert rs[0] == 3 and rs[1] == 0 and np.isnan(dn[0]).all()
        assert all(np.array_equal(x[sl], y, equal_nan=True) for x, y in zip((K, P, lv, rs, dn, an), alone)), N
        assert np.isfinite(K[1]).all() and np.isfinite(P[1]).all()
        if N:
            assert np.isnan(K[0]).all() and np.isnan(P[0]).all() and np.isnan(an[0]).all()      # a fixed horizon has no H_n to take its final step on
        else:
            assert lv[0] == 0 and np.isnan(an[0]).all() and lv[1] >= 1      # no level completed: the single-step triple stays, the final step is taken on H = Q
            assert not np.isfinite(K[0]).any()      # (R + D'QD = 0 there: the gain is written, finite or not)
    # the healthy problem converges to the scalar DARE's root: p = q + a^2 p r / (r + d^2 p)
    K, P = capi.riccati_doubling(A[sl], Bu[sl], Bl[sl], G[sl], Q[sl], R[sl], 0, tol=1e-14, max_levels=8)[:2]
    p = P[0, 0, 0]
    assert abs(p - (1.0 + 0.25 * p / (1.0 + p))) <= 1e-12 * p


def test_every_refusal_code_and_untouched_outputs(cclqr):
    capi = cclqr._capi
    pr = rdc.build_case("rd_36")
    Bl = np.ascontiguousarray(pr["Bl"])
    call = rdc.refusal_call(capi, pr)
    assert call()[0] == capi.OK and call(N=0)[0] == capi.OK and call(N=0, max_levels=1)[0] == capi.OK and call(N=0, max_levels=60, tol=1e300)[0] == capi.OK
    assert call(N=2)[0] == capi.OK and call(max_levels=0)[0] == capi.OK      # (max_levels is not read for a fixed horizon)
    cases = rdc.refusal_cases(pr)
    refused = {what: call(**kw) for what, kw in cases.items()}
    for what, (rc, untouched, msg) in refused.items():
        assert rc == capi.EINVAL and untouched, (what, rc, untouched, msg)
    assert call(**cases["Q_nonsym"])[0] == capi.EINVAL and "not symmetric" in capi.lib().cclqr_last_error().decode()
    assert call(Bl_=np.zeros_like(Bl))[0] == capi.ESINGULAR and call(N=0, Bl_=np.zeros_like(Bl))[0] == capi.ESINGULAR
