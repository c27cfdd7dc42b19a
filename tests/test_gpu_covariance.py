"""cclqr_covariance_doubling on the device: every case of tests/covariance_common.py on every path its shape has, against the extended-precision STEPPING references
and the acceptance rule stated there (the CPU twin tests/test_covariance_reference.py shows that the cases cannot pass vacuously).
  * fixed horizons (with and without Σ0, Wu shared and per problem) and the run to convergence: Σ, the moments, levels, reason and the norms within the rule.
  * bitwise: shared against replicated K / Q / R / Wu, a problem alone against inside its batch, path 0 against path 1 where 0 is the resident kernel, and 4 Wu, 4 Σ0
    against Wu, Σ0: exactly 4 Σ, 4 cost, 2 zstd, 2 ustd, 4 dnorm with the same levels, reason and gnorm -- the point of the scale w.
  * duality with the cost recursion on the device: tr(Q Σ) + tr(R K Σ K') = tr(P W) up to the terminal term P carries and Σ does not.
  * the unstable closed loop stops with reason 2 and a finite Σ; every refusal of both entry points returns its code with the outputs untouched;
    cclqr_policy_value_doubling returns the same bits before and after a covariance call."""
import numpy as np
import pytest

import covariance_common as cc
import dlqr_reference as ref
import policy_doubling_common as pdc

pytestmark = pytest.mark.gpu

LD = np.longdouble
RUNS = [(name, path) for name in cc.NAMES for path in pdc.BY_NAME[name]["paths"]]


def _models(pr, sl=slice(None)):
    return pr["A"][sl], pr["Bu"][sl], pr["Bl"][sl], pr["G"][sl]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _moments_are_those_of_the_device_sigma(pr, S, zs, us):
    """zstd is sqrt(max(Σ_ii, 0)) of the Σ the device returned, bitwise (sqrt is correctly rounded on both sides); ustd² is the diagonal of K Σ K' of that Σ to the
    rounding of two nested float64 sums of mx terms, (2 mx + 8) eps of the magnitude sum |K_j| |Σ| |K_j|' (8: the square root and its square)"""
    assert np.array_equal(zs, np.sqrt(np.maximum(np.diag(S), 0.0)))
    K, SL = np.asarray(pr["K"], dtype=LD), np.asarray(S, dtype=LD)
    for j in range(pr["mu"]):
        want, mag = float(K[j] @ SL @ K[j]), float(np.abs(K[j]) @ np.abs(SL) @ np.abs(K[j]))
        assert abs(us[j] ** 2 - max(want, 0.0)) <= (2 * pr["mx"] + 8) * np.finfo(float).eps * mag, (j, us[j] ** 2, want, mag)


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_fixed_horizon_against_extended_precision(cclqr, name, path):
    capi = cclqr._capi
    pr = cc.build_case(name)
    for vname, v in pr["variants"].items():
        for n, rows in v["fixed"].items():
            S, cost, zs, us, lv, rs, dn, gn = capi.covariance_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], v["Wu"], v["Sigma0"], n + 1, path=path)
            for p in range(pr["nprob"]):
                cc.check_fixed(S[p], cost[p], zs[p], us[p], lv[p], gn[p], dn[p], rows[p], "%s %s path %d problem %d, %d steps" % (name, vname, path, p, n))
                assert rs[p] == 0
                _moments_are_those_of_the_device_sigma(pr, S[p], zs[p], us[p])
                if n == 0:
                    assert np.array_equal(S[p], v["Sigma0"])      # no step: Σ0, bitwise (the scaling by w is exact)


@pytest.mark.parametrize("name,path", [r for r in RUNS if r[0] != "pd_mu0"], ids=["%s-path%d" % r for r in RUNS if r[0] != "pd_mu0"])
def test_every_run_to_convergence_against_extended_precision(cclqr, name, path):
    pr = cc.build_case(name)
    v = pr["variants"]["nostart"]
    S, cost, zs, us, lv, rs, dn, gn = cclqr._capi.covariance_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], v["Wu"], None, 0, tol=v["tol"],
                                                                      max_levels=v["max_levels"], path=path)
    for p in range(pr["nprob"]):
        cc.check_conv(S[p], cost[p], zs[p], us[p], lv[p], rs[p], dn[p], gn[p], v["conv"][p], "%s path %d problem %d" % (name, path, p))
        _moments_are_those_of_the_device_sigma(pr, S[p], zs[p], us[p])
    if name == "pd_unstable":
        assert rs[2] == 2 and np.isfinite(S[2]).all() and gn[2, 0] > pdc.GROWTH > gn[2, 1] and rs[0] == 0 and lv[2] == v["conv"][2]["levels"]


@pytest.mark.parametrize("name,path,N", [("pd_12", 1, 38), ("pd_12", 1, 0), ("pd_30", 2, 38), ("pd_30", 2, 0), ("pd_84", 1, 10)])
def test_shared_replicated_alone_and_batched_give_the_same_bits(cclqr, name, path, N):
    capi = cclqr._capi
    pr = cc.build_case(name)
    n = pr["nprob"]
    v = pr["variants"]["nostart"]
    S0 = None if N == 0 else pr["Sigma0"]
    kw = dict(tol=v["tol"], max_levels=v["max_levels"], path=path)
    K, Q, R, Wu = pr["K"], pr["Q"], pr["R"], pr["Wu"]
    rep = lambda X: np.stack([X] * n)
    base = capi.covariance_doubling(*_models(pr), K, Q, R, Wu, S0, N, **kw)
    assert _same(base, capi.covariance_doubling(*_models(pr), rep(K), Q, R, Wu, S0, N, **kw))
    assert _same(base, capi.covariance_doubling(*_models(pr), K, rep(Q), rep(R), Wu, S0, N, **kw))
    assert _same(base, capi.covariance_doubling(*_models(pr), K, Q, R, rep(Wu), None if S0 is None else rep(S0), N, **kw))
    for p in range(n):
        alone = capi.covariance_doubling(*_models(pr, slice(p, p + 1)), K, Q, R, Wu, S0, N, **kw)
        assert _same([x[p:p + 1] for x in base], alone), p
    # per-problem noise is read per problem: twice the noise for problem 1 alone changes problem 1 alone
    W2 = rep(Wu)
    W2[1] *= 2.0
    Sz = capi.covariance_doubling(*_models(pr), K, Q, R, W2, None if S0 is None else rep(S0), N, **kw)[0]
    assert np.array_equal(Sz[0], base[0][0]) and not np.array_equal(Sz[1], base[0][1])


@pytest.mark.parametrize("N", [0, 38])
def test_path_zero_is_the_resident_kernel_where_it_chooses_it(cclqr, N):
    capi = cclqr._capi
    pr = cc.build_case("pd_12")
    assert pr["mx"] < 64 and pr["mx"] % 4 == 0      # small problems run resident whatever their number
    v = pr["variants"]["nostart"]
    args = (*_models(pr), pr["K"], pr["Q"], pr["R"], pr["Wu"], None if N == 0 else pr["Sigma0"], N)
    kw = dict(tol=v["tol"], max_levels=v["max_levels"])
    assert _same(capi.covariance_doubling(*args, path=0, **kw), capi.covariance_doubling(*args, path=1, **kw))


@pytest.mark.parametrize("name,path,N", [("pd_12", 1, 38), ("pd_12", 1, 0), ("pd_30", 2, 38), ("pd_30", 2, 0), ("pd_84", 1, 10)])
def test_four_times_the_noise_is_exactly_four_times_the_covariance(cclqr, name, path, N):
    capi = cclqr._capi
    pr = cc.build_case(name)
    v = pr["variants"]["nostart"]
    S0 = None if N == 0 else pr["Sigma0"]
    kw = dict(tol=v["tol"], max_levels=v["max_levels"], path=path)
    S, cost, zs, us, lv, rs, dn, gn = capi.covariance_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["Wu"], S0, N, **kw)
    S4, cost4, zs4, us4, lv4, rs4, dn4, gn4 = capi.covariance_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], 4.0 * pr["Wu"], None if S0 is None else 4.0 * S0, N, **kw)
    assert np.array_equal(S4, 4.0 * S) and np.array_equal(cost4, 4.0 * cost) and np.array_equal(zs4, 2.0 * zs) and np.array_equal(us4, 2.0 * us)
    assert np.array_equal(lv4, lv) and np.array_equal(rs4, rs) and np.array_equal(gn4, gn, equal_nan=True) and np.array_equal(dn4, 4.0 * dn, equal_nan=True)
    assert np.abs(S).max() > 0


@pytest.mark.parametrize("name,path", [("pd_12", 1), ("pd_30", 2)])
def test_duality_with_the_cost_recursion_on_the_device(cclqr, name, path):
    """to convergence: cost[0] + cost[1] = tr(Qbar C) = tr(S W), and the device's P = S + M' Q M, so |cost0 + cost1 - tr(P W)| <= bound x the magnitude sum of tr(P W) +
    norm(M)^2 norm(Q) norm(W); P from a tol so small that the cost recursion runs to max_levels = the levels the covariance made"""
    capi = cclqr._capi
    pr = cc.build_case(name)
    v = pr["variants"]["nostart"]
    S, cost, _, _, lv, rs, _, gn = capi.covariance_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], pr["Wu"], None, 0, tol=v["tol"], max_levels=v["max_levels"], path=path)
    assert (rs == 0).all()
    for p in range(pr["nprob"]):
        # (problem by problem, each with the levels its covariance made: the two sums of the duality then run over the same steps)
        P, lvP, _, _, _ = capi.policy_value_doubling(*_models(pr, slice(p, p + 1)), pr["K"], pr["Q"], pr["R"], 0, tol=1e-300, max_levels=int(lv[p]), path=path)
        assert lvP[0] >= lv[p]
        W = cc.noise(cc.input_map(pr["Bu"][p], pr["Bl"][p], pr["G"][p]), pr["Wu"])
        PL = np.asarray(P[0], dtype=LD)
        trPW, scale = float(np.sum(PL * W.T)), float(np.sum(np.abs(PL) * np.abs(W)))
        bound = ref.tolerance(v["conv"][p]["e64"])
        slack = bound * scale + gn[p, 0] ** 2 * float(pdc.fro(np.asarray(pr["Q"], dtype=LD))) * float(pdc.fro(W))
        print("%s problem %d: cost %.17g + %.17g against tr(P W) = %.17g: off by %.3g, allowed %.3g" % (name, p, cost[p, 0], cost[p, 1], trPW,
                                                                                                      abs(cost[p, 0] + cost[p, 1] - trPW), slack))
        assert abs(cost[p, 0] + cost[p, 1] - trPW) <= slack


def test_null_moments_and_null_diagnostics_change_nothing(cclqr):
    capi = cclqr._capi
    pr = cc.build_case("pd_30")
    args = (*_models(pr), pr["K"], pr["Q"], pr["R"], pr["Wu"], pr["Sigma0"], 38)
    S = capi.covariance_doubling(*args)[0]
    out = capi.covariance_doubling(*_models(pr), pr["K"], None, None, pr["Wu"], pr["Sigma0"], 38, want_cost=False, want_std=False, want_diag=False)
    assert np.array_equal(out[0], S) and all(x is None for x in out[1:])


def test_policy_value_doubling_returns_the_same_bits_around_a_covariance_call(cclqr):
    capi = cclqr._capi
    pr, pc = pdc.build_case("pd_12"), cc.build_case("pd_12")
    for N in (38, 0):
        call = lambda: capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], N, tol=pr["tol"], max_levels=pr["max_levels"])
        before = call()
        capi.covariance_doubling(*_models(pc), pc["K"], pc["Q"], pc["R"], pc["Wu"], None, N, tol=pc["variants"]["nostart"]["tol"])
        assert _same(before, call())


def test_every_refusal_code_and_untouched_outputs(cclqr):
    capi = cclqr._capi
    pr = cc.build_case("pd_30")
    Bl = np.ascontiguousarray(pr["Bl"])
    call = cc.refusal_call(capi, pr)
    assert call()[0] == capi.OK and call(N=0, S0_=None)[0] == capi.OK and call(Wu_=None)[0] == capi.OK and call(S0_=None)[0] == capi.OK
    assert call(cost_=False, Q_=None, R_=None)[0] == capi.OK and call(N=1)[0] == capi.OK
    refused = {what: call(**kw) for what, kw in cc.refusal_cases().items()}
    for what, (rc, untouched, msg) in refused.items():
        assert rc == capi.EINVAL and untouched, (what, rc, untouched, msg)
    rc, _, _ = call(Bl_=np.zeros_like(Bl))
    assert rc == capi.ESINGULAR and call(N=0, S0_=None, Bl_=np.zeros_like(Bl))[0] == capi.ESINGULAR
    assert call(N=1, Bl_=np.zeros_like(Bl))[0] == capi.OK      # no step reaches the model, as in the cost recursion
