"""cclqr_policy_value_tracking on the device: every case of tests/tracking_policy_common.py on every path its shape has, against the extended-precision references
and the acceptance rule stated there (the CPU twin tests/test_tracking_policy_reference.py shows that the cases cannot pass vacuously).
  * every horizon x sharing (nlin, nK in {1, N - 1}): P, P_all at every knot, price and noise_total within the rule; P == P_all[0], P_all[N - 1] == Q,
    price[N - 1] == 0 and noise_total = the prices summed from N - 2 down, all bitwise.
  * bitwise: a problem alone against inside its batch; shared against replicated gains, weights and noise; with and without P_all and the prices.
  * duality on the device: tr(P_0 Σ_0) + noise_total against the summed total of cclqr_covariance_tracking on the same arrays.
  * one model and one gain: cclqr_policy_value(nK = 1, tol = 0).
  * every refusal returns CCLQR_EINVAL with sentinel-filled outputs untouched; a singular G Bλ at a reached knot is CCLQR_ESINGULAR and names the knot."""
import numpy as np
import pytest

import dlqr_reference as ref
import tracking_policy_common as tp

pytestmark = pytest.mark.gpu

RUNS = [(name, path) for name in tp.NAMES for path in tp.paths_of(name)]
BITWISE = [("tc_12_1_5", 1, 38), ("tc_12_1_5", 2, 11), ("tc_84_7_35", 1, 11), ("tc_96_7_0", 1, 3), ("tc_30_2_6", 2, 11), ("tc_100_3_10", 2, 3), ("tc_24_0_4", 1, 11)]


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y, equal_nan=True)) for x, y in zip(a, b))


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_horizon_and_sharing_against_extended_precision(cclqr, name, path):
    capi = cclqr._capi
    pr = tp.build_case(name)
    for tvA, tvK in tp.SHARINGS:
        for N in pr["horizons"]:
            r = tp.reference(name, tvA, tvK, N)
            P, Pall, price, total = capi.policy_value_tracking(*tp.call_arrays(pr, N, tvA, tvK), pr["Q"], pr["R"], pr["Wu"], N, path=path, want_all=True)
            assert (price is None) == (pr["mu"] == 0) and (total is None) == (pr["mu"] == 0)
            for p in range(pr["nprob"]):
                tp.check_horizon(r, p, N, P[p], Pall[p], None if price is None else price[p], None if total is None else total[p],
                                 "%s nlin/nK per knot %s/%s path %d N=%d problem %d" % (name, tvA, tvK, path, N, p), Q=pr["Q"])
            if N == 1:
                assert np.array_equal(P, np.stack([pr["Q"]] * pr["nprob"]))      # no step: Q as written, bitwise


@pytest.mark.parametrize("name,path,N", BITWISE)
def test_alone_batched_shared_replicated_and_fewer_outputs_give_the_same_bits(cclqr, name, path, N):
    capi = cclqr._capi
    pr = tp.build_case(name)
    n, mu = pr["nprob"], pr["mu"]
    assert path in tp.paths_of(name)
    Q, R, Wu = pr["Q"], pr["R"], pr["Wu"]
    rep = lambda X: None if X is None else np.stack([X] * n)
    for tvA, tvK in tp.SHARINGS:
        A, Bu, Bl, G, K = tp.call_arrays(pr, N, tvA, tvK)
        base = capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, Wu, N, path=path, want_all=True)
        assert np.isfinite(base[1]).all() and np.abs(base[0]).max() > 0
        for p in range(n):
            alone = capi.policy_value_tracking(*tp.call_arrays(pr, N, tvA, tvK, slice(p, p + 1)), Q, R, Wu, N, path=path, want_all=True)
            assert _same([None if x is None else x[p:p + 1] for x in base], alone), (tvA, tvK, p)
        assert _same(base, capi.policy_value_tracking(A, Bu, Bl, G, K, rep(Q), rep(R), Wu, N, path=path, want_all=True))
        assert _same(base, capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, rep(Wu), N, path=path, want_all=True))
        if mu:      # one shared table against the same table per problem
            K1 = np.ascontiguousarray(K[:1])
            one = capi.policy_value_tracking(A, Bu, Bl, G, K1, Q, R, Wu, N, path=path, want_all=True)
            assert _same(one, capi.policy_value_tracking(A, Bu, Bl, G, np.concatenate([K1] * n), Q, R, Wu, N, path=path, want_all=True))
            assert np.array_equal(one[1][0], base[1][0]) and not np.array_equal(one[1][1], base[1][1])      # problem 0's table, read by every problem
        fewer = capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, None, N, path=path)      # no P_all, no noise: no price pass at all
        assert np.array_equal(fewer[0], base[0]) and all(x is None for x in fewer[1:])
        noall = capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, Wu, N, path=path)
        assert noall[1] is None and _same([base[i] for i in (0, 2, 3)], [noall[i] for i in (0, 2, 3)])
        if mu:
            only = capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, Wu, N, path=path, want_P=False, want_price=False)
            assert only[0] is None and only[2] is None and np.array_equal(only[3], base[3])
        if path == 1:
            assert _same(base, capi.policy_value_tracking(A, Bu, Bl, G, K, Q, R, Wu, N, path=0, want_all=True))


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_duality_with_the_tracking_covariance_on_the_device(cclqr, name, path):
    """sum(total) of cclqr_covariance_tracking = tr(P_0 Σ_0) + noise_total on the same arrays, within bound x the cost scale: bound = dlqr_reference.tolerance(e64) of
    the policy recursion, the cost scale the magnitude sum |P_0| . |Σ_0| plus the prices' magnitude sums."""
    capi = cclqr._capi
    pr = tp.build_case(name)
    N = max(pr["horizons"])
    for tvA, tvK in tp.SHARINGS:
        r = tp.reference(name, tvA, tvK, N)
        arrs = tp.call_arrays(pr, N, tvA, tvK)
        P, _, _, ntot = capi.policy_value_tracking(*arrs, pr["Q"], pr["R"], pr["Wu"], N, path=path)
        _, _, _, _, _, total = capi.covariance_tracking(*arrs, pr["Q"], pr["R"], pr["Wu"], pr["Sigma0"], N, path=path, want_std=False, want_cost=False)
        for p in range(pr["nprob"]):
            dual = float(np.sum(P[p] * pr["Sigma0"].T)) + (0.0 if ntot is None else float(ntot[p]))
            scale = float(np.sum(np.abs(np.asarray(r["P"][p][0], dtype=np.float64)) * np.abs(pr["Sigma0"]))) + float(np.sum(r["pmag"][p]))
            bound = ref.tolerance(r["e64"][p])
            err = abs(dual - float(total[p].sum()))
            print("%s path %d sharing %s/%s problem %d: tr(P0 Σ0) + noise_total = %.17g, covariance total %.17g, off by %.3g of the cost scale %.3g (bound %.3g)"
                  % (name, path, tvA, tvK, p, dual, float(total[p].sum()), err / scale, scale, bound))
            assert err <= bound * scale


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_one_model_and_one_gain_is_cclqr_policy_value(cclqr, name, path):
    capi = cclqr._capi
    pr = tp.build_case(name)
    N = 11
    r = tp.reference(name, False, False, N)
    A, Bu, Bl, G, K = tp.call_arrays(pr, N, False, False)
    P = capi.policy_value_tracking(A, Bu, Bl, G, K, pr["Q"], pr["R"], None, N, path=path)[0]
    Ppol = capi.policy_value(A[:, 0], Bu[:, 0], Bl[:, 0], G[:, 0], K, pr["Q"], pr["R"], N, tol=0.0, path=path, want_diag=False)[0]
    for p in range(pr["nprob"]):
        bound = ref.tolerance(r["e64"][p])
        err = float(np.abs(P[p] - Ppol[p]).max() / np.abs(Ppol[p]).max())
        print("%s path %d problem %d: against cclqr_policy_value off by %.3g relative (bound %.3g)" % (name, path, p, err, bound))
        assert err <= bound


def test_every_refusal_code_and_untouched_outputs(cclqr):
    capi = cclqr._capi
    pr = tp.build_case("tc_12_1_5")
    A, Bu, Bl, G, K = tp.call_arrays(pr, 11, True, True)
    call = tp.refusal_call(capi, dict(pr, A=A, Bu=Bu, Bl=Bl, G=G, K=K), 11)
    assert call()[0] == capi.OK and call(Wu_=None, price_=False, total_=False)[0] == capi.OK and call(N=1)[0] == capi.OK and call(price_=False)[0] == capi.OK
    refused = {what: call(**kw) for what, kw in tp.refusal_cases().items()}
    for what, (rc, untouched, msg) in refused.items():
        assert rc == capi.EINVAL and untouched, (what, rc, untouched, msg)
    # a singular G Bλ at a middle knot of problem 1: named with its knot, on both paths
    Bz = Bl.copy()
    Bz[1, 4] = 0.0
    rc, _, msg = call(Bl_=Bz)
    assert rc == capi.ESINGULAR and "problem 1" in msg and "knot 4" in msg, (rc, msg)
    rc, _, msg = call(Bl_=Bz, path=2)
    assert rc == capi.ESINGULAR and "problem 1" in msg and "knot 4" in msg, (rc, msg)
    assert call(N=1, Bl_=np.zeros_like(Bl))[0] == capi.OK      # no step reaches a model
