"""cclqr_covariance_tracking on the device: every case of tests/tracking_covariance_common.py on every path its shape has, against the extended-precision stepping
references and the acceptance rule stated there (the CPU twin tests/test_tracking_covariance_reference.py shows that the cases cannot pass vacuously).
  * every horizon x sharing (nlin, nK in {1, N - 1}) x variant: Sigma, Sigma_all at every knot, cost, zstd, ustd and total within the rule.
  * bitwise: a problem alone against inside its batch; shared against replicated gains, weights and noise; with and without Sigma_all and the moments;
    path 0 against path 1 where the shape fits the resident kernel; N = 1 returns Sigma0.
  * every refusal returns CCLQR_EINVAL with sentinel-filled outputs untouched; a singular G Bλ at a middle knot is CCLQR_ESINGULAR and names the knot."""
import numpy as np
import pytest

import tracking_covariance_common as tc

pytestmark = pytest.mark.gpu

RUNS = [(name, path) for name in tc.NAMES for path in tc.paths_of(name)]
BITWISE = [("tc_12_1_5", 1, 38), ("tc_84_7_35", 1, 11), ("tc_96_7_0", 1, 3), ("tc_30_2_6", 2, 11), ("tc_100_3_10", 2, 3), ("tc_24_0_4", 1, 11)]


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_horizon_sharing_and_variant_against_extended_precision(cclqr, name, path):
    capi = cclqr._capi
    pr = tc.build_case(name)
    for key, run in pr["runs"].items():
        _, tvA, tvK = key
        for N in pr["horizons"]:
            if key[0] == "nostart" and N == 1:
                continue
            S, Sall, cost, zstd, ustd, total = capi.covariance_tracking(*tc.call_arrays(pr, N, tvA, tvK), pr["Q"], pr["R"], run["Wu"], run["Sigma0"], N, path=path,
                                                                        want_all=True)
            for p in range(pr["nprob"]):
                tc.check_horizon(pr, key, N, p, S[p], Sall[p], cost[p], zstd[p], ustd[p], total[p], "%s %s path %d N=%d problem %d" % (name, key, path, N, p))
            if N == 1:
                assert np.array_equal(S, np.stack([run["Sigma0"]] * pr["nprob"]))      # no step: Σ0 as written, bitwise


@pytest.mark.parametrize("name,path,N", BITWISE)
def test_alone_batched_shared_replicated_and_fewer_outputs_give_the_same_bits(cclqr, name, path, N):
    capi = cclqr._capi
    pr = tc.build_case(name)
    n, mu = pr["nprob"], pr["mu"]
    assert path in pr["paths"]
    Q, R, Wu, S0 = pr["Q"], pr["R"], pr["Wu"], pr["Sigma0"]
    rep = lambda X: None if X is None else np.stack([X] * n)
    for tvA, tvK in tc.SHARINGS:
        A, Bu, Bl, G, K = tc.call_arrays(pr, N, tvA, tvK)
        base = capi.covariance_tracking(A, Bu, Bl, G, K, Q, R, Wu, S0, N, path=path, want_all=True)
        assert np.isfinite(base[1]).all() and np.abs(base[0]).max() > 0
        for p in range(n):
            alone = capi.covariance_tracking(*tc.call_arrays(pr, N, tvA, tvK, slice(p, p + 1)), Q, R, Wu, S0, N, path=path, want_all=True)
            assert _same([x[p:p + 1] for x in base], alone), (tvA, tvK, p)
        assert _same(base, capi.covariance_tracking(A, Bu, Bl, G, K, rep(Q), rep(R), Wu, S0, N, path=path, want_all=True))
        assert _same(base, capi.covariance_tracking(A, Bu, Bl, G, K, Q, R, rep(Wu), rep(S0), N, path=path, want_all=True))
        if mu:      # one shared table against the same table per problem
            K1 = np.ascontiguousarray(K[:1])
            one = capi.covariance_tracking(A, Bu, Bl, G, K1, Q, R, Wu, S0, N, path=path, want_all=True)
            assert _same(one, capi.covariance_tracking(A, Bu, Bl, G, np.concatenate([K1] * n), Q, R, Wu, S0, N, path=path, want_all=True))
            assert np.array_equal(one[1][0], base[1][0]) and not np.array_equal(one[1][1], base[1][1])      # problem 0's table, read by every problem
        fewer = capi.covariance_tracking(A, Bu, Bl, G, K, None, None, Wu, S0, N, path=path, want_all=False, want_cost=False, want_std=False, want_total=False)
        assert np.array_equal(fewer[0], base[0]) and all(x is None for x in fewer[1:])
        noall = capi.covariance_tracking(A, Bu, Bl, G, K, Q, R, Wu, S0, N, path=path)
        assert noall[1] is None and _same([base[i] for i in (0, 2, 3, 4, 5)], [noall[i] for i in (0, 2, 3, 4, 5)])
        if path == 1:
            assert _same(base, capi.covariance_tracking(A, Bu, Bl, G, K, Q, R, Wu, S0, N, path=0, want_all=True))


def test_every_refusal_code_and_untouched_outputs(cclqr):
    capi = cclqr._capi
    pr = tc.build_case("tc_12_1_5")
    A, Bu, Bl, G, K = tc.call_arrays(pr, 11, True, True)
    call = tc.refusal_call(capi, dict(pr, A=A, Bu=Bu, Bl=Bl, G=G, K=K), 11)
    assert call()[0] == capi.OK and call(Wu_=None)[0] == capi.OK and call(S0_=None)[0] == capi.OK and call(N=1)[0] == capi.OK
    assert call(cost_=False, total_=False, Q_=None, R_=None)[0] == capi.OK
    refused = {what: call(**kw) for what, kw in tc.refusal_cases().items()}
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
