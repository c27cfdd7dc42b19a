"""cclqr_covariance_tracking on the device: every case of tests/tracking_covariance_common.py on every path its shape has, against the extended-precision stepping
references and the acceptance rule stated there (the CPU twin tests/test_tracking_covariance_reference.py shows that the cases cannot pass vacuously).
  * every horizon x sharing (nlin, nK in {1, N - 1}) x variant: Sigma, Sigma_all at every knot, cost, zstd, ustd and total within the rule.
  * bitwise: a problem alone against inside its batch; shared against replicated gains, weights and noise; with and without Sigma_all and the moments;
    path 0 against path 1 where the shape fits the resident kernel; N = 1 returns Sigma0.
  * every refusal returns CCLQR_EINVAL with sentinel-filled outputs untouched; a singular G Bλ at a middle knot is CCLQR_ESINGULAR and names the knot."""
import ctypes as C

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
    L = capi.lib()
    pr = tc.build_case("tc_12_1_5")
    n, mx, mu, ml, N0 = pr["nprob"], pr["mx"], pr["mu"], pr["ml"], 11
    dp = C.POINTER(C.c_double)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    A, Bu, Bl, G, K = tc.call_arrays(pr, N0, True, True)
    Q, R, Wu, S0 = (np.ascontiguousarray(pr[k]) for k in ("Q", "R", "Wu", "Sigma0"))

    def call(nlin=N0 - 1, n_gains=n, nK=N0 - 1, n_weights=1, n_noise=1, N=N0, path=0, bf16=0, nprob=n, mx_=mx, mu_=mu, A_=A, K_=K, Bl_=Bl, Wu_=Wu, S0_=S0, Q_=Q, R_=R,
             cost_=True, total_=True):
        S, Sall = np.full((n, mx, mx), 7.5), np.full((n, N0, mx, mx), 7.5)
        cost, zs, us, tot = np.full((n, N0, 2), 7.5), np.full((n, N0, mx), 7.5), np.full((n, N0, mu), 7.5), np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_covariance_tracking(C.c_int32(nprob), C.c_int32(mx_), C.c_int32(mu_), C.c_int32(ml), C.c_int32(nlin), d(A_), d(Bu), d(Bl_), d(G), C.c_int32(n_gains),
                                         C.c_int32(nK), d(K_), C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), d(S0_), C.c_int32(N), d(S), d(Sall),
                                         d(cost) if cost_ else None, d(zs), d(us), d(tot) if total_ else None, C.byref(o))
        return rc, bool(all((x == 7.5).all() for x in (S, Sall, cost, zs, us, tot))), L.cclqr_last_error().decode()

    assert call()[0] == capi.OK and call(Wu_=None)[0] == capi.OK and call(S0_=None)[0] == capi.OK and call(N=1)[0] == capi.OK
    assert call(cost_=False, total_=False, Q_=None, R_=None)[0] == capi.OK
    refused = dict(nprob_0=call(nprob=0), mx_0=call(mx_=0), N_0=call(N=0), nlin_2=call(nlin=2), nlin_0=call(nlin=0), n_gains_2=call(n_gains=2), nK_2=call(nK=2),
                   n_weights_2=call(n_weights=2), n_weights_0=call(n_weights=0), n_noise_2=call(n_noise=2), n_noise_0=call(n_noise=0), no_source=call(Wu_=None, S0_=None),
                   Wu_with_mu_0=call(mu_=0), cost_without_Q=call(Q_=None), total_without_R=call(R_=None, cost_=False), A_null=call(A_=None), K_null=call(K_=None),
                   Bl_null=call(Bl_=None), path_3=call(path=3), path_neg=call(path=-1), bf16=call(bf16=1), too_many=call(nprob=65536, n_gains=1))
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
