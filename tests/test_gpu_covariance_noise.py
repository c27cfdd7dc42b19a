"""StationaryCovariance end to end on the cartpole, with the setup of tests/test_gpu_predicted_cost.py: one LQR(horizon = math.inf) at zd[0].
  * 2048 noisy rollouts of 200 steps from the setpoint (noise_scale = 1e-3, one Philox stream per instance) against the 200-step covariance: every diagonal entry of
    the sample second moment S = Δz'Δz / n with Σ_ii >= 1e-3 max Σ_ii lies within 6 sqrt(2 / n) = 0.1875 relative of Σ_ii -- six standard deviations of a Gaussian
    sample variance; the instances' streams are independent by construction of the Philox key, and at σ = 1e-3 the states stay within 1e-4 of the setpoint, so the
    nonlinear remainder is orders below that.  (On the CPU oracle with the same seed: 6 of 24 entries compared, the largest deviation 0.0204.  The 200-step Σ differs
    from the steady state by up to 62 % on those entries, so the test tells them apart; it does not resolve an off-by-one in the step count, 0.03 %: the fixed
    horizons of tests/test_gpu_covariance.py do.)
  * the actuator effort: input_std² against the sample mean of (K Δz)², under the same bound.
  * both plants to convergence: converged, spectral radius < 1, Σ and the moments within the rule of tests/covariance_common.py against the longdouble reference on the
    device's own linearisation; simulate(..., cov) and predicted_cost(..., cov, ...) raise TypeError.
  * bodyids in reversed order: Sigma0 is permuted as Q is and state_std comes back in that order (N = 1: Σ = Σ0 bitwise).
  * the refusals of cclqr_value_create_covariance_doubling, with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import covariance_common as cc
import dlqr_reference as ref
import score_common as sc
from test_gpu_policy_doubling_cost import _models, nominal
from test_gpu_predicted_cost import horizon_of, setup

pytestmark = pytest.mark.gpu

N_INST, STEPS, SIGMA, SEED = 2048, 200, 1e-3, 1234
BOUND = 6.0 * np.sqrt(2.0 / N_INST)


def test_noisy_rollouts_show_the_predicted_spread_of_states_and_of_actuator_effort(cclqr):
    s = setup(cclqr)
    lqr = nominal(cclqr)
    z0 = np.ascontiguousarray(np.tile(s["zd"][0], (N_INST, 1, 1)))
    st = cclqr.simulate(s["mech"], cclqr.Storage(STEPS, s["nb"]), lqr, z0=z0, record=False, noise_scale=SIGMA, noise_seed=SEED)
    assert (st.status > 0).all()
    dz = sc.state_errors(st.zT, s["zd"][0]).reshape(N_INST, -1)
    S = dz.T @ dz / N_INST
    cov = cclqr.StationaryCovariance(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], STEPS + 1), s["zd"][:1], noise_scale=SIGMA)
    try:
        assert cov.N == STEPS + 1 and (cov.steps == STEPS).all() and not cov.converged.any()
        Sig = cov.Sigma(0)
        d = np.diag(Sig)
        big = d >= 1e-3 * d.max()
        ratio = np.diag(S)[big] / d[big]
        print("entries compared %d of %d; S_ii / Σ_ii = %s; max |Δz| = %.3g; bound %.4f" % (big.sum(), len(d), ratio, np.abs(dz).max(), BOUND))
        assert big.sum() >= 6
        assert np.abs(ratio - 1.0).max() <= BOUND
        # state_std is sqrt(diag Σ) in the order of bodyids (here the mechanism's own)
        order = np.concatenate([12 * (int(b) - 1) + np.arange(12) for b in s["ids"]])
        assert np.array_equal(cov.state_std[0], np.sqrt(np.maximum(d[order], 0.0)))
        u2 = float(np.mean((dz @ lqr.K[0].T) ** 2))
        print("sample mean of (K Δz)² = %.6g against input_std² = %.6g: ratio %.4f" % (u2, cov.input_std[0, 0] ** 2, u2 / cov.input_std[0, 0] ** 2))
        assert abs(u2 / cov.input_std[0, 0] ** 2 - 1.0) <= BOUND
        # the expected stage costs are the traces of the same Σ
        assert abs(cov.stage_cost[0, 0] - np.sum(cov.Q[0] * Sig.T)) <= 1e-12 * np.sum(np.abs(cov.Q[0]) * np.abs(Sig))
    finally:
        cov.close()


def test_both_plants_to_convergence(cclqr):
    s = setup(cclqr)
    lqr = nominal(cclqr)
    cov = cclqr.StationaryCovariance(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], None, s["zd"], noise_scale=SIGMA, plants=s["plants"])
    try:
        print("levels %s, steps %s, reason %s, dnorm %s, gnorm %s, spectral radius %s, stage cost %s, input std %s" % (
            cov.levels, cov.steps, cov.reason, cov.dnorm, cov.gnorm, cov.spectral_radius, cov.stage_cost, cov.input_std))
        assert cov.N == 0 and cov.converged.all() and not cov.diverged.any() and (cov.spectral_radius < 1.0).all() and (cov.steps == 2 ** cov.levels).all()
        A, Bu, Bl, G = _models(cclqr, s, lqr)
        Wu = SIGMA ** 2 * np.ones((1, 1))
        order = np.concatenate([12 * (int(b) - 1) + np.arange(12) for b in s["ids"]])
        for i in range(2):
            r = cc.converge_reference(A[i], Bu[i], Bl[i], G[i], lqr.Q, lqr.R, lqr.K[0], Wu, cov.tol, cov.max_levels)
            zstd = np.empty(24)
            zstd[order] = cov.state_std[i]      # back to the mechanism's body order
            cc.check_conv(cov.Sigma(i), cov.stage_cost[i], zstd, cov.input_std[i], cov.levels[i], cov.reason[i], cov.dnorm[i], cov.gnorm[i], r,
                          "StationaryCovariance to convergence, plant %d" % i)
        with pytest.raises(TypeError, match="not a Controller"):
            cclqr.simulate(s["mech"], cclqr.Storage(2, s["nb"]), cov)
        with pytest.raises(TypeError, match="keep_value"):
            cclqr.predicted_cost(s["mech"], cov, s["zd"])
    finally:
        cov.close()


def test_reversed_bodyids_permute_sigma0_and_state_std(cclqr):
    """no step (a horizon of one knot): Σ = Σ0, so Sigma(0) is Σ0's blocks in the mechanism's body order and state_std is sqrt(diag Σ0) in the order of bodyids, bitwise"""
    s = setup(cclqr)
    lqr = nominal(cclqr)
    ids = list(reversed(s["ids"]))
    assert ids != list(s["ids"])
    S0 = ref._spd(np.random.default_rng(7), 24)                                                     # in the order of `ids`
    place = np.concatenate([12 * ids.index(b) + np.arange(12) for b in sorted(ids)])                 # where each coordinate of the mechanism's order lies in S0
    cov = cclqr.StationaryCovariance(s["mech"], lqr, ids, s["eids"], list(reversed(s["Q"])), s["R"], horizon_of(s["mech"], 1), s["zd"][:1], Sigma0=S0)
    try:
        assert cov.N == 1 and (cov.steps == 0).all()
        assert np.array_equal(cov.Sigma(0), S0[np.ix_(place, place)])
        assert np.array_equal(cov.state_std[0], np.sqrt(np.diag(S0)))
        assert not np.array_equal(cov.Sigma(0), S0)
    finally:
        cov.close()


def test_refusals_of_value_create_covariance_doubling_leave_the_outputs_untouched(cclqr):
    capi = cclqr._capi
    L = capi.lib()
    s = setup(cclqr)
    lqr = nominal(cclqr)
    dev = cclqr.lqr._device_mech(s["mech"])
    cj = np.ascontiguousarray(lqr.ctrl_joints, dtype=np.int32)
    good = lqr._ctrl_handle(dev)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    zd = np.ascontiguousarray(s["zd"])
    Q, R = np.ascontiguousarray(lqr.Q), np.ascontiguousarray(lqr.R)
    W3, S1 = np.ones((3, 1, 1)), np.ascontiguousarray(np.eye(24))
    SENTINEL = 0x5A5A

    def call(n_weights=1, Q_=Q, R_=R, n_noise=1, Wu_=W3, S0_=S1, N=10, tol=1e-8, max_levels=40):
        cost, zs, us = np.full((2, 2), 7.5), np.full((2, 24), 7.5), np.full((2, 1), 7.5)
        lv, rs = np.full(2, -9, dtype=np.int32), np.full(2, -9, dtype=np.int32)
        dn, gn = np.full((2, 2), 7.5), np.full((2, 2), 7.5)
        out = C.c_void_p(SENTINEL)
        rc = L.cclqr_value_create_covariance_doubling(dev.ptr, None, C.c_int64(0), C.c_int32(2), d(zd), C.c_int32(1), cj.ctypes.data_as(ip), None, good.ptr,
                                                      C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), d(S0_), C.c_int32(N), C.c_double(tol),
                                                      C.c_int32(max_levels), d(cost), d(zs), d(us), lv.ctypes.data_as(ip), rs.ctypes.data_as(ip), d(dn), d(gn),
                                                      C.byref(out))
        untouched = bool(all((x == 7.5).all() for x in (cost, zs, us, dn, gn)) and (lv == -9).all() and (rs == -9).all() and out.value == SENTINEL)
        if rc == capi.OK:
            capi.check(L.cclqr_value_destroy(out))
        return rc, untouched

    try:
        rc, untouched = call()
        assert rc == capi.OK and not untouched
        refused = dict(cost_without_Q=call(Q_=None), cost_without_R=call(R_=None), n_noise_3_Wu_only=call(n_noise=3, S0_=None),
                       n_noise_3_start_only=call(n_noise=3, Wu_=None, S0_=np.ascontiguousarray(np.stack([S1] * 3))), no_source=call(Wu_=None, S0_=None),
                       start_with_N_0=call(N=0), N_neg=call(N=-1), levels_61=call(N=0, S0_=None, max_levels=61), tol_nan=call(tol=float("nan")),
                       n_weights_3=call(n_weights=3))
        for what, (rc, untouched) in refused.items():
            assert rc == capi.EINVAL and untouched, (what, rc, untouched)
    finally:
        good.close()


def test_refusals_of_value_create_covariance_doubling(cclqr):
    capi = cclqr._capi
    s = setup(cclqr)
    lqr = nominal(cclqr)
    dev = cclqr.lqr._device_mech(s["mech"])
    cj = lqr.ctrl_joints
    good = lqr._ctrl_handle(dev)
    table = capi.CtrlHandle(dev, cj, K=np.zeros((40, 1, 24)), N=41, zd=s["zd"][0])
    tracking = capi.CtrlHandle(dev, cj, K=np.zeros((40, 1, 24)), N=41, zd=np.tile(s["zd"][0], (41, 1, 1)))
    loop_dev = cclqr.lqr._device_mech(cclqr.examples.fourbar()["mech"])
    handles = [good, table, tracking]
    W1, S1 = np.ones((1, 1)), np.eye(24)

    def code(mech=dev, ctrl=good, zd=s["zd"][:1], n=10, tol=0.0, max_levels=40, Q=lqr.Q, R=lqr.R, Wu=W1, S0=S1):
        try:
            v = capi.value_create_covariance_doubling(mech, ctrl, zd, cj, Q, R, Wu, S0, n, tol=tol, max_levels=max_levels)[0]
        except capi.CclqrError as e:
            return e.code
        v.close()
        return capi.OK

    try:
        assert code() == capi.OK and code(n=0, S0=None) == capi.OK and code(n=1) == capi.OK and code(Wu=None) == capi.OK
        assert code(ctrl=table) == capi.EINVAL                                               # more than one gain row
        assert code(ctrl=tracking) == capi.EUNSUPPORTED
        assert code(n=-1) == capi.EINVAL and code(n=0, S0=None, max_levels=0) == capi.EINVAL and code(n=0, S0=None, max_levels=61) == capi.EINVAL
        assert code(tol=-1.0) == capi.EINVAL and code(tol=float("nan")) == capi.EINVAL
        assert code(n=0) == capi.EINVAL                                                      # a start with the steady state
        assert code(Wu=None, S0=None) == capi.EINVAL                                         # nothing to propagate
        assert code(zd=s["zd"], Wu=np.stack([W1] * 3), S0=np.stack([S1] * 3)) == capi.EINVAL  # 3 noise matrices, 2 models
        assert code(mech=loop_dev, zd=np.zeros((1, 3, 13)), Q=np.eye(36), S0=np.eye(36)) == capi.EUNSUPPORTED
    finally:
        for h in handles:
            h.close()
