"""StationaryPolicyValue end to end on the cartpole, with the setup of tests/test_gpu_predicted_cost.py (two plants: masses and inertias of (cart, pole) scaled (1, 1)
and (0.8, 1.3)).  ONE nominal LQR(horizon = inf, keep_value=True), designed on plant A, holds one stationary gain.
  * over N = 1001 knots its StationaryPolicyValue is PolicyValue(..., tol = 0) at the same N on both plants: P(i) within the acceptance bound of
    tests/policy_doubling_common.py (the longdouble stepping reference on the device's own linearisation gives the bound), predicted_cost takes it as it stands --
    a numpy array and a device tensor give the same bits -- and V equals PolicyValue's V within the bound.
  * horizon=None, tol = 1e-5: converged on both plants, spectral_radius < 1, at most 13 levels, P within the bound of the longdouble stepping reference.
  * simulate(..., spv) raises TypeError; the refusals of cclqr_value_create_policy_doubling."""
import math

import numpy as np
import pytest

import dlqr_reference as ref
import policy_doubling_common as pdc
import policy_value_common as pvc
import score_common as sc
from test_gpu_predicted_cost import EPS, horizon_of, setup, starts

pytestmark = pytest.mark.gpu

N = 1001
_made = {}


def nominal(cclqr):
    if "lqr" not in _made:
        s = setup(cclqr)
        z = s["zd"][0]
        _made["lqr"] = cclqr.LQR(s["mech"], s["ids"], s["eids"], s["Q"], s["R"], math.inf, keep_value=True, xd=[b[0:3] for b in z], qd=[b[3:7] for b in z],
                                 vd=[b[7:10] for b in z], ωd=[b[10:13] for b in z])
    return _made["lqr"]


def _models(cclqr, s, ctl):
    dev = cclqr.lqr._device_mech(s["mech"])
    return cclqr._capi.linearize(dev, s["zd"], ctl.ctrl_joints, np.zeros((2, len(ctl.ctrl_joints))), plants=s["plants"].handle(dev))


def test_a_fixed_horizon_is_the_stepping_policy_value(cclqr):
    import torch
    s = setup(cclqr)
    lqr = nominal(cclqr)
    assert lqr.K.shape[0] == 1
    args = (s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"])
    spv = cclqr.StationaryPolicyValue(*args, plants=s["plants"])
    pv = cclqr.PolicyValue(*args, plants=s["plants"], tol=0.0)
    try:
        assert spv.N == pv.N == N and spv.n_models == 2 and (spv.steps == N - 1).all() and (spv.levels == 9).all()      # 1000 = 0b1111101000: nine doublings
        assert not spv.converged.any() and not spv.diverged.any() and np.isnan(spv.dnorm).all() and np.isfinite(spv.gnorm[:, 0]).all()
        A, Bu, Bl, G = _models(cclqr, s, lqr)
        z0 = starts(cclqr, EPS[0])
        V, Vs = cclqr.predicted_cost(s["mech"], spv, z0), cclqr.predicted_cost(s["mech"], pv, z0)
        Vt = cclqr.predicted_cost(s["mech"], spv, torch.from_numpy(z0).cuda())
        assert hasattr(Vt, "data_ptr") and Vt.is_cuda and np.array_equal(Vt.cpu().numpy(), V)      # a device tensor in and out: the same bits
        for i in range(2):
            refp = pvc.reference(A[i], Bu[i], Bl[i], G[i], lqr.Q, lqr.R, lqr.K, N, 0.0)
            Abar, Qbar = pdc.closed_loop(A[i], Bu[i], Bl[i], G[i], lqr.Q, lqr.R, lqr.K[0], np.float64, True)
            P64 = pdc.doubling_fixed(Abar, Qbar, np.asarray(lqr.Q, dtype=np.float64), N - 1)[0]
            e64 = max(refp[3], float(np.abs(P64 - refp[0]).max() / np.abs(refp[0]).max()))
            bound, scale = ref.tolerance(e64), float(np.abs(refp[0]).max())
            err, errs, dev = (float(np.abs(X).max()) / scale for X in (spv.P(i) - refp[0], pv.P(i) - refp[0], spv.P(i) - pv.P(i)))
            print("plant %d: doubling %.3g, stepping %.3g relative to the reference, doubling against stepping %.3g, bound %.3g (e64P %.3g); V %.17g against %.17g"
                  % (i, err, errs, dev, bound, e64, V[i], Vs[i]))
            assert err <= bound and dev <= bound, i
            # V = Δz' P Δz: |V - Vs| = |Δz' (P - Ps) Δz| <= (sum |Δz|)^2 max|P - Ps| <= (sum |Δz|)^2 bound max|Pref|
            dz = sc.state_errors(z0[i], s["zd"][i]).reshape(-1)
            assert abs(V[i] - Vs[i]) <= float(np.abs(dz).sum()) ** 2 * bound * scale, i
        with pytest.raises(TypeError, match="not a Controller"):
            cclqr.simulate(s["mech"], 0.1, spv)
    finally:
        spv.close()
        pv.close()


def test_the_infinite_horizon_cost_converges_on_both_plants(cclqr):
    s = setup(cclqr)
    lqr = nominal(cclqr)
    spv = cclqr.StationaryPolicyValue(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], None, s["zd"], plants=s["plants"], tol=1e-5)
    try:
        print("levels %s, steps %s, reason %s, dnorm %s, gnorm %s, spectral radius %s" % (spv.levels, spv.steps, spv.reason, spv.dnorm, spv.gnorm, spv.spectral_radius))
        assert spv.N == 0 and spv.converged.all() and not spv.diverged.any() and (spv.spectral_radius < 1.0).all() and (spv.levels <= 13).all()
        assert (spv.steps == 2 ** spv.levels).all() and (spv.dnorm[:, 0] < 1e-5).all()
        A, Bu, Bl, G = _models(cclqr, s, lqr)
        for i in range(2):
            refp = pdc.converge_reference(A[i], Bu[i], Bl[i], G[i], lqr.Q, lqr.R, lqr.K[0], 1e-5, 40)
            pdc.check_conv(spv.P(i), spv.levels[i], spv.reason[i], spv.dnorm[i], spv.gnorm[i], refp, "StationaryPolicyValue to convergence, plant %d" % i)
    finally:
        spv.close()


def test_refusals_of_value_create_policy_doubling(cclqr):
    capi = cclqr._capi
    s = setup(cclqr)
    lqr = nominal(cclqr)
    dev = cclqr.lqr._device_mech(s["mech"])
    cj = lqr.ctrl_joints
    good = lqr._ctrl_handle(dev)
    table = capi.CtrlHandle(dev, cj, K=np.zeros((40, 1, 24)), N=41, zd=s["zd"][0])
    tracking = capi.CtrlHandle(dev, cj, K=np.zeros((40, 1, 24)), N=41, zd=np.tile(s["zd"][0], (41, 1, 1)))
    no_gains = capi.CtrlHandle(dev, cj, K=None, N=0)
    loop_dev = cclqr.lqr._device_mech(cclqr.examples.fourbar()["mech"])
    handles = [good, table, tracking, no_gains]

    def code(mech=dev, ctrl=good, zd=s["zd"][:1], n=10, tol=0.0, max_levels=40, Q=lqr.Q, R=lqr.R):
        try:
            v = capi.value_create_policy_doubling(mech, ctrl, zd, cj, Q, R, n, tol=tol, max_levels=max_levels)[0]
        except capi.CclqrError as e:
            return e.code
        v.close()
        return capi.OK

    try:
        assert code() == capi.OK and code(n=0) == capi.OK and code(n=1) == capi.OK
        assert code(ctrl=table) == capi.EINVAL                                               # more than one gain row: the stepping entry's business
        assert code(ctrl=tracking) == capi.EUNSUPPORTED
        assert code(ctrl=no_gains) == capi.EINVAL
        assert code(n=-1) == capi.EINVAL and code(n=0, max_levels=0) == capi.EINVAL and code(n=0, max_levels=61) == capi.EINVAL
        assert code(tol=-1.0) == capi.EINVAL and code(tol=float("nan")) == capi.EINVAL
        assert code(zd=s["zd"], Q=np.stack([lqr.Q] * 3), R=np.stack([lqr.R] * 3)) == capi.EINVAL                     # 3 pairs of weights, 2 models
        assert code(mech=loop_dev, zd=np.zeros((1, 3, 13)), Q=np.eye(36)) == capi.EUNSUPPORTED
    finally:
        for h in handles:
            h.close()
