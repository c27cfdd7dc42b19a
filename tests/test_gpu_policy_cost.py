"""PolicyValue end to end on the cartpole, with the setup of tests/test_gpu_predicted_cost.py: two plants -- the masses and inertias of (cart, pole) scaled (1, 1)
(plant A) and (0.8, 1.3) (plant B) --, N = 41 knots, tol = 0, starts y = φ = ε for ε = 0.05 4^-j, j = 0, 1, 2.  ONE nominal LQR, designed on plant A, is rolled out on
both plants (simulate(..., plants=, score=)); J = Jx + Ju is the realised cost, V = Δz' P Δz the predicted one.
  * PolicyValue(nominal) on plant A: its P is the nominal LQR's kept P within the acceptance rule of tests/policy_value_common.py (the gains' own model).
  * With the policy P of each plant, |J / V - 1| is the nonlinear remainder on BOTH plants: it shrinks at least 8-fold per quartering of ε (16 expected) and at the
    smallest ε is at most twice the CPU value (the oracle's rollout under the same gains, the extended-precision policy reference).
  * With the nominal Riccati P in place of the policy P -- what predicted_cost(mech, nominal, z0) gives -- plant B's |J / V - 1| does NOT shrink: it is model
    mismatch, not nonlinearity.  Floor: half the smallest oracle value.
Oracle (CPU; gains: the float64 dlqr on plant A's oracle linearisation; rollout: the oracle's; P: the longdouble recursions), J / V - 1 at the three ε:
    plant A, policy P = nominal P (equal to 6e-22):  -1.054e-2   -6.742e-4   -4.220e-5
    plant B, policy P:                               -2.204e-2   -1.437e-3   -9.007e-5
    plant B, nominal Riccati P:                      +0.4111     +0.4410     +0.4429       (floor asserted: 0.2055)
The policy P of plant B differs from the nominal P by 5.6e-2 relative.  (0.8, 1.3) gives 0.41 >= 0.02: the plant is not scaled further.
  * PolicyValue of a PlantLQR (table k on plant k) reproduces its kept P(k) within the rule.
  * A stationary LQR(horizon = Inf) over N = 1001 steps with tol = 1e-5 reports converged on both plants, with contraction < 1.
  * The refusals of cclqr_value_create_policy."""
import ctypes as C
import math

import numpy as np
import pytest

import dlqr_reference as ref
import policy_value_common as pvc
import score_common as sc
from test_gpu_predicted_cost import EPS, horizon_of, realised, setup, starts

pytestmark = pytest.mark.gpu

N = 41
FLOOR_B_NOMINAL = 0.5 * 0.4111      # half the smallest oracle value of plant B's |J / V - 1| under the nominal Riccati P (module docstring)
_made = {}


def _setpoint_kw(zd0):
    return dict(xd=[z[0:3] for z in zd0], qd=[z[3:7] for z in zd0], vd=[z[7:10] for z in zd0], ωd=[z[10:13] for z in zd0])


def nominal(cclqr, horizon=None):
    """the one nominal LQR of the module (designed on the mechanism's own plant = plant A), kept value; horizon None: the N = 41 knots"""
    key = "inf" if horizon is not None else "finite"
    if key not in _made:
        s = setup(cclqr)
        _made[key] = cclqr.LQR(s["mech"], s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N) if horizon is None else horizon, keep_value=True,
                               **_setpoint_kw(s["zd"][0]))
    return _made[key]


def _models(cclqr, s, ctl):
    dev = cclqr.lqr._device_mech(s["mech"])
    return cclqr._capi.linearize(dev, s["zd"], ctl.ctrl_joints, np.zeros((2, len(ctl.ctrl_joints))), plants=s["plants"].handle(dev))


def test_policy_value_on_the_design_plant_is_the_kept_cost_to_go(cclqr):
    s = setup(cclqr)
    lqr = nominal(cclqr)
    assert lqr.kbreak == 1 and lqr.K.shape[0] == N - 1      # (the constructor's tol = 1e-5 never fired: every step ran, as with tol = 0)
    pv = cclqr.PolicyValue(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"][:1], plants=s["plants"], tol=0.0)
    try:
        A, Bu, Bl, G = _models(cclqr, s, lqr)
        refp = pvc.reference(A[0], Bu[0], Bl[0], G[0], lqr.Q, lqr.R, lqr.K, N, 0.0)
        pvc.check(pv.P(0), pv.kbreak[0], pv.dnorm[0], refp, "PolicyValue(nominal) on plant A")
        pvc.check(lqr.P, 1, None, refp, "the nominal LQR's kept P against the policy reference of its own gains")
        bound, scale = ref.tolerance(refp[3]), np.abs(lqr.P).max()
        assert np.abs(pv.P(0) - lqr.P).max() <= bound * scale
        assert pv.n_models == 1 and not pv.converged[0] and pv.dnorm.shape == (1, 2) and pv.contraction.shape == (1,)
        with pytest.raises(TypeError, match="not a Controller"):
            cclqr.simulate(s["mech"], 0.1, pv)
    finally:
        pv.close()


def test_policy_cost_is_second_order_on_both_plants_and_the_nominal_cost_is_not(cclqr, orc):
    import torch
    s = setup(cclqr)
    lqr = nominal(cclqr)
    pv = cclqr.PolicyValue(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], plants=s["plants"], tol=0.0)
    try:
        assert np.abs(pv.P(1) - lqr.P).max() > 1e-2 * np.abs(lqr.P).max()
        r, rn = np.zeros((3, 2)), np.zeros((3, 2))
        for j, eps in enumerate(EPS):
            J = realised(cclqr, s, lqr, eps, N)
            z0 = starts(cclqr, eps)
            V = cclqr.predicted_cost(s["mech"], pv, z0)
            Vt = cclqr.predicted_cost(s["mech"], pv, torch.from_numpy(z0).cuda())
            assert hasattr(Vt, "data_ptr") and Vt.is_cuda and np.array_equal(Vt.cpu().numpy(), V)      # a device tensor in and out: the same bits
            Vn = cclqr.predicted_cost(s["mech"], lqr, z0)
            r[j], rn[j] = J / V - 1.0, J / Vn - 1.0
            print("eps %.6g: J %s, policy V %s -> J/V - 1 %s; nominal V %s -> %s" % (eps, J, V, r[j], Vn, rn[j]))
        assert (np.abs(r[:-1]) >= 8.0 * np.abs(r[1:])).all(), r
        assert (np.abs(rn[:, 1]) >= FLOOR_B_NOMINAL).all(), rn
        A, Bu, Bl, G = _models(cclqr, s, lqr)
        Qb = np.stack([lqr.Q[12 * b:12 * b + 12, 12 * b:12 * b + 12] for b in range(s["nb"])])
        for i in range(2):
            Pref = pvc.policy_sweep(A[i], Bu[i], Bl[i], G[i], lqr.Q, lqr.R, lqr.K, N, 0.0)[0].astype(np.float64)
            z0 = starts(cclqr, EPS[-1])[i:i + 1]
            ctrl = orc.ctrl_desc(s["nb"], lqr.ctrl_joints, K=lqr.K, N=N, zd=s["zd"][i])
            _, traj, status = orc.rollout(s["plants"].tables(i), ctrl, z0, N, record=True)
            assert (status > 0).all()
            cx, cu, _, _ = sc.stage_costs(traj, s["zd"][i][None, None], lqr.K[None], N, Qb, lqr.R)
            dz = sc.state_errors(z0[0], s["zd"][i]).reshape(-1)
            rc = float((cx.sum() + cu.sum()) / (dz @ Pref @ dz) - 1.0)
            print("plant %d, eps %.6g: J/V - 1 = %.4g on the device, %.4g on the CPU" % (i, EPS[-1], r[-1, i], rc))
            assert abs(r[-1, i]) <= 2.0 * abs(rc), (i, r[-1, i], rc)
    finally:
        pv.close()


def test_policy_value_of_a_plant_lqr_reproduces_its_kept_cost_to_go(cclqr):
    s = setup(cclqr)
    ctl = cclqr.PlantLQR(s["mech"], s["plants"], s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], tol=0.0, keep_value=True)
    pv = None
    try:
        pv = cclqr.PolicyValue(s["mech"], ctl, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], plants=s["plants"], tol=0.0)
        A, Bu, Bl, G = _models(cclqr, s, ctl)
        for k in range(2):
            refp = pvc.reference(A[k], Bu[k], Bl[k], G[k], ctl.Q, ctl.R, ctl.gains(k), N, 0.0)
            pvc.check(pv.P(k), pv.kbreak[k], pv.dnorm[k], refp, "PolicyValue(PlantLQR) table %d on plant %d" % (k, k))
            assert np.abs(pv.P(k) - ctl.P(k)).max() <= ref.tolerance(refp[3]) * np.abs(ctl.P(k)).max(), k
        assert np.abs(pv.P(0) - pv.P(1)).max() > 1e-2 * np.abs(pv.P(0)).max()
    finally:
        if pv is not None:
            pv.close()
        ctl.close()


def test_a_stationary_gain_converges_on_both_plants(cclqr):
    s = setup(cclqr)
    lqr = nominal(cclqr, math.inf)
    assert lqr.K.shape[0] == 1
    pv = cclqr.PolicyValue(s["mech"], lqr, s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], 1001), s["zd"], plants=s["plants"], tol=1e-5)
    try:
        print("N %d, kbreak %s, dnorm %s, contraction %s" % (pv.N, pv.kbreak, pv.dnorm, pv.contraction))
        assert pv.N == 1001 and pv.converged.all() and (pv.contraction < 1.0).all() and (pv.kbreak > 1).all()
    finally:
        pv.close()


def test_refusals_of_value_create_policy(cclqr):
    capi = cclqr._capi
    s = setup(cclqr)
    lqr = nominal(cclqr)
    dev = cclqr.lqr._device_mech(s["mech"])
    cj = lqr.ctrl_joints
    good = lqr._ctrl_handle(dev)
    other_mech = cclqr.examples.cartpole_n(2)["mech"]
    other = capi.CtrlHandle(cclqr.lqr._device_mech(other_mech), cj, K=np.zeros((1, 1, 36)), N=0)
    no_gains = capi.CtrlHandle(dev, cj, K=None, N=0)
    tracking = capi.CtrlHandle(dev, cj, K=np.zeros((N - 1, 1, 24)), N=N, zd=np.tile(s["zd"][0], (N, 1, 1)))
    two_tables = capi.CtrlHandle(dev, cj, K=np.zeros((2, 1, 24)), N=0, zd=s["zd"], n_ctrl=2)
    loop = cclqr.examples.fourbar()["mech"]
    loop_dev = cclqr.lqr._device_mech(loop)
    ph = s["plants"].handle(dev)
    handles = [good, other, no_gains, tracking, two_tables]

    def code(mech=dev, ctrl=good, zd=s["zd"][:1], joints=cj, n=N, plants=None, first_plant=0, Q=lqr.Q, R=lqr.R):
        try:
            v, _, _ = capi.value_create_policy(mech, ctrl, zd, joints, Q, R, n, tol=0.0, plants=plants, first_plant=first_plant)
        except capi.CclqrError as e:
            return e.code
        v.close()
        return capi.OK

    try:
        assert code() == capi.OK
        assert code(joints=[1 - cj[0]]) == capi.EINVAL                                       # ctrl_joint that is not the controller's
        assert code(ctrl=no_gains) == capi.EINVAL
        assert code(ctrl=other) == capi.EINVAL                                               # made for another mechanism
        assert code(ctrl=tracking) == capi.EUNSUPPORTED                                      # more than one setpoint row per table
        assert code(ctrl=two_tables, zd=np.tile(s["zd"][:1], (3, 1, 1))) == capi.EINVAL      # 2 tables, 3 models
        assert code(ctrl=two_tables, zd=s["zd"]) == capi.OK
        assert code(n=N - 1) == capi.EINVAL                                                  # N - 1 gain rows require N
        assert code(zd=s["zd"], Q=np.stack([lqr.Q] * 3), R=np.stack([lqr.R] * 3)) == capi.EINVAL                     # 3 pairs of weights, 2 models
        assert code(mech=loop_dev, zd=np.zeros((1, 3, 13)), Q=np.eye(36)) == capi.EUNSUPPORTED
        assert code(plants=ph, first_plant=5) == capi.EINVAL                                 # the refusals of cclqr_linearize_plants
        out = C.c_void_p()
        rc = capi.lib().cclqr_value_create_policy(dev.ptr, None, C.c_int64(0), C.c_int32(1), None, C.c_int32(1), None, None, good.ptr, C.c_int32(1), None, None,
                                                  C.c_int32(N), C.c_double(0.0), None, None, C.byref(out))
        assert rc == capi.EINVAL and not out.value
    finally:
        for h in handles:
            h.close()
