"""StationaryLQR end to end (cclqr_ctrl_create_lqr_batch_doubling): cartpole_n(1) and cartpole_n(2) upright, on the mechanism's own plant (two weight pairs) and on
two perturbed plants (masses and inertias scaled), and the 16-link chain hanging (17 bodies, mx 204).
  * gains(i) and P(i) against cclqr_riccati_value(N = 2^levels + 1, tol = 0, keep_last) of the same library on the device's own linearisation (cclqr_linearize_plants).
    The bound is dlqr_reference.tolerance(e64) with e64 the deviation between the two numpy float64 twins of that model: the projected recursion stepped 2^levels
    times and the doubling schedule of riccati_doubling_common.  A case whose bound would reach the 1e-7 cap is not used (asserted).  The chain is held to this at
    max_levels = 6 (64 steps) and again converged (14 levels): there e64 is the larger of the float64 doubling twin's deviation from the stepping kernels at
    N = 2^levels + 1 (the parent's kernels: they share nothing with the code under test) and the two twins' deviation over 256 steps, what a numpy stepping twin of
    204 states can afford.
  * StationaryPolicyValue(.., horizon=None) of those gains reproduces P(i) within the same bound: the evaluation of the optimal gain is the Riccati P.
  * a rollout under StationaryLQR is bitwise the rollout under the same tables uploaded by the caller (what a PlantLQR's handle holds), and it balances the cartpole
    from the example's offset.
  * cartpole_n(6) upright is run and reported, not asserted: cond(I + G H) reaches 1e11 there."""
import numpy as np
import pytest

import dlqr_reference as ref
import riccati_doubling_common as rdc
from conftest import hanging_setpoint, upright_setpoint

pytestmark = pytest.mark.gpu

SCALE = np.array([[1.0, 1.0], [0.8, 1.3]])


def _case(cclqr, n, perturbed):
    """dict(mech, ids, eids, zd [2][nb][13], plants or None, Q, R as StationaryLQR takes them)"""
    ex = cclqr.examples.cartpole_n(n)
    mech = ex["mech"]
    t = mech.tables()
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    zd = np.stack([upright_setpoint(n)] * 2)
    if perturbed:
        s = np.ones((2, t.nb))
        s[:, :2] = SCALE
        plants = cclqr.PlantBatch(mech, mass=t.mass[None] * s, inertia=t.inertia[None] * s[:, :, None])
        return dict(mech=mech, ids=ids, eids=eids, zd=zd, plants=plants, Q=ex["Q"], R=ex["R"])
    return dict(mech=mech, ids=ids, eids=eids, zd=zd, plants=None, Q=[ex["Q"], [3.0 * q for q in ex["Q"]]], R=[ex["R"], ex["R"]])


def _models(cclqr, c, ctl):
    dev = cclqr.lqr._device_mech(c["mech"])
    n = c["zd"].shape[0]
    return cclqr._capi.linearize(dev, c["zd"], ctl.ctrl_joints, np.zeros((n, len(ctl.ctrl_joints))), plants=None if c["plants"] is None else c["plants"].handle(dev))


def _twin_bound(m, Q, R, levels):
    """tolerance(e64) of one model: the float64 projected recursion stepped 2^levels times against the float64 doubling schedule"""
    Ks, Ps = rdc.stepping(*m, Q, R, 2 ** levels, np.float64, True)
    Ap, D = rdc.project(*m)
    d = rdc.single_step(Ap, D, Q, R)
    for _ in range(levels):
        d = rdc.compose(d, d)[:3]
    Kd, Pd = rdc.final_step(Ap, D, Q, R, d[2])
    e64 = max(float(np.abs(Kd - Ks).max() / np.abs(Ks).max()), float(np.abs(Pd - Ps).max() / np.abs(Ps).max()))
    assert 10.0 * e64 < 1e-7, "the twins of this model differ by %.3g: the case is not usable" % e64
    return ref.tolerance(e64), e64


def _check_against_stepping(cclqr, c, sl, what):
    """gains(i), P(i) against cclqr_riccati_value at N = 2^levels + 1 on the device's own linearisation -> [bound per table]"""
    A, Bu, Bl, G = _models(cclqr, c, sl)
    bounds = []
    for i in range(c["zd"].shape[0]):
        Q, R = sl.Q[i if sl.Q.shape[0] > 1 else 0], sl.R[i if sl.R.shape[0] > 1 else 0]
        lv = int(sl.levels[i])
        Ks, Ps, _ = cclqr._capi.riccati_value(A[i], Bu[i], Bl[i], G[i], Q, R, 2 ** lv + 1, tol=0.0, keep_last=True)
        bound, e64 = _twin_bound((A[i], Bu[i], Bl[i], G[i]), Q, R, lv)
        K, P = sl.gains(i), sl.P(i)
        eK, eP = float(np.abs(K[0] - Ks[0, 0]).max() / np.abs(Ks).max()), float(np.abs(P - Ps[0]).max() / np.abs(Ps).max())
        print("%s table %d: levels %d reason %d dnorm %s anorm %s; against the stepping kernels K %.3g, P %.3g relative, bound %.3g (twins %.3g)"
              % (what, i, lv, sl.reason[i], sl.dnorm[i], sl.anorm[i], eK, eP, bound, e64))
        assert K.shape == (1, len(sl.ctrl_joints), A.shape[-1]) and eK <= bound and eP <= bound, (what, i)
        bounds.append(bound)
    return bounds


@pytest.mark.parametrize("n,perturbed", [(1, False), (1, True), (2, False), (2, True)])
def test_converged_gains_on_the_cartpoles(cclqr, n, perturbed):
    c = _case(cclqr, n, perturbed)
    sl = cclqr.StationaryLQR(c["mech"], c["ids"], c["eids"], c["Q"], c["R"], c["zd"], plants=c["plants"], keep_value=True)
    spv = None
    try:
        what = "cartpole_n(%d)%s" % (n, " on perturbed plants" if perturbed else "")
        assert sl.converged.all() and (sl.reason == 0).all() and (sl.levels <= 14).all() and (sl.steps == 2 ** sl.levels).all() and (sl.dnorm[:, 0] < 1e-5).all()
        assert sl.N == 0 and sl.n == 2 and sl.kbreak is None
        bounds = _check_against_stepping(cclqr, c, sl, what)
        # the evaluation of the optimal gain is the Riccati P
        spv = cclqr.StationaryPolicyValue(c["mech"], sl, c["ids"], c["eids"], c["Q"], c["R"], None, c["zd"], plants=c["plants"])
        assert spv.converged.all()
        for i in range(2):
            P = sl.P(i)
            dev = float(np.abs(spv.P(i) - P).max() / np.abs(P).max())
            print("%s table %d: StationaryPolicyValue of the gain against P %.3g relative, bound %.3g" % (what, i, dev, bounds[i]))
            assert dev <= bounds[i], (what, i)
    finally:
        if spv is not None:
            spv.close()
        sl.close()


def test_a_fixed_horizon_is_the_first_gain_of_that_horizon(cclqr):
    c = _case(cclqr, 1, True)
    sl = cclqr.StationaryLQR(c["mech"], c["ids"], c["eids"], c["Q"], c["R"], c["zd"], horizon=0.375, plants=c["plants"], keep_value=True)      # 38 knots
    try:
        assert (sl.steps == 37).all() and (sl.levels == 5).all() and (sl.reason == 0).all() and not sl.converged.any() and np.isnan(sl.dnorm).all()
        A, Bu, Bl, G = _models(cclqr, c, sl)
        for i in range(2):
            Ks, Ps, _ = cclqr._capi.riccati_value(A[i], Bu[i], Bl[i], G[i], sl.Q[0], sl.R[0], 38, tol=0.0, keep_last=True)
            Kt, Pt = rdc.stepping(A[i], Bu[i], Bl[i], G[i], sl.Q[0], sl.R[0], 37, np.float64, True)
            Ap, D = rdc.project(A[i], Bu[i], Bl[i], G[i])
            Kd, Pd = rdc.final_step(Ap, D, sl.Q[0], sl.R[0], rdc.doubling_fixed(rdc.single_step(Ap, D, sl.Q[0], sl.R[0]), 37)[0][2])
            bound = ref.tolerance(max(float(np.abs(Kd - Kt).max() / np.abs(Kt).max()), float(np.abs(Pd - Pt).max() / np.abs(Pt).max())))
            eK, eP = float(np.abs(sl.gains(i)[0] - Ks[0, 0]).max() / np.abs(Ks).max()), float(np.abs(sl.P(i) - Ps[0]).max() / np.abs(Ps).max())
            print("38 knots, plant %d: K %.3g, P %.3g relative to the stepping kernels, bound %.3g" % (i, eK, eP, bound))
            assert eK <= bound and eP <= bound
    finally:
        sl.close()


def test_the_hanging_chain_of_204_states(cclqr):
    ex = cclqr.examples.cartpole_n(16)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    c = dict(mech=mech, zd=hanging_setpoint(cclqr, 16)[None], plants=None)
    sl = cclqr.StationaryLQR(mech, ids, eids, ex["Q"], ex["R"], c["zd"], max_levels=6, tol=0.0, keep_value=True)
    try:
        assert sl.reason[0] == 1 and sl.levels[0] == 6 and not sl.converged[0]
        _check_against_stepping(cclqr, c, sl, "17-body chain, 64 steps")
    finally:
        sl.close()
    sl = cclqr.StationaryLQR(mech, ids, eids, ex["Q"], ex["R"], c["zd"], keep_value=True)
    try:
        print("17-body chain to convergence: levels %s reason %s dnorm %s anorm %s" % (sl.levels, sl.reason, sl.dnorm, sl.anorm))
        assert sl.converged[0] and sl.levels[0] <= 16
        A, Bu, Bl, G = _models(cclqr, c, sl)
        Ks, Ps, _ = cclqr._capi.riccati_value(A[0], Bu[0], Bl[0], G[0], sl.Q[0], sl.R[0], 2 ** int(sl.levels[0]) + 1, tol=0.0, keep_last=True)
        eK, eP = float(np.abs(sl.gains(0)[0] - Ks[0, 0]).max() / np.abs(Ks).max()), float(np.abs(sl.P(0) - Ps[0]).max() / np.abs(Ps).max())
        # the bound of the converged run: the float64 doubling twin of all its levels (14 numpy compositions) against the stepping kernels' result -- the parent's
        # kernels, which share nothing with the code under test -- and the two float64 twins against each other over the 256 steps a numpy stepping twin can afford
        lv = int(sl.levels[0])
        Ap, D = rdc.project(A[0], Bu[0], Bl[0], G[0])
        d = rdc.single_step(Ap, D, sl.Q[0], sl.R[0])
        for _ in range(lv):
            d = rdc.compose(d, d)[:3]
        Kd, Pd = rdc.final_step(Ap, D, sl.Q[0], sl.R[0], d[2])
        e_full = max(float(np.abs(Kd - Ks[0, 0]).max() / np.abs(Ks).max()), float(np.abs(Pd - Ps[0]).max() / np.abs(Ps).max()))
        e_256 = _twin_bound((A[0], Bu[0], Bl[0], G[0]), sl.Q[0], sl.R[0], 8)[1]
        e64 = max(e_full, e_256)
        assert 10.0 * e64 < 1e-7, "the twins of this model differ by %.3g: the case is not usable" % e64
        bound = ref.tolerance(e64)
        print("17-body chain to convergence against %d stepped backward steps: K %.3g, P %.3g relative, bound %.3g (doubling twin against the stepping kernels %.3g, twins "
              "over 256 steps %.3g)" % (2 ** lv, eK, eP, bound, e_full, e_256))
        assert eK <= bound and eP <= bound
    finally:
        sl.close()


def test_a_rollout_is_bitwise_that_of_the_same_tables_and_balances_the_cartpole(cclqr):
    capi = cclqr._capi
    c = _case(cclqr, 1, True)
    mech = c["mech"]
    sl = cclqr.StationaryLQR(mech, c["ids"], c["eids"], c["Q"], c["R"], c["zd"], plants=c["plants"])
    dev = cclqr.lqr._device_mech(mech)
    K = np.stack([sl.gains(i) for i in range(2)])
    host = capi.CtrlHandle(dev, sl.ctrl_joints, K=K, N=0, zd=c["zd"][:, None], Fd=np.zeros((2, 1, 1)), n_ctrl=2)
    try:
        z0 = np.tile(mech.state()[None], (2, 1, 1))      # the example's offset: y = 0.5, φ = 0.2
        steps = 1000     # the example's tend = 10 s
        st = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), sl, z0=z0, plants=c["plants"])
        zT, traj, status = capi.rollout(dev, host, z0, steps, k0=1, record=True, plants=c["plants"].handle(dev))
        assert (st.status > 0).all() and np.array_equal(st.status, status) and np.array_equal(st.zT, zT) and np.array_equal(st.z, traj)
        err = np.abs(st.zT - c["zd"]).max(axis=(1, 2))
        print("after %d steps: max |z - zd| = %s" % (steps, err))
        assert (err < 1e-2).all()
        with pytest.raises(ValueError, match="neither joint friction nor noise"):
            cclqr.simulate(mech, 0.05, sl, z0=z0, plants=c["plants"], noise_seed=1)
    finally:
        host.close()
        sl.close()


def test_predicted_cost_and_a_scored_rollout_take_it(cclqr):
    """predicted_cost(mech, StationaryLQR(keep_value=True), z0) is Δz' P(i) Δz about table i's setpoint; simulate(.., score=) scores the run and changes no state"""
    import score_common as sc
    c = _case(cclqr, 1, True)
    mech = c["mech"]
    sl = cclqr.StationaryLQR(mech, c["ids"], c["eids"], c["Q"], c["R"], c["zd"], plants=c["plants"], keep_value=True)
    try:
        z0 = np.tile(cclqr.examples.cartpole_states(1, [0.05], [[0.05]]), (2, 1, 1))
        V = cclqr.predicted_cost(mech, sl, z0)
        for i in range(2):
            dz, P = sc.state_errors(z0[i], c["zd"][i]).reshape(-1), sl.P(i)
            # a quadratic form of n = 24 terms per sum in fp64: |error| <= 2 n eps |Δz|' |P| |Δz|, whatever the order of the sums
            assert abs(V[i] - dz @ P @ dz) <= 2 * dz.size * np.finfo(float).eps * (np.abs(dz) @ np.abs(P) @ np.abs(dz)), (i, V[i], dz @ P @ dz)
        steps = 100
        plain = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), sl, z0=z0, plants=c["plants"], record=False)
        scored = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), sl, z0=z0, plants=c["plants"], record=False,
                                score=cclqr.Score(mech, c["ids"], c["eids"], c["Q"], c["R"]))
        J = scored.score[:, 0] + scored.score[:, 1]
        print("predicted %s, realised over %d steps %s" % (V, steps, J))
        assert (scored.status > 0).all() and np.array_equal(scored.zT, plain.zT) and np.array_equal(scored.status, plain.status)
        assert np.isfinite(scored.score).all() and (J > 0).all()
    finally:
        sl.close()


def test_the_six_link_cartpole_is_reported(cclqr):
    """cartpole_n(6) upright is genuinely ill-conditioned (cond(I + G H) reaches 1e11, max|P| 2.5e9): its levels, reason and deviation from stepping are printed"""
    ex = cclqr.examples.cartpole_n(6)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    c = dict(mech=mech, zd=upright_setpoint(6)[None], plants=None)
    sl = cclqr.StationaryLQR(mech, ids, eids, ex["Q"], ex["R"], c["zd"], keep_value=True)
    try:
        A, Bu, Bl, G = _models(cclqr, c, sl)
        lv = int(sl.levels[0])
        Ks, Ps, _ = cclqr._capi.riccati_value(A[0], Bu[0], Bl[0], G[0], sl.Q[0], sl.R[0], 2 ** lv + 1, tol=0.0, keep_last=True)
        K, P = sl.gains(0), sl.P(0)
        print("cartpole_n(6): levels %d reason %d dnorm %s anorm %s max|P| %.3g; against %d stepped steps K %.3g, P %.3g relative"
              % (lv, sl.reason[0], sl.dnorm[0], sl.anorm[0], np.abs(P).max(), 2 ** lv, np.abs(K[0] - Ks[0, 0]).max() / np.abs(Ks).max(), np.abs(P - Ps[0]).max() / np.abs(Ps).max()))
        assert sl.reason[0] in (0, 1, 2, 3)
    finally:
        sl.close()
