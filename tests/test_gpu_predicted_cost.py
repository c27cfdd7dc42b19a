"""The predicted cost end to end: PlantLQR and LQRSweep with keep_value=True on the cartpole, predicted_cost against the realised cost of the run.

Two plants -- the masses and inertias of (cart, pole) scaled (1, 1) and (0.8, 1.3) --, N = 41 knots, tol = 0, starts y = φ = ε for ε = 0.05 4^-j, j = 0, 1, 2.
V = Δz' P Δz is what the gains achieve on the LINEAR model over exactly the N steps the run is scored on (N - 1 gated inputs and the terminal weight Q), so
J / V - 1 with J = Jx + Ju of simulate(..., score=Score(Q, R)) is the nonlinear remainder: second order in ε.
  * each quartering of ε shrinks |J / V - 1| at least 8-fold (16 expected);
  * at the smallest ε it is at most twice the value the CPU gives from the oracle's rollout and the extended-precision reference P (the factor is a margin on a
    small difference: the device's 1e-9 state parity is far below it);
  * with the other plant's P it exceeds 0.1 -- the table index is right.
Oracle, own P: plant A -1.05e-2 / -6.7e-4 / -4.2e-5, plant B -1.34e-2 / -8.7e-4 / -5.4e-5; other plant's P: between -0.29 and +0.40 at every ε.
The trend once more with the break active (N = 1001, tol = 1e-5; oracle, plant A: kbreak 110, 3.6e-3 / 2.3e-4 / 1.5e-5)."""
import numpy as np
import pytest

import dlqr_reference as ref
import score_common as sc
from riccati_value_common import check_P, reference_P

pytestmark = pytest.mark.gpu

EPS = [0.05 * 4.0 ** -j for j in range(3)]
SCALE = np.array([[1.0, 1.0], [0.8, 1.3]])
_setup = {}


def setup(cclqr):
    """dict(mech, nb, ids, eids, Q, R, plants, zd [2][nb][13]), built once"""
    if not _setup:
        ex = cclqr.examples.cartpole_n(1)
        mech = ex["mech"]
        t = mech.tables()
        plants = cclqr.PlantBatch(mech, mass=t.mass[None] * SCALE, inertia=t.inertia[None] * SCALE[:, :, None])
        zd = cclqr.joint_position_states(mech, np.zeros((2, 2)), plants=plants)
        _setup.update(mech=mech, t=t, nb=t.nb, ids=[cclqr.getid(b) for b in ex["bodies"]], eids=[cclqr.getid(j) for j in ex["ctrl"]], Q=ex["Q"], R=ex["R"],
                      plants=plants, zd=zd)
    return _setup


def starts(cclqr, eps):
    """[2][nb][13]: the start y = φ = ε once per plant (the plants differ in mass and inertia only: one constraint manifold)"""
    return np.tile(cclqr.examples.cartpole_states(1, [eps], [[eps]]), (2, 1, 1))


def horizon_of(mech, N):
    return (N - 0.5) * mech.Δt


def realised(cclqr, s, ctl, eps, N):
    st = cclqr.simulate(s["mech"], cclqr.Storage(N, s["nb"]), ctl, z0=starts(cclqr, eps), plants=s["plants"], record=False,
                        score=cclqr.Score(s["mech"], s["ids"], s["eids"], s["Q"], s["R"]))
    assert (st.status > 0).all()
    return st.score[:, 0] + st.score[:, 1]


def cpu_remainder(cclqr, orc, s, i, K, P, eps, N):
    """J / V - 1 of plant i on the CPU: J from the oracle's rollout under the gains K (scored by score_common's restatement), V from the matrix P"""
    Qm, Rm = cclqr.lqr._weights_and_horizon(s["Q"], s["R"], horizon_of(s["mech"], N), s["mech"].Δt)[:2]
    z0 = starts(cclqr, eps)[i:i + 1]
    ctrl = orc.ctrl_desc(s["nb"], [s["mech"].joint_index(e) for e in s["eids"]], K=K, N=N, zd=s["zd"][i])
    _, traj, status = orc.rollout(s["plants"].tables(i), ctrl, z0, N, record=True)
    assert (status > 0).all()
    Qb = np.stack([Qm[12 * b:12 * b + 12, 12 * b:12 * b + 12] for b in range(s["nb"])])
    cx, cu, _, _ = sc.stage_costs(traj, s["zd"][i][None, None], K[None], N, Qb, Rm)
    dz = sc.state_errors(z0[0], s["zd"][i]).reshape(-1)
    return float((cx.sum() + cu.sum()) / (dz @ P @ dz) - 1.0)


@pytest.mark.parametrize("kind", ["PlantLQR", "LQRSweep"])
def test_keep_value_changes_no_gain_and_keeps_the_reference_cost_to_go(cclqr, kind):
    """the constructor's gains and kbreak are bitwise those of the same call without keep_value; P(i) is within the suite's bound of the extended-precision
    recursion on the model the constructor linearised (cclqr_linearize_plants: the same launch)"""
    s = setup(cclqr)
    N = 41
    args = (s["ids"], s["eids"])
    if kind == "PlantLQR":
        make = lambda **kw: cclqr.PlantLQR(s["mech"], s["plants"], *args, s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], tol=0.0, **kw)
    else:
        make = lambda **kw: cclqr.LQRSweep(s["mech"], *args, [s["Q"], [q * 3.0 for q in s["Q"]]], [s["R"]], horizon_of(s["mech"], N), s["zd"], plants=s["plants"], tol=0.0, **kw)
    kept, plain = make(keep_value=True), make()
    try:
        assert plain._handle.value is None
        with pytest.raises(ValueError, match="without keep_value=True"):
            plain.P(0)
        dev = cclqr.lqr._device_mech(s["mech"])
        A, Bu, Bl, G = cclqr._capi.linearize(dev, s["zd"], kept.ctrl_joints, kept.Fd, plants=s["plants"].handle(dev))
        for i in range(2):
            assert np.array_equal(kept.gains(i), plain.gains(i)) and kept.kbreak[i] == plain.kbreak[i], (kind, i)
            Qi, Ri = (kept.Q, kept.R) if kind == "PlantLQR" else (kept.Q[i], kept.R[i])
            check_P(kept.P(i), reference_P(A[i], Bu[i], Bl[i], G[i], Qi, Ri, N, 0.0), "%s table %d" % (kind, i))
        assert np.abs(kept.P(0) - kept.P(1)).max() > 1e-2 * np.abs(kept.P(0)).max()
    finally:
        kept.close()
        plain.close()


def test_realised_over_predicted_cost_is_second_order_in_the_start(cclqr, orc):
    import torch
    capi = cclqr._capi
    s = setup(cclqr)
    N = 41
    ctl = cclqr.PlantLQR(s["mech"], s["plants"], s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], tol=0.0, keep_value=True)
    dev = cclqr.lqr._device_mech(s["mech"])
    swapped = capi.ValueHandle(dev, np.stack([ctl.P(1), ctl.P(0)]))
    try:
        r, rw = np.zeros((3, 2)), np.zeros((3, 2))
        for j, eps in enumerate(EPS):
            J = realised(cclqr, s, ctl, eps, N)
            z0 = starts(cclqr, eps)
            V = cclqr.predicted_cost(s["mech"], ctl, z0)
            zt = torch.from_numpy(z0).cuda()
            Vt = cclqr.predicted_cost(s["mech"], ctl, zt)
            assert _is_tensor(Vt) and np.array_equal(Vt.cpu().numpy(), V)                 # a device tensor in and out: the same bits
            assert np.array_equal(cclqr.predicted_cost(s["mech"], ctl, z0[1:], first_instance=1), V[1:])
            Vw = torch.empty(2, dtype=torch.float64, device="cuda")
            capi.value_eval(dev, ctl._handle, swapped, 2, zt.data_ptr(), Vw.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            r[j], rw[j] = J / V - 1.0, J / Vw.cpu().numpy() - 1.0
            print("eps %.6g: J %s V %s J/V - 1 %s, with the other plant's P %s" % (eps, J, V, r[j], rw[j]))
        assert (np.abs(r[:-1]) >= 8.0 * np.abs(r[1:])).all(), r
        assert (np.abs(rw) > 0.1).all(), rw
        A, Bu, Bl, G = capi.linearize(dev, s["zd"], ctl.ctrl_joints, ctl.Fd, plants=s["plants"].handle(dev))
        for i in range(2):
            Pref = reference_P(A[i], Bu[i], Bl[i], G[i], ctl.Q, ctl.R, N, 0.0)[0]
            rc = cpu_remainder(cclqr, orc, s, i, ctl.gains(i), Pref, EPS[-1], N)
            print("plant %d, eps %.6g: J/V - 1 = %.4g on the device, %.4g on the CPU" % (i, EPS[-1], r[-1, i], rc))
            assert abs(r[-1, i]) <= 2.0 * abs(rc), (i, r[-1, i], rc)
    finally:
        swapped.close()
        ctl.close()


def _is_tensor(a):
    return hasattr(a, "data_ptr") and a.is_cuda


def test_the_trend_holds_with_the_break_active(cclqr):
    """N = 1001, tol = 1e-5: the recursion breaks (plant A: kbreak 110), the gains below it are back-filled and P is the Pkp1 of the step the test fired on"""
    s = setup(cclqr)
    N = 1001
    ctl = cclqr.PlantLQR(s["mech"], s["plants"], s["ids"], s["eids"], s["Q"], s["R"], horizon_of(s["mech"], N), s["zd"], tol=1e-5, keep_value=True)
    try:
        assert 1 < ctl.kbreak[0] < N - 1
        r = np.array([(realised(cclqr, s, ctl, eps, N) / cclqr.predicted_cost(s["mech"], ctl, starts(cclqr, eps)) - 1.0)[0] for eps in EPS])
        print("kbreak %s, plant A J/V - 1 %s" % (ctl.kbreak, r))
        assert (np.abs(r[:-1]) >= 8.0 * np.abs(r[1:])).all(), r
    finally:
        ctl.close()
