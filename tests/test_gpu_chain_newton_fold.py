"""The chain kernel's Newton loop after the fold (rollout_chain.hip): ONE evaluation with Jacobians at the accepted point per iteration -- at the top of the
loop body, for the start of the step and for an iteration whose accepted point was not the full-step trial -- and a full-step trial that builds no Schur
rows when every instance of the wavefront that still solves is in an iteration known to be its last.  Neither changes a result: the cases below are the
wavefront compositions in which they could.  Tolerance against the oracle: the chain parity tests' (test_gpu_rollout.py), fp64, 1e-9 over the trajectory."""
import numpy as np
import pytest
import scipy.linalg as sl

from conftest import hanging_setpoint

TOL = 1e-9


def _hanging_chain(cclqr, orc, n_links, ninst, steps, seed):
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    zd = hanging_setpoint(cclqr, n_links)
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt, steps + 50)
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-0.3, 0.3, (ninst, n_links))
    phi[:, 0] += np.pi
    z0 = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, ninst), phi)
    return t, zd, K, z0


@pytest.fixture(scope="module")
def chain17(cclqr, orc):
    """the 17-body chain under its hanging-equilibrium LQR, three starts, 60 steps, and the oracle's rollout of them (computed once, never modified)"""
    steps = 60
    t, zd, K, z0 = _hanging_chain(cclqr, orc, 16, 3, steps, 21)
    ref = orc.rollout(t, orc.ctrl_desc(t.nb, [0], K=K, N=steps + 50, zd=zd), z0, steps, record=True)
    for a in ref:
        a.setflags(write=False)
    return dict(t=t, zd=zd, K=K, z0=z0, steps=steps, ref=ref)


def _spinning_start(cclqr, n_links=3, steps=20):
    """a 3-link chain whose links spin about their joint axes at 52-76 rad/s: the full Newton step of the first iterations overshoots"""
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    rng = np.random.default_rng(3)
    phi = rng.uniform(-0.3, 0.3, (1, n_links))
    phi[:, 0] += np.pi
    z0 = cclqr.examples.cartpole_states(n_links, [0.1], phi).copy()
    axis = np.asarray(t.axis)
    for i in range(1, t.nb):
        z0[0, i, 10:13] = 40.0 * (1 + 0.3 * i) * axis[i]
    K = rng.normal(size=(steps + 5, 1, 12 * t.nb)) * 0.05
    return t, z0, K, steps


def test_spinning_start_rejects_a_full_step_and_iterates_on(cclqr, orc):
    """(CPU) the start of test_both_reevaluation_paths_in_one_solve does what that test needs, by the oracle's own count: the first iteration of a solve
    halves, and more halvings happen than the solves' last iterations account for -- a rejected full step is followed by a further iteration"""
    t, z0, K, steps = _spinning_start(cclqr)
    orc.newton_stats(True)
    _, traj, st = orc.rollout(t, orc.ctrl_desc(t.nb, [0], K=K, N=steps + 6, zd=z0[0]), z0, steps, record=True, nthreads=1, flops=True)
    halvings, _, _, in_last = orc.newton_stats(True)
    assert (st > 0).all() and np.isfinite(traj).all()
    assert halvings[0] >= 1 and halvings.sum() > (np.arange(11) * in_last).sum(), (halvings, in_last)


@pytest.mark.gpu
def test_partner_absent(cclqr, chain17):
    """three instances of the 17-body chain: packed, instances 0 and 1 share a wavefront and instance 2 has none beside it; spread (the default for a
    small batch), every instance is alone.  A lone instance's known-last trial builds no rows in every step, a pair's only when both agree -- and
    states, trajectory and Newton counts are the same bit for bit, and the oracle's"""
    capi = cclqr._capi
    c = chain17
    mech = capi.MechHandle(c["t"])
    ctrl = capi.CtrlHandle(mech, [0], K=c["K"], N=c["steps"] + 50, zd=c["zd"])
    assert mech.instances_per_wavefront(3, c["steps"]) == 1 and mech.instances_per_wavefront(3, c["steps"], capi.ROLLOUT_PACK_WAVEFRONTS) == 2
    spread = capi.rollout(mech, ctrl, c["z0"], c["steps"], record=True)
    packed = capi.rollout(mech, ctrl, c["z0"], c["steps"], record=True, flags=capi.ROLLOUT_PACK_WAVEFRONTS)
    for x, y in zip(spread, packed):
        assert np.array_equal(x, y)
    zT_o, traj_o, st_o = c["ref"]
    assert (st_o > 0).all() and (packed[2] > 0).all()
    print("max |trajectory - oracle| = %.3g" % np.abs(packed[1] - traj_o).max())
    assert np.abs(packed[1] - traj_o).max() < TOL and np.abs(packed[0] - zT_o).max() < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dead", [0, 1])
def test_dead_partner(cclqr, chain17, dead):
    """two instances of the 17-body chain in one wavefront, one of them lost in an earlier launch (CCLQR_ROLLOUT_CARRY_STATUS brings it in dead): the first
    evaluation of every step runs for the live half of the wavefront only, and the live instance equals its solo run bit for bit"""
    import torch
    capi = cclqr._capi
    c = chain17
    steps, t = c["steps"], c["t"]
    live = 1 - dead
    mech = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(mech, [0], K=c["K"], N=steps + 50, zd=c["zd"])
    dev = torch.device("cuda", 0)

    def run(z0, status, flags):
        n = z0.shape[0]
        z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
        zn = torch.empty_like(z)
        traj = torch.zeros((n, steps, t.nb, 13), dtype=torch.float64, device=dev)
        lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
        s = torch.tensor(status, dtype=torch.int32, device=dev)
        capi.rollout_dev(mech, ctrl, n, steps, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zn.data_ptr(), s.data_ptr(), 0, flags=flags)
        torch.cuda.synchronize()
        return zn.cpu().numpy(), traj.cpu().numpy(), lam.cpu().numpy(), s.cpu().numpy()

    status = [0, 0]
    status[dead] = -3                    # lost in an earlier launch, after at most three iterations
    pair = run(c["z0"][:2], status, capi.ROLLOUT_CARRY_STATUS | capi.ROLLOUT_PACK_WAVEFRONTS)
    solo = run(c["z0"][live:live + 1], [0], capi.ROLLOUT_CARRY_STATUS | capi.ROLLOUT_PACK_WAVEFRONTS)
    assert pair[3][dead] == -3 and solo[3][0] > 0
    assert np.array_equal(pair[0][dead, :, 0:7], c["z0"][dead, :, 0:7])          # frozen at the pose it came in with
    for x, y in zip(pair, solo):
        assert np.array_equal(x[live], y[0])


@pytest.mark.gpu
def test_both_reevaluation_paths_in_one_solve(cclqr, orc):
    """8-lane shape (3-link chain), 20 steps from a start whose first full steps are rejected (test_spinning_start_... above): the accepted point of such an
    iteration is evaluated with Jacobians by the same call, at the top of the next iteration, that serves the start of a step"""
    capi = cclqr._capi
    t, z0, K, steps = _spinning_start(cclqr)
    zT_o, traj_o, st_o = orc.rollout(t, orc.ctrl_desc(t.nb, [0], K=K, N=steps + 6, zd=z0[0]), z0, steps, record=True)
    mech = capi.MechHandle(t)
    assert mech.geometry()[0] == 8
    ctrl = capi.CtrlHandle(mech, [0], K=K, N=steps + 6, zd=z0[0])
    zT, traj, st = capi.rollout(mech, ctrl, z0, steps, record=True)
    print("max |trajectory - oracle| = %.3g, Newton iterations %s (oracle %s)" % (np.abs(traj - traj_o).max(), st, st_o))
    assert (st > 0).all() and (st_o > 0).all() and st.max() > 5
    assert np.abs(traj - traj_o).max() < TOL and np.abs(zT - zT_o).max() < TOL


@pytest.mark.gpu
def test_sixteen_lane_shape(cclqr, orc):
    """8-link chain (16 lanes per instance, four instances per wavefront), 5 instances, 40 steps, against the oracle; packed (a full wavefront and a
    wavefront of one) and spread agree bit for bit"""
    capi = cclqr._capi
    steps = 40
    t, zd, K, z0 = _hanging_chain(cclqr, orc, 7, 5, steps, 22)
    zT_o, traj_o, st_o = orc.rollout(t, orc.ctrl_desc(t.nb, [0], K=K, N=steps + 50, zd=zd), z0, steps, record=True)
    mech = capi.MechHandle(t)
    assert mech.geometry()[0] == 16
    ctrl = capi.CtrlHandle(mech, [0], K=K, N=steps + 50, zd=zd)
    spread = capi.rollout(mech, ctrl, z0, steps, record=True)
    packed = capi.rollout(mech, ctrl, z0, steps, record=True, flags=capi.ROLLOUT_PACK_WAVEFRONTS)
    for x, y in zip(spread, packed):
        assert np.array_equal(x, y)
    print("max |trajectory - oracle| = %.3g" % np.abs(packed[1] - traj_o).max())
    assert (st_o > 0).all() and (packed[2] > 0).all()
    assert np.abs(packed[1] - traj_o).max() < TOL and np.abs(packed[0] - zT_o).max() < TOL
