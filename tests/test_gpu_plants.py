"""Per-instance plants on the GPU (cclqr_plants_create / cclqr_rollout_plants): every kernel shape of the chain kernel and the tree kernel, packed and
spread launches, against the CPU oracle run plant by plant on each plant's own tables -- and bit for bit against itself where a lane group could
evaluate another instance's line-search trial with its own plant (the lending trap)."""

import numpy as np
import pytest

from plants_common import TREE5, TREE14, mechanism_of, random_plants, starts

pytestmark = pytest.mark.gpu
TOL = 1e-9          # the project's rollout parity tolerance (tests/test_gpu_rollout.py)

# name: (mechanism, instances, steps, lanes per instance of its kernel)
CASES = {"links1": (("chain", 1), 11, 60, 8), "links3": (("chain", 3), 11, 60, 8), "links7": (("chain", 7), 6, 40, 16), "links16": (("chain", 16), 3, 30, 32),
         "links22": (("chain", 22), 3, 20, 32), "links40": (("chain", 40), 2, 15, 64), "tree14": (("tree", TREE14), 3, 30, 32), "tree5": (("tree", TREE5), 6, 30, 16)}
NAMES = list(CASES)
# packed and spread where a wavefront can hold more than one instance
LAUNCHES = [(n, p) for n in NAMES for p in ((True, False) if CASES[n][3] < 64 else (True,))]
LAUNCH_IDS = ["%s-%s" % (n, "packed" if p else "spread") for n, p in LAUNCHES]
_cache = {}


class Setup:
    pass


def setup_case(cclqr, orc, name):
    """mechanism, nominal-plant gains at the hanging setpoint, +-30 % / +-10 % plants, starts placed per plant, and the oracle's rollout of every
    instance on its own plant's tables -- computed once per case and shared by the tests"""
    if name in _cache:
        return _cache[name]
    capi = cclqr._capi
    case, n, steps, lanes = CASES[name]
    S = Setup()
    S.name, S.n, S.steps = name, n, steps
    S.mech, th0 = mechanism_of(cclqr, case)
    S.t = S.mech.tables()
    nb = S.t.nb
    S.h = capi.MechHandle(S.t)
    assert S.h.geometry()[0] == lanes
    zd = cclqr.joint_position_states(S.mech, th0[None])[0]
    lqr = cclqr.LQR(S.mech, [cclqr.getid(b) for b in S.mech.bodies], [cclqr.getid(S.mech.eqconstraints[0])], [np.eye(12)] * nb, [np.eye(1)],
                    (steps + 20) * S.t.dt, xd=[zd[i, 0:3] for i in range(nb)], qd=[zd[i, 3:7] for i in range(nb)])
    S.kw = dict(K=lqr.K, N=lqr.N, zd=lqr.zd)
    S.cj = lqr.ctrl_joints
    S.ctrl = capi.CtrlHandle(S.h, S.cj, **S.kw)
    S.pb = random_plants(cclqr, S.mech, n, seed=100 + len(name))
    S.ph = capi.PlantsHandle(S.h, S.pb.mass, S.pb.inertia, S.pb.p1, S.pb.p2)
    S.z0, S.th = starts(cclqr, S.mech, th0, n, seed=7, plants=S.pb)
    octrl = orc.ctrl_desc(nb, S.cj, **S.kw)
    res = [orc.rollout(S.pb.tables(i), octrl, S.z0[i:i + 1], steps, record=True) for i in range(n)]
    S.zT_o, S.traj_o, S.st_o = (np.concatenate([r[k] for r in res]) for k in range(3))
    _cache[name] = S
    return S


def launch(cclqr, S, z0, plants=None, first=0, packed=False, steps=None, single_step=False, ctrl=None):
    """device-pointer launch (cclqr_rollout_plants, or cclqr_rollout_ex when plants is None): (traj, zT, lam, status); single_step: one launch per step
    with the state and the multipliers carried (k0 continuation), the statuses of every step stacked"""
    import torch
    capi = cclqr._capi
    steps = S.steps if steps is None else steps
    n, nb = z0.shape[0], S.t.nb
    dev = torch.device("cuda", torch.cuda.current_device())
    z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
    zT, lam = torch.empty_like(z), torch.zeros((n, 5 * nb), dtype=torch.float64, device=dev)
    flags = capi.ROLLOUT_PACK_WAVEFRONTS if packed else 0
    ctrl = S.ctrl if ctrl is None else ctrl
    stream = torch.cuda.current_stream().cuda_stream
    if not single_step:
        traj = torch.empty((n, steps, nb, 13), dtype=torch.float64, device=dev)
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        capi.rollout_dev(S.h, ctrl, n, steps, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zT.data_ptr(), st.data_ptr(), stream,
                         first_instance=first, flags=flags, plants=plants)
        torch.cuda.synchronize()
        return traj.cpu().numpy(), zT.cpu().numpy(), lam.cpu().numpy(), st.cpu().numpy()
    traj, sts = [], []
    for k in range(1, steps + 1):
        st = torch.zeros(n, dtype=torch.int32, device=dev)
        traj.append(z.clone())
        capi.rollout_dev(S.h, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, 0, zT.data_ptr(), st.data_ptr(), stream, first_instance=first, flags=flags,
                         plants=plants)
        z, zT = zT, z
        sts.append(st)
    torch.cuda.synchronize()
    return torch.stack(traj, 1).cpu().numpy(), z.cpu().numpy(), lam.cpu().numpy(), torch.stack(sts, 1).cpu().numpy()


def oracle_ok(S):
    """the oracle converges on every plant"""
    assert (S.st_o > 0).all(), S.st_o


@pytest.mark.parametrize("name,packed", LAUNCHES, ids=LAUNCH_IDS)
def test_parity_with_the_oracle_on_each_plants_tables(cclqr, orc, name, packed):
    S = setup_case(cclqr, orc, name)
    oracle_ok(S)
    traj, zT, lam, st = launch(cclqr, S, S.z0, plants=S.ph, packed=packed)
    print(name, "packed" if packed else "spread", "status", st, "oracle", S.st_o, "err", np.abs(traj - S.traj_o).max(), np.abs(zT - S.zT_o).max())
    assert (st > 0).all()
    assert np.abs(traj - S.traj_o).max() < TOL and np.abs(zT - S.zT_o).max() < TOL
    # a launch that ignored the table would be the plain launch: that one is far away
    traj_p, zT_p, _, _ = launch(cclqr, S, S.z0, plants=None, packed=packed)
    print(name, "plain launch differs by", np.abs(traj_p - S.traj_o).max())
    assert np.nanmax(np.abs(traj_p - S.traj_o)) > 1e-3      # (nanmax: off its manifold the plain launch may lose an instance)


@pytest.mark.parametrize("name,packed", LAUNCHES, ids=LAUNCH_IDS)
def test_an_instance_alone_equals_its_row_of_the_batch_bitwise(cclqr, orc, name, packed):
    """the lending trap: in the batch launch idle lane groups sit next to instance i's line search; launched alone (n_inst = 1, first_instance = i) nobody
    does.  State, multipliers and status agree bit for bit only if no group ever evaluates a trial of an instance whose plant it does not hold.  So does a
    shard (first_instance = 2, two instances; with three instances the last two)."""
    S = setup_case(cclqr, orc, name)
    oracle_ok(S)
    traj, zT, lam, st = launch(cclqr, S, S.z0, plants=S.ph, packed=packed)
    for i in range(S.n):
        t1, z1, l1, s1 = launch(cclqr, S, S.z0[i:i + 1], plants=S.ph, first=i, packed=packed)
        assert np.array_equal(t1[0], traj[i]) and np.array_equal(z1[0], zT[i]) and np.array_equal(l1[0], lam[i]) and s1[0] == st[i], (name, i)
    if S.n >= 3:
        lo = 2 if S.n >= 4 else 1
        t2, z2, l2, s2 = launch(cclqr, S, S.z0[lo:lo + 2], plants=S.ph, first=lo, packed=packed)
        assert np.array_equal(t2, traj[lo:lo + 2]) and np.array_equal(z2, zT[lo:lo + 2]) and np.array_equal(l2, lam[lo:lo + 2]) and np.array_equal(s2, st[lo:lo + 2])


@pytest.mark.parametrize("mode", ["persistent", "persistent-packed", "single-step"])
@pytest.mark.parametrize("name", NAMES)
def test_nominal_plants_are_the_plain_launch_bitwise(cclqr, orc, name, mode):
    """a PlantBatch whose every row is the mechanism's own numbers reproduces cclqr_rollout_ex bit for bit -- trajectory, multipliers, Newton statuses --
    although its line search lends no lanes: the accept rule and the function that evaluates a level are the same"""
    capi = cclqr._capi
    S = setup_case(cclqr, orc, name)
    t = S.t
    tile = lambda a: np.tile(a[None], (S.n,) + (1,) * a.ndim)
    ph = capi.PlantsHandle(S.h, tile(t.mass), tile(t.inertia), tile(t.p1), tile(t.p2))
    z0 = cclqr.joint_position_states(S.mech, S.th)
    kw = dict(packed=mode == "persistent-packed", single_step=mode == "single-step", steps=S.steps if mode != "single-step" else min(S.steps, 12))
    a = launch(cclqr, S, z0, plants=ph, **kw)
    b = launch(cclqr, S, z0, plants=None, **kw)
    assert (b[3] > 0).all()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # (only some of the arrays given: the others are the mechanism's own)
    ph2 = capi.PlantsHandle(S.h, mass=tile(t.mass))
    assert np.array_equal(launch(cclqr, S, z0, plants=ph2, **kw)[0], b[0])


def test_friction_and_philox_noise_with_plants(cclqr, orc):
    """the friction + noise law of the tracking triple cartpole (Philox stream keyed by the global instance index) on per-instance plants"""
    capi = cclqr._capi
    ex = cclqr.examples.triple_cartpole()
    mech = ex["mech"]
    t = mech.tables()
    n, N = 6, 60
    z00 = mech.state()
    K = np.random.default_rng(2).normal(size=(N - 1, 1, 48)) * 0.3
    kw = dict(K=K, N=N, zd=np.tile(z00, (N, 1, 1)), fric=ex["fric"], noise_scale=2.0, noise_seed=0xBEEF)
    pb = random_plants(cclqr, mech, n, seed=3)
    z0, _ = starts(cclqr, mech, np.zeros(4), n, seed=4, plants=pb)
    octrl = orc.ctrl_desc(t.nb, [0], **kw)
    # (the oracle's stream is keyed by the instance's index in ITS batch: every plant runs the whole batch, row i is instance i on plant i)
    res = [orc.rollout(pb.tables(i), octrl, np.tile(z0[i], (n, 1, 1)), N, record=True) for i in range(n)]
    traj_o, st_o = np.stack([res[i][1][i] for i in range(n)]), np.array([res[i][2][i] for i in range(n)])
    assert (st_o > 0).all()
    h = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(h, [0], **kw)
    ph = capi.PlantsHandle(h, pb.mass, pb.inertia, pb.p1, pb.p2)
    zT, traj, st = capi.rollout(h, ctrl, z0, N, record=True, plants=ph)
    assert (st > 0).all()
    print("friction + noise: err", np.abs(traj - traj_o).max())
    assert np.abs(traj - traj_o).max() < TOL
    assert np.abs(capi.rollout(h, ctrl, z0, N, record=True)[1] - traj_o).max() > 1e-3
    zT_s, _, st_s = capi.rollout(h, ctrl, z0[2:4], N, first_instance=2, plants=ph)
    assert np.array_equal(zT_s, zT[2:4]) and np.array_equal(st_s, st[2:4])
    # through the public surface
    pub = cclqr.simulate(mech, cclqr.Storage(N, t.nb), cclqr.OpenLoop(mech, [cclqr.getid(ex["ctrl"][0])], np.zeros((N, 1))), z0=z0, plants=pb)
    one = orc.rollout(pb.tables(1), orc.ctrl_desc(t.nb, [0], N=N + 1, zd=np.tile(np.eye(1, 13, 3), (N, t.nb, 1)), Fd=np.zeros((N, 1))), z0[1:2], N, record=True)
    assert (pub.status > 0).all() and np.abs(pub.z[1] - one[1][0]).max() < TOL


def test_pid_with_plants(cclqr, orc):
    """the PID law (src/control/pid.jl) on the pendulum with per-instance masses and lengths"""
    capi = cclqr._capi
    ex = cclqr.examples.pendulum()
    mech = ex["mech"]
    t = mech.tables()
    n, steps = 5, 80
    pid = dict(joint=[0], P=[12.0], I=[3.0], D=[2.5], goal=[np.pi - 0.2])
    pb = random_plants(cclqr, mech, n, seed=8)
    z0 = cclqr.joint_position_states(mech, np.pi + np.random.default_rng(1).uniform(-0.4, 0.4, (n, 1)), plants=pb)
    octrl = orc.ctrl_desc(1, [], pid=pid)
    res = [orc.rollout(pb.tables(i), octrl, z0[i:i + 1], steps, record=True) for i in range(n)]
    traj_o, st_o = np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res])
    assert (st_o > 0).all()
    h = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(h, [], pid=pid)
    ph = capi.PlantsHandle(h, pb.mass, pb.inertia, pb.p1, pb.p2)
    zT, traj, st = capi.rollout(h, ctrl, z0, steps, record=True, plants=ph)
    print("pid: err", np.abs(traj - traj_o).max())
    assert (st > 0).all() and np.abs(traj - traj_o).max() < TOL
    assert np.abs(capi.rollout(h, ctrl, z0, steps, record=True)[1] - traj_o).max() > 1e-3
    st2 = cclqr.simulate(mech, cclqr.Storage(steps, 1), cclqr.PID(mech, cclqr.getid(ex["joints"][0]), np.pi - 0.2, P=12.0, I=3.0, D=2.5), z0=z0, plants=pb)
    assert np.array_equal(st2.z, traj)


def test_create_time_behaviour(cclqr, orc):
    """device pointers give bitwise the host-pointer result; the device-side validation names the right (plant, body); a closed-loop mechanism is
    CCLQR_EUNSUPPORTED; first_index slices; a launch outside the table is refused"""
    import torch
    capi = cclqr._capi
    S = setup_case(cclqr, orc, "links3")
    pb, n = S.pb, S.n
    ref = launch(cclqr, S, S.z0, plants=S.ph)
    dev = torch.device("cuda", torch.cuda.current_device())
    tens = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)]
    torch.cuda.synchronize()
    phd = capi.PlantsHandle(S.h, *[x.data_ptr() for x in tens], n_plant=n, on_device=True, stream=torch.cuda.current_stream().cuda_stream)
    for x, y in zip(launch(cclqr, S, S.z0, plants=phd), ref):
        assert np.array_equal(x, y)
    # first_index: the table of a shard
    sh = capi.PlantsHandle(S.h, pb.mass[4:9], pb.inertia[4:9], pb.p1[4:9], pb.p2[4:9], first_index=4)
    got = launch(cclqr, S, S.z0[5:8], plants=sh, first=5)
    assert np.array_equal(got[0], ref[0][5:8]) and np.array_equal(got[2], ref[2][5:8])
    for first, cnt in ((3, 2), (8, 2), (0, 1)):
        with pytest.raises(capi.CclqrError) as e:
            launch(cclqr, S, S.z0[:cnt], plants=sh, first=first)
        assert e.value.code == capi.EINVAL and "plants 4 .. 8" in str(e.value)
    other = capi.MechHandle(S.t)
    with pytest.raises(capi.CclqrError) as e:
        capi.rollout(other, capi.CtrlHandle(other, S.cj, **S.kw), S.z0, 2, plants=S.ph)
    assert e.value.code == capi.EINVAL and "another mechanism" in str(e.value)
    # device-side validation (the binding's handle uploads what it is given: the Python-side checks of PlantBatch are not in the way)
    m = pb.mass.copy(); m[6, 2] = 0.0; m[9, 0] = -1.0
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(S.h, mass=m)
    assert e.value.code == capi.EINVAL and "plant 6, body 2" in str(e.value) and "mass" in str(e.value)
    p = pb.p2.copy(); p[3, 1, 0] = np.inf
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(S.h, p2=p)
    assert e.value.code == capi.EINVAL and "plant 3, body 1" in str(e.value) and "non-finite" in str(e.value)
    J = pb.inertia.copy().reshape(n, 4, 3, 3); J[10, 3] = np.diag([1.0, 1.0, -1e-3])
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(S.h, inertia=J)
    assert e.value.code == capi.EINVAL and "plant 10, body 3" in str(e.value) and "inertia" in str(e.value)
    # body numbers are the caller's: on the permuted forest the offending body is reported under its own number
    from conftest import long_and_short_chain_forest
    t2 = long_and_short_chain_forest(cclqr)[0]
    h2 = capi.MechHandle(t2)
    m2 = np.tile(t2.mass[None], (3, 1)); m2[1, 11] = np.nan
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(h2, mass=m2)
    assert "plant 1, body 11" in str(e.value)
    # closed loops are out of scope
    db = cclqr.examples.deltabot()["mech"].tables()
    hd = capi.MechHandle(db)
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(hd, mass=np.tile(db.mass[None], (2, 1)))
    assert e.value.code == capi.EUNSUPPORTED
    with pytest.raises(capi.CclqrError) as e:
        capi.PlantsHandle(S.h, n_plant=0)
    assert e.value.code == capi.EINVAL
