"""cclqr_rollout_score on the device (csrc/score.hip): synthetic slabs against the numpy restatement of the definition (tests/score_common.py: Jx, Ju, peak within
1e-10 A, last_out exact), chunk invariance bit for bit, scored real rollouts through simulate(..., score=), and the refusals of the C ABI."""
import math

import numpy as np
import pytest

import plants_common as pc
import score_common as sc
from conftest import long_and_short_chain_forest

pytestmark = pytest.mark.gpu

_MECH = {}


def _chain(cclqr, nb):
    if nb not in _MECH:
        _MECH[nb] = cclqr._capi.MechHandle(sc.chain_tables(cclqr, nb))
    return _MECH[nb]


def gpu_score(cclqr, mech, case, settle_tol, cj, k0=1, first_instance=0, init=None, slab=None):
    """controller and weights of `case` on the device, one cclqr_rollout_score launch over `slab` (default: the case's whole slab); returns score [n][4].
    The score buffer comes in as `init` (k0 > 1) or full of NaN (k0 = 1: it must not be read)."""
    import torch
    capi = cclqr._capi
    nb = mech.tables.nb
    n_ctrl = case["zd"].shape[0]
    mu = case["R"].shape[0]
    K = case["K"]
    ctrl = capi.CtrlHandle(mech, cj, K=None if K is None else K.reshape(-1, mu, 12 * nb), N=case["N"], zd=case["zd"].reshape(-1, nb, 13), n_ctrl=n_ctrl if n_ctrl > 1 else 0)
    sh = capi.ScoreHandle(mech, case["Qb"], case["R"], settle_tol)
    try:
        traj = torch.from_numpy(np.ascontiguousarray(case["traj"] if slab is None else slab)).cuda()
        n, steps = traj.shape[:2]
        s = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda") if init is None else torch.from_numpy(np.ascontiguousarray(init)).cuda()
        capi.rollout_score(mech, ctrl, sh, n, steps, k0, traj.data_ptr(), s.data_ptr(), torch.cuda.current_stream().cuda_stream, first_instance=first_instance)
        torch.cuda.synchronize()
        return s.cpu().numpy()
    finally:
        sh.close()
        ctrl.close()


def check_case(cclqr, mech, case, cj, k0=1, first_instance=0, what=""):
    cx, cu, Ax, Au = sc.stage_costs(case["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"], k0=k0, first_instance=first_instance)
    tol = sc.settle_tol_between(cx)
    n = cx.shape[0]
    init = None
    if k0 > 1:
        init = np.abs(np.random.default_rng(7).normal(size=(n, 4)))
        init[:, 3] = np.arange(n) % k0
    ref, A = sc.score_of(cx, cu, Ax, Au, tol, k0=k0, init=init)
    got = gpu_score(cclqr, mech, case, tol, cj, k0=k0, first_instance=first_instance, init=init)
    sc.assert_score(got, ref, A, what)
    return got, ref


# ---------------------------------------------------------------- a. synthetic slabs
@pytest.mark.parametrize("kind", ["inf", "gated", "tracking"])
@pytest.mark.parametrize("nb", [1, 2, 5, 8, 9, 17, 33, 64])
def test_synthetic_slabs_match_the_definition(cclqr, nb, kind):
    """nb: every lane-group size (8, 16, 32, 64 lanes) and its first overflow; inside: mu 1, 3, 7 (at most the mechanism's joints), one table and first_instance 2 of
    n_inst + 2 tables (5 instances: 2 of 7), n_inst 1, 5, 67 (no multiple of the instances per wavefront), k0 1 and 4; an 8-step window (it crosses N = 5 / 6)"""
    mech = _chain(cclqr, nb)
    for mu in sorted({min(m, nb) for m in (1, 3, 7)}):
        for multi in (False, True):
            for n_inst in (1, 5, 67):
                for k0 in (1, 4):
                    n_ctrl, first = (n_inst + 2, 2) if multi else (1, 0)
                    case = sc.synthetic_case(nb, mu, kind, n_ctrl, n_inst, 8, seed=100000 * nb + 1000 * mu + 10 * n_inst + 2 * k0 + multi)
                    check_case(cclqr, mech, case, list(range(mu)), k0=k0, first_instance=first,
                               what="nb %d mu %d %s n_ctrl %d n_inst %d k0 %d" % (nb, mu, kind, n_ctrl, n_inst, k0))


def test_permuted_body_numbering(cclqr):
    """the link-order trap: the slab is in the caller's body order, the controller's K columns and setpoints in link order -- a 13-link and a 3-link chain with their
    bodies interleaved in the caller's numbering"""
    t2, _, zd, K, cj = long_and_short_chain_forest(cclqr)
    mech = cclqr._capi.MechHandle(t2)
    assert list(cclqr.link_order(t2)[0]) != list(range(t2.nb))
    case = sc.synthetic_case(t2.nb, 2, "inf", 1, 5, 8, seed=21)
    zd = zd.copy()
    zd[:, 7:] = np.random.default_rng(3).normal(size=(t2.nb, 6)) * 0.1
    case.update(N=21, K=K[None], zd=zd[None, None])
    rng = np.random.default_rng(4)
    traj = zd[None, None] + 0.1 * rng.normal(size=(5, 8, t2.nb, 13))
    traj[..., 3:7] /= np.linalg.norm(traj[..., 3:7], axis=-1, keepdims=True)
    case["traj"] = traj
    check_case(cclqr, mech, case, cj, what="forest")
    check_case(cclqr, mech, case, cj, k0=15, what="forest k0 15")      # (crosses nK = 20 and N = 21)


def test_branching_tree_and_closed_loops(cclqr):
    """TREE5 (a body with two child joints) and the two closed-loop mechanisms, where the joints outnumber the bodies (deltabot 7 on 5, four-bar 4 on 3: mu up to 7)"""
    tree = pc.hanging_tree(cclqr, pc.TREE5).tables()
    delta = cclqr.examples.deltabot()["mech"].tables()
    four = cclqr.examples.fourbar()["mech"].tables()
    for seed, (name, t, mu) in enumerate((("tree5", tree, 3), ("deltabot", delta, 7), ("deltabot", delta, 2), ("fourbar", four, 4), ("fourbar", four, 1))):
        assert mu <= t.ne
        mech = cclqr._capi.MechHandle(t)
        for kind in ("inf", "gated", "tracking"):
            for multi in (False, True):
                case = sc.synthetic_case(t.nb, mu, kind, 7 if multi else 1, 5, 8, seed=100 * seed + 10 * len(kind) + multi)
                check_case(cclqr, mech, case, list(range(mu)), first_instance=2 if multi else 0, what="%s mu %d %s" % (name, mu, kind))


def test_a_nan_in_one_row_changes_that_instance_alone(cclqr):
    mech = _chain(cclqr, 5)
    case = sc.synthetic_case(5, 3, "gated", 1, 5, 8, seed=3)
    clean = dict(case, traj=case["traj"].copy())
    case["traj"][2, 3, 1, 8] = np.nan
    cx, cu, Ax, Au = sc.stage_costs(clean["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"])
    tol = sc.settle_tol_between(cx)
    ref, A = sc.score_of(*sc.stage_costs(case["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"]), tol)
    assert np.isnan(ref[2, :3]).all() and ref[2, 3] >= 4
    got = gpu_score(cclqr, mech, case, tol, [0, 1, 2])
    got0 = gpu_score(cclqr, mech, clean, tol, [0, 1, 2])
    sc.assert_score(got, ref, A, "planted NaN")
    others = [0, 1, 3, 4]
    assert np.array_equal(got[others], got0[others])
    # behind the gate (k >= N = 5) the feedback command is zero: a NaN there leaves Ju alone
    late = dict(clean, traj=clean["traj"].copy())
    late["traj"][2, 6, 1, 8] = np.nan
    gl = gpu_score(cclqr, mech, late, tol, [0, 1, 2])
    assert np.isnan(gl[2, 0]) and np.isnan(gl[2, 2]) and gl[2, 1] == got0[2, 1] and gl[2, 3] >= 7


# ---------------------------------------------------------------- b. chunk invariance
@pytest.mark.parametrize("nb,kind", [(9, "tracking"), (17, "gated"), (64, "inf")])
def test_chunked_scoring_is_bitwise_one_call(cclqr, nb, kind):
    mech = _chain(cclqr, nb)
    case = sc.synthetic_case(nb, min(3, nb), kind, 1, 5, 23, seed=nb)
    cj = list(range(min(3, nb)))
    whole = gpu_score(cclqr, mech, case, 0.5, cj)
    assert np.isfinite(whole).all()
    for plan in ([1] * 23, [7, 7, 7, 2], [20, 3]):
        s, k0 = None, 1
        for n in plan:
            s = gpu_score(cclqr, mech, case, 0.5, cj, k0=k0, init=s, slab=case["traj"][:, k0 - 1:k0 - 1 + n])
            k0 += n
        assert np.array_equal(s, whole), plan


# ---------------------------------------------------------------- c. real rollouts
def scored_runs(cclqr, mech, steps, ctl, score, z0, K, zd, N, **kw):
    """simulate without score, with score= unrecorded in chunks of 7, and recorded: zT and status bitwise equal, the two scores bitwise equal, and the score of the
    recorded trajectory within the tolerance of the numpy reference.  Returns (recorded Storage, reference score)"""
    z00 = mech.state()
    plain = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), ctl, record=False, z0=z0, **kw)
    mech.set_state(z00)
    a = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), ctl, record=False, z0=z0, score=score, chunk_steps=7, **kw)
    mech.set_state(z00)
    b = cclqr.simulate(mech, cclqr.Storage(steps, len(mech.bodies)), ctl, record=True, z0=z0, score=score, **kw)
    mech.set_state(z00)
    assert (plain.status > 0).all()
    assert np.array_equal(a.zT, plain.zT) and np.array_equal(a.status, plain.status) and a.z.shape[1] == 0
    assert np.array_equal(b.zT, plain.zT) and np.array_equal(b.status, plain.status) and b.z.shape[1] == steps
    assert a.score.shape == (len(z0), 4) and np.array_equal(a.score, b.score)
    first = kw.get("first_instance", 0)
    cx, cu, Ax, Au = sc.stage_costs(b.z, zd, K, N, score.Qb, score.R, first_instance=first)
    ref, A = sc.score_of(cx, cu, Ax, Au, score.settle_tol)
    return b, ref, A, cx


def with_threshold(cclqr, mech, ids, eq, Q, R, run):
    """two passes: the first run's recorded stage costs choose settle_tol (between two neighbours, score_common.settle_tol_between), the second is checked"""
    probe = cclqr.Score(mech, ids, eq, Q, R, settle_tol=0.0)
    _, _, _, cx = run(probe)
    score = cclqr.Score(mech, ids, eq, Q, R, settle_tol=sc.settle_tol_between(cx))
    b, ref, A, _ = run(score)
    sc.assert_score(b.score, ref, A, "rollout")
    return b, ref


def test_scored_cartpole_under_an_infinite_horizon_lqr(cclqr):
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eq = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])]
    lqr = cclqr.LQR(mech, ids, eq, ex["Q"], ex["R"], math.inf, xd=ex["xd"])
    rng = np.random.default_rng(0)
    z0 = cclqr.examples.cartpole_states(1, rng.uniform(-0.5, 0.5, 5), rng.uniform(0.05, 0.3, (5, 1)))
    b, ref = with_threshold(cclqr, mech, ids, eq, ex["Q"], ex["R"],
                            lambda s: scored_runs(cclqr, mech, 40, lqr, s, z0, lqr.K[None], lqr.zd[None], lqr.N))
    assert (b.score[:, 0] > 0).all() and (b.score[:, 1] > 0).all() and (b.score[:, 2] <= b.score[:, 0]).all()
    one = b.instance(3)
    assert np.array_equal(one.score, b.score[3:4]) and np.array_equal(one.zT, b.zT[3:4])
    # an OpenLoop controller has no feedback command: Ju is exactly zero
    ol = cclqr.OpenLoop(mech, eq, np.zeros((40, 1)))
    s = cclqr.Score(mech, ids, eq, ex["Q"], ex["R"], settle_tol=1e-3)
    so = cclqr.simulate(mech, cclqr.Storage(40, 2), ol, record=False, z0=z0, score=s, chunk_steps=7)
    assert (so.score[:, 1] == 0.0).all() and (so.score[:, 0] > 0).all()


def test_scored_triple_cartpole_tracking_with_friction_and_philox_noise(cclqr):
    ex = cclqr.examples.triple_cartpole()
    mech = ex["mech"]
    N = 40
    ids, eq = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])]
    z00 = mech.state()
    U = 5.0 * np.sin(np.arange(N) * 0.1).reshape(N, 1)
    ref_run = cclqr.simulate(mech, cclqr.Storage(N, 4), cclqr.OpenLoop(mech, eq, U), z0=z00[None])
    mech.set_state(z00)
    trk = cclqr.TrackingLQR(mech, ref_run, U, eq, ex["Q"], ex["R"])
    z0 = np.tile(z00, (5, 1, 1))
    kw = dict(fric=ex["fric"], noise_scale=2.0, noise_seed=0xC0FFEE, first_instance=3)
    b, ref = with_threshold(cclqr, mech, ids, eq, ex["Q"], ex["R"],
                            lambda s: scored_runs(cclqr, mech, N, trk, s, z0, trk.K[None], trk.zd[None], trk.N, **kw))
    assert len({float(x) for x in b.score[:, 0]}) == 5      # (the Philox streams differ by instance)


def test_scored_run_with_injected_noise_indexes_it_by_the_absolute_step(cclqr):
    """an injected noise array [n_inst][steps] under chunked launches: every chunk reads column k - 1 of the SAME array (base unshifted, stride = steps), so the
    chunked scored run is bitwise the one-launch run -- an offset by k0 would change zT"""
    ex = cclqr.examples.triple_cartpole()
    mech = ex["mech"]
    N = 40
    ids, eq = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])]
    z00 = mech.state()
    U = 5.0 * np.sin(np.arange(N) * 0.1).reshape(N, 1)
    ref_run = cclqr.simulate(mech, cclqr.Storage(N, 4), cclqr.OpenLoop(mech, eq, U), z0=z00[None])
    mech.set_state(z00)
    trk = cclqr.TrackingLQR(mech, ref_run, U, eq, ex["Q"], ex["R"])
    z0 = np.tile(z00, (5, 1, 1))
    noise = np.random.default_rng(9).normal(size=(5, N))
    kw = dict(fric=ex["fric"], noise_scale=2.0, noise=noise)
    b, ref = with_threshold(cclqr, mech, ids, eq, ex["Q"], ex["R"],
                            lambda s: scored_runs(cclqr, mech, N, trk, s, z0, trk.K[None], trk.zd[None], trk.N, **kw))
    quiet = cclqr.simulate(mech, cclqr.Storage(N, 4), trk, record=False, z0=z0, fric=ex["fric"])
    mech.set_state(z00)
    assert not np.array_equal(quiet.zT, b.zT)      # (the noise acts)
    shifted = cclqr.simulate(mech, cclqr.Storage(N, 4), trk, record=False, z0=z0, fric=ex["fric"], noise_scale=2.0, noise=np.roll(noise, 7, axis=1))
    mech.set_state(z00)
    assert not np.array_equal(shifted.zT, b.zT)    # (and a shift of its columns by one chunk would show)


def test_scored_deltabot_lqr_with_holding_inputs(cclqr):
    ex = cclqr.examples.deltabot()
    mech = ex["mech"]
    z00 = mech.state()
    ids = [cclqr.getid(b) for b in mech.bodies]
    lq = cclqr.LQR(mech, ids, ex["eqcids"], ex["Q"], ex["R"], math.inf, xd=[z00[i, 0:3] for i in range(5)], qd=[z00[i, 3:7] for i in range(5)],
                   Fτd=[[ex["Fd"][0]], [ex["Fd"][1]]])
    zall, yz = cclqr.examples.deltabot_initial_states(ex)
    near = np.argsort(np.hypot(yz[:, 0] - z00[4, 1], yz[:, 1] - z00[4, 2]))[1:6]
    z0 = zall[near]
    with_threshold(cclqr, mech, ids, ex["eqcids"], ex["Q"], ex["R"],
                   lambda s: scored_runs(cclqr, mech, 40, lq, s, z0, lq.K[None], lq.zd[None], lq.N))


def test_scored_run_on_per_instance_plants(cclqr):
    mech, th0 = pc.mechanism_of(cclqr, ("chain", 2))
    ex = cclqr.examples.cartpole_n(2)
    ids, eq = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[0])]
    plants = pc.random_plants(cclqr, mech, 8, seed=5)
    z0, _ = pc.starts(cclqr, mech, th0, 5, seed=6, plants=plants, first_instance=2)
    zd = cclqr.joint_position_states(mech, th0[None])[0]
    lqr = cclqr.LQR(mech, ids, eq, ex["Q"], ex["R"], 0.3, xd=[zd[i, 0:3] for i in range(3)], qd=[zd[i, 3:7] for i in range(3)])
    kw = dict(plants=plants, first_instance=2)
    with_threshold(cclqr, mech, ids, eq, ex["Q"], ex["R"],
                   lambda s: scored_runs(cclqr, mech, 40, lqr, s, z0, lqr.K[None], lqr.zd[None], lqr.N, **kw))


def test_scored_pid_run_carries_its_integrators_across_chunks(cclqr):
    ex = cclqr.examples.double_pendulum(0.2, -0.1)
    mech = ex["mech"]
    ids = [cclqr.getid(b) for b in ex["bodies"]]
    pid = cclqr.PID(mech, [cclqr.getid(j) for j in ex["joints"]], ex["goals"], P=ex["P"], I=ex["I"], D=ex["D"])
    z0 = np.stack([cclqr.examples.double_pendulum(a, b)["mech"].state() for a, b in ((0.2, -0.1), (-0.5, 0.3), (0.0, 0.0), (0.4, 0.4), (-0.1, 0.2))])
    Q = [np.eye(12), 2 * np.eye(12)]
    zd = np.zeros((1, 1, 2, 13))
    zd[..., 3] = 1.0
    b, ref = with_threshold(cclqr, mech, ids, [], Q, [], lambda s: scored_runs(cclqr, mech, 40, pid, s, z0, None, zd, 0))
    assert (b.score[:, 1] == 0.0).all()


# ---------------------------------------------------------------- d. refusals
def test_refusals_name_their_cause_and_leave_the_controller_alone(cclqr):
    """every refusal of cclqr_score_create / cclqr_rollout_score that can be reached through the public constructors (a controller without a setpoint table cannot be
    built: cclqr_ctrl_create refuses it; a second device needs a second GPU) returns CCLQR_EINVAL and a message naming the cause, before anything is launched"""
    import torch
    capi = cclqr._capi
    mech, other = _chain(cclqr, 2), capi.MechHandle(sc.chain_tables(cclqr, 2))
    case = sc.synthetic_case(2, 1, "gated", 5, 3, 8, seed=1)
    ctrl = capi.CtrlHandle(mech, [0], K=case["K"].reshape(-1, 1, 24), N=5, zd=case["zd"].reshape(-1, 2, 13), n_ctrl=5)
    z0 = cclqr.examples.cartpole_states(1, [0.1, -0.2, 0.3], np.full((3, 1), 0.1))
    before = capi.rollout(mech, ctrl, z0, 6)
    good = capi.ScoreHandle(mech, case["Qb"], case["R"], 0.1)
    traj = torch.from_numpy(case["traj"]).cuda()
    s = torch.full((3, 4), 7.0, dtype=torch.float64, device="cuda")

    def refused(match, fn):
        with pytest.raises(capi.CclqrError, match=match) as e:
            fn()
        assert e.value.code == capi.EINVAL

    call = lambda m=mech, c=ctrl, sh=good, n=3, steps=8, k0=1, first=0: capi.rollout_score(m, c, sh, n, steps, k0, traj.data_ptr(), s.data_ptr(), first_instance=first)
    two = capi.ScoreHandle(mech, case["Qb"], np.eye(2), 0.1)
    refused("mu", lambda: call(sh=two))
    refused("n_ctrl", lambda: call(first=3))
    refused("steps", lambda: call(steps=0))
    refused("k0", lambda: call(k0=0))
    refused("another mechanism", lambda: call(m=other))
    m3 = _chain(cclqr, 5)
    c3 = capi.CtrlHandle(m3, [0], K=None, N=0)
    refused("another mechanism", lambda: call(c=c3))
    refused("settle_tol", lambda: capi.ScoreHandle(mech, case["Qb"], case["R"], math.nan))
    bad = case["Qb"].copy()
    bad[1, 3, 4] = math.inf
    refused("not finite", lambda: capi.ScoreHandle(mech, bad, case["R"], 0.1))
    refused("not finite", lambda: capi.ScoreHandle(mech, case["Qb"], np.array([[math.nan]]), 0.1))
    torch.cuda.synchronize()
    assert (s == 7.0).all()      # nothing was launched
    call()
    torch.cuda.synchronize()
    assert np.isfinite(s.cpu().numpy()).all()
    after = capi.rollout(mech, ctrl, z0, 6)
    assert all(np.array_equal(x, y) for x, y in zip((before[0], before[2]), (after[0], after[2])))
