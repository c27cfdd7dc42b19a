"""cclqr_rollout_ensemble on the device (csrc/ensemble.hip): synthetic slabs against the numpy restatement of the definition (tests/ensemble_common.py: the sums
over instances in longdouble, two passes; mean, M2 and the co-moment matrices within 1e-10 A), a planted NaN, the bitwise independence of the launch plan,
permuted body numberings, real rollouts through simulate(..., ensemble=), the refusals of the C ABI -- and the per-knot tie to TrackingCovariance.

The tie.  chain3 (the cart with two pendulum links of tests/test_gpu_tracking_covariance_noise.py: N = 24 knots along the open-loop rollout under U_k = 4 sin(2 pi k
/ 24), one TrackingLQR, Q = 10 Δt I, R = 0.1 Δt), 2048 rollouts of N steps from zd[0] under input noise of scale 1e-3, Philox seed 1234.  Row j of the ensemble is
knot j of TrackingCovariance: at every knot j >= 1, every coordinate with Σ_{j,ii} >= 1e-3 max_i Σ_{j,ii} has rms_{j,i}² / Σ_{j,ii} within 6 sqrt(2 / n) = 0.1875 of
1 -- six standard deviations of a Gaussian sample variance, the bound and the argument of tests/test_gpu_covariance_noise.py -- and input_rms² likewise against
input_std² at the knots where a gain acts (j <= N - 2).  Row 0 has M2 = 0 exactly: every instance starts at zd[0].
The CPU twin of this check (2048 oracle rollouts with the same Philox seed; the longdouble recursion tracking_covariance_common.step_tracking on the oracle's
linearisation at every knot and the oracle's gains): 5, 5, 5, 5, 5, 6, 6, 6, 7, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9 coordinates compared at the knots 1 .. 23,
170 in all (9 at the last knot, as tests/test_gpu_tracking_covariance_noise.py states); the largest per-knot deviation |rms² / Σ_ii - 1| is 0.0714 (knot 22; 0.0448 at
the last knot, the figure of that file), of the input 0.0328 (knot 8); the full sample second moment at the last knot lies within 0.0448 of Σ_{N-1} in the metric
sqrt(Σ_ii Σ_kk) (an entry's sampling spread is at most sqrt(2 Σ_ii Σ_kk / n), so the same bound holds there).  The oracle alone stays under the bound at every knot."""
import numpy as np
import pytest

import ensemble_common as ec
import plants_common as pc
import score_common as sc
from conftest import long_and_short_chain_forest
from plant_tracking_common import open_loop

pytestmark = pytest.mark.gpu

_MECH = {}


def _chain(cclqr, nb):
    if nb not in _MECH:
        _MECH[nb] = cclqr._capi.MechHandle(sc.chain_tables(cclqr, nb))
    return _MECH[nb]


def gpu_ensemble(cclqr, mech, case, cj, k0=1, first_instance=0, slab=None, cov_steps=(), calls=1):
    """the controller of `case` on the device and `calls` identical cclqr_rollout_ensemble launches over `slab` (default: the case's whole slab) into buffers full
    of NaN; returns (mean, M2 [steps][12 nb + mu], cov [len(cov_steps)][12 nb][12 nb]) of the last call"""
    import torch
    capi = cclqr._capi
    nb = mech.tables.nb
    n_ctrl = case["zd"].shape[0]
    K = case["K"]
    mu = len(cj)
    ctrl = capi.CtrlHandle(mech, cj, K=None if K is None else K.reshape(-1, mu, 12 * nb), N=case["N"], zd=case["zd"].reshape(-1, nb, 13), n_ctrl=n_ctrl if n_ctrl > 1 else 0)
    try:
        traj = torch.from_numpy(np.ascontiguousarray(case["traj"] if slab is None else slab)).cuda()
        n, steps = traj.shape[:2]
        nx, mx = 12 * nb + mu, 12 * nb
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        ws_bytes = capi.rollout_ensemble_ws_bytes(mech, mu, n, steps, len(cov_steps))
        for _ in range(calls):
            mean, m2, cov, ws = nan(steps, nx), nan(steps, nx), nan(max(1, len(cov_steps)), mx, mx), nan(ws_bytes // 8 + 1)
            capi.rollout_ensemble(mech, ctrl, n, steps, k0, traj.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), ws_bytes, cov_steps=cov_steps,
                                  cov_ptr=cov.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, first_instance=first_instance)
            torch.cuda.synchronize()
        return mean.cpu().numpy(), m2.cpu().numpy(), cov.cpu().numpy()[:len(cov_steps)]
    finally:
        ctrl.close()


def check_cov(C, M2, x, xm, mx, rows, what):
    """the co-moment matrices of the slab rows `rows` against longdouble numpy; exactly symmetric; the diagonal is M2 within the bound"""
    for q, r in enumerate(rows):
        Cref, AC = ec.comoment_of(x[r], xm[r], mx)
        ec.assert_close(C[q], Cref, AC, "%s C of row %d" % (what, r))
        assert np.array_equal(C[q], C[q].T), "%s: C of row %d is not symmetric" % (what, r)
        ec.assert_close(np.diag(C[q]), M2[r, :mx].astype(ec.LD), np.diag(AC), "%s diag C against M2, row %d" % (what, r))


# ---------------------------------------------------------------- a. synthetic slabs
@pytest.mark.parametrize("kind", ["inf", "gated", "tracking"])
@pytest.mark.parametrize("nb", [1, 8, 9, 17, 33, 64])
def test_synthetic_slabs_match_the_definition(cclqr, nb, kind):
    """nb: every lane-group size (8, 16, 32, 64 lanes) at its upper edge and its first overflow; n_inst 1, 65 (a tile of 64 and one), 257 (four tiles and one); one
    table and first_instance 2 of n_inst + 2 tables; k0 1 and 4 (the window crosses N = 5 / 6)"""
    mech = _chain(cclqr, nb)
    mu = min(3, nb)
    for n_inst in (1, 65, 257):
        for multi, k0 in ((False, 1), (True, 4)):
            n_ctrl, first = (n_inst + 2, 2) if multi else (1, 0)
            steps = 8 if n_inst < 257 else 3
            case = sc.synthetic_case(nb, mu, kind, n_ctrl, n_inst, steps, seed=100000 * nb + 10 * n_inst + k0)
            mean, M2, _ = gpu_ensemble(cclqr, mech, case, list(range(mu)), k0=k0, first_instance=first)
            ec.assert_moments(mean, M2, case, k0=k0, first_instance=first, what="nb %d %s n_inst %d n_ctrl %d k0 %d" % (nb, kind, n_inst, n_ctrl, k0))
            if n_inst == 1:
                assert (M2 == 0.0).all()


def test_a_controller_without_gains_commands_nothing(cclqr):
    case = dict(sc.synthetic_case(5, 2, "inf", 1, 9, 4, seed=2), K=None)
    mean, M2, _ = gpu_ensemble(cclqr, _chain(cclqr, 5), case, [0, 1])
    assert mean.shape == (4, 62) and (mean[:, 60:] == 0.0).all() and (M2[:, 60:] == 0.0).all()
    ec.assert_moments(mean[:, :60], M2[:, :60], case, what="no gains")


def test_centred_sums_survive_a_mean_far_above_the_spread(cclqr):
    for nb in (2, 17, 33):
        case = ec.cancellation_case(nb, 257, seed=nb)
        _, M2, _ = gpu_ensemble(cclqr, _chain(cclqr, nb), case, [])
        print("nb %d: centred variances within %.3g relative of the longdouble two-pass" % (nb, ec.assert_cancellation(M2, case)))


# ---------------------------------------------------------------- b. the co-moment matrices
@pytest.mark.parametrize("nb,n_inst,k0", [(1, 257, 1), (3, 1100, 4), (9, 65, 1), (17, 257, 1)])
def test_comoment_matrices_at_the_first_a_middle_and_the_last_step(cclqr, nb, n_inst, k0):
    """mx = 12 (below one 16-tile), 36 (no multiple of 32), 108, 204 = 6 x 32 + 12; 1100 instances are two K-splits, the second short and no multiple of 4"""
    mu = min(2, nb)
    case = sc.synthetic_case(nb, mu, "tracking", 1, n_inst, 5, seed=7 * nb)
    listed = (k0, k0 + 2, k0 + 4)
    mean, M2, C = gpu_ensemble(cclqr, _chain(cclqr, nb), case, list(range(mu)), k0=k0, cov_steps=listed)
    x, xm = ec.assert_moments(mean, M2, case, k0=k0, what="nb %d" % nb)
    check_cov(C, M2, x, xm, 12 * nb, (0, 2, 4), "nb %d" % nb)
    assert all(np.linalg.eigvalsh(c).min() > -1e-9 * np.trace(c) for c in C)


def test_a_nan_in_one_body_is_that_bodys_coordinates_alone(cclqr):
    mech = _chain(cclqr, 5)
    case = sc.synthetic_case(5, 3, "gated", 1, 70, 8, seed=3)
    clean = dict(case, traj=case["traj"].copy())
    case["traj"][66, 3, 1, 8] = np.inf           # body 1, step 4 (k < N = 5: the feedback reads it); step 7 lies behind the gate
    case["traj"][2, 6, 1, 8] = np.nan
    mean, M2, C = gpu_ensemble(cclqr, mech, case, [0, 1, 2], cov_steps=(4, 5))
    m0, q0, C0 = gpu_ensemble(cclqr, mech, clean, [0, 1, 2], cov_steps=(4, 5))
    hit = np.zeros(mean.shape, dtype=bool)
    hit[3, 12 + 4] = hit[6, 12 + 4] = True       # entry 8 of the state is v_y: coordinate 4 of the body's error
    hit[3, 60:] = True
    assert np.isnan(mean[hit]).all() and np.isnan(M2[hit]).all()
    assert np.array_equal(mean[~hit], m0[~hit]) and np.array_equal(M2[~hit], q0[~hit]) and np.isfinite(m0).all() and np.isfinite(q0).all()
    cross = np.zeros((60, 60), dtype=bool)
    cross[16, :] = cross[:, 16] = True
    assert np.isnan(C[0][cross]).all() and np.array_equal(C[0][~cross], C0[0][~cross]) and np.array_equal(C[1], C0[1]) and np.isfinite(C0).all()


# ---------------------------------------------------------------- c. one summation order
@pytest.mark.parametrize("nb,kind", [(9, "tracking"), (17, "gated")])
def test_any_launch_plan_and_a_second_call_give_the_same_bits(cclqr, nb, kind):
    mech = _chain(cclqr, nb)
    mu = min(3, nb)
    case = sc.synthetic_case(nb, mu, kind, 1, 150, 23, seed=nb)
    cj, listed = list(range(mu)), (1, 12, 23)
    whole = gpu_ensemble(cclqr, mech, case, cj, cov_steps=listed, calls=2)
    once = gpu_ensemble(cclqr, mech, case, cj, cov_steps=listed)
    assert all(np.array_equal(a, b) and np.isfinite(a).all() for a, b in zip(whole, once))
    for plan in ([1] * 23, [7, 7, 7, 2]):
        k0, got = 1, []
        for s in plan:
            here = [k for k in listed if k0 <= k < k0 + s]
            got.append(gpu_ensemble(cclqr, mech, case, cj, k0=k0, slab=case["traj"][:, k0 - 1:k0 - 1 + s], cov_steps=here))
            k0 += s
        for i in range(3):
            assert np.array_equal(np.concatenate([g[i] for g in got]), whole[i]), (plan, i)


# ---------------------------------------------------------------- d. permuted body numbering, trees, closed loops
def test_permuted_body_numbering(cclqr):
    """the link-order trap: the slab and every output are in the caller's body order, the controller's K columns and setpoints in link order -- a 13-link and a
    3-link chain with their bodies interleaved in the caller's numbering"""
    t2, _, zd, K, cj = long_and_short_chain_forest(cclqr)
    mech = cclqr._capi.MechHandle(t2)
    assert list(cclqr.link_order(t2)[0]) != list(range(t2.nb))
    zd = zd.copy()
    zd[:, 7:] = np.random.default_rng(3).normal(size=(t2.nb, 6)) * 0.1
    rng = np.random.default_rng(4)
    traj = zd[None, None] + 0.1 * rng.normal(size=(70, 8, t2.nb, 13)) * (1 + np.arange(t2.nb))[None, None, :, None]      # (every body its own spread)
    traj[..., 3:7] /= np.linalg.norm(traj[..., 3:7], axis=-1, keepdims=True)
    case = dict(N=21, K=K[None], zd=zd[None, None], traj=np.ascontiguousarray(traj))
    for k0 in (1, 15):      # (15: crosses nK = 20 and N = 21)
        mean, M2, C = gpu_ensemble(cclqr, mech, case, cj, k0=k0, cov_steps=(k0 + 1,))
        x, xm = ec.assert_moments(mean, M2, case, k0=k0, what="forest k0 %d" % k0)
        check_cov(C, M2, x, xm, 12 * t2.nb, (1,), "forest k0 %d" % k0)


def test_branching_tree_and_closed_loops(cclqr):
    """the 14-body tree (bodies with two and three child joints) and the deltabot, where the joints outnumber the bodies (7 on 5: mu up to 7)"""
    tree = pc.hanging_tree(cclqr, pc.TREE14).tables()
    delta = cclqr.examples.deltabot()["mech"].tables()
    for seed, (name, t, mu) in enumerate((("tree14", tree, 3), ("deltabot", delta, 7), ("deltabot", delta, 2))):
        assert mu <= t.ne
        mech = cclqr._capi.MechHandle(t)
        for kind in ("inf", "gated", "tracking"):
            for multi in (False, True):
                case = sc.synthetic_case(t.nb, mu, kind, 72 if multi else 1, 70, 8, seed=100 * seed + 10 * len(kind) + multi)
                first = 2 if multi else 0
                mean, M2, C = gpu_ensemble(cclqr, mech, case, list(range(mu)), first_instance=first, cov_steps=(3,))
                x, xm = ec.assert_moments(mean, M2, case, first_instance=first, what="%s mu %d %s" % (name, mu, kind))
                check_cov(C, M2, x, xm, 12 * t.nb, (2,), "%s mu %d %s" % (name, mu, kind))


# ---------------------------------------------------------------- e. real rollouts and the tie to TrackingCovariance
N, N_INST, SIGMA, SEED = 24, 2048, 1e-3, 1234
BOUND = 6.0 * np.sqrt(2.0 / N_INST)
KNOTS = (0, 1, 11, 23)
_s = {}


def setup(cclqr, orc):
    if _s:
        return _s
    mech, th0 = pc.mechanism_of(cclqr, ("chain", 2))
    t = mech.tables()
    nb = t.nb
    U = 4.0 * np.sin(2 * np.pi * np.arange(N) / N)[:, None]
    zd = open_loop(orc, t, [0], U, cclqr.joint_position_states(mech, th0[None])[0])
    ids, eids = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[0])]
    Qb, Rb = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1]
    trk = cclqr.TrackingLQR(mech, cclqr.Storage(N, nb, 1, z=np.ascontiguousarray(zd[None])), U, eids, Qb, Rb)
    z0 = np.ascontiguousarray(np.tile(zd[0], (N_INST, 1, 1)))
    z00 = mech.state()
    kw = dict(z0=z0, noise_scale=SIGMA, noise_seed=SEED)
    ens, score = cclqr.Ensemble(mech, cov_knots=KNOTS), cclqr.Score(mech, ids, eids, Qb, Rb)

    def run(**more):
        mech.set_state(z00)
        return cclqr.simulate(mech, cclqr.Storage(N, nb), trk, **kw, **more)

    _s.update(mech=mech, nb=nb, zd=zd, ids=ids, eids=eids, Qb=Qb, Rb=Rb, trk=trk, plain=run(record=False), chunked=run(record=False, ensemble=ens, chunk_steps=7),
              recorded=run(record=True, ensemble=ens), scored=run(record=False, score=score, chunk_steps=7), both=run(record=False, score=score, ensemble=ens, chunk_steps=7))
    mech.set_state(z00)
    return _s


def _same(a, b):
    return (a.count == b.count and np.array_equal(a.mean, b.mean) and np.array_equal(a.M2, b.M2) and np.array_equal(a.input_mean, b.input_mean)
            and np.array_equal(a.input_M2, b.input_M2) and sorted(a.C) == sorted(b.C) and all(np.array_equal(a.C[j], b.C[j]) for j in a.C))


def test_the_unrecorded_chunked_ensemble_is_bitwise_the_recorded_one(cclqr, orc):
    s = setup(cclqr, orc)
    plain, a, b, both = s["plain"], s["chunked"], s["recorded"], s["both"]
    assert (plain.status > 0).all() and plain.ensemble is None and plain.score is None
    assert a.z.shape[1] == 0 and b.z.shape[1] == N and a.score is None
    for r in (a, b, both):
        assert np.array_equal(r.zT, plain.zT) and np.array_equal(r.status, plain.status)
    e = a.ensemble
    assert e.count == N_INST and e.mean.shape == (N, 12 * s["nb"]) and e.input_mean.shape == (N, 1) and sorted(e.C) == list(KNOTS)
    assert _same(e, b.ensemble) and _same(e, both.ensemble)
    assert np.array_equal(both.score, s["scored"].score) and np.isfinite(both.score).all()
    assert (e.M2[0] == 0.0).all() and (e.input_M2[0] == 0.0).all() and (e.C[0] == 0.0).all() and (e.M2[1:].max(axis=1) > 0.0).all()      # every instance starts at zd[0]
    with pytest.raises(KeyError):
        e.cov(2)


def test_the_ensemble_of_a_recorded_run_is_numpys(cclqr, orc):
    s = setup(cclqr, orc)
    b, trk = s["recorded"], s["trk"]
    e = b.ensemble
    case = dict(N=trk.N, K=trk.K[None], zd=trk.zd[None], traj=b.z)
    mx = 12 * s["nb"]
    x, xm = ec.assert_moments(np.hstack([e.mean, e.input_mean]), np.hstack([e.M2, e.input_M2]), case, what="rollout")
    check_cov(np.stack([e.C[j] for j in KNOTS]), e.M2, x, xm, mx, KNOTS, "rollout")
    assert np.array_equal(e.var(), e.M2 / N_INST) and np.array_equal(e.std, np.sqrt(e.M2 / N_INST)) and np.array_equal(e.cov(11), e.C[11] / N_INST)
    assert np.allclose(e.rms ** 2, (x[:, :, :mx] ** 2).mean(axis=1), rtol=1e-9, atol=0.0)
    assert np.allclose(e.second_moment(23), x[23, :, :mx].T @ x[23, :, :mx] / N_INST, rtol=1e-9, atol=1e-30)
    # two shards of the batch, merged on the host, are the whole
    h = N_INST // 2 + 64
    parts = []
    for lo, hi in ((0, h), (h, N_INST)):
        mean, M2, _, _ = ec.moments_of(x[:, lo:hi], xm[:, lo:hi])
        mean, M2 = mean.astype(np.float64), M2.astype(np.float64)
        C = {j: ec.comoment_of(x[j, lo:hi], xm[j, lo:hi], mx)[0].astype(np.float64) for j in KNOTS}
        parts.append(cclqr.EnsembleStats(hi - lo, mean[:, :mx], M2[:, :mx], mean[:, mx:], M2[:, mx:], C))
    m = parts[0].merge(parts[1])
    assert m.count == N_INST and np.allclose(m.M2, e.M2, rtol=1e-9, atol=0.0) and np.allclose(m.C[23], e.C[23], rtol=1e-9, atol=1e-12 * np.abs(e.C[23]).max())


def test_every_knot_shows_the_spread_tracking_covariance_predicts(cclqr, orc):
    s = setup(cclqr, orc)
    e = s["chunked"].ensemble
    cov = cclqr.TrackingCovariance(s["mech"], s["trk"], s["ids"], s["eids"], s["Qb"], s["Rb"], noise_scale=SIGMA)
    try:
        var, uvar, Sig = cov.state_std[0] ** 2, cov.input_std[0] ** 2, cov.Sigma(0)
        assert cov.N == N and s["ids"] == sorted(s["ids"])
    finally:
        cov.close()
    worst, worst_u, compared = 0.0, 0.0, []
    for j in range(1, N):
        big = var[j] >= 1e-3 * var[j].max()
        ratio = e.rms[j, big] ** 2 / var[j, big]
        compared.append(int(big.sum()))
        worst = max(worst, float(np.abs(ratio - 1.0).max()))
        assert big.sum() >= 1 and np.abs(ratio - 1.0).max() <= BOUND, "knot %d: rms² / Σ_ii = %s" % (j, ratio)
        if j <= N - 2:
            ru = e.input_rms[j] ** 2 / uvar[j]
            worst_u = max(worst_u, float(np.abs(ru - 1.0).max()))
            assert np.abs(ru - 1.0).max() <= BOUND, "knot %d: input_rms² / (K Σ K') = %s" % (j, ru)
    print("entries compared per knot %s; largest |rms² / Σ_ii - 1| = %.4f, of the input %.4f; bound %.4f" % (compared, worst, worst_u, BOUND))
    assert compared[-1] >= 6
    assert not uvar[N - 1].any() and not e.input_rms[N - 1].any()      # no gain acts at the last knot
    # and the full matrix at the last knot: the sample second moment against Σ_{N-1}, on the block of the compared coordinates, in the metric of its diagonal
    big = np.diag(Sig) >= 1e-3 * np.diag(Sig).max()
    d = np.sqrt(np.diag(Sig)[big])
    dev = np.abs((e.second_moment(N - 1) - Sig)[np.ix_(big, big)] / np.outer(d, d)).max()
    print("largest |S_ik - Σ_ik| / sqrt(Σ_ii Σ_kk) at the last knot: %.4f" % dev)
    assert dev <= BOUND


# ---------------------------------------------------------------- f. refusals
def test_refusals_name_their_cause_and_leave_the_controller_usable(cclqr):
    import torch
    capi = cclqr._capi
    mech = _chain(cclqr, 2)
    case = sc.synthetic_case(2, 1, "gated", 5, 3, 8, seed=1)
    ctrl = capi.CtrlHandle(mech, [0], K=case["K"].reshape(-1, 1, 24), N=5, zd=case["zd"].reshape(-1, 2, 13), n_ctrl=5)
    z0 = cclqr.examples.cartpole_states(1, [0.1, -0.2, 0.3], np.full((3, 1), 0.1))
    before = capi.rollout(mech, ctrl, z0, 6)
    traj = torch.from_numpy(case["traj"]).cuda()
    full = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    mean, m2, cov = full(8, 25), full(8, 25), full(2, 24, 24)
    ws_bytes = capi.rollout_ensemble_ws_bytes(mech, 1, 3, 8, 2)
    assert ws_bytes > 0 and ws_bytes % 8 == 0 and capi.rollout_ensemble_ws_bytes(mech, 1, 3, 8, 0) < ws_bytes
    ws = full(ws_bytes // 8)

    def refused(match, fn):
        with pytest.raises(capi.CclqrError, match=match) as e:
            fn()
        assert e.value.code == capi.EINVAL

    def call(m=mech, c=ctrl, n=3, steps=8, k0=1, first=0, listed=(2, 8), w=ws.data_ptr(), wb=ws_bytes):
        capi.rollout_ensemble(m, c, n, steps, k0, traj.data_ptr(), mean.data_ptr(), m2.data_ptr(), w, wb, cov_steps=listed, cov_ptr=cov.data_ptr(), first_instance=first)

    refused("null workspace", lambda: call(w=0))
    refused("workspace too small", lambda: call(wb=ws_bytes - 8))
    refused(r"cov_steps\[1\] = 9", lambda: call(listed=(2, 9)))
    refused(r"cov_steps\[0\] = 3", lambda: call(k0=4, listed=(3, 5)))
    refused("n_inst = 0", lambda: call(n=0))
    refused("n_ctrl", lambda: call(first=3))
    refused("steps", lambda: call(steps=0))
    refused("k0", lambda: call(k0=0))
    refused("n_cov = 65", lambda: call(listed=tuple([1] * 65)))
    refused("n_inst = 0", lambda: capi.rollout_ensemble_ws_bytes(mech, 1, 0, 8, 0))
    m5 = _chain(cclqr, 5)
    c5 = capi.CtrlHandle(m5, [0], K=None, N=0)
    refused("another mechanism", lambda: call(c=c5))
    refused("another mechanism", lambda: call(m=m5))
    c5.close()
    torch.cuda.synchronize()
    assert (mean == 7.0).all() and (m2 == 7.0).all() and (cov == 7.0).all() and (ws == 7.0).all()      # nothing was launched
    call()
    torch.cuda.synchronize()
    assert np.isfinite(mean.cpu().numpy()).all() and np.isfinite(cov.cpu().numpy()).all()
    after = capi.rollout(mech, ctrl, z0, 6)
    assert all(np.array_equal(x, y) for x, y in zip((before[0], before[2]), (after[0], after[2])))
    ctrl.close()
