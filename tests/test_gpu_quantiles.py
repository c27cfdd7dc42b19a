"""cclqr_rollout_quantiles on the device (csrc/quantiles.hip): synthetic slabs against the numpy restatement of the definition (tests/quantile_common.py), exact bits
where the slab's own numbers are the data, planted Inf and NaN, the bitwise independence of the workspace size, the launch plan and the order of the instances,
permuted body numberings, trees and closed loops, the upper edge of 16384 instances, the refusals of the C ABI, real rollouts through simulate(..., ensemble=
Ensemble(mech, quantiles=)) -- and the tie to the prediction.

The bound.  The device's x differs from numpy's at rounding.  An order statistic is 1-Lipschitz in the sup norm of its data, and so is an interpolation between two
neighbouring ones, so per (row, coordinate) |got - ref| <= RTOL max_i xm_i with ensemble_common's RTOL = 1e-10 and magnitudes xm: no new tolerance.

The tie.  chain3, N = 24, 2048 noisy rollouts at sigma = 1e-3, Philox seed 1234 (the setting of tests/test_gpu_ensemble.py).  A Gaussian sample's median has the
asymptotic variance pi s^2 / 2n, its mean s^2 / n and their covariance is s^2 / n, so median - mean has the standard deviation sqrt(pi/2 - 1) s / sqrt(n); at every
knot j >= 1 every coordinate with Σ_{j,ii} >= 1e-3 max_i Σ_{j,ii} must have |median - mean| <= 6 sqrt(pi/2 - 1) std / sqrt(n).
The CPU twin of this check (tools/cpu_quantile_twin.py: 2048 oracle rollouts with the same Philox seed under the oracle's gains, Σ by the longdouble recursion
tracking_covariance_common.step_tracking on the oracle's linearisation, mean and std in longdouble, the median by the numpy definition) compares 170 entries and
stays inside the bound at every one of them: its largest |median - mean| / bound is 0.3418 (knot 9).  The device: 0.3418 (knot 9), 170 entries."""
import numpy as np
import pytest

import ensemble_common as ec
import plants_common as pc
import quantile_common as qc
import score_common as sc
from conftest import long_and_short_chain_forest
from plant_tracking_common import open_loop

pytestmark = pytest.mark.gpu

P5 = (0.0, 0.05, 0.5, 0.95, 1.0)
_MECH = {}


def _chain(cclqr, nb):
    if nb not in _MECH:
        _MECH[nb] = cclqr._capi.MechHandle(sc.chain_tables(cclqr, nb))
    return _MECH[nb]


def _ensemble_mean(cclqr, mech, case, cj):
    """cclqr_rollout_ensemble's mean of the case's slab, [steps][12 nb + mu]"""
    import torch
    capi = cclqr._capi
    nb, mu, K = mech.tables.nb, len(cj), case["K"]
    ctrl = capi.CtrlHandle(mech, cj, K=None if K is None else K.reshape(-1, mu, 12 * nb), N=case["N"], zd=case["zd"].reshape(-1, nb, 13))
    try:
        traj = torch.from_numpy(case["traj"]).cuda()
        n, steps = traj.shape[:2]
        mean, m2 = (torch.zeros((steps, 12 * nb + mu), dtype=torch.float64, device="cuda") for _ in range(2))
        wb = capi.rollout_ensemble_ws_bytes(mech, mu, n, steps, 0)
        ws = torch.zeros(wb // 8 + 1, dtype=torch.float64, device="cuda")
        capi.rollout_ensemble(mech, ctrl, n, steps, 1, traj.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), wb)
        torch.cuda.synchronize()
        return mean.cpu().numpy()
    finally:
        ctrl.close()


# ---------------------------------------------------------------- a. synthetic slabs
@pytest.mark.parametrize("kind", ["inf", "gated", "tracking"])
@pytest.mark.parametrize("nb", [1, 9, 17, 64])
def test_synthetic_slabs_match_the_definition(cclqr, nb, kind):
    """nb: the lane-group sizes 8, 16, 32, 64 (64 bodies: the window is shorter than a tile); n_inst: a tile and one, four tiles and one, a power of two and its first
    overflow of the pad; one table and first_instance 2 of n_inst + 2 tables; k0 1 and 4 (the window crosses N = 5 / 6)"""
    mech = _chain(cclqr, nb)
    mu = min(3, nb)
    for n_inst in (1, 2, 3, 64, 65, 257, 1024, 1025):
        for multi, k0 in ((False, 1), (True, 4)):
            n_ctrl, first = (n_inst + 2, 2) if multi else (1, 0)
            steps = 4 if n_inst < 257 else 2
            case = sc.synthetic_case(nb, mu, kind, n_ctrl, n_inst, steps, seed=100000 * nb + 10 * n_inst + k0)
            got, fin = qc.gpu_quantiles(cclqr, mech, case, list(range(mu)), qc.PROBS, k0=k0, first_instance=first)
            qc.assert_quantiles(got, fin, case, qc.PROBS, k0=k0, first_instance=first, what="nb %d %s n_inst %d n_ctrl %d k0 %d" % (nb, kind, n_inst, n_ctrl, k0))
            assert (got[:, 0] <= got[:, 2]).all() and (got[:, 2] <= got[:, 1]).all()      # min <= median <= max


def test_a_controller_without_gains_commands_nothing(cclqr):
    case = dict(sc.synthetic_case(5, 2, "inf", 1, 9, 4, seed=2), K=None)
    got, fin = qc.gpu_quantiles(cclqr, _chain(cclqr, 5), case, [0, 1], P5)
    assert got.shape == (4, 5, 62) and (got[:, :, 60:] == 0.0).all() and (fin == 9).all()
    x, xm = ec.rows_of(case["traj"], case["zd"], None, 0)
    ref, _ = qc.quantiles_of(x, P5)
    assert (np.abs(got[:, :, :60] - ref) <= ec.RTOL * xm.max(axis=1)[:, None, :]).all()


# ---------------------------------------------------------------- b. exact bits
@pytest.mark.parametrize("nb,n", [(2, 70), (17, 257)])
def test_the_slabs_own_numbers_come_back_bit_for_bit(cclqr, nb, n):
    """zero setpoint with identity quaternions (ensemble_common.cancellation_case): the position, velocity and angular-velocity coordinates of Δz are the slab's own
    numbers, so every quantile there is bitwise the numpy definition; ties and signed zeros planted"""
    case = ec.cancellation_case(nb, n, seed=nb)
    t = case["traj"]
    t[: n // 3, 0, :, 0] = t[0, 0, :, 0]            # a third of the instances tie in x
    t[::2, 1, :, 7] = 0.0
    t[1::2, 1, :, 7] = -0.0                         # v_x: nothing but signed zeros
    t[::3, 1, :, 12] = -0.0                         # w_z: zeros of both signs among the values
    t[1::3, 1, :, 12] = 0.0
    got, fin = qc.gpu_quantiles(cclqr, _chain(cclqr, nb), case, [], qc.PROBS)
    x, _ = ec.rows_of(t, case["zd"], None, 0)
    ref, cnt = qc.quantiles_of(x, qc.PROBS)
    own = np.zeros(12 * nb, dtype=bool)
    for b in range(nb):
        own[12 * b:12 * b + 6] = own[12 * b + 9:12 * b + 12] = True
    assert qc.same_bits(got[:, :, own], ref[:, :, own]) and np.array_equal(fin, cnt)
    vx = np.arange(nb) * 12 + 3
    assert np.signbit(got[1, 0, vx]).all() and not np.signbit(got[1, 1, vx]).any()      # min -0.0, max +0.0


@pytest.mark.parametrize("nb,kind", [(1, "inf"), (9, "tracking"), (33, "gated")])
def test_one_instance_is_its_own_quantile_and_the_ensembles_mean(cclqr, nb, kind):
    mu = min(3, nb)
    case = sc.synthetic_case(nb, mu, kind, 1, 1, 6, seed=nb)
    cj = list(range(mu))
    got, fin = qc.gpu_quantiles(cclqr, _chain(cclqr, nb), case, cj, qc.PROBS)
    mean = _ensemble_mean(cclqr, _chain(cclqr, nb), case, cj)
    assert (fin == 1).all() and all(qc.same_bits(got[:, j], mean) for j in range(len(qc.PROBS)))


# ---------------------------------------------------------------- c. planted Inf and NaN
def test_a_value_that_is_not_finite_leaves_the_count_of_the_coordinates_it_enters(cclqr):
    """the case of test_gpu_ensemble.py::test_a_nan_in_one_body_is_that_bodys_coordinates_alone"""
    mech = _chain(cclqr, 5)
    case = sc.synthetic_case(5, 3, "gated", 1, 70, 8, seed=3)
    clean = dict(case, traj=case["traj"].copy())
    case["traj"][66, 3, 1, 8] = np.inf           # body 1, step 4 (k < N = 5: the feedback reads it); step 7 lies behind the gate
    case["traj"][2, 6, 1, 8] = np.nan
    got, fin = qc.gpu_quantiles(cclqr, mech, case, [0, 1, 2], qc.PROBS)
    g0, f0 = qc.gpu_quantiles(cclqr, mech, clean, [0, 1, 2], qc.PROBS)
    hit = np.zeros(fin.shape, dtype=bool)
    hit[3, 12 + 4] = hit[6, 12 + 4] = True       # entry 8 of the state is v_y: coordinate 4 of the body's error
    hit[3, 60:] = True
    assert (f0 == 70).all() and np.array_equal(fin, np.where(hit, 69, 70))
    keep = np.broadcast_to(~hit[:, None, :], got.shape)
    assert qc.same_bits(got[keep], g0[keep]) and np.isfinite(got).all()
    # on the hit coordinates: the definition on the finite subset, i.e. the clean slab without that instance
    for r, inst in ((3, 66), (6, 2)):
        x, xm = ec.rows_of(np.delete(clean["traj"], inst, axis=0), clean["zd"], clean["K"], clean["N"])
        ref, _ = qc.quantiles_of(x[r:r + 1], qc.PROBS)
        cols = np.flatnonzero(hit[r])
        assert (np.abs(got[r][:, cols] - ref[0][:, cols]) <= ec.RTOL * xm[r].max(axis=0)[cols]).all()
    # a coordinate that is not finite in any instance: NaN with count 0
    case["traj"][:, 5, 4, 0] = np.nan
    got, fin = qc.gpu_quantiles(cclqr, mech, case, [0, 1, 2], qc.PROBS)
    assert (fin[5, 48] == 0) and np.isnan(got[5, :, 48]).all() and (fin[5, :48] == 70).all() and qc.same_bits(got[5, :, :48], g0[5, :, :48])
    assert (fin[5, 60:] == 70).all() and (got[5, :, 60:] == 0.0).all()      # (step 6 lies behind the gate N = 5: Δu = 0 there)


# ---------------------------------------------------------------- d. one multiset, one answer
@pytest.mark.parametrize("nb,kind", [(9, "tracking"), (17, "gated")])
def test_workspace_launch_plan_second_call_and_instance_order_leave_the_bits(cclqr, nb, kind):
    mech = _chain(cclqr, nb)
    mu = min(3, nb)
    case = sc.synthetic_case(nb, mu, kind, 1, 150, 23, seed=nb)
    cj = list(range(mu))
    whole = qc.gpu_quantiles(cclqr, mech, case, cj, qc.PROBS, calls=2)
    assert np.isfinite(whole[0]).all()
    lo = cclqr._capi.rollout_quantiles_ws_bytes(mech, mu, 150, 23)[0]
    for wb in ("min", None, 2 * lo, 7 * lo + 8):      # one row, all rows, one row more than min_bytes, blocks of 7 (and a byte count that is no multiple of a row)
        got = qc.gpu_quantiles(cclqr, mech, case, cj, qc.PROBS, ws_bytes=wb)
        assert qc.same_bits(got[0], whole[0]) and np.array_equal(got[1], whole[1]), wb
    for plan in ([1] * 23, [7, 7, 7, 2]):
        k0, got = 1, []
        for s in plan:
            got.append(qc.gpu_quantiles(cclqr, mech, case, cj, qc.PROBS, k0=k0, slab=case["traj"][:, k0 - 1:k0 - 1 + s]))
            k0 += s
        assert qc.same_bits(np.concatenate([g[0] for g in got]), whole[0]) and np.array_equal(np.concatenate([g[1] for g in got]), whole[1]), plan
    perm = np.random.default_rng(5).permutation(150)
    got = qc.gpu_quantiles(cclqr, mech, dict(case, traj=np.ascontiguousarray(case["traj"][perm])), cj, qc.PROBS)
    assert qc.same_bits(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    assert qc.same_bits(qc.gpu_quantiles(cclqr, mech, case, cj, qc.PROBS, with_finite=False)[0], whole[0])      # finite_dev = NULL


# ---------------------------------------------------------------- e. permuted body numbering, trees, closed loops
def test_permuted_body_numbering(cclqr):
    """a 13-link and a 3-link chain with their bodies interleaved in the caller's numbering: the slab and the outputs in the caller's order, K and zd in link order"""
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
        got, fin = qc.gpu_quantiles(cclqr, mech, case, cj, P5, k0=k0)
        qc.assert_quantiles(got, fin, case, P5, k0=k0, what="forest k0 %d" % k0)


def test_branching_tree_and_closed_loops(cclqr):
    """the 14-body tree and the deltabot, where the joints outnumber the bodies (mu = 7 on 5 bodies)"""
    tree = pc.hanging_tree(cclqr, pc.TREE14).tables()
    delta = cclqr.examples.deltabot()["mech"].tables()
    for seed, (name, t, mu) in enumerate((("tree14", tree, 3), ("deltabot", delta, 7))):
        mech = cclqr._capi.MechHandle(t)
        for kind in ("inf", "gated", "tracking"):
            for multi in (False, True):
                case = sc.synthetic_case(t.nb, mu, kind, 72 if multi else 1, 70, 8, seed=100 * seed + 10 * len(kind) + multi)
                first = 2 if multi else 0
                got, fin = qc.gpu_quantiles(cclqr, mech, case, list(range(mu)), P5, first_instance=first)
                qc.assert_quantiles(got, fin, case, P5, first_instance=first, what="%s mu %d %s" % (name, mu, kind))


# ---------------------------------------------------------------- f. the upper edge and the refusals
def test_sixteen_thousand_instances_and_one_more(cclqr):
    import torch
    capi = cclqr._capi
    mech = _chain(cclqr, 1)
    case = sc.synthetic_case(1, 1, "inf", 1, 16384, 2, seed=9)
    got, fin = qc.gpu_quantiles(cclqr, mech, case, [0], qc.PROBS)
    qc.assert_quantiles(got, fin, case, qc.PROBS, what="16384 instances")
    with pytest.raises(capi.CclqrError, match="CCLQR_QUANTILE_MAX_INST = 16384") as e:
        capi.rollout_quantiles_ws_bytes(mech, 1, 16385, 2)
    assert e.value.code == capi.EUNSUPPORTED
    ctrl = capi.CtrlHandle(mech, [0], K=case["K"].reshape(-1, 1, 12), N=0, zd=case["zd"].reshape(-1, 1, 13))
    try:
        traj = torch.zeros((16385, 2, 1, 13), dtype=torch.float64, device="cuda")
        quant = torch.full((2, 1, 13), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.zeros(13 * 16448 * 2, dtype=torch.float64, device="cuda")
        with pytest.raises(capi.CclqrError, match="CCLQR_QUANTILE_MAX_INST = 16384") as e:
            capi.rollout_quantiles(mech, ctrl, 16385, 2, 1, traj.data_ptr(), (0.5,), quant.data_ptr(), 0, ws.data_ptr(), 8 * ws.numel())
        torch.cuda.synchronize()
        assert e.value.code == capi.EUNSUPPORTED and torch.isnan(quant).all()
    finally:
        ctrl.close()


def test_refusals_name_their_cause_and_leave_everything_untouched(cclqr):
    import torch
    capi = cclqr._capi
    mech = _chain(cclqr, 2)
    case = sc.synthetic_case(2, 1, "gated", 5, 3, 8, seed=1)
    ctrl = capi.CtrlHandle(mech, [0], K=case["K"].reshape(-1, 1, 24), N=5, zd=case["zd"].reshape(-1, 2, 13), n_ctrl=5)
    traj = torch.from_numpy(case["traj"]).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    quant, fin = nan(8, 5, 25), torch.full((8, 25), -1, dtype=torch.int32, device="cuda")
    lo, full = capi.rollout_quantiles_ws_bytes(mech, 1, 3, 8)
    assert lo == 8 * 25 * 64 and full == 8 * lo
    ws = nan(full // 8 + 1)

    def refused(match, fn, code=capi.EINVAL):
        with pytest.raises(capi.CclqrError, match=match) as e:
            fn()
        assert e.value.code == code

    def call(m=mech, c=ctrl, n=3, steps=8, k0=1, first=0, probs=P5, w=ws.data_ptr(), wb=full):
        capi.rollout_quantiles(m, c, n, steps, k0, traj.data_ptr(), probs, quant.data_ptr(), fin.data_ptr(), w, wb, first_instance=first)

    refused("null workspace", lambda: call(w=0))
    refused("workspace too small", lambda: call(wb=lo - 8))
    refused("aligned", lambda: call(w=ws.data_ptr() + 4))
    refused("n_prob = 17", lambda: call(probs=tuple(np.linspace(0, 1, 17))))
    refused("null argument|n_prob = 0", lambda: call(probs=()))
    refused(r"prob\[1\] = 1\.5", lambda: call(probs=(0.5, 1.5)))
    refused(r"prob\[0\] = -0\.1", lambda: call(probs=(-0.1,)))
    refused(r"prob\[2\] = nan", lambda: call(probs=(0.0, 1.0, float("nan"))))
    refused("n_inst = 0", lambda: call(n=0))
    refused("n_ctrl", lambda: call(first=3))
    refused("steps", lambda: call(steps=0))
    refused("k0", lambda: call(k0=0))
    refused("n_inst = 0", lambda: capi.rollout_quantiles_ws_bytes(mech, 1, 0, 8))
    m5 = _chain(cclqr, 5)
    c5 = capi.CtrlHandle(m5, [0], K=None, N=0)
    refused("another mechanism", lambda: call(c=c5))
    refused("another mechanism", lambda: call(m=m5))
    c5.close()
    torch.cuda.synchronize()
    assert torch.isnan(quant).all() and (fin == -1).all() and torch.isnan(ws).all()      # nothing was launched
    call(wb=lo)
    torch.cuda.synchronize()
    assert np.isfinite(quant.cpu().numpy()).all() and (fin == 3).all()
    ctrl.close()


# ---------------------------------------------------------------- g. through simulate
def test_simulate_returns_the_quantiles_of_the_recorded_run(cclqr):
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    nb = len(mech.bodies)
    lqr = cclqr.LQR(mech, [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])], ex["Q"], ex["R"], 10.0, xd=ex["xd"])
    rng = np.random.default_rng(0)
    n, steps = 300, 30
    z0 = cclqr.examples.cartpole_states(1, rng.uniform(-0.5, 0.5, n), rng.uniform(0, 1 / 3, (n, 1)))
    z00 = mech.state()

    def run(ens, **more):
        mech.set_state(z00)
        return cclqr.simulate(mech, cclqr.Storage(steps, nb), lqr, z0=z0, ensemble=ens, **more)

    ens = cclqr.Ensemble(mech, quantiles=P5)
    a, b, c = run(ens, record=False), run(ens, record=True), run(ens, record=False, chunk_steps=7)
    old, plain = run(cclqr.Ensemble(mech), record=False), run(None, record=False)
    mech.set_state(z00)
    e = a.ensemble
    assert e.quantile(0.5).shape == (steps, 12 * nb) and e.input_quantile(0.5).shape == (steps, 1) and (e.finite_count == n).all()
    for other in (b.ensemble, c.ensemble):
        assert all(qc.same_bits(e.quantile(p), other.quantile(p)) and qc.same_bits(e.input_quantile(p), other.input_quantile(p)) for p in P5)
        assert np.array_equal(e.finite_count, other.finite_count) and np.array_equal(e.mean, other.mean) and np.array_equal(e.M2, other.M2)
    # against the definition on the recorded trajectory
    case = dict(N=lqr.N, K=lqr.K[None], zd=lqr.zd[None], traj=b.z)
    got = np.stack([np.hstack([e.quantile(p), e.input_quantile(p)]) for p in P5], axis=1)
    qc.assert_quantiles(got, e.finite_count, case, P5, what="simulate")
    assert (e.min <= e.median).all() and (e.median <= e.max).all() and (e.min <= e.mean).all() and (e.mean <= e.max).all()
    assert (e.quantile(0.05) <= e.median).all() and (e.median <= e.quantile(0.95)).all()
    with pytest.raises(KeyError, match="0.25"):
        e.quantile(0.25)
    # without quantiles= everything is as it was
    o = old.ensemble
    assert o.probs is None and o.finite_count is None and np.array_equal(o.mean, e.mean) and np.array_equal(o.M2, e.M2) and np.array_equal(o.input_mean, e.input_mean)
    for r in (a, b, c, old):
        assert np.array_equal(r.zT, plain.zT) and np.array_equal(r.status, plain.status)
    assert plain.ensemble is None


# ---------------------------------------------------------------- h. the tie to the prediction
N, N_INST, SIGMA, SEED = 24, 2048, 1e-3, 1234
BOUND = 6.0 * np.sqrt(np.pi / 2.0 - 1.0) / np.sqrt(N_INST)      # in units of the coordinate's std


def tie_ratios(var, mean, std, median):
    """per knot j >= 1 the compared coordinates (Σ_jj,ii >= 1e-3 max) and |median - mean| / (BOUND std) there: (entries compared, largest ratio, its knot)"""
    compared, worst, at = 0, 0.0, -1
    for j in range(1, N):
        big = var[j] >= 1e-3 * var[j].max()
        assert big.sum() >= 1 and (std[j, big] > 0.0).all()
        ratio = np.abs(median[j, big] - mean[j, big]) / (BOUND * std[j, big])
        compared += int(big.sum())
        if ratio.max() > worst:
            worst, at = float(ratio.max()), j
    return compared, worst, at


def test_the_median_lies_where_a_gaussian_samples_median_lies(cclqr, orc):
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
    out = cclqr.simulate(mech, cclqr.Storage(N, nb), trk, z0=z0, noise_scale=SIGMA, noise_seed=SEED, record=False, chunk_steps=7,
                         ensemble=cclqr.Ensemble(mech, quantiles=(0.5,)))
    mech.set_state(z00)
    cov = cclqr.TrackingCovariance(mech, trk, ids, eids, Qb, Rb, noise_scale=SIGMA)
    try:
        var = cov.state_std[0] ** 2
    finally:
        cov.close()
    e = out.ensemble
    assert (out.status > 0).all() and (e.finite_count == N_INST).all()
    compared, worst, at = tie_ratios(var, e.mean, e.std, e.median)
    print("entries compared %d; largest |median - mean| / bound = %.4f at knot %d (bound = %.4f std)" % (compared, worst, at, BOUND))
    assert compared >= 100 and worst <= 1.0
