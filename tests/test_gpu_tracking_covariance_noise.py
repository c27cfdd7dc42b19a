"""TrackingCovariance end to end on chain3 (the cart with two pendulum links, 3 bodies, hanging; tests/plant_tracking_common.py's reference: the open-loop rollout of 24
steps under U_k = 4 sin(2 pi k / 24) from the hanging pose), one TrackingLQR along it, Q = 10 Δt I, R = 0.1 Δt.  These are the tests that tie the knot convention
-- knot j = row j of a recorded rollout = the state the law sees at step j + 1 -- and expected_score to actual rollouts.

Deterministic (resolves the indexing).  Wu = None, Sigma0 = δδ' with δ = the state error of joint_position_states(mech, th0 + ε dθ) about zd[0]: a perturbation ON the
constraint manifold.  A noise-free simulate(..., steps = N, score = Score(...)) from that start gives J = Jx + Ju; r(ε) = J / sum(expected_score) - 1 is the nonlinear
remainder.  J is even in ε for a rotation of the hanging links (r falls 12 to 16-fold per quartering there: second order), so the first-order regime the check asks
for is a displacement of the cart, dθ = (1, 0, 0), made first order by the reference's own motion.  The CPU twin (oracle rollout, scored by
score_common.stage_costs; the longdouble recursion on the oracle's linearisation at every knot), ε = 1.6, 0.4, 0.1:
    r = 2.028e-06, 5.355e-07, 1.356e-07      folds 3.79 and 3.95
the same twin with the gain rows applied one knot LATE:   r = -9.728e-06, -1.122e-05, -1.162e-05   folds 0.87 and 0.97  -- it does not pass;
one knot EARLY:                                           r = -1.079e-05, -1.228e-05, -1.268e-05   folds 0.88 and 0.97.
(The oracle records the start as row 0: traj[0] - z0 = 0 exactly, which is the convention above.)  The device test asserts both folds >= 3 and prints the figures.

Monte-Carlo.  2048 noisy rollouts of N - 1 steps from zd[0] (noise_scale = 1e-3, one seed): every diagonal entry of the sample second moment of zT - zd[N-1] with
Σ_ii >= 1e-3 max Σ_ii lies within 6 sqrt(2 / n) = 0.1875 relative of Σ_{N-1,ii} -- six standard deviations of a Gaussian sample variance, as
tests/test_gpu_covariance_noise.py argues -- and at least 6 entries are compared; the sample mean of Jx of a scored run of N steps lies within the same bound of
expected_score[0] (the relative spread of a sum of correlated χ² terms is at most that of one).  On the CPU oracle with the same seed, against the longdouble
recursion alone: 9 of 36 entries compared, the largest deviation 0.0448; mean Jx 3.17524e-09 against 3.18259e-09 (-0.0023), mean Ju 1.49848e-09 against 1.50131e-09
(-0.0019).  The same sample against Σ_{N-2} deviates by 0.159 and against Σ_{N-3} by 0.332: the Monte-Carlo check tells two knots apart, not one; the deterministic
check above is the one that resolves a single knot."""
import numpy as np
import pytest

import score_common as sc
from plant_tracking_common import open_loop
from plants_common import mechanism_of

pytestmark = pytest.mark.gpu

N, N_INST, SIGMA, SEED = 24, 2048, 1e-3, 1234
BOUND = 6.0 * np.sqrt(2.0 / N_INST)
EPS, DTH = (1.6, 0.4, 0.1), np.array([1.0, 0.0, 0.0])
_s = {}


def setup(cclqr, orc):
    if _s:
        return _s
    mech, th0 = mechanism_of(cclqr, ("chain", 2))
    t = mech.tables()
    nb = t.nb
    U = 4.0 * np.sin(2 * np.pi * np.arange(N) / N)[:, None]
    zd = open_loop(orc, t, [0], U, cclqr.joint_position_states(mech, th0[None])[0])
    ids, eids = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[0])]
    Qb, Rb = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1]
    trk = cclqr.TrackingLQR(mech, cclqr.Storage(N, nb, 1, z=np.ascontiguousarray(zd[None])), U, eids, Qb, Rb)
    _s.update(mech=mech, th0=th0, nb=nb, U=U, zd=zd, ids=ids, eids=eids, Qb=Qb, Rb=Rb, trk=trk, score=cclqr.Score(mech, ids, eids, Qb, Rb))
    return _s


def test_a_perturbed_start_without_noise_is_scored_as_predicted_to_first_order(cclqr, orc):
    s = setup(cclqr, orc)
    r = []
    for eps in EPS:
        z0 = cclqr.joint_position_states(s["mech"], (s["th0"] + eps * DTH)[None])
        d = sc.state_errors(z0[0], s["zd"][0]).reshape(-1)
        cov = cclqr.TrackingCovariance(s["mech"], s["trk"], s["ids"], s["eids"], s["Qb"], s["Rb"], Sigma0=np.outer(d, d))
        try:
            expected = float(cov.expected_score[0].sum())
            assert cov.N == N and not cov.input_std[0, N - 1].any()
        finally:
            cov.close()
        st = cclqr.simulate(s["mech"], cclqr.Storage(N, s["nb"]), s["trk"], z0=z0, record=False, score=s["score"])
        assert (st.status > 0).all()
        J = float(st.score[0, 0] + st.score[0, 1])
        r.append(J / expected - 1.0)
        print("eps %.4g: Jx + Ju = %.12g, sum(expected_score) = %.12g, realised / predicted - 1 = %.4g" % (eps, J, expected, r[-1]))
    folds = [r[0] / r[1], r[1] / r[2]]
    print("folds per quartering: %.3f and %.3f (the CPU twin: 3.79 and 3.95; gain rows one knot late: 0.87 and 0.97)" % tuple(folds))
    assert all(np.isfinite(folds)) and min(folds) >= 3.0, (r, folds)


def test_noisy_rollouts_show_the_predicted_spread_and_the_predicted_score(cclqr, orc):
    s = setup(cclqr, orc)
    z0 = np.ascontiguousarray(np.tile(s["zd"][0], (N_INST, 1, 1)))
    cov = cclqr.TrackingCovariance(s["mech"], s["trk"], s["ids"], s["eids"], s["Qb"], s["Rb"], noise_scale=SIGMA)
    try:
        Sig, ex = cov.Sigma(0), cov.expected_score[0].copy()
        zstd_last = cov.state_std[0, N - 1].copy()
    finally:
        cov.close()
    st = cclqr.simulate(s["mech"], cclqr.Storage(N - 1, s["nb"]), s["trk"], z0=z0, record=False, noise_scale=SIGMA, noise_seed=SEED)
    assert (st.status > 0).all()
    dz = sc.state_errors(st.zT, s["zd"][N - 1]).reshape(N_INST, -1)
    S = dz.T @ dz / N_INST
    d = np.diag(Sig)
    big = d >= 1e-3 * d.max()
    ratio = np.diag(S)[big] / d[big]
    print("entries compared %d of %d; S_ii / Σ_ii = %s; max |Δz| = %.3g; bound %.4f (the oracle: 9 entries, largest deviation 0.0448)" % (
        big.sum(), len(d), ratio, np.abs(dz).max(), BOUND))
    assert big.sum() >= 6
    assert np.abs(ratio - 1.0).max() <= BOUND
    assert s["ids"] == sorted(s["ids"]) and np.array_equal(zstd_last, np.sqrt(np.maximum(d, 0.0)))      # state_std of the last knot is that Σ's diagonal
    sc_run = cclqr.simulate(s["mech"], cclqr.Storage(N, s["nb"]), s["trk"], z0=z0, record=False, noise_scale=SIGMA, noise_seed=SEED, score=s["score"])
    assert (sc_run.status > 0).all()
    Jx, Ju = float(sc_run.score[:, 0].mean()), float(sc_run.score[:, 1].mean())
    print("sample mean of Jx = %.6g against expected_score[0] = %.6g: ratio - 1 = %.4f; of Ju = %.6g against %.6g: %.4f (the oracle: -0.0023 and -0.0019)" % (
        Jx, ex[0], Jx / ex[0] - 1.0, Ju, ex[1], Ju / ex[1] - 1.0))
    assert abs(Jx / ex[0] - 1.0) <= BOUND
