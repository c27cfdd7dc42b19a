"""TrackingPolicyValue and predicted_cost end to end on chain3, with the setup of tests/test_gpu_tracking_covariance_noise.py (the cart with two pendulum links
hanging; the open-loop rollout of 24 steps under U_k = 4 sin(2 pi k / 24), one TrackingLQR along it, Q = 10 Δt I, R = 0.1 Δt): the test that ties P_0 to actual
rollouts.

A cart displacement ε = 1.6, 0.4, 0.1 on the constraint manifold, z0 = joint_position_states(mech, th0 + ε (1, 0, 0)).  A noise-free simulate(..., steps = N,
score = Score(...)) from that start gives J = Jx + Ju; r(ε) = J / predicted_cost(mech, tpv, z0) - 1 is the nonlinear remainder, first order in ε along the
reference's own motion.  predicted_cost is Δz' P_0 Δz = tr(P_0 δδ'), which is TrackingCovariance's sum(expected_score) for Sigma0 = δδ' without noise, so the CPU
twin's figures recorded in that test are the yardstick here:
    r = 2.03e-6, 5.4e-7, 1.4e-7      folds 3.79 and 3.95
(with the gain rows one knot late or early the folds are 0.87 .. 0.97: a cost-to-go whose rows are shifted by a knot does not pass).  The test asserts both folds
>= 3 and prints r."""
import numpy as np
import pytest

from plant_tracking_common import open_loop
from plants_common import mechanism_of

pytestmark = pytest.mark.gpu

N = 24
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
    tpv = cclqr.TrackingPolicyValue(mech, trk, ids, eids, Qb, Rb)
    _s.update(mech=mech, th0=th0, nb=nb, U=U, zd=zd, ids=ids, eids=eids, Qb=Qb, Rb=Rb, trk=trk, tpv=tpv, score=cclqr.Score(mech, ids, eids, Qb, Rb))
    return _s


def test_a_perturbed_start_is_scored_as_predicted_to_first_order(cclqr, orc):
    s = setup(cclqr, orc)
    assert s["tpv"].N == N and s["tpv"].knot == 0 and s["tpv"].n_models == 1
    r = []
    for eps in EPS:
        z0 = cclqr.joint_position_states(s["mech"], (s["th0"] + eps * DTH)[None])
        predicted = float(cclqr.predicted_cost(s["mech"], s["tpv"], z0)[0])
        st = cclqr.simulate(s["mech"], cclqr.Storage(N, s["nb"]), s["trk"], z0=z0, record=False, score=s["score"])
        assert (st.status > 0).all()
        J = float(st.score[0, 0] + st.score[0, 1])
        r.append(J / predicted - 1.0)
        print("eps %.4g: Jx + Ju = %.12g, predicted_cost = %.12g, realised / predicted - 1 = %.4g" % (eps, J, predicted, r[-1]))
    folds = [r[0] / r[1], r[1] / r[2]]
    print("folds per quartering: %.3f and %.3f (the CPU twin of the tracking covariance: r = 2.03e-6, 5.4e-7, 1.4e-7, folds 3.79 and 3.95)" % tuple(folds))
    assert all(np.isfinite(folds)) and min(folds) >= 3.0, (r, folds)


def test_a_device_tensor_start_gives_the_host_paths_bits_and_a_bare_tracking_lqr_still_raises(cclqr, orc):
    import torch
    s = setup(cclqr, orc)
    z0 = np.concatenate([cclqr.joint_position_states(s["mech"], (s["th0"] + eps * DTH)[None]) for eps in EPS])
    host = cclqr.predicted_cost(s["mech"], s["tpv"], z0)
    dev = cclqr.predicted_cost(s["mech"], s["tpv"], torch.from_numpy(np.ascontiguousarray(z0)).cuda())
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and host.shape == (len(EPS),) and np.array_equal(dev.cpu().numpy(), host) and (host > 0).all()
    with pytest.raises(TypeError, match="TrackingPolicyValue"):
        cclqr.predicted_cost(s["mech"], s["trk"], z0)
