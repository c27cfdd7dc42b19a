"""LQRSweep on the device (cclqr_ctrl_create_lqr_batch_weights): one LQR per weight candidate in one call, on the cartpole (mx 24, mu 1: the resident
register-fragment kernel) and the Sawyer arm (mx 84, mu 7, two candidates: the tiled step).  Table p is bitwise table p of the shared-weights constructor with
candidate p, within the project's gain-parity bound (1e-7) of LQR(mech, ..., Q_p, R_p, horizon).K, invariant under a permutation of bodyids, and what simulate
and the score then run on."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_GAIN = 1e-7          # the project's gain-parity bound (tests/test_gpu_setup.py)
_cases = {}


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def case(cclqr, name):
    """dict(mech, mh, ids, eids, Qs, Rs, n, horizon, N, zd [nb][13], kw): the candidates differ per body and by orders of magnitude across the sweep"""
    if name in _cases:
        return _cases[name]
    if name == "cartpole":
        ex = cclqr.examples.cartpole_n(1)
        n, steps = 4, 60
        kw = dict(xd=ex["xd"])
    else:
        ex = cclqr.examples.sawyer(json.load(open(os.path.join(ROOT, "tests", "golden", "sawyer_arm_tables.json"))))
        n, steps = 2, 6
        kw = dict(xd=ex["xd"], qd=ex["qd"])
    mech = ex["mech"]
    nb = len(mech.bodies)
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    rng = np.random.default_rng(12)
    Qs = [[np.diag(rng.uniform(0.5, 2.0, 12)) * 10.0 ** (p - 1) for _ in range(nb)] for p in range(n)]
    Rs = [[np.eye(1) * rng.uniform(0.5, 2.0) * 10.0 ** (1 - p) for _ in eids] for p in range(n)]
    horizon = (steps - 0.5) * mech.Δt
    lqrs = [cclqr.LQR(mech, ids, eids, Qs[p], Rs[p], horizon, **kw) for p in range(n)]
    c = dict(name=name, mech=mech, mh=cclqr.lqr._device_mech(mech), nb=nb, ids=ids, eids=eids, Qs=Qs, Rs=Rs, n=n, horizon=horizon, N=steps, zd=lqrs[0].zd[0], lqrs=lqrs)
    c["sweep"] = cclqr.LQRSweep(mech, ids, eids, Qs, Rs, horizon, c["zd"])
    _cases[name] = c
    return c


def shared_batch(cclqr, c, p, **kw):
    """the shared-weights constructor (cclqr_ctrl_create_lqr_batch) on the same n setpoints with candidate p's pair"""
    s = c["sweep"]
    return cclqr._capi.BatchLqrHandle(c["mh"], s.zd, s.ctrl_joints, s.Q[p], s.R[p], kw.pop("N", c["N"]), Fd=s.Fd, **kw)


@pytest.mark.parametrize("name", ["cartpole", "sawyer"])
def test_tables_are_the_shared_constructors_and_match_lqr(cclqr, name):
    capi = cclqr._capi
    c = case(cclqr, name)
    s = c["sweep"]
    assert s.n == c["n"] and s.N == c["N"] and s.kbreak.shape == (c["n"],) and s.converged.all()
    assert s.Q.shape == (c["n"], 12 * c["nb"], 12 * c["nb"]) and s.R.shape == (c["n"], len(c["eids"]), len(c["eids"]))
    for p in range(c["n"]):
        h = shared_batch(cclqr, c, p)
        assert np.array_equal(s.gains(p), capi.ctrl_gains(c["mh"], h, p)) and s.kbreak[p] == h.kbreak[p], (name, p)
        h.close()
        lq = c["lqrs"][p]
        assert np.array_equal(s.Q[p], lq.Q) and np.array_equal(s.R[p], lq.R)
        print(name, p, "kbreak", s.kbreak[p], "gain err vs LQR", _rel(s.gains(p), lq.K))
        assert s.kbreak[p] == lq.kbreak and _rel(s.gains(p), lq.K) <= TOL_GAIN
    # the candidates matter: neighbouring tables differ by far more than the bound
    assert all(_rel(s.gains(p), s.gains(p - 1)) > 1e-2 for p in range(1, c["n"]))


def test_bodyids_permutation(cclqr):
    """bodyids reversed and every candidate's Q blocks reversed with them: bitwise the same gains"""
    c = case(cclqr, "cartpole")
    r = cclqr.LQRSweep(c["mech"], c["ids"][::-1], c["eids"], [Q[::-1] for Q in c["Qs"]], c["Rs"], c["horizon"], c["zd"])
    assert np.array_equal(r.Q, c["sweep"].Q)
    for p in range(c["n"]):
        assert np.array_equal(r.gains(p), c["sweep"].gains(p)), p
    r.close()


def test_broadcast_and_infinite_horizon(cclqr):
    """one shared R (length-1 Rs) and horizon = math.inf (LQR{T,Inf}: Ntemp = ceil(10/Δt) steps, one gain per table): per-table kbreak / converged and gains
    bitwise those of the shared-weights constructor with infinite_horizon"""
    capi = cclqr._capi
    c = case(cclqr, "cartpole")
    s = cclqr.LQRSweep(c["mech"], c["ids"], c["eids"], c["Qs"], c["Rs"][:1], math.inf, c["zd"])
    Ntemp = int(math.ceil(10 / c["mech"].Δt))
    assert s.n == 4 and s.N == 0 and s.R.shape[0] == 4 and all(np.array_equal(s.R[p], s.R[0]) for p in range(4))
    assert s.kbreak.shape == (4,) and s.converged.shape == (4,) and np.array_equal(s.converged, s.kbreak > 1)
    print("infinite horizon kbreak", s.kbreak, "converged", s.converged)
    for p in range(4):
        h = capi.BatchLqrHandle(c["mh"], s.zd, s.ctrl_joints, s.Q[p], s.R[p], Ntemp, Fd=s.Fd, infinite_horizon=True)
        g = s.gains(p)
        assert g.shape == (1, 1, 24) and np.array_equal(g, capi.ctrl_gains(c["mh"], h, p)) and s.kbreak[p] == h.kbreak[p], p
        h.close()
    s.close()


def test_on_a_plant_batch(cclqr):
    """plants=: candidate k is designed on plant k -- table p is bitwise table p of PlantLQR with candidate p shared"""
    c = case(cclqr, "cartpole")
    mech = c["mech"]
    plants = cclqr.PlantBatch.scaled(mech, 4, mass=(0.8, 1.2), length=(0.95, 1.05), seed=0)
    zd = cclqr.joint_position_states(mech, np.zeros((4, 2)), plants=plants)
    s = cclqr.LQRSweep(mech, c["ids"], c["eids"], c["Qs"], c["Rs"], c["horizon"], zd, plants=plants)
    assert s.first_plant == 0
    for p in range(4):
        pl = cclqr.PlantLQR(mech, plants, c["ids"], c["eids"], c["Qs"][p], c["Rs"][p], c["horizon"], zd)
        assert np.array_equal(s.gains(p), pl.gains(p)) and s.kbreak[p] == pl.kbreak[p], p
        pl.close()
    assert _rel(s.gains(1), c["sweep"].gains(1)) > 1e-3      # (the plants matter)
    s.close()


def test_simulate_and_score(cclqr):
    """simulate(mech, Storage, sweep, z0 = one start replicated): instance p's trajectory and status are bitwise those of instance p under the shared-weights
    controller of candidate p; record=False, score=Score(common Q, R) returns [4][4], bitwise the score of the recorded run; friction and noise are refused"""
    capi = cclqr._capi
    c = case(cclqr, "cartpole")
    mech, s, steps = c["mech"], c["sweep"], 50
    z0 = np.tile(cclqr.examples.cartpole_states(1, [0.2], [[0.15]]), (4, 1, 1))
    st = cclqr.simulate(mech, cclqr.Storage(steps, c["nb"]), s, z0=z0)
    assert st.z.shape == (4, steps, c["nb"], 13) and (st.status > 0).all()
    for p in range(4):
        h = shared_batch(cclqr, c, p)
        zT, tr, status = capi.rollout(c["mh"], h, z0, steps, record=True)
        assert np.array_equal(st.z[p], tr[p]) and np.array_equal(st.zT[p], zT[p]) and st.status[p] == status[p], p
        h.close()
    assert not np.array_equal(st.z[0], st.z[1])
    yard = cclqr.Score(mech, c["ids"], c["eids"], [np.eye(12)] * c["nb"], [np.eye(1)])
    lean = cclqr.simulate(mech, cclqr.Storage(steps, c["nb"]), s, z0=z0, record=False, score=yard)
    full = cclqr.simulate(mech, cclqr.Storage(steps, c["nb"]), s, z0=z0, record=True, score=yard)
    print("scores", lean.score)
    assert lean.score.shape == (4, 4) and np.array_equal(lean.score, full.score) and np.array_equal(full.z, st.z)
    assert len({float(x) for x in lean.score[:, 0]}) == 4
    with pytest.raises(ValueError, match="neither joint friction nor noise"):
        cclqr.simulate(mech, cclqr.Storage(2, c["nb"]), s, z0=z0, noise_seed=3)
