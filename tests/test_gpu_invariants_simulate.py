"""GPU tests of simulate(..., invariants=Invariants(...)): record or not and any chunking give the same bits, on a cartpole under LQR and on an uncontrolled double
pendulum; the series is the pass applied to the recorded trajectory and the summary the numpy min / max / first of the series; the statistics are those of
cclqr_series_*; the run itself is untouched; it combines with score=, ensemble=, joints= and plants=; and the physics the feature exists for, with the figures the
project already holds itself to: SURVEY's per-step contract (constraints and quaternions under 1e-9) on real rollouts, the first-order energy oscillation of
tests/test_oracle.py (halving the step halves it: ratio in (1.8, 2.2)) from the device summary, and a start state that is off its own plant's manifold by 1e-3."""
import numpy as np
import pytest

import ensemble_common as ec
import invariants_common as ic
import joints_common as jc

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)


def _cartpole(cclqr, n, steps):
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    lqr = cclqr.LQR(mech, [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])], ex["Q"], ex["R"], 10.0, xd=ex["xd"])
    rng = np.random.default_rng(0)
    z0 = cclqr.examples.cartpole_states(1, rng.uniform(-0.5, 0.5, n), rng.uniform(0, 1 / 3, (n, 1)))
    return dict(ex=ex, mech=mech, ctl=lqr, z0=z0, steps=steps, chunks=(7, 16))


def _double_pendulum(cclqr, n, steps):
    ex = cclqr.examples.double_pendulum(1.0, -0.5)
    mech = ex["mech"]
    ctl = cclqr.OpenLoop(mech, [cclqr.getid(ex["joints"][0])], np.zeros((steps, 1)))
    th = np.stack([np.linspace(0.6, 1.4, n), np.linspace(-0.9, 0.1, n)], axis=1)
    return dict(ex=ex, mech=mech, ctl=ctl, z0=cclqr.joint_position_states(mech, th), steps=steps, chunks=(1, 13))


@pytest.fixture(scope="module", params=["cartpole", "double_pendulum"])
def runs(cclqr, request):
    S = _cartpole(cclqr, 70, 30) if request.param == "cartpole" else _double_pendulum(cclqr, 70, 30)
    mech, nb = S["mech"], len(S["mech"].bodies)
    z00 = mech.state()

    def run(inv, **more):
        mech.set_state(z00)
        return cclqr.simulate(mech, cclqr.Storage(S["steps"], nb), S["ctl"], z0=S["z0"], invariants=inv, **more)

    iv = lambda **k: cclqr.Invariants(mech, rows=True, quantiles=PROBS, **k)
    S["plain"] = run(None, record=True)
    S["rec"] = run(iv(), record=True)
    S["norec"] = run(iv(), record=False, chunk_steps=S["chunks"][0])
    S["chunk"] = run(iv(), record=False, chunk_steps=S["chunks"][1])
    S["nokeep"] = run(cclqr.Invariants(mech, keep=False, quantiles=PROBS), record=False)
    mech.set_state(z00)
    return S


def test_record_or_not_and_any_chunking_give_the_same_bits(cclqr, runs):
    a = runs["rec"].invariants
    n, steps, ne = runs["z0"].shape[0], runs["steps"], len(runs["mech"].eqconstraints)
    assert a.count == n and a.series.shape == (n, steps, 6) and a.g.shape == (n, steps, ne, 5) and a.summary.shape == (n, 8) and a.energy.shape == (n, steps)
    for name in ("norec", "chunk"):
        b = runs[name].invariants
        for f in ("series", "g", "summary", "mean", "M2", "_quantiles"):
            assert ic.same_bits(getattr(a, f), getattr(b, f)), (name, f)
        assert np.array_equal(a.finite_count, b.finite_count)
        assert runs[name].z.shape[1] == 0
    k = runs["nokeep"].invariants
    assert k.series is None and k.energy is None and k.gap is None and k.g is None
    for f in ("summary", "mean", "M2", "_quantiles"):
        assert ic.same_bits(getattr(a, f), getattr(k, f)), f
    # with record=True the series is the pass applied to Storage's trajectory, and within the definition's bounds of it
    mh = runs["mech"]._cclqr_handle
    iv, rw, sm = ic.gpu_invariants(cclqr, mh, runs["rec"].z)
    assert ic.same_bits(iv, a.series) and ic.same_bits(rw, a.g) and ic.same_bits(sm, a.summary)
    ref = ic.reference(runs["mech"].tables(), runs["rec"].z)
    ic.assert_series(a.series, ref, "simulate")


def test_the_summary_is_the_numpy_min_max_first_of_the_series(runs):
    a = runs["rec"].invariants
    assert ic.same_bits(a.summary, ic.summary_of(a.series))
    E = a.energy
    assert ic.same_bits(a.energy_first, E[:, 0]) and ic.same_bits(a.energy_min, E.min(axis=1)) and ic.same_bits(a.energy_max, E.max(axis=1))
    assert ic.same_bits(a.gap_max, a.gap.max(axis=1)) and np.array_equal(a.gap_step, a.gap.argmax(axis=1) + 1)
    assert ic.same_bits(a.twist_max, a.twist.max(axis=1)) and ic.same_bits(a.quat_max, a.quat.max(axis=1)) and (a.bad_rows == 0).all()
    assert ic.same_bits(a.energy_drift, np.maximum(E.max(axis=1) - E[:, 0], E[:, 0] - E.min(axis=1)))
    assert ic.same_bits(a.energy, a.kinetic + a.potential)      # E is that one addition of outputs 0 and 1


def test_statistics_are_those_of_the_series(runs):
    a = runs["rec"].invariants
    n = a.count
    x = a.series
    rm, rq, Am, Aq = jc.series_moments(x)
    ec.assert_close(a.mean, rm, Am, "mean")
    ec.assert_close(a.M2, rq, Aq, "M2")
    assert np.allclose(a.std, np.sqrt(a.M2 / n))
    _, cnt = jc.assert_series_quantiles(a._quantiles, a.finite_count, x, PROBS, "quantiles")      # (p = 0 and p = 1 are the extremes, bit for bit)
    assert (cnt == n).all()
    assert ic.same_bits(a.min, x.min(axis=0)) and ic.same_bits(a.max, x.max(axis=0)) and ic.same_bits(a.median, a.quantile(0.5))
    assert (a.min <= a.median).all() and (a.median <= a.max).all()
    with pytest.raises(KeyError, match=r"0\.25.*\[0\.0, 0\.05, 0\.5, 0\.95, 1\.0\]"):
        a.quantile(0.25)


def test_the_run_itself_is_untouched(runs):
    plain = runs["plain"]
    assert plain.invariants is None
    for name in ("rec", "norec", "chunk", "nokeep"):
        assert ic.same_bits(runs[name].zT, plain.zT) and np.array_equal(runs[name].status, plain.status), name
    assert ic.same_bits(runs["rec"].z, plain.z) and (plain.status > 0).all()


def test_it_combines_with_score_ensemble_joints_and_plants(cclqr):
    S = _cartpole(cclqr, 40, 20)
    ex, mech, nb = S["ex"], S["mech"], len(S["mech"].bodies)
    plants = cclqr.PlantBatch.scaled(mech, 48, mass=(0.9, 1.1), length=(0.95, 1.05), seed=2, first_index=3)
    z0 = cclqr.joint_position_states(mech, np.stack([np.linspace(-0.3, 0.3, 40), np.linspace(0.0, 0.3, 40)], axis=1), plants=plants, first_instance=5)
    z00 = mech.state()
    sc_ = cclqr.Score(mech, [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])], ex["Q"], ex["R"])

    def run(**more):
        mech.set_state(z00)
        return cclqr.simulate(mech, cclqr.Storage(20, nb), S["ctl"], z0=z0, record=False, plants=plants, first_instance=5, **more)

    iv = lambda: cclqr.Invariants(mech, rows=True)
    alone = run(invariants=iv())
    every = run(invariants=iv(), score=sc_, ensemble=cclqr.Ensemble(mech, quantiles=(0.5,)), joints=cclqr.Joints(mech), chunk_steps=6)
    scored = run(score=sc_)
    mech.set_state(z00)
    assert every.score.shape == (40, 4) and every.ensemble.count == 40 and every.joints.theta.shape == (40, 20, 2)
    assert ic.same_bits(every.score, scored.score) and ic.same_bits(every.zT, scored.zT)
    for f in ("series", "g", "summary", "mean", "M2"):
        assert ic.same_bits(getattr(every.invariants, f), getattr(alone.invariants, f)), f
    with pytest.raises(KeyError, match="not asked for"):
        alone.invariants.median
    # every instance was measured on its own plant: the start states lie on the plants' manifolds, and the masses in T and V are the plants'
    assert (alone.invariants.gap[:, 0] < 1e-9).all() and (alone.invariants.gap_max < 1e-9).all()
    rows = list(plants.rows_for(5, 40))
    tt = ic.Tables(mech.tables())
    V0 = -tt.g * (plants.mass[rows] * z0[:, :, 2]).sum(axis=1)
    assert np.abs(alone.invariants.potential[:, 0] - V0).max() <= 1e-10 * np.abs(V0).max()
    assert np.abs(alone.invariants.potential[:, 0] + tt.g * (tt.mass[None] * z0[:, :, 2]).sum(axis=1)).max() > 1e-3      # (the nominal masses would not give it)


# ---------------------------------------------------------------- physics, with the project's own figures

def test_constraints_and_quaternions_hold_surveys_contract_on_real_rollouts(cclqr):
    """64 instances, 50 steps: the cartpole under LQR and the 17-body chain falling freely from near its upright pose; every step of every instance has its
    constraint rows and its quaternion norms under 1e-9 ('Integrator invariants'), read from the summary of a run that kept no trajectory"""
    S = _cartpole(cclqr, 64, 50)
    out = cclqr.simulate(S["mech"], cclqr.Storage(50, 2), S["ctl"], z0=S["z0"], record=False, invariants=cclqr.Invariants(S["mech"], keep=False))
    v = out.invariants
    assert (out.status > 0).all() and (v.bad_rows == 0).all()
    print("cartpole: gap_max %.3g twist_max %.3g quat_max %.3g" % (v.gap_max.max(), v.twist_max.max(), v.quat_max.max()))
    assert (v.gap_max < 1e-9).all() and (v.twist_max < 1e-9).all() and (v.quat_max < 1e-9).all()
    ex = cclqr.examples.cartpole_n(16)
    mech = ex["mech"]
    th0 = np.zeros(17)
    rng = np.random.default_rng(1)
    th = th0[None] + np.concatenate([rng.uniform(-0.5, 0.5, (64, 1)), rng.uniform(-0.2, 0.2, (64, 16))], axis=1)
    z0 = cclqr.joint_position_states(mech, th)
    ctl = cclqr.OpenLoop(mech, [cclqr.getid(ex["ctrl"][0])], np.zeros((50, 1)))
    out = cclqr.simulate(mech, cclqr.Storage(50, 17), ctl, z0=z0, record=False, invariants=cclqr.Invariants(mech), chunk_steps=20)
    v = out.invariants
    assert (out.status > 0).all() and (v.bad_rows == 0).all()
    print("17-body chain: gap_max %.3g twist_max %.3g quat_max %.3g" % (v.gap_max.max(), v.twist_max.max(), v.quat_max.max()))
    assert (v.gap_max < 1e-9).all() and (v.twist_max < 1e-9).all() and (v.quat_max < 1e-9).all()
    assert (v.gap < 1e-9).all() and (v.kinetic[:, -1] > v.kinetic[:, 0]).all()      # it really falls


def test_energy_oscillation_of_the_double_pendulum_halves_with_the_step(cclqr):
    """the uncontrolled double pendulum (1.0, -0.5) for 10 s at dt = 0.01 and 0.005: energy_max - energy_min halves (the assertion of tests/test_oracle.py on the
    oracle's trajectory, here from the device summary of a run that kept no trajectory)"""
    osc = []
    for dt in (0.01, 0.005):
        ex = cclqr.examples.double_pendulum(1.0, -0.5)
        mech = ex["mech"]
        mech.Δt = dt
        n = int(round(10 / dt))
        ctl = cclqr.OpenLoop(mech, [cclqr.getid(ex["joints"][0])], np.zeros((n, 1)))
        out = cclqr.simulate(mech, cclqr.Storage(n, 2), ctl, z0=mech.state()[None], record=False, invariants=cclqr.Invariants(mech, keep=False), chunk_steps=400)
        v = out.invariants
        assert (out.status > 0).all() and v.bad_rows[0] == 0
        osc.append(float(v.energy_max[0] - v.energy_min[0]))
        assert v.gap_max[0] < 1e-9 and v.twist_max[0] < 1e-9 and v.quat_max[0] < 1e-9
        assert v.energy_drift[0] <= osc[-1]
    print("energy oscillation %.6g at dt = 0.01, %.6g at dt = 0.005, ratio %.4f" % (osc[0], osc[1], osc[0] / osc[1]))
    assert 1.8 < osc[0] / osc[1] < 2.2


def test_a_start_state_off_its_plants_manifold_shows_at_step_one(cclqr):
    """the check the feature exists for: a start placed with the NOMINAL vertices on a plant whose p2 is moved by 1e-3 has gap ~ 1e-3 at step 1 -- the moved vertex
    seen from the parent, a vector of length 1e-3, whose largest component lies in [1e-3 / sqrt 3, 1e-3] --; the same start from joint_position_states(...,
    plants=) has gap < 1e-9"""
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    t = mech.tables()
    n = 5
    p2 = np.tile(np.asarray(t.p2, dtype=np.float64).reshape(1, t.ne, 3), (n, 1, 1))
    p2[:, 1, 2] += 1e-3      # the pole's own vertex, along its axis
    plants = cclqr.PlantBatch(mech, p2=p2)
    th = np.stack([np.linspace(-0.2, 0.2, n), np.linspace(0.1, 0.3, n)], axis=1)
    ctl = cclqr.OpenLoop(mech, [cclqr.getid(ex["ctrl"][0])], np.zeros((3, 1)))
    z00 = mech.state()
    off = cclqr.simulate(mech, cclqr.Storage(3, 2), ctl, z0=cclqr.joint_position_states(mech, th), record=False, plants=plants, invariants=cclqr.Invariants(mech))
    mech.set_state(z00)
    on = cclqr.simulate(mech, cclqr.Storage(3, 2), ctl, z0=cclqr.joint_position_states(mech, th, plants=plants), record=False, plants=plants,
                        invariants=cclqr.Invariants(mech))
    mech.set_state(z00)
    g1 = off.invariants.gap[:, 0]
    print("gap at step 1: off the manifold %s, on it %s" % (g1, on.invariants.gap[:, 0]))
    assert (g1 >= 1e-3 / np.sqrt(3) * (1 - 1e-6)).all() and (g1 <= 1e-3 * (1 + 1e-6)).all()
    assert (on.invariants.gap[:, 0] < 1e-9).all() and (on.invariants.gap_max < 1e-9).all()
    assert (off.invariants.twist[:, 0] < 1e-9).all()      # orientations do not know about vertices
