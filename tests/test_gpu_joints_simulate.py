"""GPU test of simulate(..., joints=Joints(...)): the pendulum of examples/lqr_pendulum.jl released with enough angular velocity to go over the top at least twice
under a controller that applies no input, 300 instances with spread initial rates, 60 steps.  The joint series the chunk loop returns is the numpy definition
(tests/joints_common.py) evaluated on the recorded trajectory; record or not and any chunking give the same bits; the statistics are those of the series."""
import numpy as np
import pytest

import ensemble_common as ec
import joints_common as jc

pytestmark = pytest.mark.gpu

N, STEPS = 300, 60
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)


@pytest.fixture(scope="module")
def runs(cclqr):
    ex = cclqr.examples.pendulum()
    mech = ex["mech"]
    rate = np.linspace(26.0, 36.0, N)      # rad/s about the joint axis: 0.26 .. 0.36 rad per step of 0.01 s, two turns need 12.6 rad in 0.6 s
    z0 = cclqr.joint_position_states(mech, np.full((N, 1), 0.3))
    z0[:, 0, 10] = rate
    z0[:, 0, 7:10] = np.cross(np.stack([rate, 0 * rate, 0 * rate], axis=1), z0[:, 0, 0:3])      # the centre of mass goes round the joint at the origin
    ctl = cclqr.OpenLoop(mech, [cclqr.getid(ex["joints"][0])], np.zeros((STEPS, 1)))
    tend = STEPS * mech.Δt - 1e-9
    jn = lambda **k: cclqr.Joints(mech, quantiles=PROBS, **k)
    out = dict(mech=mech, z0=z0)
    out["plain"] = cclqr.simulate(mech, tend, ctl, record=True, z0=z0)
    out["rec"] = cclqr.simulate(mech, tend, ctl, record=True, z0=z0, joints=jn())
    out["norec"] = cclqr.simulate(mech, tend, ctl, record=False, z0=z0, joints=jn())
    out["chunk7"] = cclqr.simulate(mech, tend, ctl, record=False, z0=z0, joints=jn(), chunk_steps=7)
    out["nokeep"] = cclqr.simulate(mech, tend, ctl, record=False, z0=z0, joints=jn(keep=False), chunk_steps=16)
    out["raw"] = cclqr.simulate(mech, tend, ctl, record=False, z0=z0, joints=cclqr.Joints(mech, continuous=False, rates=False))
    return out


def test_the_run_goes_over_the_top_twice_and_the_series_is_the_definition(runs):
    rec = runs["rec"]
    assert rec.steps == STEPS and rec.z.shape == (N, STEPS, 1, 13) and (rec.status > 0).all()
    t = runs["mech"].tables()
    ref = jc.reference(t, rec.z, jc.CONTINUOUS)
    jc.assert_generated(ref)
    assert np.abs(ref["turns"]).max() >= 2 and (np.abs(ref["theta"][:, -1, 0]) > 4 * np.pi).all()      # every instance has gone round at least twice
    j = rec.joints
    assert j.theta.shape == j.rate.shape == (N, STEPS, 1) and j.count == N and j.continuous
    jc.assert_joints(j.theta, j.rate, ref, "simulate")
    raw = runs["raw"].joints
    jc.assert_joints(raw.theta, None, jc.reference(t, rec.z, jc.RAW), "raw")
    assert raw.rate is None and raw.rate_mean is None and np.abs(raw.theta).max() <= 2 * np.pi and not raw.continuous
    with pytest.raises(KeyError, match="rates=False"):
        raw.rate_std


def test_record_or_not_and_any_chunking_give_the_same_bits(runs):
    a = runs["rec"].joints
    for name in ("norec", "chunk7"):
        b = runs[name].joints
        for f in ("theta", "rate", "mean", "M2", "rate_mean", "rate_M2", "_quantiles"):
            assert jc.same_bits(getattr(a, f), getattr(b, f)), (name, f)
        assert np.array_equal(a.finite_count, b.finite_count)
    assert runs["norec"].z.shape[1] == 0
    k = runs["nokeep"].joints
    assert k.theta is None and k.rate is None
    for f in ("mean", "M2", "rate_mean", "rate_M2", "_quantiles"):
        assert jc.same_bits(getattr(a, f), getattr(k, f)), f


def test_statistics_are_those_of_the_series(runs):
    j = runs["rec"].joints
    x = np.concatenate([j.theta, j.rate], axis=2)
    rm, rq, Am, Aq = jc.series_moments(x)
    ec.assert_close(np.concatenate([j.mean, j.rate_mean], axis=1), rm, Am, "mean")
    ec.assert_close(np.concatenate([j.M2, j.rate_M2], axis=1), rq, Aq, "M2")
    assert np.allclose(j.std, np.sqrt(j.M2 / N)) and np.allclose(j.rate_std, np.sqrt(j.rate_M2 / N))
    quant, cnt = jc.assert_series_quantiles(j._quantiles, j.finite_count, x, PROBS, "quantiles")
    assert (cnt == N).all()
    assert jc.same_bits(j.median, j._quantiles[:, 2, :1]) and jc.same_bits(j.rate_quantile(0.95), j._quantiles[:, 3, 1:])
    assert jc.same_bits(j.min, x[..., :1].min(axis=0)) and jc.same_bits(j.max, x[..., :1].max(axis=0))
    assert (j.min <= j.median).all() and (j.median <= j.max).all() and (j.min <= j.mean).all() and (j.mean <= j.max).all()
    assert (j.rate_quantile(0) <= j.rate_mean).all() and (j.rate_mean <= j.rate_quantile(1)).all()
    with pytest.raises(KeyError, match=r"0\.25.*\[0\.0, 0\.05, 0\.5, 0\.95, 1\.0\]"):
        j.quantile(0.25)


def test_the_run_itself_is_untouched(runs):
    plain = runs["plain"]
    assert plain.joints is None
    for name in ("rec", "norec", "chunk7", "nokeep"):
        assert jc.same_bits(runs[name].zT, plain.zT) and np.array_equal(runs[name].status, plain.status), name
    assert jc.same_bits(runs["rec"].z, plain.z)


def test_joints_combine_with_score_and_ensemble(cclqr, runs):
    mech, z0 = runs["mech"], runs["z0"][:40]
    ex = cclqr.examples.pendulum()
    ctl = cclqr.OpenLoop(mech, [cclqr.getid(mech.eqconstraints[0])], np.zeros((STEPS, 1)))
    sc_ = cclqr.Score(mech, [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[0])], ex["Q"], ex["R"])
    both = cclqr.simulate(mech, STEPS * mech.Δt - 1e-9, ctl, record=False, z0=z0, score=sc_, ensemble=cclqr.Ensemble(mech, quantiles=(0.5,)),
                          joints=cclqr.Joints(mech), chunk_steps=25)
    alone = cclqr.simulate(mech, STEPS * mech.Δt - 1e-9, ctl, record=False, z0=z0, joints=cclqr.Joints(mech))
    assert both.score.shape == (40, 4) and both.ensemble.count == 40 and both.ensemble.median.shape == (STEPS, 12)
    assert jc.same_bits(both.joints.theta, alone.joints.theta) and jc.same_bits(both.joints.M2, alone.joints.M2)
    with pytest.raises(KeyError, match="not asked for"):
        alone.joints.median
