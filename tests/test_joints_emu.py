"""CPU tests of the joint pass's per-joint functions (csrc/cclqr_joints.h), run lane by lane on the host by tests/emu/emu_joints.cpp, against the numpy restatement
of the definition (tests/joints_common.py): both modes within the bounds, the turn count exact over several turns either way, a q -> -q flip, the carry over chunk
plans bit for bit, a NaN row, and the tile moments of a series in the defined order."""
import numpy as np
import pytest

import ensemble_common as ec
import joints_common as jc


@pytest.fixture(scope="module")
def emu():
    return jc.emu_joints()


@pytest.mark.parametrize("nb", [1, 9, 17])
@pytest.mark.parametrize("mode", [jc.RAW, jc.CONTINUOUS])
def test_header_functions_are_the_definition(cclqr, emu, nb, mode):
    t = jc.mixed_chain(cclqr, nb, seed=nb)
    traj, _ = jc.slab(t, 5, 8, seed=nb)
    ref = jc.reference(t, traj, mode)
    jc.assert_generated(jc.reference(t, traj, jc.CONTINUOUS))
    th, rt, cr = jc.emu_joints_run(emu, t, traj, mode)
    jc.assert_joints(th, rt, ref, "nb %d mode %d" % (nb, mode))
    if mode == jc.CONTINUOUS:
        assert np.array_equal(cr[..., 1], ref["carry"][..., 1])      # the turn counts, exactly
        assert np.abs(ref["turns"]).max() >= 2 or nb == 1
    th2, _, _ = jc.emu_joints_run(emu, t, traj, mode, rates=False)
    assert jc.same_bits(th, th2)


def test_turns_are_exact_over_several_turns_in_both_directions(cclqr, emu):
    t = cclqr.examples.pendulum()["mech"].tables()
    steps = 24
    ang = np.concatenate([np.linspace(0, 6 * np.pi + 1.0, 8), np.linspace(6 * np.pi + 1.0, -6 * np.pi - 1.0, steps - 8)])   # up three turns in steps of 2.8 rad, down six in steps of 2.65
    assert np.abs(np.diff(ang)).max() <= 3.0
    tt = jc.Tables(t)
    traj = np.zeros((1, steps, 1, 13))
    traj[0, :, 0, 3:7] = jc._qmul(jc._axis_angle(tt.axis[0], ang), np.broadcast_to(tt.qoff[0], (steps, 4)))
    ref = jc.reference(t, traj, jc.CONTINUOUS)
    jc.assert_generated(ref)
    th, _, cr = jc.emu_joints_run(emu, t, traj, jc.CONTINUOUS)
    jc.assert_joints(th, None, ref, "pendulum")
    assert ref["turns"].max() >= 3 and ref["turns"].min() <= -3
    assert np.abs(th[0, :, 0] - ang).max() < 1e-9      # the continuous angle IS the generating angle (which starts inside [-pi, pi])
    raw, _, _ = jc.emu_joints_run(emu, t, traj, jc.RAW)
    assert np.abs(raw).max() <= 2 * np.pi


def test_a_quaternion_flip_between_rows_leaves_theta_within_the_bound(cclqr, emu):
    t = jc.mixed_chain(cclqr, 5, seed=2)
    traj, _ = jc.slab(t, 3, 9, seed=4)
    ref = jc.reference(t, traj, jc.CONTINUOUS)
    flipped = traj.copy()
    flipped[:, 4:, 1, 3:7] *= -1.0
    flipped[:, 6, 3, 3:7] *= -1.0
    th, rt, _ = jc.emu_joints_run(emu, t, flipped, jc.CONTINUOUS)
    jc.assert_joints(th, rt, ref, "flipped")


@pytest.mark.parametrize("plan", [[1] * 8, [3, 3, 2]])
def test_carry_over_a_chunk_plan_gives_the_bits_of_one_pass(cclqr, emu, plan):
    t = jc.mixed_chain(cclqr, 9, seed=1)
    traj, _ = jc.slab(t, 4, 8, seed=6)
    whole_th, whole_rt, whole_cr = jc.emu_joints_run(emu, t, traj, jc.CONTINUOUS)
    th, rt, cr, k0 = np.full_like(whole_th, np.nan), np.full_like(whole_rt, np.nan), None, 1
    for s in plan:
        a, b, cr = jc.emu_joints_run(emu, t, traj[:, k0 - 1:k0 - 1 + s], jc.CONTINUOUS, k0=k0, out_steps=8, carry=cr)
        th[:, k0 - 1:k0 - 1 + s], rt[:, k0 - 1:k0 - 1 + s] = a[:, k0 - 1:k0 - 1 + s], b[:, k0 - 1:k0 - 1 + s]
        assert np.isnan(a[:, :k0 - 1]).all() and np.isnan(a[:, k0 - 1 + s:]).all()      # only the launch's rows are written
        k0 += s
    assert jc.same_bits(th, whole_th) and jc.same_bits(rt, whole_rt) and jc.same_bits(cr, whole_cr)


def test_a_nan_row_gives_nan_there_and_resumes_from_the_last_finite_row(cclqr, emu):
    t = jc.mixed_chain(cclqr, 4, seed=7)      # joints 0 (prismatic), 1, 2 (revolute), 3 (prismatic)
    traj, _ = jc.slab(t, 2, 10, seed=8, max_step=1.4)      # (two increments stay under 3 rad, so that the row after the gap decides as the definition does)
    bad = traj.copy()
    bad[0, 4, 1, 3:7] = np.nan          # body 1's orientation at row 4: joints 1 (child) and 2 (parent) have no angle there; the prismatic joints 0, 3 do not read it
    bad[1, 6, 2, 5] = np.inf
    ref = jc.reference(t, bad, jc.CONTINUOUS)
    th, rt, _ = jc.emu_joints_run(emu, t, bad, jc.CONTINUOUS)
    jc.assert_joints(th, rt, ref, "planted")
    nan = np.isnan(th)
    want = np.zeros_like(nan)
    want[0, 4, [1, 2]] = True
    want[1, 6, [2, 3]] = True           # body 2 is joint 2's child and joint 3's parent (prismatic: its R_a reads the orientation)
    assert np.array_equal(nan, want)
    assert not np.isinf(th).any() and not np.isinf(rt).any()
    good = jc.reference(t, traj, jc.CONTINUOUS)
    assert np.array_equal(ref["turns"][0, 5:, 1], good["turns"][0, 5:, 1])      # the count goes on from row 3's


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_tile_moments_in_the_defined_order_stay_within_the_bounds(emu, n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 3, 5)) * 10.0 ** rng.integers(-2, 3, size=(1, 1, 5))
    x[:, 1, 2] = 1.0 + 1e-6 * rng.normal(size=n)      # |mean| >> spread
    if n > 2:
        x[n // 2, 2, 0], x[1, 2, 1] = np.nan, np.inf
    mean, M2 = jc.emu_series_moments(emu, x)
    rm, rq, Am, Aq = jc.series_moments(x)
    ec.assert_close(mean, rm, Am, "mean n %d" % n)
    ec.assert_close(M2, rq, Aq, "M2 n %d" % n)
    if n == 1:
        assert jc.same_bits(mean, x[0]) and (M2 == 0).all()
    if n > 2:
        assert np.isnan(mean[2, :2]).all() and np.isnan(M2[2, :2]).all() and np.isfinite(mean[2, 2:]).all()
