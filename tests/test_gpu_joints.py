"""GPU tests of cclqr_rollout_joints (csrc/joints.hip) on synthetic slabs: the definition of tests/joints_common.py within its bounds on the four lane-group sizes,
exact bits where the definition is a copy, continuity over several turns with the carry, planted values that are not finite, trees / a permuted forest / the
closed-loop deltabot, per-instance plants, and the refusals."""
import numpy as np
import pytest

import joints_common as jc
import plants_common as pc
from conftest import long_and_short_chain_forest

pytestmark = pytest.mark.gpu

_MECH = {}


def _chain(cclqr, nb):
    if nb not in _MECH:
        t = jc.mixed_chain(cclqr, nb, seed=nb)
        _MECH[nb] = (cclqr._capi.MechHandle(t), t)
    return _MECH[nb]


@pytest.mark.parametrize("nb,n_inst", [(1, 257), (9, 65), (17, 3), (64, 1), (17, 65)])
def test_definition_on_every_lane_group_size(cclqr, nb, n_inst):
    """chains of 1, 9, 17, 64 bodies (lane groups of 8, 16, 32, 64) with prismatic and revolute joints; both modes, k0 = 1 and 4, rate_dev given and NULL"""
    mech, t = _chain(cclqr, nb)
    steps = 8 if nb < 64 else 5
    traj, _ = jc.slab(t, n_inst, steps, seed=nb + n_inst)
    jc.assert_generated(jc.reference(t, traj, jc.CONTINUOUS))
    for mode in (jc.RAW, jc.CONTINUOUS):
        ref = jc.reference(t, traj, mode)
        th, rt, cr = jc.gpu_joints(cclqr, mech, traj, mode)
        jc.assert_joints(th, rt, ref, "nb %d n %d mode %d" % (nb, n_inst, mode))
        if mode == jc.CONTINUOUS:
            assert np.array_equal(cr[..., 1], ref["carry"][..., 1])      # the turn counts, exactly
        th2, none, _ = jc.gpu_joints(cclqr, mech, traj, mode, rates=False)
        assert none is None and jc.same_bits(th, th2)
        # k0 = 4: rows 3 .. of a longer series are written, the others stay as they were; the continuous mode goes on from the carry of rows 0 .. 2
        head = jc.reference(t, traj[:, :3], mode)
        th4, rt4, cr4 = jc.gpu_joints(cclqr, mech, traj[:, 3:], mode, k0=4, out_steps=steps + 2, carry=head["carry"])
        assert np.isnan(th4[:, :3]).all() and np.isnan(th4[:, steps:]).all() and np.isnan(rt4[:, :3]).all() and np.isnan(rt4[:, steps:]).all()
        assert jc.same_bits(th4[:, 3:steps], th[:, 3:]) and jc.same_bits(rt4[:, 3:steps], rt[:, 3:])


def test_exact_bits_where_the_definition_is_a_copy(cclqr):
    """a prismatic joint off the origin along e_y with p1 = p2 = 0: theta = x_y and the rate = v_y of the slab; a revolute off the origin about e_x: the rate = w_x"""
    z = np.zeros(3)
    box = lambda: cclqr.Box(0.1, 0.1, 1.0, 1.0)
    o1, b1 = cclqr.Origin(), box()
    slider = cclqr.Mechanism(o1, [b1], [cclqr.EqualityConstraint(cclqr.Prismatic(o1, b1, np.array([0.0, 1.0, 0.0]), p1=z, p2=z))])
    o2, b2 = cclqr.Origin(), box()
    hinge = cclqr.Mechanism(o2, [b2], [cclqr.EqualityConstraint(cclqr.Revolute(o2, b2, np.array([1.0, 0.0, 0.0]), p1=z, p2=z))])
    rng = np.random.default_rng(0)
    traj = rng.normal(size=(5, 4, 1, 13))
    traj[..., 3:7] = np.array([1.0, 0, 0, 0])
    th, rt, _ = jc.gpu_joints(cclqr, cclqr._capi.MechHandle(slider.tables()), traj, jc.RAW)
    assert jc.same_bits(th[..., 0], traj[:, :, 0, 1]) and jc.same_bits(rt[..., 0], traj[:, :, 0, 8])
    traj[..., 3:7] = jc._unit(rng.normal(size=(5, 4, 1, 4)))
    th, rt, _ = jc.gpu_joints(cclqr, cclqr._capi.MechHandle(hinge.tables()), traj, jc.RAW)
    assert jc.same_bits(rt[..., 0], traj[:, :, 0, 10])


def test_continuity_through_three_turns_either_way_and_the_carry(cclqr):
    """one pendulum driven up three turns and down six in steps of up to 3 rad; chunk plans with the carry and a second call give the bits of the whole call"""
    t = cclqr.examples.pendulum()["mech"].tables()
    mech = cclqr._capi.MechHandle(t)
    steps = 23
    ang = np.concatenate([np.linspace(0, 6 * np.pi + 1.0, 8), np.linspace(6 * np.pi + 1.0, -6 * np.pi - 1.0, steps - 8)])
    assert np.abs(np.diff(ang)).max() <= 3.0 and 2.5 < np.abs(np.diff(ang)).max()
    tt = jc.Tables(t)
    traj = np.zeros((2, steps, 1, 13))
    traj[0, :, 0, 3:7] = jc._qmul(jc._axis_angle(tt.axis[0], ang), np.broadcast_to(tt.qoff[0], (steps, 4)))
    traj[1, :, 0, 3:7] = jc._qmul(jc._axis_angle(tt.axis[0], -ang[::-1] + 0.3), np.broadcast_to(tt.qoff[0], (steps, 4)))
    ref = jc.reference(t, traj, jc.CONTINUOUS)
    jc.assert_generated(ref)
    assert ref["turns"].max() >= 3 and ref["turns"].min() <= -3
    th, rt, cr = jc.gpu_joints(cclqr, mech, traj, jc.CONTINUOUS)
    jc.assert_joints(th, rt, ref, "pendulum")
    assert np.abs(th[0, :, 0] - ang).max() <= float(ref["bound_theta"].max()) + 1e-9      # the continuous angle follows the generating angle
    raw, _, _ = jc.gpu_joints(cclqr, mech, traj, jc.RAW)
    jc.assert_joints(raw, None, jc.reference(t, traj, jc.RAW), "raw")
    assert np.abs(raw).max() <= 2 * np.pi and np.abs(th).max() > 6 * np.pi
    for plan in ([1] * 23, [7, 7, 7, 2]):
        a, b, c = jc.gpu_joints_chunked(cclqr, mech, traj, jc.CONTINUOUS, plan)
        assert jc.same_bits(a, th) and jc.same_bits(b, rt) and jc.same_bits(c, cr), plan
    a, b, c = jc.gpu_joints(cclqr, mech, traj, jc.CONTINUOUS)
    assert jc.same_bits(a, th) and jc.same_bits(b, rt) and jc.same_bits(c, cr)


def test_values_that_are_not_finite_stay_where_they_enter(cclqr):
    mech, t = _chain(cclqr, 9)      # joints 0, 3, 6 prismatic, the others revolute
    traj, _ = jc.slab(t, 3, 10, seed=8, max_step=1.4)      # (two increments stay under 3 rad: the row after a gap decides as the definition does)
    bad = traj.copy()
    bad[0, 4, 1, 3:7] = np.nan      # an orientation: the angles of joints 1 (child) and 2 (parent); no rate reads it (joint 2 is a revolute)
    bad[1, 6, 2, 5] = np.inf        # ... of body 2: the angle of joint 2, and joint 3 (prismatic, parent 2) reads R_a for its coordinate and its rate
    bad[2, 2, 4, 11] = -np.inf      # an angular velocity of body 4: the rates of the revolutes 4 (child) and 5 (parent), no coordinate
    bad[2, 7, 5, 1] = np.nan        # a position of body 5: the coordinate of the prismatic joint 6 (parent 5) alone
    for mode in (jc.CONTINUOUS, jc.RAW):
        ref = jc.reference(t, bad, mode)
        th, rt, _ = jc.gpu_joints(cclqr, mech, bad, mode)
        jc.assert_joints(th, rt, ref, "planted mode %d" % mode)
        want_th, want_rt = np.zeros(th.shape, dtype=bool), np.zeros(th.shape, dtype=bool)
        want_th[0, 4, [1, 2]] = want_th[1, 6, [2, 3]] = want_th[2, 7, 6] = True
        want_rt[1, 6, 3] = want_rt[2, 2, [4, 5]] = True
        assert np.array_equal(np.isnan(th), want_th) and np.array_equal(np.isnan(rt), want_rt)
        assert not np.isinf(th).any() and not np.isinf(rt).any()
    good = jc.reference(t, traj, jc.CONTINUOUS)
    ref = jc.reference(t, bad, jc.CONTINUOUS)
    assert np.array_equal(ref["turns"][0, 5:, 1:3], good["turns"][0, 5:, 1:3])      # later rows go on from the last finite row's turn count


def test_other_topologies(cclqr, orc):
    """the permuted forest of two chains, the 14-body tree (also against the oracle's minimal coordinates) and the deltabot: 7 joints on 5 bodies, two per lane, a
    FixedOrientation constraint that gives 0"""
    forest = long_and_short_chain_forest(cclqr)[0]
    tree = pc.hanging_tree(cclqr, pc.TREE14).tables()
    rtree = cclqr.examples.tree_mechanism(pc.TREE14, seed=3, prismatic=(0, 5, 9))["mech"].tables()
    delta = cclqr.examples.deltabot()["mech"].tables()
    for seed, (name, t) in enumerate((("forest", forest), ("tree14", tree), ("random tree14", rtree), ("deltabot", delta))):
        mech = cclqr._capi.MechHandle(t)
        traj, _ = jc.slab(t, 5, 6, seed=40 + seed)
        for mode in (jc.RAW, jc.CONTINUOUS):
            ref = jc.reference(t, traj, mode)
            th, rt, _ = jc.gpu_joints(cclqr, mech, traj, mode)
            jc.assert_joints(th, rt, ref, "%s mode %d" % (name, mode))
        if name != "deltabot":
            jc.assert_generated(jc.reference(t, traj, jc.CONTINUOUS))
            raw = jc.reference(t, traj, jc.RAW)
            got = np.array([[orc.minimal_coordinates(t, traj[i, k]) for k in range(traj.shape[1])] for i in range(traj.shape[0])])
            jc.assert_close(got, raw["theta"], raw["bound_theta"], name + " oracle")
        else:
            fixed = np.asarray(t.type) == jc.FIXED
            assert t.ne == 7 and t.nb == 5 and fixed.sum() == 1
            assert (th[..., fixed] == 0).all() and (rt[..., fixed] == 0).all() and (th[..., ~fixed] != 0).all()


def test_per_instance_plants(cclqr):
    """a cart on a prismatic joint and prismatic links below it, every instance with its own p1, p2; first_instance != 0 picks the plant rows"""
    origin = cclqr.Origin()
    rng = np.random.default_rng(3)
    bodies, joints = [], []
    for i in range(4):
        b = cclqr.Box(0.1, 0.1, 0.5, 1.0)
        ax = rng.normal(size=3)
        kind = cclqr.Prismatic if i != 2 else cclqr.Revolute
        joints.append(cclqr.EqualityConstraint(kind(origin if i == 0 else bodies[-1], b, ax, p1=rng.normal(size=3) * 0.3, p2=rng.normal(size=3) * 0.3)))
        bodies.append(b)
    m = cclqr.Mechanism(origin, bodies, joints)
    n, first = 7, 5
    plants = cclqr.PlantBatch.scaled(m, 16, mass=(0.8, 1.2), length=(0.5, 1.5), seed=2, first_index=2)
    dev = cclqr._capi.MechHandle(m.tables())
    ph = plants.handle(dev)
    traj, _ = jc.slab(m.tables(), n, 5, seed=9)
    rows = list(plants.rows_for(first, n))
    p1, p2 = np.stack([plants.tables(i).p1 for i in rows]), np.stack([plants.tables(i).p2 for i in rows])
    assert np.abs(p1 - m.tables().p1).max() > 0.01
    for mode in (jc.RAW, jc.CONTINUOUS):
        ref = jc.reference(m.tables(), traj, mode, p1=p1, p2=p2)
        th, rt, _ = jc.gpu_joints(cclqr, dev, traj, mode, plants=ph, first_instance=first)
        jc.assert_joints(th, rt, ref, "plants mode %d" % mode)
    own = jc.reference(m.tables(), traj, jc.RAW)
    assert np.abs((ref["theta"] - own["theta"]).astype(np.float64)).max() > 1e-3      # the plants' vertices matter
    with pytest.raises(cclqr._capi.CclqrError, match="not all among the plants"):
        jc.gpu_joints(cclqr, dev, traj, jc.RAW, plants=ph, first_instance=12)
    other = cclqr._capi.MechHandle(m.tables())
    with pytest.raises(cclqr._capi.CclqrError, match="another mechanism"):
        jc.gpu_joints(cclqr, other, traj, jc.RAW, plants=ph, first_instance=first)


def test_refusals_name_their_cause_and_touch_nothing(cclqr):
    import torch
    capi = cclqr._capi
    mech, t = _chain(cclqr, 9)
    n, steps, ne = 3, 4, 9
    d = torch.from_numpy(jc.slab(t, n, steps, seed=1)[0]).cuda()
    th = torch.full((n, steps + 3, ne), float("nan"), dtype=torch.float64, device="cuda")
    rt, cr = torch.full_like(th, float("nan")), torch.full((n, ne, 2), float("nan"), dtype=torch.float64, device="cuda")
    ok = dict(n_inst=n, steps=steps, k0=1, traj_ptr=d.data_ptr(), mode=jc.CONTINUOUS, out_steps=steps + 3, theta_ptr=th.data_ptr(), rate_ptr=rt.data_ptr(), carry_ptr=cr.data_ptr())
    for change, cause in ((dict(n_inst=0), "n_inst >= 1"), (dict(steps=0), "steps >= 1"), (dict(k0=0), "k0 >= 1"), (dict(k0=5), "out_steps"), (dict(out_steps=3), "out_steps"),
                          (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(carry_ptr=0), "carry_dev"), (dict(traj_ptr=0), "null"), (dict(theta_ptr=0), "null")):
        with pytest.raises(capi.CclqrError, match=cause) as e:
            capi.rollout_joints(mech, **dict(ok, **change))
        assert e.value.code == capi.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(th).all() and torch.isnan(rt).all() and torch.isnan(cr).all()
    capi.rollout_joints(mech, **dict(ok, mode=jc.RAW, carry_ptr=0))      # mode 0 needs no carry
    torch.cuda.synchronize()
    assert torch.isfinite(th[:, :steps]).all() and torch.isnan(th[:, steps:]).all() and torch.isnan(cr).all()
