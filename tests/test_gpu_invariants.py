"""GPU tests of cclqr_rollout_invariants (csrc/invariants.hip) on synthetic slabs off the manifold: the definition of tests/invariants_common.py within its bounds
on every lane-group size with partly empty last groups and sentinel-filled buffers, each output NULL in turn, chunk plans with the summary carried, closed loops
(two joint slots per lane) and a branching tree, per-instance plants with first_instance != 0, planted values that are not finite, a second launch, and the
refusals."""
import numpy as np
import pytest

import invariants_common as ic
import joints_common as jc

pytestmark = pytest.mark.gpu

_MECH = {}
FILL = -7.0


def _chain(cclqr, nb):
    if nb not in _MECH:
        t = jc.mixed_chain(cclqr, nb, seed=nb)
        _MECH[nb] = (cclqr._capi.MechHandle(t), t)
    return _MECH[nb]


def _whole_groups_plus_one(nb):
    """one instance more than a whole number of workgroups: four wavefronts of 64 / G instances each"""
    G = 8 if nb <= 8 else 16 if nb <= 16 else 32 if nb <= 32 else 64
    return 2 * 4 * (64 // G) + 1


@pytest.mark.parametrize("nb", [1, 8, 9, 17, 33])
def test_definition_on_every_lane_group_size(cclqr, nb):
    """chains of 1, 8, 9, 17, 33 bodies (lane groups of 8, 8, 16, 32, 64) with prismatic and revolute joints, 6 rows, n_inst = 1, 5 and one more than two workgroups
    hold: the last lane group is partly empty and nothing beyond n_inst is written (the buffers hold n_inst instances exactly, a sentinel row on either side of
    the launch's rows)"""
    mech, t = _chain(cclqr, nb)
    steps = 6
    for n_inst in (1, 5, _whole_groups_plus_one(nb)):
        traj = ic.slab(t, n_inst, steps, seed=nb + n_inst)
        ref = ic.reference(t, traj)
        iv, rw, sm = ic.gpu_invariants(cclqr, mech, traj, k0=2, out_steps=steps + 2)
        what = "nb %d n %d" % (nb, n_inst)
        assert (iv[:, 0] == FILL).all() and (iv[:, -1] == FILL).all() and (rw[:, 0] == FILL).all() and (rw[:, -1] == FILL).all(), what
        ic.assert_series(iv[:, 1:-1], ref, what)
        jc.assert_close(rw[:, 1:-1], ref["g"], ref["bound_g"], what + " rows")
        # k0 = 2 and a summary full of the sentinel going in: the launch merges into what it reads (here: the sentinel, which is finite)
        assert ic.same_bits(sm, ic.summary_of(iv[:, 1:-1], k0=2, carry=np.full((n_inst, 8), FILL))), what
        # each output NULL in turn: the others keep their bits
        full = ic.gpu_invariants(cclqr, mech, traj)
        assert ic.same_bits(full[0], iv[:, 1:-1]) and ic.same_bits(full[1], rw[:, 1:-1]) and ic.same_bits(full[2], ic.summary_of(full[0])), what
        for drop in range(3):
            want = tuple(i != drop for i in range(3))
            got = ic.gpu_invariants(cclqr, mech, traj, want=want)
            for i in range(3):
                assert (got[i] is None) == (i == drop) and (i == drop or ic.same_bits(got[i], full[i])), (what, drop, i)


@pytest.mark.parametrize("plan", [[1] * 8, [3, 3, 2]])
def test_a_chunk_plan_with_the_summary_carried_gives_the_bits_of_one_launch(cclqr, plan):
    mech, t = _chain(cclqr, 9)
    traj = ic.slab(t, 9, 8, seed=6)
    traj[1, 0, 2, 7] = np.nan        # the first row's energy is not finite: E_first comes from row 2, whichever launch holds it
    traj[2, 5, :, :] = np.inf
    whole = ic.gpu_invariants(cclqr, mech, traj)
    assert whole[2][1, 7] == 1 and ic.same_bits(whole[2][1, 0], whole[0][1, 1, 2]) and whole[2][2, 7] == 1
    parts = ic.gpu_invariants_chunked(cclqr, mech, traj, plan)
    for a, b in zip(parts, whole):
        assert ic.same_bits(a, b)
    assert ic.same_bits(whole[2], ic.summary_of(whole[0]))


@pytest.mark.parametrize("name", ["fourbar", "deltabot", "tree"])
def test_closed_loops_and_a_branching_tree(cclqr, name):
    """fourbar and deltabot: more joints than bodies, two joint slots per lane, the deltabot's FixedOrientation constraint with rotational rows only; a branching
    9-body tree with prismatic joints through the tree tables"""
    if name == "tree":
        t = cclqr.examples.tree_mechanism((-1, 0, 0, 1, 1, 2, 5, 5, 3), seed=3, prismatic=(0, 4, 7))["mech"].tables()
    else:
        t = getattr(cclqr.examples, name)()["mech"].tables()
    mech = cclqr._capi.MechHandle(t)
    traj = ic.slab(t, 9, 4, seed=11)
    ref = ic.reference(t, traj)
    iv, rw, sm = ic.gpu_invariants(cclqr, mech, traj)
    ic.assert_series(iv, ref, name)
    jc.assert_close(rw, ref["g"], ref["bound_g"], name + " rows")
    assert ic.same_bits(sm, ic.summary_of(iv))
    fixed = np.asarray(t.type) == ic.FIXED
    assert fixed.any() == (name == "deltabot")
    if fixed.any():
        assert (rw[:, :, fixed, :2] == 0).all() and (rw[:, :, fixed, 2:] != 0).all()


def test_plants_with_a_first_instance(cclqr):
    """per-instance masses, inertias and vertices: instance i reads plant first_instance + i of a table that starts at plant 2"""
    mech, t = _chain(cclqr, 9)
    n, first = 7, 5
    mass, inertia, p1, p2 = ic.random_plant_arrays(t, 16, seed=1)
    plants = cclqr.PlantBatch(t, mass=mass, inertia=inertia, p1=p1, p2=p2, first_index=2)
    ph = plants.handle(mech)
    rows = list(plants.rows_for(first, n))
    assert rows[0] == 3
    traj = ic.slab(t, n, 5, seed=9)
    ref = ic.reference(t, traj, mass=mass[rows], inertia=inertia[rows], p1=p1[rows], p2=p2[rows])
    iv, rw, sm = ic.gpu_invariants(cclqr, mech, traj, plants=ph, first_instance=first)
    ic.assert_series(iv, ref, "plants")
    jc.assert_close(rw, ref["g"], ref["bound_g"], "plants rows")
    off = ic.reference(t, traj, mass=mass[:n], inertia=inertia[:n], p1=p1[:n], p2=p2[:n])      # what reading plant i instead of first + i would give
    assert np.abs((off["series"] - ref["series"]).astype(np.float64))[..., :4].min() > 1e-6
    with pytest.raises(cclqr._capi.CclqrError, match="not all among the plants"):
        ic.gpu_invariants(cclqr, mech, traj, plants=ph, first_instance=12)
    other = cclqr._capi.MechHandle(t)
    with pytest.raises(cclqr._capi.CclqrError, match="another mechanism"):
        ic.gpu_invariants(cclqr, other, traj, plants=ph, first_instance=first)


def test_values_that_are_not_finite_stay_where_they_enter(cclqr):
    t = jc.mixed_chain(cclqr, 5, seed=7)      # joints 0 and 3 prismatic, the others revolute
    mech = cclqr._capi.MechHandle(t)
    traj = ic.slab(t, 3, 6, seed=8)
    bad = traj.copy()
    bad[0, 2, 1, :] = np.nan         # a whole body: T, V, E, quat and -- through joints 1 (child) and 2 (parent) -- gap and twist of that row
    bad[1, 4, 3, 8] = np.inf         # a velocity: T and E of that row, nothing else
    bad[2, 1, 2, 0] = -np.inf        # a position x: the translational rows of joints 2 and 3, so gap alone
    bad[2, 3, 4, 2] = np.nan         # a position z of the last body: V, E and gap
    bad[2, 5, 0, 4] = np.nan         # a quaternion entry: quat, gap (R_b p2, and R_a of joint 1) and twist
    ref = ic.reference(t, bad)
    iv, rw, sm = ic.gpu_invariants(cclqr, mech, bad)
    ic.assert_series(iv, ref, "planted")
    jc.assert_close(rw, ref["g"], ref["bound_g"], "planted rows")
    want = np.zeros(iv.shape, dtype=bool)
    want[0, 2, :] = True
    want[1, 4, [0, 2]] = True
    want[2, 1, 3] = True
    want[2, 3, [1, 2, 3]] = True
    want[2, 5, [3, 4, 5]] = True
    assert np.array_equal(np.isnan(iv), want)
    assert not np.isinf(iv).any() and not np.isinf(rw).any() and not np.isinf(sm).any()
    assert np.array_equal(sm[:, 7], [1, 1, 3])      # bad_rows, exactly
    assert ic.same_bits(sm, ic.summary_of(iv))
    good, _, _ = ic.gpu_invariants(cclqr, mech, traj)
    assert ic.same_bits(iv[~want], good[~want])      # and nothing else moved
    # a second launch gives the same bits
    again = ic.gpu_invariants(cclqr, mech, bad)
    assert ic.same_bits(again[0], iv) and ic.same_bits(again[1], rw) and ic.same_bits(again[2], sm)


def test_refusals_name_their_cause_and_touch_nothing(cclqr):
    import torch
    capi = cclqr._capi
    mech, t = _chain(cclqr, 9)
    n, steps, ne = 3, 4, 9
    d = torch.from_numpy(ic.slab(t, n, steps, seed=1)).cuda()
    full = lambda *shape: torch.full(shape, FILL, dtype=torch.float64, device="cuda")
    iv, rw, sm = full(n, steps + 3, 6), full(n, steps + 3, ne, 5), full(n, 8)
    ok = dict(n_inst=n, steps=steps, k0=1, traj_ptr=d.data_ptr(), out_steps=steps + 3, inv_ptr=iv.data_ptr(), rows_ptr=rw.data_ptr(), summary_ptr=sm.data_ptr())
    for change, cause in ((dict(n_inst=0), "n_inst >= 1"), (dict(steps=0), "steps >= 1"), (dict(k0=0), "k0 >= 1"), (dict(k0=5), "out_steps"), (dict(out_steps=3), "out_steps"),
                          (dict(out_steps=3, inv_ptr=0), "out_steps"), (dict(out_steps=3, rows_ptr=0), "out_steps"), (dict(traj_ptr=0), "null traj_dev"),
                          (dict(inv_ptr=0, rows_ptr=0, summary_ptr=0), "all NULL"), (dict(first_instance=-1), "first_instance")):
        with pytest.raises(capi.CclqrError, match=cause) as e:
            capi.rollout_invariants(mech, **dict(ok, **change))
        assert e.value.code == capi.EINVAL
    mass = np.tile(np.asarray(t.mass)[None], (4, 1))
    ph = cclqr.PlantBatch(t, mass=mass, first_index=2).handle(mech)
    for change, cause in ((dict(first_instance=0), "not all among the plants"), (dict(first_instance=4), "not all among the plants")):
        with pytest.raises(capi.CclqrError, match=cause) as e:
            capi.rollout_invariants(mech, plants=ph, **dict(ok, **change))
        assert e.value.code == capi.EINVAL
    with pytest.raises(capi.CclqrError, match="another mechanism") as e:
        capi.rollout_invariants(_chain(cclqr, 8)[0], plants=ph, **ok)
    assert e.value.code == capi.EINVAL
    loop = capi.MechHandle(cclqr.examples.fourbar()["mech"].tables())
    with pytest.raises(capi.CclqrError, match="another mechanism"):
        capi.rollout_invariants(loop, plants=ph, **ok)
    torch.cuda.synchronize()
    assert (iv == FILL).all() and (rw == FILL).all() and (sm == FILL).all()
    capi.rollout_invariants(mech, **dict(ok, out_steps=0, inv_ptr=0, rows_ptr=0))      # the summary alone needs no out_steps
    torch.cuda.synchronize()
    assert (iv == FILL).all() and (rw == FILL).all() and torch.isfinite(sm).all() and (sm[:, 7] == 0).all() and (sm[:, 4] >= 1).all()
