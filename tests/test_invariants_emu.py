"""CPU tests of the invariants pass's header functions (csrc/cclqr_invariants.h), run lane by lane on the host by tests/emu/emu_invariants.cpp with the butterflies
in the defined order, against the numpy restatement of the definition (tests/invariants_common.py): every lane-group size, the raw rows against the oracle's
orc.constraints on chains and on a branching tree and against oracle/loops.py on closed loops, per-instance plants, values that are not finite, chunk plans bit for
bit, and bits that do not depend on the lane-group width."""
import numpy as np
import pytest

import invariants_common as ic
import joints_common as jc


@pytest.fixture(scope="module")
def emu():
    return ic.emu_invariants()


@pytest.mark.parametrize("nb", [1, 8, 9, 17, 33])
def test_header_functions_are_the_definition(cclqr, orc, emu, nb):
    """chains with revolute and prismatic joints on lane groups of 8, 8 (full), 16, 32, 64 lanes; the raw rows also against orc.constraints"""
    t = jc.mixed_chain(cclqr, nb, seed=nb)
    traj = ic.slab(t, 3, 4, seed=nb)
    ref = ic.reference(t, traj)
    iv, rw, sm = ic.emu_run(emu, orc, t, traj)
    ic.assert_series(iv, ref, "nb %d" % nb)
    jc.assert_close(rw, ref["g"], ref["bound_g"], "nb %d rows" % nb)
    assert (ref["series"][..., 3:] > 1e-7).all()      # off the manifold, quaternions off unit length: nothing here is round-off (1e-16)
    got = np.array([[orc.constraints(t, traj[i, k]) for k in range(traj.shape[1])] for i in range(traj.shape[0])]).reshape(rw.shape)
    jc.assert_close(got, ref["g"], ref["bound_g"], "nb %d oracle" % nb)      # the independent restatement in C states the same rows
    assert ic.same_bits(sm, ic.summary_of(iv)) and ic.same_bits(sm, ic.emu_summary(emu, iv))


def test_raw_rows_on_a_branching_tree_are_the_oracles(cclqr, orc, emu):
    t = cclqr.examples.tree_mechanism((-1, 0, 0, 1, 1, 2, 5, 5, 3), seed=3, prismatic=(0, 4, 7))["mech"].tables()
    traj = ic.slab(t, 3, 3, seed=5)
    ref = ic.reference(t, traj)
    iv, rw, _ = ic.emu_run(emu, orc, t, traj)
    ic.assert_series(iv, ref, "tree")
    jc.assert_close(rw, ref["g"], ref["bound_g"], "tree rows")
    got = np.array([[orc.constraints(t, traj[i, k]) for k in range(traj.shape[1])] for i in range(traj.shape[0])]).reshape(rw.shape)
    jc.assert_close(got, ref["g"], ref["bound_g"], "tree oracle")


@pytest.mark.parametrize("name", ["fourbar", "deltabot"])
def test_closed_loops_against_the_loop_oracle(cclqr, orc, emu, name):
    """two joint slots per lane; a FixedOrientation constraint has its three rotational rows and no translational one, whatever the positions are"""
    from oracle import loops
    t = getattr(cclqr.examples, name)()["mech"].tables()
    tt = ic.Tables(t)
    assert t.ne > t.nb
    traj = ic.slab(t, 2, 3, seed=11)
    ref = ic.reference(t, traj)
    iv, rw, sm = ic.emu_run(emu, orc, t, traj)
    ic.assert_series(iv, ref, name)
    jc.assert_close(rw, ref["g"], ref["bound_g"], name + " rows")
    lm = loops.LoopMechanism(tt.mass, tt.inertia.reshape(-1, 3, 3), [loops.Joint(int(tt.type[j]), int(tt.parent[j]), int(tt.child[j]), np.asarray(t.axis).reshape(-1, 3)[j],
                                                                                 tt.p1[j], tt.p2[j], tt.qoff[j]) for j in range(t.ne)], dt=t.dt, g=t.g)
    for i in range(traj.shape[0]):
        for k in range(traj.shape[1]):
            for j, joint in enumerate(lm.joints):
                g = lm._blocks(joint, traj[i, k])[0]
                lo = 5 - len(g)      # (a FixedOrientation constraint: rows 2 .. 4)
                jc.assert_close(g, ref["g"][i, k, j, lo:], ref["bound_g"][i, k, j, lo:], "%s loop oracle joint %d" % (name, j))
                assert (rw[i, k, j, :lo] == 0).all()
    fixed = np.asarray(t.type) == ic.FIXED
    if fixed.any():
        bad = traj.copy()
        bad[0, 1, t.child[int(np.flatnonzero(fixed)[0])], 0] = np.nan      # a position the constraint does not read
        _, rw2, _ = ic.emu_run(emu, orc, t, bad)
        assert np.isfinite(rw2[0, 1, fixed]).all() and (rw2[0, 1, fixed, :2] == 0).all()


def test_per_instance_masses_inertias_and_vertices(cclqr, orc, emu):
    t = jc.mixed_chain(cclqr, 9, seed=4)
    n, first = 4, 3
    mass, inertia, p1, p2 = ic.random_plant_arrays(t, 8, seed=1)
    pb = cclqr.PlantBatch(t, mass=mass, inertia=inertia, p1=p1, p2=p2, first_index=1)
    rows = list(pb.rows_for(first, n))
    traj = ic.slab(t, n, 3, seed=6)
    ref = ic.reference(t, traj, mass=mass[rows], inertia=inertia[rows], p1=p1[rows], p2=p2[rows])
    iv, rw, _ = ic.emu_run(emu, orc, t, traj, records=pb.link_records(), plant_off=first - 1)
    ic.assert_series(iv, ref, "plants")
    jc.assert_close(rw, ref["g"], ref["bound_g"], "plants rows")
    own = ic.reference(t, traj)
    assert np.abs((own["series"] - ref["series"]).astype(np.float64))[..., :4].min() > 1e-6      # the plants' numbers matter to T, V, E and gap


def test_values_that_are_not_finite_stay_where_they_enter(cclqr, orc, emu):
    t = jc.mixed_chain(cclqr, 5, seed=7)
    traj = ic.slab(t, 3, 6, seed=8)
    bad = traj.copy()
    bad[0, 2, 1, :] = np.nan         # a whole body: T, V, E, quat and -- through joints 1 (child) and 2 (parent) -- gap and twist of that row
    bad[1, 4, 3, 8] = np.inf         # a velocity: T and E of that row, nothing else
    bad[2, 1, 2, 0] = -np.inf        # a position x: the translational rows of joints 2 and 3, so gap alone
    bad[2, 3, 4, 2] = np.nan         # a position z of the last body: V, E and gap
    bad[2, 5, 0, 4] = np.nan         # a quaternion entry: quat, gap (R_b p2, and R_a of joint 1) and twist
    ref = ic.reference(t, bad)
    iv, rw, sm = ic.emu_run(emu, orc, t, bad)
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
    good, _, _ = ic.emu_run(emu, orc, t, traj)
    assert ic.same_bits(iv[~want], good[~want])      # and nothing else moved


def test_an_instance_without_a_finite_row(cclqr, orc, emu):
    t = jc.mixed_chain(cclqr, 2, seed=1)
    traj = ic.slab(t, 2, 3, seed=2)
    traj[1] = np.nan
    iv, _, sm = ic.emu_run(emu, orc, t, traj)
    assert np.isnan(iv[1]).all() and np.isnan(sm[1, [0, 1, 2, 3, 5, 6]]).all() and sm[1, 4] == 0 and sm[1, 7] == 3
    assert np.isfinite(sm[0]).all() and sm[0, 7] == 0 and 1 <= sm[0, 4] <= 3


@pytest.mark.parametrize("plan", [[1] * 8, [3, 3, 2]])
def test_a_chunk_plan_gives_the_bits_of_one_pass(cclqr, orc, emu, plan):
    t = jc.mixed_chain(cclqr, 9, seed=1)
    traj = ic.slab(t, 4, 8, seed=6)
    traj[1, 0, 2, 7] = np.nan        # the first row's energy is not finite: E_first comes from row 2
    traj[2, 5, :, :] = np.inf
    whole_iv, whole_rw, whole_sm = ic.emu_run(emu, orc, t, traj)
    assert whole_sm[1, 7] == 1 and ic.same_bits(whole_sm[1, 0], whole_iv[1, 1, 2])
    iv, rw, sm, k0 = np.full_like(whole_iv, np.nan), np.full_like(whole_rw, np.nan), None, 1
    for s in plan:
        a, b, sm = ic.emu_run(emu, orc, t, traj[:, k0 - 1:k0 - 1 + s], k0=k0, out_steps=8, summary=sm)
        iv[:, k0 - 1:k0 - 1 + s], rw[:, k0 - 1:k0 - 1 + s] = a[:, k0 - 1:k0 - 1 + s], b[:, k0 - 1:k0 - 1 + s]
        assert (a[:, :k0 - 1] == -7.0).all() and (a[:, k0 - 1 + s:] == -7.0).all() and (b[:, :k0 - 1] == -7.0).all()      # only the launch's rows are written
        k0 += s
    assert ic.same_bits(iv, whole_iv) and ic.same_bits(rw, whole_rw) and ic.same_bits(sm, whole_sm)
    assert ic.same_bits(sm, ic.summary_of(whole_iv))


def test_bits_do_not_depend_on_the_lane_group_width(cclqr, orc, emu):
    """the same 5-body mechanism on 8 and on 64 lanes: the padding zeros add exactly, so the sums depend on the link order alone"""
    t = jc.mixed_chain(cclqr, 5, seed=9)
    traj = ic.slab(t, 3, 5, seed=10)
    a = ic.emu_run(emu, orc, t, traj, lanes=8)
    b = ic.emu_run(emu, orc, t, traj, lanes=64)
    c = ic.emu_run(emu, orc, t, traj, lanes=16)
    for x, y, z in zip(a, b, c):
        assert ic.same_bits(x, y) and ic.same_bits(x, z)


def test_launch_arithmetic(emu):
    import ctypes as C
    emu.emu_invariants_lds.restype = C.c_longlong
    for nb, per_wave in ((1, 8), (8, 8), (9, 4), (17, 2), (33, 1), (64, 1)):
        assert emu.emu_invariants_lds(nb) == 8 * 4 * per_wave * ((13 * nb) | 1) <= 64 * 1024
