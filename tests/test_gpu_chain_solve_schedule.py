"""The chain kernel's block-tridiagonal solve after its LDS reads were changed (cclqr_chain.h): ck_tri_mid reads the middle block AND the scratch block
unconditionally and selects afterwards (so the scratch words are read by plans that do not merge, too), ck_tri_back and the chain kernel's gk_t_apply read
single words; the 8-lane kernel, whose one front never merges, reads no scratch word (a compile-time switch of ck_tri_mid).  The arithmetic is unchanged; one case for each plan of the solve the edits touch: hanging chains under their LQR as
test_gpu_chain_newton_fold.py builds them, 3 instances, 30 steps.  Packed and spread launches agree bit for bit (status included), both agree with the
oracle within that file's 1e-9 (fp64, over the trajectory)."""
import numpy as np
import pytest
import scipy.linalg as sl

from conftest import hanging_setpoint

TOL = 1e-9
STEPS = 30
NINST = 3

# bodies, lanes per instance, links of the LDS layout, reduction level, links the two-front sweep runs over, fronts, merge
PLANS = [
    (4, 8, 4, False, 4, 1, 0),        # one front
    (7, 16, 8, False, 7, 2, 1),       # two fronts, balanced: front 1 folds into the scratch block
    (8, 16, 8, False, 8, 2, 0),       # two fronts, the scratch block is read and selected away
    (11, 32, 16, False, 11, 2, 1),    # below CR_MIN_LINKS: no reduction level
    (12, 32, 16, True, 6, 2, 0),      # reduction level, sweep over every second link
    (13, 32, 16, True, 7, 2, 1),
    (17, 32, 17, True, 9, 2, 1),      # the headline layout
    (18, 32, 32, False, 18, 2, 0),    # the 32-link layout has no reduction level
]


def _plan_of(nb, lanes, layout):
    """a Python re-statement of the plan rule of rollout_chain.hip and tri_plan_balanced (cclqr_chain.h); the library does not export the plan, so
    the reduction-level, sweep, fronts and merge columns of the table say what each case is FOR and are not checked against the kernel -- lanes and
    layout links are (mech.geometry(), mech.layout_links() in test_solve_plan)"""
    cr = lanes == 32 and layout <= 17 and nb >= 12
    swept = (nb + 1) // 2 if cr else nb
    fronts = 2 if lanes >= 16 else 1
    rest = swept - 1
    merge = 1 if (fronts == 2 and rest > 0 and rest % 2 == 0) else 0
    return cr, swept, fronts, merge


@pytest.mark.parametrize("nb,lanes,layout,cr,swept,fronts,merge", PLANS)
def test_case_table_names_the_plans(nb, lanes, layout, cr, swept, fronts, merge):
    """(CPU) the table above is consistent with _plan_of: no row claims a plan the rule would not give its size"""
    assert _plan_of(nb, lanes, layout) == (cr, swept, fronts, merge)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,lanes,layout,cr,swept,fronts,merge", PLANS)
def test_solve_plan(cclqr, orc, nb, lanes, layout, cr, swept, fronts, merge):
    capi = cclqr._capi
    n_links = nb - 1
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    assert t.nb == nb
    zd = hanging_setpoint(cclqr, n_links)
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt, STEPS + 50)
    rng = np.random.default_rng(100 + nb)
    phi = rng.uniform(-0.3, 0.3, (NINST, n_links))
    phi[:, 0] += np.pi
    z0 = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, NINST), phi)
    zT_o, traj_o, st_o = orc.rollout(t, orc.ctrl_desc(t.nb, [0], K=K, N=STEPS + 50, zd=zd), z0, STEPS, record=True)

    mech = capi.MechHandle(t)
    assert mech.geometry()[0] == lanes and mech.layout_links() == layout
    ctrl = capi.CtrlHandle(mech, [0], K=K, N=STEPS + 50, zd=zd)
    # spread: every instance alone in its wavefront; packed: 3 in one wavefront (8 and 16 lanes), 2 + 1 (32 lanes)
    assert mech.instances_per_wavefront(NINST, STEPS) == 1
    assert mech.instances_per_wavefront(NINST, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS) == 64 // lanes
    spread = capi.rollout(mech, ctrl, z0, STEPS, record=True)
    packed = capi.rollout(mech, ctrl, z0, STEPS, record=True, flags=capi.ROLLOUT_PACK_WAVEFRONTS)
    for x, y in zip(spread, packed):
        assert np.array_equal(x, y)
    err_traj = max(np.abs(spread[1] - traj_o).max(), np.abs(packed[1] - traj_o).max())
    err_final = max(np.abs(spread[0] - zT_o).max(), np.abs(packed[0] - zT_o).max())
    print("%d bodies: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, Newton iterations %s (oracle %s)" % (nb, err_traj, err_final, packed[2], st_o))
    assert (st_o > 0).all() and (packed[2] > 0).all() and (spread[2] > 0).all()
    assert err_traj < TOL and err_final < TOL
