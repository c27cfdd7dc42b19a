"""The chain kernels that split the Schur rows and the tree kernel form a full-step trial's ||f|| in front of the row block and build the rows only when
some instance of the wavefront will read them (cclqr_chain.h chain_rows_verdict): not for a trial that ends its instance's solve, not for a full step that
is rejected.  What can go wrong on the device and shows as wrong numbers: a vote that is not wavefront-wide (an instance reads rows its partner's verdict
dropped), a helper lane voting by another norm than its link's lane, a group without an instance voting at all, rows left over in LDS from an earlier launch
read in place of skipped ones.  So, on every kind of kernel the rule runs in:

  chains of 9, 16 and 17 bodies      16-link image with idle lanes / every lane a link or a helper / 17-link image (lane 16 owns the leaf)
  forest 9 + 8                       two chains in a 17-link group
  the 14-body tree, a 4-body tree    32 lanes, two instances per wavefront / 16 lanes, four
  17 bodies, setpoint + far start    one instance is done after its first iteration while its partner in the wavefront goes on solving

Chains with 6 and 3 instances, trees with 2 and 3 (a full wavefront and a half-empty one).  Each case: trajectory, final state, multipliers and status
bitwise equal between the packed and the spread launch, between one launch and carried single-step launches, and between clean LDS and LDS poisoned
with signalling NaNs; trajectory and final state within the suite's 1e-9 of the oracle, which runs once per problem.  None of this can see a wrongly
SKIPPED build whose stale rows still let Newton converge to the same tolerance: tests/test_chain_rows_verdict_emu.py is the check for that."""
import numpy as np
import pytest

from conftest import hanging_setpoint
from test_gpu_chain_schur_split import NINST, STEPS, TOL, _chain_problem, _forest_problem, _launcher, _reference, poison  # noqa: F401 (poison: a fixture)
from test_gpu_treereg import _starts
from test_tree import build

pytestmark = pytest.mark.gpu


def _tree_problem(cclqr, name):
    ex = build(cclqr, name)
    t = ex["mech"].tables()
    rng = np.random.default_rng(900 + t.nb)
    z0 = _starts(cclqr, ex, rng, 3)
    cj = [0, t.ne - 1]
    K = rng.normal(size=(STEPS + 2, len(cj), 12 * t.nb)) * 0.05
    return t, cj, K, STEPS + 3, z0[0], z0


def _setpoint_and_far_problem(cclqr, orc):
    """17 bodies under their hanging LQR: instance 0 starts AT the setpoint (nothing to solve: done with its first trial, every step), instance 1 far
    from it (the longest solves of this file)"""
    t, cj, K, N, zd, z0 = _chain_problem(cclqr, orc, 17)
    rng = np.random.default_rng(77)
    phi = rng.uniform(-0.6, 0.6, (1, 16))
    phi[:, 0] += np.pi
    far = cclqr.examples.cartpole_states(16, [0.5], phi)
    return t, cj, K, N, zd, np.concatenate([zd[None], far])


def _check(cclqr, orc, poison, key, make, lanes, n):
    capi = cclqr._capi
    (t, cj, K, N, zd, z0), (zT_o, traj_o, st_o) = _reference(orc, key, make)
    mech, run = _launcher(cclqr, t, cj, K, N, zd, np.array(z0[:n]))
    assert mech.geometry()[0] == lanes
    assert mech.instances_per_wavefront(n, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS) == 64 // lanes
    spread = run(STEPS)
    packed = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    single = run(1, capi.ROLLOUT_PACK_WAVEFRONTS)
    dirty = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS, poison)
    for name, x, y, w, v in zip(("final state", "trajectory", "multipliers", "status"), spread, packed, single, dirty):
        assert np.array_equal(x, y), "packed / spread: " + name
        assert np.array_equal(y, w), "one launch / single steps: " + name
        assert y.tobytes() == v.tobytes(), "clean / poisoned LDS: " + name
    err_traj, err_final = np.abs(packed[1] - traj_o[:n]).max(), np.abs(packed[0] - zT_o[:n]).max()
    print("%s, %d instances: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, Newton iterations %s" % (key, n, err_traj, err_final, packed[3]))
    assert (packed[3] > 0).all() and (spread[3] > 0).all() and (single[3] > 0).all()
    assert err_traj < TOL and err_final < TOL
    return packed


@pytest.mark.parametrize("n", [NINST, 3])
@pytest.mark.parametrize("nb", [9, 16, 17])
def test_chain(cclqr, orc, poison, nb, n):
    _check(cclqr, orc, poison, "%d bodies" % nb, lambda: _chain_problem(cclqr, orc, nb), 32, n)


@pytest.mark.parametrize("n", [NINST, 3])
def test_forest_in_a_17_link_group(cclqr, orc, poison, n):
    _check(cclqr, orc, poison, "forest 9 + 8", lambda: _forest_problem(cclqr, (9, 8)), 32, n)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,lanes", [("deep", 32), ("small4", 16)])
def test_tree(cclqr, orc, poison, name, lanes, n):
    _check(cclqr, orc, poison, "tree " + name, lambda: _tree_problem(cclqr, name), lanes, n)


def test_one_instance_finishes_while_its_partner_goes_on(cclqr, orc, poison):
    packed = _check(cclqr, orc, poison, "17 bodies, setpoint + far", lambda: _setpoint_and_far_problem(cclqr, orc), 32, 2)
    assert 0 < packed[3][0] < packed[3][1], packed[3]       # the largest Newton count of a step: the two instances of the wavefront did solve differently
