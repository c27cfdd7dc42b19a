"""CPU tests of the numpy restatement of the joint coordinates (tests/joints_common.py) against the CPU oracle: the raw coordinate is orc.minimal_coordinates
(oracle/cclqr_oracle.c joint_coordinate, the minimalCoordinates of pid.jl:43-57), the rate is the relative joint velocity of the oracle's friction law
(trackingLQR_triple_cartpole.jl:98-101): -uj of orc.control with fric = 1, no gains and no noise."""
import numpy as np
import pytest

import joints_common as jc


@pytest.fixture(scope="module")
def chain(cclqr):
    return jc.mixed_chain(cclqr, 7, seed=3)


def _poses(t, seed):
    traj, _ = jc.slab(t, 6, 5, seed=seed)
    return traj


def test_the_generated_chain_mixes_joint_types_with_offsets(chain):
    assert set(chain.type.tolist()) == {jc.REVOLUTE, jc.PRISMATIC}
    assert (np.abs(chain.qoff[:, 1:]).sum(axis=1) > 0.1).all() and (np.abs(chain.p1).sum(axis=1) > 0).all() and (np.abs(chain.p2).sum(axis=1) > 0).all()
    assert not np.allclose(np.linalg.norm(chain.axis, axis=1), 1.0)      # (the axis is normalised by the tables, not by the caller)


@pytest.mark.parametrize("seed", [0, 1])
def test_raw_coordinate_is_the_oracles_minimal_coordinate(orc, chain, seed):
    traj = _poses(chain, seed)
    ref = jc.reference(chain, traj, jc.RAW)
    jc.assert_generated(jc.reference(chain, traj, jc.CONTINUOUS))
    got = np.array([[orc.minimal_coordinates(chain, traj[i, k]) for k in range(traj.shape[1])] for i in range(traj.shape[0])])
    jc.assert_close(got, ref["theta"], ref["bound_theta"], "minimal_coordinates")
    f64 = jc.reference(chain, traj, jc.RAW, dtype=np.float64)
    jc.assert_close(f64["theta"], ref["theta"], ref["bound_theta"], "float64 definition")
    assert np.abs(got[..., chain.type == jc.REVOLUTE]).max() <= 2 * np.pi      # the raw angle lies in [-2 pi, 2 pi]


@pytest.mark.parametrize("seed", [0, 1])
def test_rate_is_the_oracles_relative_joint_velocity(orc, chain, seed):
    traj = _poses(chain, seed)
    ref = jc.reference(chain, traj, jc.RAW)
    ctrl = orc.ctrl_desc(chain.nb, [], fric=np.ones(chain.ne))
    got = np.array([[-orc.control(chain, ctrl, traj[i, k], 1) for k in range(traj.shape[1])] for i in range(traj.shape[0])])
    jc.assert_close(got, ref["rate"], ref["bound_rate"], "friction law")


def test_continuation_counts_turns_and_survives_a_quaternion_flip(chain):
    traj, angle = jc.slab(chain, 4, 12, seed=5)
    ref = jc.reference(chain, traj, jc.CONTINUOUS)
    jc.assert_generated(ref)
    rev = chain.type == jc.REVOLUTE
    # theta follows the generating angle up to the constant the tilt and the start's wrap add: its increments are the angle's
    d = np.diff(ref["theta"].astype(np.float64), axis=1)[..., rev] - np.diff(angle, axis=1)[..., rev]
    assert np.abs(d).max() < 1e-9
    assert np.abs(ref["turns"]).max() >= 2
    flipped = traj.copy()
    flipped[:, 5:, 2, 3:7] *= -1.0      # q -> -q of one body from row 5 on: the same rotations
    ref2 = jc.reference(chain, flipped, jc.CONTINUOUS)
    assert np.abs((ref2["theta"] - ref["theta"]).astype(np.float64)).max() < 1e-12
