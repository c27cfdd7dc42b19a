"""Shared by tests/test_plants_host.py and tests/test_gpu_plants.py: the mechanisms, plant sets and starts of the per-instance-plant tests."""
import ctypes as C
import os

import numpy as np

from build_common import host_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TREE14 = [-1, 0, 1, 2, 3, 2, 5, 6, 1, 8, 8, 10, 0, 12]
TREE5 = [-1, 0, 1, 1, 2]          # body 1 carries two child joints


def hanging_tree(cclqr, parents):
    """a cart on a prismatic joint along y (body 0) and pendulum links Box(0.1, 0.1, 1, 1) on revolutes about x, every link hanging below its parent
    (the vertices of the triple cartpole: p1 = -[0, 0, 0.5] on a parent link -- 0 on the cart --, p2 = +[0, 0, 0.5]).  All joint coordinates zero is the
    hanging equilibrium, a stable one whatever the masses and lengths."""
    ex_, ey, h = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 0.5])
    origin = cclqr.Origin()
    bodies, joints = [cclqr.Box(0.1, 0.5, 0.1, 0.5)], []
    joints.append(cclqr.EqualityConstraint(cclqr.Prismatic(origin, bodies[0], ey)))
    assert parents[0] == -1
    for i in range(1, len(parents)):
        b = cclqr.Box(0.1, 0.1, 1.0, 1.0)
        bodies.append(b)
        a = parents[i]
        joints.append(cclqr.EqualityConstraint(cclqr.Revolute(bodies[a], b, ex_, p1=(0 * h if a == 0 else -h), p2=h)))
    return cclqr.Mechanism(origin, bodies, joints, g=-9.81)


def mechanism_of(cclqr, case):
    """case: ("chain", pendulum links) -> the n-link cartpole (examples/lqr_cartpole_n_pendulum.jl), hanging at joint angle pi; ("tree", parents) -> hanging_tree.
    Returns (mechanism, hanging joint coordinates [ne])"""
    kind, arg = case
    if kind == "chain":
        mech = cclqr.examples.cartpole_n(arg)["mech"]
        th = np.zeros(arg + 1)
        th[1] = np.pi
        return mech, th
    mech = hanging_tree(cclqr, arg)
    return mech, np.zeros(len(arg))


def random_plants(cclqr, mech, n, seed, first_index=0):
    """masses and inertias x U(0.7, 1.3) per body, p1 and p2 x U(0.9, 1.1) per joint"""
    return cclqr.PlantBatch.scaled(mech, n, mass=(0.7, 1.3), length=(0.9, 1.1), seed=seed, first_index=first_index)


def starts(cclqr, mech, th0, n, seed, plants=None, first_instance=0):
    """n starts near the hanging pose (cart within +-0.3, joint angles within +-0.25), placed on each instance's own plant"""
    rng = np.random.default_rng(seed)
    th = th0[None] + rng.uniform(-1, 1, (n, len(th0))) * ([0.3] + [0.25] * (len(th0) - 1))
    return cclqr.joint_position_states(mech, th, plants=plants, first_instance=first_instance), th


def patched_copy(mech, tables):
    """a deep copy of the mechanism with the masses, inertias and joint vertices of `tables`"""
    import copy
    handle = mech.__dict__.pop("_cclqr_handle", None)      # (a device handle is not copied)
    try:
        m2 = copy.deepcopy(mech)
    finally:
        if handle is not None:
            mech._cclqr_handle = handle
    for b, m, J in zip(m2.bodies, tables.mass, tables.inertia):
        b.m, b.J = float(m), np.array(J).reshape(3, 3)
    for e, p1, p2 in zip(m2.eqconstraints, tables.p1, tables.p2):
        e.joint.p1, e.joint.p2 = np.array(p1), np.array(p2)
    return m2


def emu_plants():
    """tests/emu/emu_plants.cpp, compiled for the host the way conftest.emu compiles the other emulation sources"""
    return host_library("libemu_plants.so", ["emu/emu_plants.cpp"])
