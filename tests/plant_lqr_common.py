"""Shared by tests/test_plant_lqr_host.py and tests/test_gpu_plant_lqr.py: the mechanisms, plants, setpoints and oracle references of the
one-LQR-per-plant tests (cclqr_linearize_plants, cclqr_ctrl_create_lqr_batch_plants, PlantLQR).  Every case and every reference is built once per session."""
import ctypes as C
import json
import os

import numpy as np

from build_common import host_library
from plants_common import ROOT, TREE5, mechanism_of, random_plants

N_PLANTS, HORIZON = 6, 40          # plants per case, knots N of the recursion (N - 1 = 39 recorded steps)
SLIDER_P1, SLIDER_P2 = np.array([0.05, 0.0, -0.3]), np.array([0.0, 0.02, 0.0])
CASES = ("chain2", "chain-slider", "tree-slider", "sawyer")
SLIDERS = ("chain-slider", "tree-slider")


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def slider_mechanism(cclqr, parents):
    """plants_common.hanging_tree(parents) plus a slider Box(0.2, 0.1, 0.1, 0.4) on body 1, on Prismatic(link, slider, ex; p1, p2) with p1 != 0: a controlled
    prismatic joint whose parent is a body -- the only configuration in which the linearisation reads a CHILD joint's vertex p1 (the force of the joint input on
    the parent body, and the parent-side Bu column).  Returns (mechanism, joint index of the slider)"""
    ex_, ey, h = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 0.5])
    origin = cclqr.Origin()
    bodies, joints = [cclqr.Box(0.1, 0.5, 0.1, 0.5)], []
    joints.append(cclqr.EqualityConstraint(cclqr.Prismatic(origin, bodies[0], ey)))
    for i in range(1, len(parents)):
        b = cclqr.Box(0.1, 0.1, 1.0, 1.0)
        bodies.append(b)
        a = parents[i]
        joints.append(cclqr.EqualityConstraint(cclqr.Revolute(bodies[a], b, ex_, p1=(0 * h if a == 0 else -h), p2=h)))
    slider = cclqr.Box(0.2, 0.1, 0.1, 0.4)
    bodies.append(slider)
    joints.append(cclqr.EqualityConstraint(cclqr.Prismatic(bodies[1], slider, ex_, p1=SLIDER_P1, p2=SLIDER_P2)))
    return cclqr.Mechanism(origin, bodies, joints, g=-9.81), len(joints) - 1


_cases = {}


def case(cclqr, name):
    """dict(mech, t, th0, cj, slider, plants, n, N, zd [n][nb][13], Fd [n][mu], Q, R): the mechanism at its hanging pose (the Sawyer arm: one random pose within
    +-0.8 rad per plant, g = 0) with every plant's setpoint on that plant's own constraint manifold, Q = 10 dt I, R = 0.1 dt I, zero holding inputs"""
    if name in _cases:
        return _cases[name]
    slider = None
    if name == "chain2":
        mech, th0 = mechanism_of(cclqr, ("chain", 2))
        cj = [0]
    elif name == "chain-slider":
        mech, slider = slider_mechanism(cclqr, [-1, 0])
        th0, cj = np.zeros(3), [0, 2]
    elif name == "tree-slider":
        mech, slider = slider_mechanism(cclqr, TREE5)
        th0, cj = np.zeros(6), [0, 5]
    else:
        tab = json.load(open(os.path.join(ROOT, "tests", "golden", "sawyer_arm_tables.json")))
        mech = cclqr.examples.sawyer(tab)["mech"]
        th0, cj = None, list(range(7))
    t = mech.tables()
    n, N = (4, 12) if name == "sawyer" else (N_PLANTS, HORIZON)
    plants = random_plants(cclqr, mech, n, seed=3)
    th = np.random.default_rng(47).uniform(-0.8, 0.8, (n, 7)) if th0 is None else np.tile(th0, (n, 1))
    c = dict(name=name, mech=mech, t=t, th0=th0, th=th, cj=cj, slider=slider, plants=plants, n=n, N=N, zd=cclqr.joint_position_states(mech, th, plants=plants),
             zd_nominal=cclqr.joint_position_states(mech, th[:1])[0], Fd=np.zeros((n, len(cj))), Q=np.eye(12 * t.nb) * 10.0 * t.dt, R=np.eye(len(cj)) * 0.1 * t.dt)
    _cases[name] = c
    return c


_refs = {}


def oracle_models(orc, c):
    """the oracle's linear model of every plant at its setpoint, [(A, Bu, Bl, G)] * n, and of the mechanism's own plant at its own setpoint"""
    key = ("lin", c["name"])
    if key not in _refs:
        _refs[key] = ([orc.linearize(c["plants"].tables(i), c["zd"][i], c["cj"], c["Fd"][i]) for i in range(c["n"])],
                      orc.linearize(c["t"], c["zd_nominal"], c["cj"], c["Fd"][0]))
    return _refs[key]


def oracle_gains(orc, c):
    """the oracle's dlqr on oracle_models: ([K_i [N-1][mu][mx]], [kbreak_i]) per plant and (K, kbreak) of the mechanism's own plant"""
    key = ("ric", c["name"])
    if key not in _refs:
        per, nom = oracle_models(orc, c)
        got = [orc.riccati(*m, c["Q"], c["R"], c["N"]) for m in per]
        _refs[key] = ([g[0] for g in got], [int(g[1]) for g in got], orc.riccati(*nom, c["Q"], c["R"], c["N"]))
    return _refs[key]


def emu_lin_plants():
    """tests/emu/emu_lin_plants.cpp, compiled for the host the way plants_common.emu_plants compiles its source"""
    return host_library("libemu_lin_plants.so", ["emu/emu_lin_plants.cpp"])


def emu_linearize_on(lib, fn, orc, t, z, cj, Fd, records=None):
    """one knot through a CPU twin of the linearisation kernel: fn = "emu_linearize" (tests/emu/emu_rollout.cpp: the mechanism `t` alone) or "emu_lin_plants"
    (the mechanism `t` and link-order records [nb][16], None = its own) -> (A, Bu, Bl, G)"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    mx, ml, mu = 12 * t.nb, 5 * t.ne, len(cj)
    A, Bu, Bl, G = np.zeros((mx, mx)), np.zeros((mx, mu)), np.zeros((mx, ml)), np.zeros((ml, mx))
    m = orc.mech_desc(t)
    z, Fd, cja = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(Fd, dtype=np.float64), np.ascontiguousarray(cj, dtype=np.int32)
    out = [a.ctypes.data_as(dp) for a in (A, Bu, Bl, G)]
    if fn == "emu_linearize":
        rc = lib.emu_linearize(C.byref(m.desc), z.ctypes.data_as(dp), C.c_int(mu), cja.ctypes.data_as(ip), Fd.ctypes.data_as(dp), *out)
    else:
        rec = None if records is None else np.ascontiguousarray(records, dtype=np.float64)
        rc = lib.emu_lin_plants(C.byref(m.desc), None if rec is None else rec.ctypes.data_as(dp), z.ctypes.data_as(dp), C.c_int(mu), cja.ctypes.data_as(ip),
                                Fd.ctypes.data_as(dp), *out)
    assert rc == 0, rc
    return A, Bu, Bl, G
