"""Shared by tests/test_plant_tracking_host.py and tests/test_gpu_plant_tracking.py: the mechanisms, plants, reference trajectories and oracle references of the
one-TrackingLQR-per-plant tests (cclqr_ctrl_create_tracking_batch_plants, cclqr_ctrl_get_gains, PlantTrackingLQR).  Every case and every reference is built once
per session and never modified."""
import ctypes as C
import json
import os

import numpy as np

from build_common import host_library
from plant_lqr_common import _rel, slider_mechanism
from plants_common import ROOT, TREE5, mechanism_of, random_plants

# name -> (plants, N, plants whose gains are compared with the oracle (None = all))
CASES = {"chain3": (5, 24, None), "chain4": (5, 24, None), "tree-slider": (4, 16, None), "sawyer": (4, 12, None), "tree-slider-128": (128, 6, (0, 63, 127)),
         "break": (5, 120, None)}
SMALL = ("chain3", "chain4", "tree-slider", "sawyer")      # the cases whose oracle facts the issue states
HANGING = ("chain3", "chain4", "tree-slider", "tree-slider-128")
BREAK_TOL = 2.0

_cases, _refs = {}, {}


def case(cclqr, orc, name):
    """dict(mech, t, cj, plants, n, N, tol, th [n][ne], z_start [n][nb][13], z_nominal [nb][13] (the first plant's pose on the mechanism's own plant), U [N][mu], zd [n][N][nb][13], Fd [n][N][mu], Q, R, check): every plant's reference
    is its OWN open-loop rollout (the oracle's, on that plant's tables) from its start pose on its own constraint manifold under the inputs U -- except `break`,
    whose references rest at the hanging pose.  Q = 10 dt I, R = 0.1 dt I."""
    if name in _cases:
        return _cases[name]
    n, N, check = CASES[name]
    k = np.arange(N)
    s, c_ = np.sin(2 * np.pi * k / N), np.cos(2 * np.pi * k / N)
    if name in ("chain3", "break"):
        mech, th0 = mechanism_of(cclqr, ("chain", 2))
        cj, U = [0], 4.0 * s[:, None]
    elif name == "chain4":
        mech, th0 = mechanism_of(cclqr, ("chain", 3))
        cj, U = [0], 4.0 * s[:, None]
    elif name.startswith("tree-slider"):
        mech, _ = slider_mechanism(cclqr, TREE5)
        th0, cj, U = np.zeros(6), [0, 5], np.stack([3.0 * s, 1.5 * c_], axis=1)
    else:
        tab = json.load(open(os.path.join(ROOT, "tests", "golden", "sawyer_arm_tables.json")))
        mech = cclqr.examples.sawyer(tab)["mech"]
        th0, cj = None, list(range(7))
        U = 0.5 * np.sin(2 * np.pi * k[:, None] / N + np.arange(7)[None])
    t = mech.tables()
    plants = random_plants(cclqr, mech, n, seed=3)
    th = np.random.default_rng(47).uniform(-0.8, 0.8, (n, 7)) if th0 is None else np.tile(th0, (n, 1))
    z_start = cclqr.joint_position_states(mech, th, plants=plants)
    mu = len(cj)
    if name == "break":
        U = np.zeros((N, 1))
        zd = np.ascontiguousarray(np.broadcast_to(z_start[:, None], (n, N, t.nb, 13)))
    else:
        zd = np.stack([open_loop(orc, plants.tables(i), cj, U, z_start[i]) for i in range(n)])
    c = dict(name=name, mech=mech, t=t, cj=cj, plants=plants, n=n, N=N, tol=BREAK_TOL if name == "break" else 1e-5, th0=th0, th=th, z_start=z_start, U=U, zd=zd,
             Fd=np.ascontiguousarray(np.broadcast_to(U[None], (n, N, mu))), Q=np.eye(12 * t.nb) * 10.0 * t.dt, R=np.eye(mu) * 0.1 * t.dt,
             check=tuple(range(n)) if check is None else check, z_nominal=cclqr.joint_position_states(mech, th[:1])[0])
    for a in (c["zd"], c["Fd"], c["z_start"], c["U"]):
        a.setflags(write=False)
    _cases[name] = c
    return c


def open_loop(orc, tables, cj, U, z0):
    """the oracle's N recorded steps of the plant `tables` from z0 under the joint inputs U [N][mu] (simulate! with the open-loop closure of
    examples/trackingLQR_triple_cartpole.jl:46-48)"""
    N = U.shape[0]
    ol = orc.ctrl_desc(tables.nb, cj, K=None, N=N + 1, zd=np.tile(orc._identity_state(tables.nb)[None], (N, 1, 1)), Fd=U)
    _, traj, st = orc.rollout(tables, ol, z0[None], N, record=True)
    assert (st > 0).all(), st
    return traj[0]


def oracle_gains(orc, c, tol=None):
    """orc.riccati_tracking on every checked plant's tables and trajectory: {i: (K [N-1][mu][mx], kbreak)}"""
    tol = c["tol"] if tol is None else tol
    key = ("gains", c["name"], tol)
    if key not in _refs:
        _refs[key] = {i: orc.riccati_tracking(c["plants"].tables(i), c["cj"], c["zd"][i], c["Fd"][i], c["Q"], c["R"], c["N"], tol=tol) for i in c["check"]}
    return _refs[key]


def oracle_nominal(orc, c):
    """the same design on the mechanism's OWN plant: its own open-loop rollout (or rest trajectory) from the nominal start pose -> (K, kbreak)"""
    key = ("nominal", c["name"])
    if key not in _refs:
        zn = c["z_nominal"]
        zd = np.tile(zn[None], (c["N"], 1, 1)) if c["name"] == "break" else open_loop(orc, c["t"], c["cj"], c["U"], zn)
        _refs[key] = orc.riccati_tracking(c["t"], c["cj"], zd, c["Fd"][0], c["Q"], c["R"], c["N"], tol=c["tol"])
    return _refs[key]


def emu_tracking_plan():
    """tests/emu/emu_tracking_plan.cpp, compiled for the host the way plants_common.emu_plants compiles its source"""
    lib = host_library("libemu_tracking_plan.so", ["emu/emu_tracking_plan.cpp"])
    for f in ("emu_tracking_default_budget", "emu_tracking_max_chunk", "emu_tracking_problem_bytes", "emu_tracking_chunk_problems", "emu_tracking_chunk_count"):
        getattr(lib, f).restype = C.c_longlong
    lib.emu_tracking_problem_bytes.argtypes = [C.c_int] * 4 + [C.c_longlong]
    lib.emu_tracking_chunk_problems.argtypes = [C.c_longlong] * 4
    lib.emu_tracking_chunk_count.argtypes = [C.c_longlong] * 2
    lib.emu_lin_knot_rows.restype = None
    lib.emu_lin_knot_rows.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_longlong)]
    return lib


__all__ = ["CASES", "SMALL", "HANGING", "BREAK_TOL", "case", "open_loop", "oracle_gains", "oracle_nominal", "emu_tracking_plan", "_rel"]
