"""A full-step trial builds its Schur rows only if a solve will read them (cclqr_chain.h chain_rows_verdict: the chain kernels that split the rows, and the
tree kernel, form the trial's ||f|| in front of the row block).  A wrongly skipped build cannot be seen on the GPU -- the solve would read the rows of an
earlier point and Newton would still converge -- so tests/emu/emu_chain_rows_verdict.cpp runs emu_chain.cpp's Newton loop twice on the CPU: once building
rows in every evaluation with Jacobians, once with the kernel's rule (the same function), one instance to a vote, and signalling NaNs written over
everything a skipped build leaves unwritten.  Final states, multipliers and the Newton count of every step must be the same bits, and every case of the
rule must have occurred: a trial that ended its instance's solve, a full step that was rejected, a trial whose rows were kept.  CPU suite."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl

from build_common import host_library
from conftest import hanging_setpoint

dp = C.POINTER(C.c_double)

# (links, instances, steps, amplitude of the start angles)
CASES = {
    "bench_recipe_16_links": (16, 6, 40, 0.2),      # bench.py build_workload at --links 16: seed 0, y0 ~ U(-0.5, 0.5), phi_i ~ U(-0.2, 0.2)
    "chain_9_bodies": (8, 6, 40, 0.3),              # a 16-link image with idle lanes, no reduction level
}


@pytest.fixture(scope="module")
def lib():
    return host_library("libemu_chain_rows_verdict.so", ["emu/emu_chain_rows_verdict.cpp"])


def _problem(cclqr, orc, n_links, n_inst, steps, amp):
    """the benchmark's workload (bench.py build_workload, rank 0, seed 0) with the hanging-equilibrium LQR made by the oracle"""
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    zd = hanging_setpoint(cclqr, n_links)
    rng = np.random.default_rng(0)
    phi = rng.uniform(-amp, amp, (n_inst, n_links))
    phi[:, 0] += np.pi
    z0 = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, n_inst), phi)
    Q, R = sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, Q, R, steps + 50)
    return t, orc.ctrl_desc(t.nb, [0], K=K, N=steps + 50, zd=zd), z0


def _run(lib, orc, t, ctrl, z0, steps, mode):
    m = orc.mech_desc(t)
    z0 = np.ascontiguousarray(z0, dtype=np.float64).reshape(-1, t.nb, 13)
    n = z0.shape[0]
    zT, lam = np.zeros_like(z0), np.zeros((n, 5 * t.nb))
    its, counts = np.zeros((n, steps), dtype=np.int32), np.zeros(3, dtype=np.int64)
    rc = lib.emu_chain_rows_verdict(C.byref(m.desc), C.byref(ctrl.desc), C.c_int64(n), C.c_int(steps), z0.ctypes.data_as(dp), C.c_int(mode),
                                    zT.ctypes.data_as(dp), lam.ctypes.data_as(dp), its.ctypes.data_as(C.POINTER(C.c_int32)),
                                    counts.ctypes.data_as(C.POINTER(C.c_longlong)))
    assert rc == 0, rc
    return zT, lam, its, counts


@pytest.mark.parametrize("case", list(CASES))
def test_skipped_builds_are_never_read(cclqr, orc, lib, case):
    n_links, n_inst, steps, amp = CASES[case]
    t, ctrl, z0 = _problem(cclqr, orc, n_links, n_inst, steps, amp)
    zT0, lam0, its0, _ = _run(lib, orc, t, ctrl, z0, steps, 0)
    zT1, lam1, its1, (finished, rejected, kept) = _run(lib, orc, t, ctrl, z0, steps, 1)
    print("%s: %d trials; no rows because the solve ended %d, because the full step was rejected %d, rows kept %d; Newton iterations %d .. %d"
          % (case, finished + rejected + kept, finished, rejected, kept, its0.min(), its0.max()))
    assert (its0 > 0).all()
    assert finished > 0 and rejected > 0 and kept > 0
    assert finished + rejected >= n_inst * steps       # the last trial of a solve is read by nobody: it ended the solve, or it was rejected
    assert finished + rejected + kept == int(its0.sum())
    assert np.array_equal(its0, its1)
    assert zT0.tobytes() == zT1.tobytes() and lam0.tobytes() == lam1.tobytes()
    assert np.isfinite(zT1).all() and np.isfinite(lam1).all()
