"""Shared by tests/test_value_host.py and tests/test_gpu_value.py: the definition of cclqr_value_eval restated in numpy (float64, everything in the caller's body
order), synthetic tables in the style of score_common.synthetic_case, and the host emulation of the kernel's row functions (tests/emu/emu_value.cpp)."""
import ctypes as C

import numpy as np

from build_common import host_library
from score_common import RTOL, state_errors      # noqa: F401  (RTOL: |got - ref| <= RTOL * A, A = |dz|' |P| |dz|)


def synthetic_case(nb, n_ctrl, n_tables, n_inst, seed):
    """random setpoints zd [n_ctrl][1][nb][13], a random NON-symmetric P [n_tables][12 nb][12 nb] and states of order 0.1 about one of the setpoints, unit
    quaternions.  Returns dict(zd, P, z [n_inst][nb][13])"""
    rng = np.random.default_rng(seed)
    mx = 12 * nb
    zd = rng.normal(size=(n_ctrl, 1, nb, 13))
    zd[..., 3:7] /= np.linalg.norm(zd[..., 3:7], axis=-1, keepdims=True)
    H = rng.normal(size=(n_tables, mx, mx))
    P = H @ H.transpose(0, 2, 1) / mx + 0.3 * rng.normal(size=(n_tables, mx, mx))
    z = zd[rng.integers(0, n_ctrl, n_inst), 0] + 0.1 * rng.normal(size=(n_inst, nb, 13))
    z[..., 3:7] /= np.linalg.norm(z[..., 3:7], axis=-1, keepdims=True)
    return dict(zd=zd, P=np.ascontiguousarray(P), z=np.ascontiguousarray(z))


def value_of(z, zd, P, first_instance=0):
    """V [n] and the magnitude sums A [n]: instance i reads setpoint table first_instance + i when zd holds several and P table first_instance + i when P does"""
    n = z.shape[0]
    tc = (first_instance + np.arange(n)) if zd.shape[0] > 1 else np.zeros(n, dtype=int)
    tp = (first_instance + np.arange(n)) if P.shape[0] > 1 else np.zeros(n, dtype=int)
    with np.errstate(invalid="ignore"):
        dz = state_errors(z, zd[tc, 0]).reshape(n, -1)
        V = np.einsum("ni,nij,nj->n", dz, P[tp], dz)
        A = np.einsum("ni,nij,nj->n", np.abs(dz), np.abs(P[tp]), np.abs(dz))
    return V, A


def assert_value(got, V, A, what=""):
    got = np.asarray(got)
    nan = np.isnan(V)
    assert (np.isnan(got) == nan).all(), "%s: NaN pattern differs: got %s, reference %s" % (what, got, V)
    err, bound = np.abs(got[~nan] - V[~nan]), RTOL * A[~nan]
    print("%s: worst |got - ref| / (RTOL A) = %.3g" % (what, (err / bound).max() if err.size else 0.0))
    assert (err <= bound).all(), "%s: |got - ref| max %.3g over its bound %.3g" % (what, err.max(), bound[err.argmax()])


def emu_value():
    return host_library("libemu_value.so", ["emu/emu_value.cpp"])


def emu_value_run(lib, case, perm, first_instance=0, z=None, z_stride=None):
    """the kernel's row functions lane by lane on the host: zd goes in permuted to link order (perm[l] = caller's body of link l), as cclqr_ctrl_create uploads
    it; the states and P stay in the caller's order"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    zd, P = case["zd"], case["P"]
    z = case["z"] if z is None else z
    nb = zd.shape[2]
    n = z.shape[0]
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    zl = np.ascontiguousarray(zd[:, :, perm])
    zc = np.ascontiguousarray(z)
    out = np.full(n, -7.0)
    d = lambda a: a.ctypes.data_as(dp)
    lib.emu_value.restype = C.c_int
    rc = lib.emu_value(C.c_int(nb), C.c_int64(n), C.c_int64(first_instance), perm.ctypes.data_as(ip), d(zc), C.c_int64(13 * nb if z_stride is None else z_stride), d(zl),
                       C.c_int(zd.shape[0]), C.c_int(zd.shape[1]), d(P), C.c_int64(P.shape[0]), d(out))
    assert rc == 0
    return out
