"""Shared by tests/test_ensemble_host.py and tests/test_gpu_ensemble.py: the definition of cclqr_rollout_ensemble restated in numpy (the errors in float64 by
score_common.state_errors, every sum over instances in longdouble, two passes, everything in the caller's body order), the bound that goes with it and the host
emulation of the kernel's row and tile functions (tests/emu/emu_ensemble.cpp)."""
import ctypes as C

import numpy as np

import score_common as sc
from build_common import host_library

RTOL = sc.RTOL      # |got - ref| <= RTOL * A, A = the reference's sum with every product and difference replaced by its magnitude
LD = np.longdouble


def error_magnitudes(traj, zd):
    """state_errors with every product and difference replaced by its magnitude, [..., nb, 12]"""
    t, d = np.abs(traj), np.abs(zd)
    m = np.empty(traj.shape[:-1] + (12,))
    m[..., 0:3] = t[..., 0:3] + d[..., 0:3]
    m[..., 3:6] = t[..., 7:10] + d[..., 7:10]
    m[..., 9:12] = t[..., 10:13] + d[..., 10:13]
    s0, a, s1, b = d[..., 3:4], d[..., 4:7], t[..., 3:4], t[..., 4:7]
    cross = np.stack([a[..., 1] * b[..., 2] + a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] + a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], axis=-1)
    m[..., 6:9] = s0 * b + s1 * a + cross
    return m


def rows_of(traj, zd, K, N, k0=1, first_instance=0):
    """x [steps][n][12 nb + mu] = (Δz, Δu) of every instance at the steps k0 .. k0 + steps - 1 and its magnitudes, float64.
    traj [n][steps][nb][13]; zd [n_ctrl][nsp][nb][13]; K [n_ctrl][nK][mu][12 nb] or None (mu then comes as 0 columns unless mu is given by K)."""
    n, steps, nb = traj.shape[:3]
    n_ctrl, nsp = zd.shape[:2]
    mu = 0 if K is None else K.shape[2]
    tab = (first_instance + np.arange(n)) if n_ctrl > 1 else np.zeros(n, dtype=int)
    x, xm = np.zeros((steps, n, 12 * nb + mu)), np.zeros((steps, n, 12 * nb + mu))
    with np.errstate(invalid="ignore"):
        for j in range(steps):
            k = k0 + j
            ksp = min(k, nsp) - 1
            dz = sc.state_errors(traj[:, j], zd[tab, ksp]).reshape(n, -1)
            dm = error_magnitudes(traj[:, j], zd[tab, ksp]).reshape(n, -1)
            x[j, :, :12 * nb], xm[j, :, :12 * nb] = dz, dm
            if K is not None and mu > 0 and (N <= 0 or k < N):
                kidx = 0 if N <= 0 else min(k, K.shape[1]) - 1
                Kk = K[tab, kidx]
                x[j, :, 12 * nb:] = -np.einsum("nmc,nc->nm", Kk, dz)
                xm[j, :, 12 * nb:] = np.einsum("nmc,nc->nm", np.abs(Kk), dm)
    return x, xm


def moments_of(x, xm):
    """mean, M2 [steps][nx] in longdouble, two passes over the instances, and their bounds' magnitudes Amean, AM2"""
    n = x.shape[1]
    with np.errstate(invalid="ignore"):
        xl = x.astype(LD)
        mean = xl.sum(axis=1) / n
        M2 = ((xl - mean[:, None]) ** 2).sum(axis=1)
        Amean = xm.astype(LD).sum(axis=1) / n
        AM2 = ((xm.astype(LD) + Amean[:, None]) ** 2).sum(axis=1)
    return mean, M2, Amean, AM2


def comoment_of(x, xm, mx):
    """C [mx][mx] of one step's x [n][nx] in longdouble and its magnitude"""
    xl, ml = x[:, :mx].astype(LD), xm[:, :mx].astype(LD)
    n = x.shape[0]
    d = xl - xl.sum(axis=0) / n
    a = ml + ml.sum(axis=0) / n
    return d.T @ d, a.T @ a


def assert_close(got, ref, A, what=""):
    """within RTOL * A, NaN exactly where the reference has NaN"""
    got, ref, A = np.asarray(got), np.asarray(ref), np.asarray(A)
    nan = np.isnan(ref.astype(np.float64))
    assert (np.isnan(got) == nan).all(), "%s: NaN pattern differs" % what
    err = np.abs(got.astype(LD) - ref)[~nan]
    bound = (RTOL * A)[~nan]
    assert (err <= bound).all(), "%s: |got - ref| max %.3g over its bound %.3g (worst ratio %.3g)" % (
        what, float(err.max()), float(bound[err.argmax()]), float((err / np.maximum(bound, LD(1e-300))).max()))


def assert_moments(got_mean, got_M2, case, k0=1, first_instance=0, what=""):
    x, xm = rows_of(case["traj"], case["zd"], case["K"], case["N"], k0=k0, first_instance=first_instance)
    mean, M2, Amean, AM2 = moments_of(x, xm)
    assert_close(got_mean, mean, Amean, what + " mean")
    assert_close(got_M2, M2, AM2, what + " M2")
    return x, xm


def emu_ensemble():
    """tests/emu/emu_ensemble.cpp, compiled for the host"""
    return host_library("libemu_ensemble.so", ["emu/emu_ensemble.cpp"])


def emu_ensemble_run(lib, case, perm, k0=1, first_instance=0):
    """the kernel's row and tile functions lane by lane on the host: the tables go in permuted to link order (perm[l] = caller's body of link l), the slab stays in
    the caller's order.  Returns mean, M2 [steps][12 nb + mu] in the caller's order"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    K, zd, traj = case["K"], case["zd"], case["traj"]
    n, steps, nb = traj.shape[:3]
    n_ctrl, nsp = zd.shape[:2]
    mu = 0 if K is None else K.shape[2]
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    zl = np.ascontiguousarray(zd[:, :, perm])
    Kl = None if K is None else np.ascontiguousarray(K.reshape(n_ctrl, K.shape[1], mu, nb, 12)[:, :, :, perm].reshape(n_ctrl, K.shape[1], mu, 12 * nb))
    mean, M2 = np.full((steps, 12 * nb + mu), np.nan), np.full((steps, 12 * nb + mu), np.nan)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    lib.emu_ensemble.restype = C.c_int
    rc = lib.emu_ensemble(C.c_int(nb), C.c_int(mu), C.c_int64(n), C.c_int(steps), C.c_int(k0), C.c_int64(first_instance), perm.ctypes.data_as(ip),
                          d(np.ascontiguousarray(traj)), d(zl), C.c_int(n_ctrl), C.c_int(nsp), d(Kl), C.c_int(0 if K is None else K.shape[1]), C.c_int(case["N"]),
                          d(mean), d(M2))
    assert rc == 0
    return mean, M2


def cancellation_case(nb, n, seed=0):
    """|mean| >> spread: the setpoint is zero positions and velocities and identity quaternions, so that Δz = z exactly, and every coordinate of z is 1 + 1e-6 g,
    g standard normal.  No gains."""
    rng = np.random.default_rng(seed)
    zd = np.zeros((1, 1, nb, 13))
    zd[..., 3] = 1.0
    traj = 1.0 + 1e-6 * rng.normal(size=(n, 2, nb, 13))
    return dict(N=0, K=None, zd=zd, traj=np.ascontiguousarray(traj))


def assert_cancellation(got_M2, case):
    """every centred variance within 1e-8 relative of the longdouble two-pass (a centred scheme leaves about 4e-10, S2 / n - mean^2 about 2e-4)"""
    x, xm = rows_of(case["traj"], case["zd"], None, 0)
    _, M2, _, _ = moments_of(x, xm)
    rel = np.abs(got_M2.astype(LD) - M2) / M2
    assert (rel <= 1e-8).all(), "centred variance off by %.3g relative" % float(rel.max())
    return float(rel.max())
