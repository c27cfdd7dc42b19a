"""Shared by tests/test_score_host.py and tests/test_gpu_score.py: the definition of cclqr_rollout_score restated in numpy (float64, everything in the
caller's body order), the tolerance that goes with it, synthetic slabs and the host emulation of the kernel's row functions."""
import ctypes as C

import numpy as np

from build_common import host_library

RTOL = 1e-10      # |got - ref| <= RTOL * A, A = the reference's sum with every product replaced by its magnitude


def state_errors(traj, zd):
    """Δz [..., nb, 12] of lqr.jl:92-103: per body x - xd, v - vd, vec(qd^-1 (x) q) (raw: no sign fix, no factor 2), ω - ωd"""
    dz = np.empty(traj.shape[:-1] + (12,))
    dz[..., 0:3] = traj[..., 0:3] - zd[..., 0:3]
    dz[..., 3:6] = traj[..., 7:10] - zd[..., 7:10]
    dz[..., 9:12] = traj[..., 10:13] - zd[..., 10:13]
    s0, a = zd[..., 3:4], -zd[..., 4:7]
    s1, b = traj[..., 3:4], traj[..., 4:7]
    dz[..., 6:9] = s0 * b + s1 * a + np.cross(a, b)
    return dz


def stage_costs(traj, zd, K, N, Qb, R, k0=1, first_instance=0):
    """cx, cu [n][steps] and their magnitude sums Ax, Au for the steps k0 .. k0 + steps - 1.
    traj [n][steps][nb][13]; zd [n_ctrl][nsp][nb][13]; K [n_ctrl][nK][mu][12 nb] or None; N <= 0: infinite horizon; Qb [nb][12][12]; R [mu][mu].
    Instance i reads table first_instance + i when n_ctrl > 1, table 0 otherwise."""
    n, steps, nb = traj.shape[:3]
    n_ctrl, nsp = zd.shape[:2]
    mu = R.shape[0]
    tab = (first_instance + np.arange(n)) if n_ctrl > 1 else np.zeros(n, dtype=int)
    cx, cu, Ax, Au = (np.zeros((n, steps)) for _ in range(4))
    with np.errstate(invalid="ignore"):
        for j in range(steps):
            k = k0 + j
            ksp = min(k, nsp) - 1
            dz = state_errors(traj[:, j], zd[tab, ksp])                       # [n][nb][12]
            cx[:, j] = np.einsum("nbi,bij,nbj->n", dz, Qb, dz)
            Ax[:, j] = np.einsum("nbi,bij,nbj->n", np.abs(dz), np.abs(Qb), np.abs(dz))
            if K is not None and mu > 0 and (N <= 0 or k < N):
                kidx = 0 if N <= 0 else min(k, K.shape[1]) - 1
                Kk = K[tab, kidx]                                               # [n][mu][12 nb]
                flat = dz.reshape(n, -1)
                du = -np.einsum("nmc,nc->nm", Kk, flat)
                dum = np.einsum("nmc,nc->nm", np.abs(Kk), np.abs(flat))
                cu[:, j] = np.einsum("ni,ij,nj->n", du, R, du)
                Au[:, j] = np.einsum("ni,ij,nj->n", dum, np.abs(R), dum)
    return cx, cu, Ax, Au


def score_of(cx, cu, Ax, Au, settle_tol, k0=1, init=None):
    """score [n][4] = Jx, Ju, peak, last_out accumulated in step order from `init` (k0 > 1), and A [n][3]: the magnitude sums that bound Jx, Ju and peak"""
    n, steps = cx.shape
    s = np.zeros((n, 4))
    s[:, 2] = -np.inf
    A = np.zeros((n, 3))
    if k0 > 1:
        s[:] = init
        A[:, 0], A[:, 1], A[:, 2] = np.abs(init[:, 0]), np.abs(init[:, 1]), np.abs(init[:, 2])
    with np.errstate(invalid="ignore"):
        for j in range(steps):
            c = np.where(np.isfinite(cx[:, j]), cx[:, j], np.nan)
            s[:, 0] += c
            s[:, 1] += cu[:, j]
            A[:, 0] += Ax[:, j]
            A[:, 1] += Au[:, j]
            up = (c > s[:, 2]) | np.isnan(c)
            s[:, 2] = np.where(up, c, s[:, 2])
            A[:, 2] = np.where(up, Ax[:, j], A[:, 2])
            s[:, 3] = np.where(~(c <= settle_tol), float(k0 + j), s[:, 3])
    return s, A


def settle_tol_between(cx):
    """a threshold no stage cost is within rounding of: the geometric mean of two neighbours of the sorted positive stage costs whose ratio is >= 1 + 1e-6,
    as close to the median as such a pair lies"""
    v = np.sort(cx[np.isfinite(cx) & (cx > 0)].ravel())
    assert v.size >= 2, "the case has no two positive stage costs to put a threshold between"
    mid = v.size // 2
    for d in range(v.size):
        for i in (mid + d, mid - d):
            if 0 <= i < v.size - 1 and v[i + 1] / v[i] >= 1 + 1e-6:
                return float(np.sqrt(v[i] * v[i + 1]))
    raise AssertionError("no two neighbouring stage costs are 1e-6 apart")


def assert_score(got, ref, A, what=""):
    """Jx, Ju, peak within RTOL * A (NaN where the reference has NaN), last_out exact"""
    got, ref = np.asarray(got), np.asarray(ref)
    for c, name in enumerate(("Jx", "Ju", "peak")):
        nan = np.isnan(ref[:, c])
        assert (np.isnan(got[:, c]) == nan).all(), "%s %s: NaN pattern differs: got %s, reference %s" % (what, name, got[:, c], ref[:, c])
        err = np.abs(got[~nan, c] - ref[~nan, c])
        bound = RTOL * A[~nan, c]
        assert (err <= bound).all(), "%s %s: |got - ref| max %.3g over its bound %.3g (worst ratio %.3g)" % (what, name, err.max(), bound[err.argmax()],
                                                                                                             (err / np.maximum(bound, 1e-300)).max())
    assert (got[:, 3] == ref[:, 3]).all(), "%s last_out: got %s, reference %s" % (what, got[:, 3], ref[:, 3])


def synthetic_case(nb, mu, kind, n_ctrl, n_inst, steps, seed):
    """random controller tables and a random slab about them, deviations of order 0.1, unit quaternions, weights that are not symmetric.
    kind: "inf" = infinite horizon with one gain; "gated" = N = 5 with 4 gains; "tracking" = nsp = N = 6 per-step setpoints with 5 gains.
    Returns dict(N, K [n_ctrl][nK][mu][12 nb], zd [n_ctrl][nsp][nb][13], Qb, R, traj [n_inst][steps][nb][13])"""
    rng = np.random.default_rng(seed)
    N, nK, nsp = {"inf": (0, 1, 1), "gated": (5, 4, 1), "tracking": (6, 5, 6)}[kind]
    zd = rng.normal(size=(n_ctrl, nsp, nb, 13))
    zd[..., 3:7] /= np.linalg.norm(zd[..., 3:7], axis=-1, keepdims=True)
    K = rng.normal(size=(n_ctrl, nK, mu, 12 * nb)) * 0.3
    G = rng.normal(size=(nb, 12, 12))
    Qb = G @ G.transpose(0, 2, 1) / 12 + 0.3 * rng.normal(size=(nb, 12, 12))
    H = rng.normal(size=(mu, mu))
    R = H @ H.T / max(mu, 1) + 0.2 * rng.normal(size=(mu, mu))
    base = zd[rng.integers(0, n_ctrl, n_inst), 0]                             # every instance near one of the setpoints
    traj = base[:, None] + 0.1 * rng.normal(size=(n_inst, steps, nb, 13))
    traj[..., 3:7] /= np.linalg.norm(traj[..., 3:7], axis=-1, keepdims=True)
    return dict(N=N, K=K, zd=zd, Qb=Qb, R=R, traj=np.ascontiguousarray(traj))


def chain_tables(cclqr, nb):
    """mechanism tables of an nb-body chain: the pendulum (1 body) or the (nb - 1)-link cartpole"""
    if nb == 1:
        return cclqr.examples.pendulum()["mech"].tables()
    return cclqr.examples.cartpole_n(nb - 1)["mech"].tables()


def emu_score():
    """tests/emu/emu_score.cpp, compiled for the host the way plants_common.emu_plants compiles its source"""
    return host_library("libemu_score.so", ["emu/emu_score.cpp"])


def emu_score_run(lib, case, perm, settle_tol, k0=1, first_instance=0, init=None):
    """the kernel's row functions lane by lane on the host: the tables go in permuted to link order (perm[l] = caller's body of link l), as
    cclqr_ctrl_create and cclqr_score_create upload them; the slab stays in the caller's order.  Returns score [n_inst][4]"""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    K, zd, Qb, R, traj = case["K"], case["zd"], case["Qb"], case["R"], case["traj"]
    n, steps, nb = traj.shape[:3]
    n_ctrl, nsp = zd.shape[:2]
    mu = R.shape[0]
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    zl = np.ascontiguousarray(zd[:, :, perm])
    Kl = None if K is None else np.ascontiguousarray(K.reshape(n_ctrl, K.shape[1], mu, nb, 12)[:, :, :, perm].reshape(n_ctrl, K.shape[1], mu, 12 * nb))
    Ql = np.ascontiguousarray(Qb[perm])
    Rc = np.ascontiguousarray(R)
    score = np.full((n, 4), np.nan) if init is None else np.ascontiguousarray(init, dtype=np.float64).copy()
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    lib.emu_score.restype = C.c_int
    rc = lib.emu_score(C.c_int(nb), C.c_int(mu), C.c_int64(n), C.c_int(steps), C.c_int(k0), C.c_int64(first_instance), perm.ctypes.data_as(ip), d(traj),
                       d(zl), C.c_int(n_ctrl), C.c_int(nsp), d(Kl), C.c_int(0 if K is None else K.shape[1]), C.c_int(case["N"]), d(Ql), d(Rc),
                       C.c_double(settle_tol), d(score))
    assert rc == 0
    return score
