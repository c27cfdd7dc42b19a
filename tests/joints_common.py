"""Shared by the joint-coordinate tests (test_joints_reference / _host / _emu, test_gpu_joints, test_gpu_series, test_gpu_joints_simulate): the definition of
cclqr_rollout_joints restated in numpy, the bounds that go with it, the generators of synthetic slabs and the device calls.

The definition (include/cclqr.h).  Joint j hangs its child body b off its parent a (or the origin: x = 0, q = 1, velocities 0); with the normalised axis
    revolute   e = conj(q_a) q_b conj(qoff),  s = axis . vec(e),  c = e_0,  theta_raw = 2 atan2(s, c),     rate = axis . w_b - axis . w_a
    prismatic  theta_raw = axis . (R_a'(x_b + R_b p2 - x_a) - p1),                                         rate = axis . R_a'(v_b - v_a)
    a FixedOrientation constraint gives 0 for both.
Continuous mode of a revolute: w = 2 atan2(s, c) with (s, c) negated when c < 0, theta_k = w_k + 2 pi turns_k, turns = 0 at step 1, one down where
w_k - w_prev > pi and one up where it is < -pi; a w that is not finite gives NaN and leaves (w_prev, turns) alone.

The bounds.  A is the reference's value with every product and difference replaced by its magnitude (ensemble_common.error_magnitudes does the same for the
errors), RTOL = score_common.RTOL, no new tolerance:
    prismatic coordinate and every rate   |got - ref| <= RTOL A
    revolute                              |got - ref| <= RTOL (2 A_sc / h + |ref|),  h = hypot(s, c) of the reference, A_sc = A_s + A_c:
                                          d(2 atan2(s, c)) = 2 (c ds - s dc) / h^2, at most 2 (|ds| + |dc|) / h, plus the rounding of atan2 and of w + 2 pi turns.
The generators build a revolute's child pose as the joint rotation about the axis times a tilt of at most 0.3 rad that stays the same along time, so h >= cos(0.15)
and w_k - w_{k-1} is the generating angle's increment (at most 3 rad) modulo 2 pi: | |w_k - w_{k-1}| - pi | >= 0.1, rounding cannot change a turn decision and turns
is compared exactly.  Both are asserted on the reference (assert_generated)."""
import numpy as np

import score_common as sc

RTOL = sc.RTOL
LD = np.longdouble
REVOLUTE, PRISMATIC, FIXED = 0, 1, 2
RAW, CONTINUOUS = 0, 1


class Tables:
    """what the definition needs of a mechanism, in the caller's order: any object with nb, ne, parent, child, type, p1, p2, axis, qoff (MechTables, PlantBatch.tables)"""

    def __init__(self, t, p1=None, p2=None):
        self.nb, self.ne = int(t.nb), int(t.ne)
        self.parent, self.child, self.type = (np.asarray(a, dtype=int) for a in (t.parent, t.child, t.type))
        ax = np.asarray(t.axis, dtype=np.float64).reshape(self.ne, 3)
        self.axis = ax / np.sqrt((ax * ax).sum(axis=1))[:, None]      # (the library normalises the axis when it builds its tables)
        self.p1 = np.asarray(t.p1 if p1 is None else p1, dtype=np.float64).reshape(self.ne, 3)
        self.p2 = np.asarray(t.p2 if p2 is None else p2, dtype=np.float64).reshape(self.ne, 3)
        self.qoff = np.asarray(t.qoff, dtype=np.float64).reshape(self.ne, 4)


def _qmul(a, b, mag=False):
    """quaternion product over the leading axes; mag: every term taken positive (inputs are magnitudes then)"""
    m = 1.0 if mag else -1.0
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    b0, b1, b2, b3 = (b[..., i] for i in range(4))
    return np.stack([a0 * b0 + m * (a1 * b1) + m * (a2 * b2) + m * (a3 * b3),
                     a0 * b1 + a1 * b0 + a2 * b3 + m * (a3 * b2),
                     a0 * b2 + m * (a1 * b3) + a2 * b0 + a3 * b1,
                     a0 * b3 + a1 * b2 + m * (a2 * b1) + a3 * b0], axis=-1)


def _rotmat(q, mag=False):
    m = 1.0 if mag else -1.0
    s, x, y, z = (q[..., i] for i in range(4))
    R = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    R[..., 0, 0] = s * s + x * x + m * (y * y) + m * (z * z); R[..., 0, 1] = 2 * (x * y + m * (s * z)); R[..., 0, 2] = 2 * (x * z + s * y)
    R[..., 1, 0] = 2 * (x * y + s * z); R[..., 1, 1] = s * s + m * (x * x) + y * y + m * (z * z); R[..., 1, 2] = 2 * (y * z + m * (s * x))
    R[..., 2, 0] = 2 * (x * z + m * (s * y)); R[..., 2, 1] = 2 * (y * z + s * x); R[..., 2, 2] = s * s + m * (x * x) + m * (y * y) + z * z
    return R


def terms(t, z, dtype=np.float64, p1=None, p2=None):
    """z [..., nb, 13] -> dict of [..., ne] arrays: s, c (revolutes; 0, 1 elsewhere), lin (prismatic coordinate), rate, and the magnitudes As, Ac, Alin, Arate.
    p1, p2 [..., ne, 3]: per-instance vertices (broadcast against z's leading axes), default the tables'"""
    z = np.asarray(z, dtype=dtype)
    lead = z.shape[:-2]
    out = {k: np.zeros(lead + (t.ne,), dtype=dtype) for k in ("s", "lin", "rate", "As", "Ac", "Alin", "Arate")}
    out["c"] = np.ones(lead + (t.ne,), dtype=dtype)
    P1 = np.broadcast_to(np.asarray(t.p1 if p1 is None else p1, dtype=dtype), lead + (t.ne, 3))
    P2 = np.broadcast_to(np.asarray(t.p2 if p2 is None else p2, dtype=dtype), lead + (t.ne, 3))
    origin = np.zeros(lead + (13,), dtype=dtype)
    origin[..., 3] = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(t.ne):
            if t.type[j] == FIXED:
                continue
            za = z[..., t.parent[j], :] if t.parent[j] >= 0 else origin
            zb = z[..., t.child[j], :]
            ax = t.axis[j].astype(dtype)
            aax = np.abs(ax)
            if t.type[j] == REVOLUTE:
                qac = za[..., 3:7] * np.array([1, -1, -1, -1], dtype=dtype)
                qoc = (t.qoff[j] * np.array([1, -1, -1, -1])).astype(dtype)
                e = _qmul(_qmul(qac, zb[..., 3:7]), qoc)
                em = _qmul(_qmul(np.abs(qac), np.abs(zb[..., 3:7]), True), np.abs(qoc), True)
                out["s"][..., j] = ax[0] * e[..., 1] + ax[1] * e[..., 2] + ax[2] * e[..., 3]
                out["c"][..., j] = e[..., 0]
                out["As"][..., j] = aax[0] * em[..., 1] + aax[1] * em[..., 2] + aax[2] * em[..., 3]
                out["Ac"][..., j] = em[..., 0]
                out["rate"][..., j] = (ax * zb[..., 10:13]).sum(axis=-1) - ((ax * za[..., 10:13]).sum(axis=-1) if t.parent[j] >= 0 else 0)
                out["Arate"][..., j] = (aax * np.abs(zb[..., 10:13])).sum(axis=-1) + (aax * np.abs(za[..., 10:13])).sum(axis=-1)
            else:
                Ra, Rb = _rotmat(za[..., 3:7]), _rotmat(zb[..., 3:7])
                Ram, Rbm = _rotmat(np.abs(za[..., 3:7]), True), _rotmat(np.abs(zb[..., 3:7]), True)
                w = zb[..., 0:3] + np.einsum("...ij,...j->...i", Rb, P2[..., j, :]) - za[..., 0:3]
                wm = np.abs(zb[..., 0:3]) + np.einsum("...ij,...j->...i", Rbm, np.abs(P2[..., j, :])) + np.abs(za[..., 0:3])
                gT = np.einsum("...ji,...j->...i", Ra, w)
                gTm = np.einsum("...ji,...j->...i", Ram, wm)
                out["lin"][..., j] = (ax * (gT - P1[..., j, :])).sum(axis=-1)
                out["Alin"][..., j] = (aax * (gTm + np.abs(P1[..., j, :]))).sum(axis=-1)
                dv = zb[..., 7:10] - za[..., 7:10]
                dvm = np.abs(zb[..., 7:10]) + np.abs(za[..., 7:10])
                out["rate"][..., j] = (ax * np.einsum("...ji,...j->...i", Ra, dv)).sum(axis=-1)
                out["Arate"][..., j] = (aax * np.einsum("...ji,...j->...i", Ram, dvm)).sum(axis=-1)
    return out


def _finite_or_nan(v):
    return np.where(np.isfinite(v), v, np.nan)


def principal(s, c):
    """w in [-pi, pi]: 2 atan2(s, c) with (s, c) negated when c < 0; NaN where s or c is not finite"""
    with np.errstate(invalid="ignore"):
        neg = c < 0
        w = 2 * np.arctan2(np.where(neg, -s, s), np.where(neg, -c, c))
    return np.where(np.isfinite(s) & np.isfinite(c), w, np.nan)


def continue_angles(w, carry=None):
    """w [n][steps][ne] -> (theta, turns [n][steps][ne], carry (w_prev, turns) [n][ne][2]); carry: the state before the first row, default (NaN, 0)"""
    n, steps, ne = w.shape
    wp = np.full((n, ne), np.nan, dtype=w.dtype) if carry is None else carry[..., 0].astype(w.dtype)
    tn = np.zeros((n, ne)) if carry is None else carry[..., 1].astype(np.float64).copy()
    theta, turns = np.full(w.shape, np.nan, dtype=w.dtype), np.zeros(w.shape)
    pi = w.dtype.type(np.pi) if w.dtype != LD else LD("3.14159265358979323846264338327950288")
    with np.errstate(invalid="ignore"):
        for k in range(steps):
            fin = np.isfinite(w[:, k])
            d = w[:, k] - wp
            tn = np.where(fin & (d > pi), tn - 1, np.where(fin & (d < -pi), tn + 1, tn))
            wp = np.where(fin, w[:, k], wp)
            theta[:, k] = np.where(fin, w[:, k] + 2 * pi * tn.astype(w.dtype), np.nan)
            turns[:, k] = tn
    return theta, turns, np.stack([wp.astype(np.float64), tn], axis=-1)


def reference(t, traj, mode, carry=None, p1=None, p2=None, dtype=LD):
    """traj [n][steps][nb][13] -> dict(theta, rate, bound_theta, bound_rate [n][steps][ne], turns, carry, h, w): the definition in `dtype` (the reference:
    longdouble) and the bounds; p1, p2 [n][ne][3] per-instance vertices"""
    t = t if isinstance(t, Tables) else Tables(t)
    q = terms(t, traj, dtype, None if p1 is None else np.asarray(p1)[:, None], None if p2 is None else np.asarray(p2)[:, None])
    rev, pri = (t.type == REVOLUTE)[None, None], (t.type == PRISMATIC)[None, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = np.hypot(q["s"], q["c"])
        if mode == CONTINUOUS:
            w = principal(q["s"], q["c"])
            ang, turns, carry_out = continue_angles(np.where(rev, w, 0).astype(dtype), carry)
        else:
            w = np.where(np.isfinite(q["s"]) & np.isfinite(q["c"]), 2 * np.arctan2(q["s"], q["c"]), np.nan)
            ang, turns, carry_out = w, np.zeros(w.shape), None
        theta = np.where(rev, ang, np.where(pri, _finite_or_nan(q["lin"]), 0))
        rate = _finite_or_nan(q["rate"])
        b_rev = RTOL * (2 * (q["As"] + q["Ac"]) / h + np.abs(theta))
        bound_theta = np.where(rev, b_rev, RTOL * q["Alin"])
    return dict(theta=theta, rate=rate, bound_theta=bound_theta, bound_rate=RTOL * q["Arate"], turns=turns, carry=carry_out, h=np.where(rev, h, 1), w=np.where(rev, w, 0))


def assert_close(got, ref, bound, what=""):
    """within the bound, NaN exactly where the reference has NaN, never an infinity"""
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound)
    nan = np.isnan(ref.astype(np.float64))
    assert (np.isnan(got) == nan).all(), "%s: NaN pattern differs (got %d, reference %d)" % (what, int(np.isnan(got).sum()), int(nan.sum()))
    err, b = np.abs(got.astype(LD) - ref)[~nan], bound[~nan]
    if err.size:
        assert (err <= b).all(), "%s: |got - ref| max %.3g over its bound %.3g (worst ratio %.3g)" % (what, float(err.max()), float(b[err.argmax()]),
                                                                                                     float((err / np.maximum(b, LD(1e-300))).max()))


def assert_joints(got_theta, got_rate, ref, what=""):
    """theta and rate within their bounds and the turn count exact: theta - w is a whole number of turns, the reference's"""
    assert_close(got_theta, ref["theta"], ref["bound_theta"], what + " theta")
    if got_rate is not None:
        assert_close(got_rate, ref["rate"], ref["bound_rate"], what + " rate")
    fin = np.isfinite(ref["theta"].astype(np.float64)) & (ref["turns"] != 0)
    got_turns = np.rint((got_theta.astype(LD) - ref["w"]) / (2 * LD(np.pi)))
    assert (got_turns[fin] == ref["turns"][fin]).all(), what + ": turn counts differ"


def assert_generated(ref):
    """the two properties the generators promise, on the reference: h >= cos(0.15), and no decision of the continuation within 0.1 of its threshold"""
    h, w = ref["h"].astype(np.float64), ref["w"].astype(np.float64)
    assert (h[np.isfinite(h)] >= np.cos(0.15) - 1e-12).all(), "a generated pose has hypot(s, c) = %.6f" % h[np.isfinite(h)].min()
    d = np.abs(np.abs(np.diff(w, axis=1)) - np.pi)
    assert not (d[np.isfinite(d)] < 0.1).any(), "a generated increment lies within 0.1 of pi"


# ---- generators

def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _axis_angle(axis, ang):
    return np.concatenate([np.cos(ang / 2)[..., None], np.sin(ang / 2)[..., None] * axis], axis=-1)


def mixed_chain(cclqr, nb, seed=0, prismatic_every=3):
    """MechTables of an nb-body chain off the origin, every `prismatic_every`-th joint prismatic (the first one too), the others revolute; random axes (not
    normalised), vertices and unit qoff"""
    rng = np.random.default_rng(1000 + seed)
    typ = np.array([PRISMATIC if j % prismatic_every == 0 else REVOLUTE for j in range(nb)], dtype=np.int32)
    parent, child = np.arange(-1, nb - 1, dtype=np.int32), np.arange(nb, dtype=np.int32)
    axis = _unit(rng.normal(size=(nb, 3))) * rng.uniform(0.5, 2.0, (nb, 1))
    return cclqr.MechTables(nb, nb, 0.01, -9.81, rng.uniform(0.5, 2.0, nb), np.tile(np.eye(3).reshape(9) * 0.1, (nb, 1)), parent, child, typ,
                            rng.normal(size=(nb, 3)) * 0.5, rng.normal(size=(nb, 3)) * 0.5, axis, _unit(rng.normal(size=(nb, 4))))


def slab(t, n, steps, seed=0, max_step=3.0):
    """(traj [n][steps][nb][13], angle [n][steps][ne]): every revolute's child orientation is q_a (rot(axis, angle_k) tilt) qoff with a tilt of at most 0.3 rad
    fixed along time and an angle that walks in steps of up to max_step rad from a start in [-pi, pi] (several turns either way over a few steps); prismatic
    children carry the tilt alone; positions and velocities are random.  Bodies are placed parents first."""
    t = t if isinstance(t, Tables) else Tables(t)
    rng = np.random.default_rng(2000 + seed)
    traj = np.zeros((n, steps, t.nb, 13))
    traj[..., 0:3] = rng.normal(size=(n, steps, t.nb, 3))
    traj[..., 7:13] = rng.normal(size=(n, steps, t.nb, 6))
    traj[..., 3] = 1.0
    angle = rng.uniform(-np.pi, np.pi, (n, 1, t.ne)) + np.cumsum(rng.uniform(-max_step, max_step, (n, steps, t.ne)), axis=1)
    tilt = _axis_angle(_unit(rng.normal(size=(n, 1, t.ne, 3))), rng.uniform(0, 0.3, (n, 1, t.ne)))
    done, todo = set(), list(range(t.ne))
    while todo:
        for j in list(todo):
            a, b = t.parent[j], t.child[j]
            if (a >= 0 and a not in done) or b in done:      # (a body that closes a loop keeps the pose its first joint gave it)
                if b in done:
                    todo.remove(j)
                continue
            qa = traj[:, :, a, 3:7] if a >= 0 else np.broadcast_to(np.array([1.0, 0, 0, 0]), (n, steps, 4))
            e = np.broadcast_to(tilt[:, :, j], (n, steps, 4))
            if t.type[j] == REVOLUTE:
                e = _qmul(_axis_angle(t.axis[j], angle[:, :, j]), e)
            traj[:, :, b, 3:7] = _qmul(_qmul(qa, e), np.broadcast_to(t.qoff[j], (n, steps, 4)))
            done.add(b)
            todo.remove(j)
    return np.ascontiguousarray(traj), angle


# ---- the device calls

def gpu_joints(cclqr, mech, traj, mode, k0=1, out_steps=None, rates=True, carry=None, plants=None, first_instance=0, fill=np.nan):
    """one cclqr_rollout_joints launch over the slab traj [n][steps][nb][13] into buffers full of `fill`; carry [n][ne][2] goes in (k0 > 1) and comes back.
    Returns (theta [n][out_steps][ne], rate or None, carry or None)"""
    import torch
    capi = cclqr._capi
    n, steps = traj.shape[:2]
    ne = mech.tables.ne
    out_steps = k0 + steps - 1 if out_steps is None else out_steps
    d = torch.from_numpy(np.ascontiguousarray(traj)).cuda()
    th = torch.full((n, out_steps, ne), fill, dtype=torch.float64, device="cuda")
    rt = torch.full((n, out_steps, ne), fill, dtype=torch.float64, device="cuda") if rates else None
    cr = None
    if mode == CONTINUOUS:
        cr = torch.full((n, ne, 2), fill, dtype=torch.float64, device="cuda") if carry is None else torch.from_numpy(np.ascontiguousarray(carry, dtype=np.float64)).cuda()
    capi.rollout_joints(mech, n, steps, k0, d.data_ptr(), mode, out_steps, th.data_ptr(), 0 if rt is None else rt.data_ptr(), 0 if cr is None else cr.data_ptr(),
                        torch.cuda.current_stream().cuda_stream, first_instance=first_instance, plants=plants)
    torch.cuda.synchronize()
    return th.cpu().numpy(), None if rt is None else rt.cpu().numpy(), None if cr is None else cr.cpu().numpy()


def gpu_joints_chunked(cclqr, mech, traj, mode, plan, rates=True):
    """the horizon of traj taken in launches of plan = [steps, ...] rows into one series, the carry travelling; returns (theta, rate, carry)"""
    import torch
    capi = cclqr._capi
    n, steps = traj.shape[:2]
    ne = mech.tables.ne
    assert sum(plan) == steps
    th = torch.full((n, steps, ne), np.nan, dtype=torch.float64, device="cuda")
    rt = torch.full((n, steps, ne), np.nan, dtype=torch.float64, device="cuda") if rates else None
    cr = torch.full((n, ne, 2), np.nan, dtype=torch.float64, device="cuda") if mode == CONTINUOUS else None
    k0 = 1
    for s in plan:
        d = torch.from_numpy(np.ascontiguousarray(traj[:, k0 - 1:k0 - 1 + s])).cuda()
        capi.rollout_joints(mech, n, s, k0, d.data_ptr(), mode, steps, th.data_ptr(), 0 if rt is None else rt.data_ptr(), 0 if cr is None else cr.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        k0 += s
    return th.cpu().numpy(), None if rt is None else rt.cpu().numpy(), None if cr is None else cr.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the statistics of a series across its instances, in numpy (longdouble two-pass moments, the quantile definition of quantile_common)

def series_moments(x):
    """x [n][steps][nc] -> mean, M2 [steps][nc] (NaN where a value is not finite) and the magnitudes Amean, AM2 of ensemble_common.moments_of"""
    import ensemble_common as ec
    xs = np.where(np.isfinite(x), x, np.nan).transpose(1, 0, 2)
    return ec.moments_of(xs, np.abs(xs))


def series_quantiles(x, probs):
    import quantile_common as qc
    return qc.quantiles_of(np.ascontiguousarray(x.transpose(1, 0, 2)), probs)


# ---- the host twin of the kernel's per-joint functions (tests/emu/emu_joints.cpp)

def emu_joints():
    from build_common import host_library
    return host_library("libemu_joints.so", ["emu/emu_joints.cpp"])


def emu_joints_run(lib, t, traj, mode, k0=1, out_steps=None, carry=None, rates=True):
    """csrc/cclqr_joints.h lane by lane over the slab; returns (theta [n][out_steps][ne], rate or None, carry [n][ne][2] or None); buffers start full of NaN"""
    import ctypes as C
    t = t if isinstance(t, Tables) else Tables(t)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n, steps = traj.shape[:2]
    out_steps = k0 + steps - 1 if out_steps is None else out_steps
    th = np.full((n, out_steps, t.ne), np.nan)
    rt = np.full((n, out_steps, t.ne), np.nan) if rates else None
    cr = None
    if mode == CONTINUOUS:
        cr = np.full((n, t.ne, 2), np.nan) if carry is None else np.ascontiguousarray(carry, dtype=np.float64).copy()
    d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
    i = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(ip)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (t.axis, t.qoff, t.p1, t.p2, traj)]
    lib.emu_joints.restype = C.c_int
    rc = lib.emu_joints(C.c_int(t.nb), C.c_int(t.ne), C.c_longlong(n), C.c_int(steps), C.c_int(k0), C.c_int(mode), i(t.type), i(t.parent), i(t.child),
                        *(a.ctypes.data_as(dp) for a in keep), C.c_longlong(out_steps), th.ctypes.data_as(dp), None if rt is None else rt.ctypes.data_as(dp),
                        None if cr is None else cr.ctypes.data_as(dp))
    assert rc == 0
    return th, rt, cr


def emu_series_moments(lib, x):
    import ctypes as C
    dp = C.POINTER(C.c_double)
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, steps, nc = x.shape
    mean, m2 = np.full((steps, nc), 7.0), np.full((steps, nc), 7.0)
    lib.emu_series_moments.restype = C.c_int
    assert lib.emu_series_moments(C.c_longlong(n), C.c_int(steps), C.c_int(nc), x.ctypes.data_as(dp), mean.ctypes.data_as(dp), m2.ctypes.data_as(dp)) == 0
    return mean, m2


def assert_series_quantiles(got, finite, x, probs, what=""):
    """the quantiles of the series x [n][steps][nc] against the definition: the counts exact; an order statistic is 1-Lipschitz in the sup norm of its data and so is
    an interpolation between two (quantile_common.assert_quantiles), so |got - ref| <= RTOL max_i |x_i| over the finite values per (row, coordinate); p = 0 and
    p = 1 are the extremes themselves, bit for bit"""
    import quantile_common as qc
    ref, cnt = series_quantiles(x, probs)
    assert finite is None or np.array_equal(finite, cnt), what + ": finite counts differ"
    with np.errstate(invalid="ignore"):
        top = np.nanmax(np.where(np.isfinite(x), np.abs(x), 0.0), axis=0)      # [steps][nc]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN pattern differs"
    err = np.where(nan, 0.0, np.abs(got - ref))
    assert (err <= RTOL * top[:, None, :]).all(), "%s: |got - ref| max %.3g" % (what, err.max())
    for j, p in enumerate(probs):
        if p in (0.0, 1.0):
            assert qc.same_bits(got[:, j][~nan[:, j]], ref[:, j][~nan[:, j]]), "%s: p = %g is not the extreme itself" % (what, p)
    return ref, cnt
