"""Shared by the invariants tests (test_invariants_emu / _host, test_gpu_invariants, test_gpu_invariants_simulate): the definition of cclqr_rollout_invariants
restated in numpy longdouble, the bounds that go with it, the generators of synthetic slabs and the device and emu calls.

The definition (include/cclqr.h).  Row r of instance i, 13 entries per body as stored (x 0..2, q 3..6, v 7..9, w 10..12):
    0 T = sum_b 0.5 m_b v_b.v_b + 0.5 w_b.(J_b w_b)     1 V = -g sum_b m_b x_b[2]     2 E = T + V
    3 gap = max |g_r| over translational rows          4 twist = max |g_r| over rotational rows     5 quat = max_b |q_b.q_b - 1|
g_r: the rows of R(q_a)'(x_b + R(q_b) p2 - x_a) - p1 and vec(conj(q_a) q_b conj(qoff)) picked by the row selectors of the library's tables (cclqr_tables.h
fill_joint_consts, restated in `selectors`): a revolute has the three translational rows and the two rotational rows orthogonal to its axis, a prismatic joint the
two translational rows orthogonal to its axis and the three rotational rows, a FixedOrientation constraint the prismatic layout with its translational rows 0.
Whatever is not finite in float64 is NaN, and a max propagates it.

The bounds.  A is the reference's value with every product, sum and difference replaced by its magnitude (the scheme of joints_common.terms), RTOL =
score_common.RTOL, no new tolerance: |got - ref| <= RTOL A for T, V, E and every raw row; a max is 1-Lipschitz in the sup norm, so gap / twist / quat are held to
the LARGEST bound among the rows they are taken over.

Synthetic slabs are OFF the manifold (joints_common.slab: random positions), so every g_r is O(1) and the relative bound bites; their unit quaternions are scaled by
1 + O(1e-3) so that quat is not all round-off."""
import ctypes as C

import numpy as np

import joints_common as jc
import score_common as sc

RTOL = sc.RTOL
LD = np.longdouble
REVOLUTE, PRISMATIC, FIXED = jc.REVOLUTE, jc.PRISMATIC, jc.FIXED
LEN, SUMMARY_LEN = 6, 8
NAMES = ("T", "V", "E", "gap", "twist", "quat")
same_bits = jc.same_bits


class Tables(jc.Tables):
    """joints_common.Tables plus what the energy needs: mass [nb], inertia [nb][9], g"""

    def __init__(self, t):
        jc.Tables.__init__(self, t)
        self.mass = np.asarray(t.mass, dtype=np.float64).reshape(self.nb)
        self.inertia = np.asarray(t.inertia, dtype=np.float64).reshape(self.nb, 9)
        self.g, self.dt = float(t.g), float(t.dt)


def selectors(t):
    """(sel [ne][5][3], rot [ne][5] bool, absent [ne][5] bool): the row selectors of cclqr_tables.h fill_joint_consts from the normalised axis"""
    sel, rot, absent = np.zeros((t.ne, 5, 3)), np.zeros((t.ne, 5), dtype=bool), np.zeros((t.ne, 5), dtype=bool)
    for j in range(t.ne):
        a = t.axis[j]
        e, best = 0, abs(a[0])
        for i in (1, 2):
            if abs(a[i]) < best:
                best, e = abs(a[i]), i
        v1 = np.zeros(3)
        v1[e] = 1.0
        v1 = v1 - a[e] * a
        v1 = v1 / np.sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2])
        V12 = np.stack([v1, np.array([a[1] * v1[2] - a[2] * v1[1], a[2] * v1[0] - a[0] * v1[2], a[0] * v1[1] - a[1] * v1[0]])])
        nt = 3 if t.type[j] == REVOLUTE else 2
        for r in range(5):
            rot[j, r] = r >= nt
            q, nrows = (r - nt, 5 - nt) if r >= nt else (r, nt)
            sel[j, r] = np.eye(3)[q] if nrows == 3 else V12[q]
            absent[j, r] = t.type[j] == FIXED and r < nt
    return sel, rot, absent


def _canon(v):
    """longdouble values that are not finite IN FLOAT64 become NaN"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isfinite(np.asarray(v, dtype=LD).astype(np.float64)), v, np.nan)


def reference(t, traj, mass=None, inertia=None, p1=None, p2=None):
    """traj [n][steps][nb][13] -> dict(series, bound [n][steps][6], g, bound_g [n][steps][ne][5]) in longdouble; mass [n][nb], inertia [n][nb][9], p1, p2 [n][ne][3]:
    per-instance plants (default the tables')"""
    t = t if isinstance(t, Tables) else Tables(t)
    z = np.asarray(traj, dtype=LD)
    n, steps = z.shape[:2]
    lead = (n, steps)
    m = np.broadcast_to(np.asarray(t.mass if mass is None else np.asarray(mass)[:, None], dtype=LD), lead + (t.nb,))
    J = np.broadcast_to(np.asarray(t.inertia if inertia is None else np.asarray(inertia).reshape(n, 1, t.nb, 9), dtype=LD), lead + (t.nb, 9)).reshape(lead + (t.nb, 3, 3))
    P1 = np.broadcast_to(np.asarray(t.p1 if p1 is None else np.asarray(p1)[:, None], dtype=LD), lead + (t.ne, 3))
    P2 = np.broadcast_to(np.asarray(t.p2 if p2 is None else np.asarray(p2)[:, None], dtype=LD), lead + (t.ne, 3))
    sel, rot, absent = selectors(t)
    with np.errstate(invalid="ignore", over="ignore"):
        v, w, q = z[..., 7:10], z[..., 10:13], z[..., 3:7]
        T = (LD(0.5) * m * (v * v).sum(-1) + LD(0.5) * (w * np.einsum("...ij,...j->...i", J, w)).sum(-1)).sum(-1)
        AT = (LD(0.5) * m * (v * v).sum(-1) + LD(0.5) * (np.abs(w) * np.einsum("...ij,...j->...i", np.abs(J), np.abs(w))).sum(-1)).sum(-1)
        V = -LD(t.g) * (m * z[..., 2]).sum(-1)
        AV = abs(LD(t.g)) * (m * np.abs(z[..., 2])).sum(-1)
        qq = (q * q).sum(-1)
        quat_b, Aquat_b = _canon(np.abs(qq - 1)), qq + 1
        g, Ag = np.zeros(lead + (t.ne, 5), dtype=LD), np.zeros(lead + (t.ne, 5), dtype=LD)
        origin = np.zeros(lead + (13,), dtype=LD)
        origin[..., 3] = 1.0
        for j in range(t.ne):
            za = z[..., t.parent[j], :] if t.parent[j] >= 0 else origin
            zb = z[..., t.child[j], :]
            Ra, Rb = jc._rotmat(za[..., 3:7]), jc._rotmat(zb[..., 3:7])
            Ram, Rbm = jc._rotmat(np.abs(za[..., 3:7]), True), jc._rotmat(np.abs(zb[..., 3:7]), True)
            wv = zb[..., 0:3] + np.einsum("...ij,...j->...i", Rb, P2[..., j, :]) - za[..., 0:3]
            wm = np.abs(zb[..., 0:3]) + np.einsum("...ij,...j->...i", Rbm, np.abs(P2[..., j, :])) + np.abs(za[..., 0:3])
            gT = np.einsum("...ji,...j->...i", Ra, wv) - P1[..., j, :]
            gTm = np.einsum("...ji,...j->...i", Ram, wm) + np.abs(P1[..., j, :])
            qac = za[..., 3:7] * np.array([1, -1, -1, -1], dtype=LD)
            qoc = (t.qoff[j] * np.array([1, -1, -1, -1])).astype(LD)
            e = jc._qmul(jc._qmul(qac, zb[..., 3:7]), qoc)
            em = jc._qmul(jc._qmul(np.abs(qac), np.abs(zb[..., 3:7]), True), np.abs(qoc), True)
            for r in range(5):
                if absent[j, r]:
                    continue
                s = sel[j, r].astype(LD)
                src, srcm = (e[..., 1:4], em[..., 1:4]) if rot[j, r] else (gT, gTm)
                g[..., j, r] = s[0] * src[..., 0] + s[1] * src[..., 1] + s[2] * src[..., 2]
                Ag[..., j, r] = np.abs(s[0]) * srcm[..., 0] + np.abs(s[1]) * srcm[..., 1] + np.abs(s[2]) * srcm[..., 2]
        g = _canon(g)
        T, V = _canon(T), _canon(V)
        E = _canon(T + V)
        rt = np.broadcast_to(rot, g.shape)
        # (np.max propagates a NaN, as the definition does; rows of the other kind and rows a joint does not have count as 0)
        gap = np.where(rt, 0, np.abs(g)).reshape(lead + (-1,)).max(-1)
        twist = np.where(rt, np.abs(g), 0).reshape(lead + (-1,)).max(-1)
        quat = quat_b.max(-1)
        Agap = np.where(rt, 0, Ag).reshape(lead + (-1,)).max(-1)
        Atwist = np.where(rt, Ag, 0).reshape(lead + (-1,)).max(-1)
    series = np.stack([T, V, E, gap, twist, quat], axis=-1)
    bound = RTOL * np.stack([AT, AV, AT + AV, Agap, Atwist, Aquat_b.max(-1)], axis=-1)
    return dict(series=series, bound=bound, g=g, bound_g=RTOL * Ag)


def assert_series(got, ref, what=""):
    for c, name in enumerate(NAMES):
        jc.assert_close(got[..., c], ref["series"][..., c], ref["bound"][..., c], "%s %s" % (what, name))


def summary_of(series, k0=1, carry=None):
    """the summary [n][8] of a float64 series [n][steps][6] by its definition in numpy: first / min / max pick values, so the device's must equal it bit for bit"""
    series = np.asarray(series, dtype=np.float64)
    n = series.shape[0]
    out = np.full((n, SUMMARY_LEN), np.nan) if carry is None else np.array(carry, dtype=np.float64)
    if carry is None:
        out[:, 4] = out[:, 7] = 0.0
    for i in range(n):
        E, gap, twist, quat = (series[i, :, c] for c in (2, 3, 4, 5))
        fin = np.flatnonzero(np.isfinite(E))
        if fin.size:
            if np.isnan(out[i, 0]):
                out[i, 0] = E[fin[0]]
            out[i, 1] = np.nanmin([out[i, 1], E[fin].min()])
            out[i, 2] = np.nanmax([out[i, 2], E[fin].max()])
        fin = np.flatnonzero(np.isfinite(gap))
        if fin.size:
            top = gap[fin].max()
            if np.isnan(out[i, 3]) or top > out[i, 3]:
                out[i, 3], out[i, 4] = top, k0 + fin[np.argmax(gap[fin])]
        for c, v in ((5, twist), (6, quat)):
            if np.isfinite(v).any():
                out[i, c] = np.nanmax([out[i, c], v[np.isfinite(v)].max()])
        out[i, 7] += np.isnan(series[i]).any(axis=1).sum()
    return out


# ---- generators

def slab(t, n, steps, seed=0):
    """joints_common.slab (random positions and velocities, orientations built joint by joint: OFF the manifold), every quaternion scaled by 1 + 1e-3 N(0, 1)"""
    traj, _ = jc.slab(t, n, steps, seed=seed)
    rng = np.random.default_rng(3000 + seed)
    traj[..., 3:7] *= 1.0 + 1e-3 * rng.normal(size=traj.shape[:3] + (1,))
    return np.ascontiguousarray(traj)


def random_plant_arrays(t, n, seed=0):
    """per-instance mass [n][nb], inertia [n][nb][9] (symmetric positive definite, not diagonal), p1, p2 [n][ne][3]"""
    rng = np.random.default_rng(4000 + seed)
    A = rng.normal(size=(n, t.nb, 3, 3)) * 0.3
    inertia = (A @ A.transpose(0, 1, 3, 2) + 0.1 * np.eye(3)).reshape(n, t.nb, 9)
    return rng.uniform(0.5, 2.0, (n, t.nb)), inertia, rng.normal(size=(n, t.ne, 3)) * 0.5, rng.normal(size=(n, t.ne, 3)) * 0.5


# ---- the device call

def gpu_invariants(cclqr, mech, traj, k0=1, out_steps=None, want=(True, True, True), summary=None, plants=None, first_instance=0, fill=-7.0):
    """one cclqr_rollout_invariants launch over the slab traj [n][steps][nb][13] into buffers full of `fill`; want = (inv, rows, summary): which outputs are given;
    summary [n][8] goes in (k0 > 1) and comes back.  Returns (inv [n][out_steps][6], rows [n][out_steps][ne][5], summary [n][8]), None where not given"""
    import torch
    n, steps = traj.shape[:2]
    ne = mech.tables.ne
    out_steps = k0 + steps - 1 if out_steps is None else out_steps
    d = torch.from_numpy(np.ascontiguousarray(traj)).cuda()
    full = lambda shape: torch.full(shape, fill, dtype=torch.float64, device="cuda")
    iv = full((n, out_steps, LEN)) if want[0] else None
    rw = full((n, out_steps, ne, 5)) if want[1] else None
    sm = None
    if want[2]:
        sm = full((n, SUMMARY_LEN)) if summary is None else torch.from_numpy(np.ascontiguousarray(summary, dtype=np.float64)).cuda()
    ptr = lambda b: 0 if b is None else b.data_ptr()
    cclqr._capi.rollout_invariants(mech, n, steps, k0, d.data_ptr(), out_steps, ptr(iv), ptr(rw), ptr(sm), torch.cuda.current_stream().cuda_stream,
                                   first_instance=first_instance, plants=plants)
    torch.cuda.synchronize()
    host = lambda b: None if b is None else b.cpu().numpy()
    return host(iv), host(rw), host(sm)


def gpu_invariants_chunked(cclqr, mech, traj, plan):
    """the horizon of traj taken in launches of plan = [steps, ...] rows into one series, the summary travelling; returns (inv, rows, summary)"""
    n, steps = traj.shape[:2]
    assert sum(plan) == steps
    iv, rw, sm, k0 = None, None, None, 1
    for s in plan:
        a, b, sm = gpu_invariants(cclqr, mech, traj[:, k0 - 1:k0 - 1 + s], k0=k0, out_steps=steps, summary=sm)
        if iv is None:
            iv, rw = a, b
        else:
            assert (a[:, :k0 - 1] == -7.0).all() and (a[:, k0 - 1 + s:] == -7.0).all()      # only the launch's rows are written
            iv[:, k0 - 1:k0 - 1 + s], rw[:, k0 - 1:k0 - 1 + s] = a[:, k0 - 1:k0 - 1 + s], b[:, k0 - 1:k0 - 1 + s]
        k0 += s
    return iv, rw, sm


# ---- the host twin of the kernel (tests/emu/emu_invariants.cpp)

def emu_invariants():
    from build_common import host_library
    return host_library("libemu_invariants.so", ["emu/emu_invariants.cpp"])


def emu_run(lib, orc, t, traj, k0=1, out_steps=None, summary=None, lanes=0, records=None, plant_off=0, fill=-7.0):
    """csrc/cclqr_invariants.h lane by lane over the slab with the library's own tables of t; records [n_plant][nb][16]: PlantBatch.link_records().  Returns (inv
    [n][out_steps][6], rows [n][out_steps][ne][5], summary [n][8]); buffers start full of `fill`"""
    dp = C.POINTER(C.c_double)
    n, steps = traj.shape[:2]
    out_steps = k0 + steps - 1 if out_steps is None else out_steps
    iv, rw = np.full((n, out_steps, LEN), fill), np.full((n, out_steps, int(t.ne), 5), fill)
    sm = np.full((n, SUMMARY_LEN), fill) if summary is None else np.ascontiguousarray(summary, dtype=np.float64).copy()
    tr = np.ascontiguousarray(traj, dtype=np.float64)
    rec = None if records is None else np.ascontiguousarray(records, dtype=np.float64)
    desc = orc.mech_desc(t)
    lib.emu_invariants.restype = C.c_int
    rc = lib.emu_invariants(C.byref(desc.desc), C.c_int(lanes), None if rec is None else rec.ctypes.data_as(dp), C.c_longlong(plant_off), C.c_longlong(n),
                            C.c_int(steps), C.c_int(k0), tr.ctypes.data_as(dp), C.c_longlong(out_steps), iv.ctypes.data_as(dp), rw.ctypes.data_as(dp),
                            sm.ctypes.data_as(dp))
    assert rc == 0, rc
    return iv, rw, sm


def emu_summary(lib, series, k0=1, carry=None):
    """inv_summary_init / inv_summary_fold (the one-lane statement) over a float64 series [n][steps][6]"""
    dp = C.POINTER(C.c_double)
    series = np.ascontiguousarray(series, dtype=np.float64)
    n, steps = series.shape[:2]
    out = np.zeros((n, SUMMARY_LEN)) if carry is None else np.ascontiguousarray(carry, dtype=np.float64).copy()
    lib.emu_invariants_summary.restype = None
    for i in range(n):
        lib.emu_invariants_summary(C.c_int(steps), C.c_int(k0), series[i].ctypes.data_as(dp), out[i].ctypes.data_as(dp))
    return out
