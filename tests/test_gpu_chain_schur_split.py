"""The 32-lane chain kernels of at most 17 links build the Schur rows split by block (ck_schur_rows_split, cclqr_chain.h): the link's lane builds S_jj and
S_jp, the idle lane sixteen above it takes the link's W by a swap of DPP rows (rollout_chain.hip schur_split_take) and builds S_jc.  A wrong lane of the
swap, a helper that stores for a link without a child, lane 16 of a 17-link group losing its own W, or lane 0 of such a group (no helper: lane 16 owns the
leaf) building its child-side block from the wrong words shows as wrong numbers, so every role is reached here at the smallest chain that has it:

  bodies   layout  what the split does
     9       16    no reduction level; lanes 9 .. 15 idle, helpers 25 .. 31 idle
    12       16    reduction level on
    16       16    every lane a link or a helper
    17       17    link 0 without a helper (child-side block in the parent-side slot), the leaf on lane 16 keeps its W through the swap
   9 + 7     16    a forest of two chains: link 8 a leaf (its helper stores nothing), link 9 a root with a helper
   9 + 8     17    the same in a 17-link group
   1 + 11    16    a forest whose first chain is ONE link: link 0 has neither parent nor child
  16 + 1     17    17 links whose last chain is one link: lane 16 owns a root that is a leaf

Hanging chains under their LQR (the forests under random gains), recorded, 24 steps, with 6 instances and with 3 (a packed launch of 3 leaves a lane
group without an instance).  Each case: trajectory, final state, multipliers and status bitwise equal between the packed and the spread launch, between one
launch and carried single-step launches, and between a launch on clean LDS and one on LDS poisoned with signalling NaNs (tests/gpu/poison_lds.hip, as
tests/test_gpu_lds_poison.py does); trajectory and final state within the suite's 1e-9 of the oracle, which runs once per problem."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl

from build_common import host_library
from conftest import hanging_setpoint

pytestmark = pytest.mark.gpu
TOL = 1e-9
STEPS = 24
NINST = 6
SNAN = 0x7FF4000000000001

CHAINS = [(9, 16), (12, 16), (16, 16), (17, 17)]
FORESTS = [((9, 7), 16), ((9, 8), 17), ((1, 11), 16), ((16, 1), 17)]


@pytest.fixture(scope="module")
def poison():
    import torch
    torch.zeros(1, device="cuda")      # torch's HIP runtime first (the order every other GPU test has)
    lib = host_library("libpoison_lds.so", ["gpu/poison_lds.hip"], flags=("-O2", "--offload-arch=gfx950", "-shared", "-fPIC"))
    lib.poison_lds.argtypes = [C.c_ulonglong, C.c_int, C.c_int]

    def run():
        rc = lib.poison_lds(SNAN, 160 * 1024, 8 * 256)
        assert rc == 0, "poison_lds failed: %d" % rc
    return run


def _chain_problem(cclqr, orc, nb):
    rng = np.random.default_rng(700 + nb)
    n_links = nb - 1
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    assert t.nb == nb
    zd = hanging_setpoint(cclqr, n_links)
    phi = rng.uniform(-0.3, 0.3, (NINST, n_links))
    phi[:, 0] += np.pi
    z0 = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, NINST), phi)
    Q, R = sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, Q, R, STEPS + 50)
    return t, [0], K, STEPS + 50, zd, z0


def _forest_problem(cclqr, parts):
    """chains of parts[i] bodies off one origin, numbered chain by chain (1 body = a cart alone on its prismatic joint: a chain of one link)"""
    rng = np.random.default_rng(800 + 31 * parts[0] + parts[1])
    nb = sum(parts)
    mass, inertia = np.zeros(nb), np.zeros((nb, 9))
    parent, child, typ = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    p1, p2, axis, qoff = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 4))
    z0, zd, roots, base, dt, g = np.zeros((NINST, nb, 13)), np.zeros((nb, 13)), [], 0, None, None
    for n in parts:
        ids = list(range(base, base + n))
        if n == 1:
            origin = cclqr.Origin()
            cart = cclqr.Box(0.1, 0.5, 0.1, 0.5)
            tt = cclqr.Mechanism(origin, [cart], [cclqr.EqualityConstraint(cclqr.Prismatic(origin, cart, cclqr.examples.EY))], g=-9.81).tables()
            z0[:, base, 3] = 1.0
            z0[:, base, 1] = rng.uniform(-0.5, 0.5, NINST)
            z0[:, base, 8] = rng.uniform(-2.0, 2.0, NINST)
            zd[base, 3] = 1.0
        else:
            tt = cclqr.examples.cartpole_n(n - 1)["mech"].tables()
            phi = rng.uniform(-0.3, 0.3, (NINST, n - 1))
            phi[:, 0] += np.pi
            z0[:, ids] = cclqr.examples.cartpole_states(n - 1, rng.uniform(-0.5, 0.5, NINST), phi)
            zd[ids] = hanging_setpoint(cclqr, n - 1)
        dt, g = tt.dt, tt.g
        for k in range(tt.nb):
            j = ids[k]
            mass[j], inertia[j] = tt.mass[k], tt.inertia[k]
            parent[j] = -1 if tt.parent[k] < 0 else ids[tt.parent[k]]
            child[j], typ[j], p1[j], p2[j], axis[j], qoff[j] = ids[k], tt.type[k], tt.p1[k], tt.p2[k], tt.axis[k], tt.qoff[k]
        roots.append(base)
        base += n
    t = cclqr.MechTables(nb, nb, dt, g, mass, inertia, parent, child, typ, p1, p2, axis, qoff)
    K = rng.normal(size=(STEPS + 2, len(parts), 12 * nb)) * 0.05
    return t, roots, K, STEPS + 3, zd, z0


_REFERENCE = {}


def _reference(orc, key, make):
    """(problem, the oracle's rollout of its six instances): made once per problem, shared by its cases, read-only"""
    if key not in _REFERENCE:
        problem = make()
        t, cj, K, N, zd, z0 = problem
        ref = orc.rollout(t, orc.ctrl_desc(t.nb, cj, K=K, N=N, zd=zd), z0, STEPS, record=True)
        assert (ref[2] > 0).all()
        for a in ref:
            a.setflags(write=False)
        z0.setflags(write=False)
        _REFERENCE[key] = (problem, ref)
    return _REFERENCE[key]


def _launcher(cclqr, t, cj, K, N, zd, z0):
    """run(steps_per_launch, flags, prep) -> (final state, trajectory, multipliers, status) of STEPS steps; prep() runs in front of every launch"""
    import torch
    capi = cclqr._capi
    mech = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(mech, cj, K=K, N=N, zd=zd)
    dev = torch.device("cuda", 0)
    n = z0.shape[0]

    def run(per_launch, flags=0, prep=lambda: None):
        z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
        zn = torch.empty_like(z)
        traj = torch.zeros((n, STEPS, t.nb, 13), dtype=torch.float64, device=dev)
        lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
        s = torch.zeros(n, dtype=torch.int32, device=dev)
        if per_launch == STEPS:
            prep()
            capi.rollout_dev(mech, ctrl, n, STEPS, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zn.data_ptr(), s.data_ptr(), 0, flags=flags)
            z = zn
        else:       # carried single-step launches: state, multipliers and status round-trip HBM; every launch records its one row
            rows = torch.zeros((STEPS, n, 1, t.nb, 13), dtype=torch.float64, device=dev)
            for k in range(1, STEPS + 1):
                prep()
                capi.rollout_dev(mech, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, rows[k - 1].data_ptr(), zn.data_ptr(), s.data_ptr(), 0,
                                 flags=flags | (capi.ROLLOUT_CARRY_STATUS if k > 1 else 0))
                z, zn = zn, z
            traj = rows[:, :, 0].permute(1, 0, 2, 3).contiguous()
        torch.cuda.synchronize()
        return z.cpu().numpy(), traj.cpu().numpy(), lam.cpu().numpy(), s.cpu().numpy()
    return mech, run


def _check(cclqr, orc, poison, key, make, layout, n):
    capi = cclqr._capi
    (t, cj, K, N, zd, z0), (zT_o, traj_o, st_o) = _reference(orc, key, make)
    mech, run = _launcher(cclqr, t, cj, K, N, zd, np.array(z0[:n]))
    assert mech.geometry()[0] == 32 and mech.layout_links() == layout
    per_wave = mech.instances_per_wavefront(n, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    assert per_wave == 2, per_wave
    spread = run(STEPS)
    packed = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    single = run(1, capi.ROLLOUT_PACK_WAVEFRONTS)
    dirty = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS, poison)
    for name, x, y, w, v in zip(("final state", "trajectory", "multipliers", "status"), spread, packed, single, dirty):
        assert np.array_equal(x, y), "packed / spread: " + name
        assert np.array_equal(y, w), "one launch / single steps: " + name
        assert y.tobytes() == v.tobytes(), "clean / poisoned LDS: " + name
    err_traj, err_final = np.abs(packed[1] - traj_o[:n]).max(), np.abs(packed[0] - zT_o[:n]).max()
    print("%s, %d instances: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, Newton iterations %s" % (key, n, err_traj, err_final, packed[3]))
    assert (packed[3] > 0).all() and (spread[3] > 0).all() and (single[3] > 0).all()
    assert err_traj < TOL and err_final < TOL


@pytest.mark.parametrize("n", [NINST, 3])
@pytest.mark.parametrize("nb,layout", CHAINS)
def test_chain(cclqr, orc, poison, nb, layout, n):
    _check(cclqr, orc, poison, "%d bodies" % nb, lambda: _chain_problem(cclqr, orc, nb), layout, n)


@pytest.mark.parametrize("n", [NINST, 3])
@pytest.mark.parametrize("parts,layout", FORESTS, ids=["%d+%d" % p for p, _ in FORESTS])
def test_forest(cclqr, orc, poison, parts, layout, n):
    _check(cclqr, orc, poison, "forest %d + %d" % parts, lambda: _forest_problem(cclqr, parts), layout, n)
