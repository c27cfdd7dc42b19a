"""The chain kernel's phase boundaries are wavefront hand-overs (WAVE_HANDOVER, cclqr_rollout_step.h): an ordering point for the compiler and no wait, on the
argument that the LDS executes one wavefront's instructions in issue order.  A boundary that did need the drain would show as wrong numbers, so every
boundary is reached here at the smallest shape that has it -- the plan columns say what each size is FOR, as in test_gpu_chain_solve_schedule.py:

  bodies  lanes  layout  what the solve does
     1      8      4     one front, three lanes per link (one link)
     2      8      4     one front, three lanes per link (two links: the cartpole)
     3      8      4     one front, one lane per link, odd length
     4      8      4     one front, even length
     7     16      8     two fronts, the plan merges (front 1 folds into the scratch block)
     8     16      8     two fronts, no merge (the scratch block is read and selected away)
    11     32     16     32 lanes, below CR_MIN_LINKS: the sweep without the reduction level
    12     32     16     reduction level, even length
    16     32     16     reduction level, the 16-link layout
    17     32     17     the headline layout
    18     32     32     the 32-link layout: no reduction level at any length
  13 + 3   32     16     a forest of two chains: one with the reduction level, one without, solved one after the other in one Newton iteration

Hanging chains under their LQR, 6 instances (a full wavefront and more at every lane count but 8), 12 steps, recorded.  Each case asserts, from the
oracle's own Newton counts on the CPU, that at least one solve of the run halves its step (the line search's phases are reached), then: trajectory, final state,
multipliers and status are bitwise equal between the packed and the spread launch and between one 12-step launch and twelve carried single-step launches, and
the trajectory and the final state match the oracle within the suite's 1e-9 (fp64).  One more case runs the 17-body chain behind the LDS poison of
tests/gpu/poison_lds.hip.  Every case is a run the kernel is expected to pass."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl

from build_common import host_library
from conftest import hanging_setpoint, long_and_short_chain_forest

TOL = 1e-9
STEPS = 12
NINST = 6
SNAN = 0x7FF4000000000001

# bodies, lanes per instance, links of the LDS layout
CHAINS = [(1, 8, 4), (2, 8, 4), (3, 8, 4), (4, 8, 4), (7, 16, 8), (8, 16, 8), (11, 32, 16), (12, 32, 16), (16, 32, 16), (17, 32, 17), (18, 32, 32)]


def _single_cart(cclqr):
    """the cart of the cartpole alone on its prismatic joint: a chain of one link"""
    origin = cclqr.Origin()
    cart = cclqr.Box(0.1, 0.5, 0.1, 0.5)
    return cclqr.Mechanism(origin, [cart], [cclqr.EqualityConstraint(cclqr.Prismatic(origin, cart, cclqr.examples.EY))], g=-9.81)


def _chain_problem(cclqr, orc, nb):
    """(tables, controlled joints, gains, N, setpoint, starts) of the hanging nb-body chain under its LQR; seed fixed so that a solve halves (asserted by the caller)"""
    rng = np.random.default_rng(300 + nb)
    if nb == 1:
        t = _single_cart(cclqr).tables()
        zd = np.zeros((1, 13)); zd[0, 3] = 1.0
        z0 = np.tile(zd, (NINST, 1, 1))
        z0[:, 0, 1] = rng.uniform(-0.5, 0.5, NINST)
        z0[:, 0, 8] = rng.uniform(-2.0, 2.0, NINST)            # the cart moves along its joint axis
        # ... and starts tilted by 0.5 to 1 rad about a random axis: a cart on its joint is a linear system whose solves never halve, this start's first
        # step has to turn the cart back onto the joint's orientation and does
        ax = rng.normal(size=(NINST, 3))
        ax /= np.linalg.norm(ax, axis=1)[:, None]
        ang = rng.uniform(0.5, 1.0, NINST)
        z0[:, 0, 3], z0[:, 0, 4:7] = np.cos(ang / 2), np.sin(ang / 2)[:, None] * ax
        Q, R = np.eye(12) * t.dt, np.eye(1) * t.dt
    else:
        n_links = nb - 1
        ex = cclqr.examples.cartpole_n(n_links)
        t = ex["mech"].tables()
        zd = hanging_setpoint(cclqr, n_links)
        phi = rng.uniform(-0.3, 0.3, (NINST, n_links))
        phi[:, 0] += np.pi
        z0 = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, NINST), phi)
        Q, R = sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt
    assert t.nb == nb
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, Q, R, STEPS + 50)
    return t, [0], K, STEPS + 50, zd, z0


def _forest_problem(cclqr):
    t, z0, zd, K, cj = long_and_short_chain_forest(cclqr)
    z0 = np.repeat(z0, NINST, 0)
    z0[:, :, 8] += np.random.default_rng(316).uniform(-1.0, 1.0, NINST)[:, None]      # both carts slide along y: every body of instance i moves with it
    return t, cj, K, 21, zd, z0


def _oracle(orc, t, cj, K, N, zd, z0):
    """the oracle's rollout and the halvings its solves made (instrumented build, one thread: the counters are the calling thread's)"""
    oc = orc.ctrl_desc(t.nb, cj, K=K, N=N, zd=zd)
    ref = orc.rollout(t, oc, z0, STEPS, record=True)
    orc.newton_stats(True)
    orc.rollout(t, oc, z0, STEPS, record=True, nthreads=1, flops=True)
    halvings = orc.newton_stats(True)[0]
    return ref, halvings


def _launcher(cclqr, t, cj, K, N, zd, z0):
    """run(steps_per_launch, flags, prep) -> (final state, trajectory, multipliers, status) of STEPS steps"""
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


def _check(cclqr, orc, problem, lanes, layout):
    capi = cclqr._capi
    t = problem[0]
    (zT_o, traj_o, st_o), halvings = _oracle(orc, *problem)
    print("%d bodies: oracle Newton iterations %s, halvings by iteration %s" % (t.nb, st_o, halvings[:8]))
    assert (st_o > 0).all()
    assert halvings.sum() >= 1, "no solve of this start halves: choose another seed"
    mech, run = _launcher(cclqr, *problem)
    assert mech.geometry()[0] == lanes and mech.layout_links() == layout
    assert mech.instances_per_wavefront(NINST, STEPS) == 1
    assert mech.instances_per_wavefront(NINST, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS) == 64 // lanes
    spread = run(STEPS)
    packed = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    single = run(1, capi.ROLLOUT_PACK_WAVEFRONTS)
    for name, x, y, w in zip(("final state", "trajectory", "multipliers", "status"), spread, packed, single):
        assert np.array_equal(x, y), "packed / spread: " + name
        assert np.array_equal(y, w), "one launch / single steps: " + name      # (a carried status is the worst step of the launches so far: the same number)
    err_traj, err_final = np.abs(packed[1] - traj_o).max(), np.abs(packed[0] - zT_o).max()
    print("max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, Newton iterations %s" % (err_traj, err_final, packed[3]))
    assert (packed[3] > 0).all() and (spread[3] > 0).all() and (single[3] > 0).all()
    assert err_traj < TOL and err_final < TOL
    return run, packed


@pytest.mark.gpu
@pytest.mark.parametrize("nb,lanes,layout", CHAINS)
def test_chain(cclqr, orc, nb, lanes, layout):
    _check(cclqr, orc, _chain_problem(cclqr, orc, nb), lanes, layout)


@pytest.mark.gpu
def test_forest_of_two_chains(cclqr, orc):
    _check(cclqr, orc, _forest_problem(cclqr), 32, 16)


@pytest.fixture(scope="module")
def poison():
    """tests/gpu/poison_lds.hip (test_gpu_lds_poison.py): fills the LDS of every compute unit with a pattern"""
    import torch
    torch.zeros(1, device="cuda")      # torch's HIP runtime first, as every other GPU test has it
    lib = host_library("libpoison_lds.so", ["gpu/poison_lds.hip"], flags=("-O2", "--offload-arch=gfx950", "-shared", "-fPIC"))
    lib.poison_lds.argtypes = [C.c_ulonglong, C.c_int, C.c_int]

    def run():
        rc = lib.poison_lds(SNAN, 160 * 1024, 8 * 256)
        assert rc == 0, "poison_lds failed: %d" % rc
    return run


@pytest.mark.gpu
def test_headline_chain_behind_poisoned_lds(cclqr, orc, poison):
    """the 17-body chain again, every launch behind an LDS full of signalling NaNs: a read that overtook the store it depends on would see one"""
    capi = cclqr._capi
    _, run = _launcher(cclqr, *_chain_problem(cclqr, orc, 17))
    for per_launch in (STEPS, 1):
        clean = run(per_launch, capi.ROLLOUT_PACK_WAVEFRONTS)
        dirty = run(per_launch, capi.ROLLOUT_PACK_WAVEFRONTS, prep=poison)
        assert (clean[3] > 0).all()
        for x, y in zip(clean, dirty):
            assert x.tobytes() == y.tobytes()
