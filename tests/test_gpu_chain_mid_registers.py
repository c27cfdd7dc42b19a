"""The two-front chain kernels (16, 32 and 64 lanes) solve the middle link of the block-tridiagonal sweep from registers (ck_tri_mid_regs, cclqr_chain.h):
the last sweep step's update never goes to LDS, the two fronts' shares are merged by a DPP row rotation, gathered by row broadcasts and solved by every
sweep lane, and the first back step takes dl of the middle link from those registers.  A wrong lane predicate, a stale share or a skipped store that was
needed after all shows as wrong numbers, so every plan such a kernel can meet is reached here at the smallest chain that has it:

  bodies  lanes  layout  what the solve does
     5     16      8     two fronts, the plan merges 2 + 2
     6     16      8     no merge: front 1 alone runs the last step, front 0's share is zeros by a select
     9     32     16     32 lanes, no reduction level, merge 4 + 4
    10     32     16     32 lanes, no reduction level, no merge
    12     32     16     reduction level -> 6 links, no merge
    13     32     16     reduction level -> 7 links, merge 3 + 3
    17     32     17     the headline layout (reduction level -> 9 links, merge 4 + 4)
    19     32     32     the 32-link layout, merge 9 + 9
  13 + 3   32     16     a forest of two chains: two middle solves in one Newton iteration
   5 + 1   16      8     a forest with a ONE-LINK chain: no sweep step, the middle system comes from LDS, no back step

Hanging chains under their LQR (the forests under random gains), recorded, 12 steps, each with 6 instances and with 3: with 3 a packed launch leaves an
instance alone in its wavefront or a lane group empty, and groups finish their solves at different iterations.  Each case asserts, from the oracle's
own Newton counts on the CPU, that at least one solve of its first three instances halves its step, then: trajectory, final state, multipliers and status
are bitwise equal between the packed and the spread launch and between one 12-step launch and twelve carried single-step launches, and the trajectory
and the final state match the oracle within the suite's 1e-9 (fp64).  The oracle runs once per problem, on six instances; the three-instance runs are
checked against its first three.  Every case is a run the kernel is expected to pass."""
import numpy as np
import pytest
import scipy.linalg as sl

from conftest import hanging_setpoint, long_and_short_chain_forest

TOL = 1e-9
STEPS = 12
NINST = 6

# bodies, lanes per instance, links of the LDS layout
CHAINS = [(5, 16, 8), (6, 16, 8), (9, 32, 16), (10, 32, 16), (12, 32, 16), (13, 32, 16), (17, 32, 17), (19, 32, 32)]
# seed of each problem's starts, chosen on the CPU so that a solve of the first three instances halves (asserted in _reference)
SEED = {5: 405, 6: 406, 9: 409, 10: 410, 12: 412, 13: 413, 17: 417, 19: 419, "forest": 316, "one-link": 431}


def _chain_problem(cclqr, orc, nb):
    """(tables, controlled joints, gains, N, setpoint, starts) of the hanging nb-body chain under its LQR"""
    rng = np.random.default_rng(SEED[nb])
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
    z0[:, :, 8] += np.random.default_rng(SEED["forest"]).uniform(-1.0, 1.0, NINST)[:, None]      # both carts slide along y: every body of instance i moves with it
    return t, cj, K, 21, zd, z0


def _one_link_forest_problem(cclqr):
    """a 5-body cartpole chain and a cart alone on its prismatic joint -- a chain of ONE link -- off the same origin, the cart numbered in the middle"""
    ex = cclqr.examples.cartpole_n(4)
    ta = ex["mech"].tables()
    origin = cclqr.Origin()
    cart = cclqr.Box(0.1, 0.5, 0.1, 0.5)
    tb = cclqr.Mechanism(origin, [cart], [cclqr.EqualityConstraint(cclqr.Prismatic(origin, cart, cclqr.examples.EY))], g=-9.81).tables()
    nb = ta.nb + tb.nb
    ia, ib = [0, 1, 2, 4, 5], [3]
    mass, inertia = np.zeros(nb), np.zeros((nb, 9))
    parent, child, typ = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    p1, p2, axis, qoff = np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 3)), np.zeros((nb, 4))
    for ids, tt in ((ia, ta), (ib, tb)):
        for k in range(tt.nb):
            j = ids[k]
            mass[j], inertia[j] = tt.mass[k], tt.inertia[k]
            parent[j] = -1 if tt.parent[k] < 0 else ids[tt.parent[k]]
            child[j], typ[j], p1[j], p2[j], axis[j], qoff[j] = ids[k], tt.type[k], tt.p1[k], tt.p2[k], tt.axis[k], tt.qoff[k]
    t = cclqr.MechTables(nb, nb, ta.dt, ta.g, mass, inertia, parent, child, typ, p1, p2, axis, qoff)
    rng = np.random.default_rng(SEED["one-link"])
    phi = rng.uniform(-0.3, 0.3, (NINST, 4)); phi[:, 0] += np.pi
    z0 = np.zeros((NINST, nb, 13))
    z0[:, ia] = cclqr.examples.cartpole_states(4, rng.uniform(-0.5, 0.5, NINST), phi)
    # the lone cart: displaced and moving along its joint axis, and tilted by 0.5 to 1 rad about a random axis -- its first step has to turn it back onto
    # the joint's orientation, and that solve halves (a cart sitting on its joint is a linear system whose solves never do)
    z0[:, 3, 1] = rng.uniform(-0.5, 0.5, NINST)
    z0[:, 3, 8] = rng.uniform(-2.0, 2.0, NINST)
    ax = rng.normal(size=(NINST, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    ang = rng.uniform(0.5, 1.0, NINST)
    z0[:, 3, 3], z0[:, 3, 4:7] = np.cos(ang / 2), np.sin(ang / 2)[:, None] * ax
    zd = np.zeros((nb, 13))
    zd[ia] = hanging_setpoint(cclqr, 4)
    zd[3, 3] = 1.0
    K = rng.normal(size=(20, 2, 12 * nb)) * 0.05
    return t, [0, 3], K, 21, zd, z0


_REFERENCE = {}


def _reference(orc, key, make):
    """(problem, the oracle's rollout of its six instances), made once per problem and shared by its two cases; asserts that a solve of the first three
    instances halves (instrumented build, one thread: the counters are the calling thread's)"""
    if key not in _REFERENCE:
        problem = make()
        t, cj, K, N, zd, z0 = problem
        oc = orc.ctrl_desc(t.nb, cj, K=K, N=N, zd=zd)
        ref = orc.rollout(t, oc, z0, STEPS, record=True)
        orc.newton_stats(True)
        orc.rollout(t, oc, z0[:3], STEPS, record=True, nthreads=1, flops=True)
        halvings = orc.newton_stats(True)[0]
        print("%s: oracle Newton iterations %s, halvings of the first three instances by iteration %s" % (key, ref[2], halvings[:8]))
        assert (ref[2] > 0).all()
        assert halvings.sum() >= 1, "no solve of these starts halves: choose another seed"
        for a in ref:
            a.setflags(write=False)
        z0.setflags(write=False)
        _REFERENCE[key] = (problem, ref)
    return _REFERENCE[key]


def _launcher(cclqr, t, cj, K, N, zd, z0):
    """run(steps_per_launch, flags) -> (final state, trajectory, multipliers, status) of STEPS steps"""
    import torch
    capi = cclqr._capi
    mech = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(mech, cj, K=K, N=N, zd=zd)
    dev = torch.device("cuda", 0)
    n = z0.shape[0]

    def run(per_launch, flags=0):
        z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
        zn = torch.empty_like(z)
        traj = torch.zeros((n, STEPS, t.nb, 13), dtype=torch.float64, device=dev)
        lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
        s = torch.zeros(n, dtype=torch.int32, device=dev)
        if per_launch == STEPS:
            capi.rollout_dev(mech, ctrl, n, STEPS, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zn.data_ptr(), s.data_ptr(), 0, flags=flags)
            z = zn
        else:       # carried single-step launches: state, multipliers and status round-trip HBM; every launch records its one row
            rows = torch.zeros((STEPS, n, 1, t.nb, 13), dtype=torch.float64, device=dev)
            for k in range(1, STEPS + 1):
                capi.rollout_dev(mech, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, rows[k - 1].data_ptr(), zn.data_ptr(), s.data_ptr(), 0,
                                 flags=flags | (capi.ROLLOUT_CARRY_STATUS if k > 1 else 0))
                z, zn = zn, z
            traj = rows[:, :, 0].permute(1, 0, 2, 3).contiguous()
        torch.cuda.synchronize()
        return z.cpu().numpy(), traj.cpu().numpy(), lam.cpu().numpy(), s.cpu().numpy()
    return mech, run


def _check(cclqr, orc, key, make, lanes, layout, n):
    capi = cclqr._capi
    (t, cj, K, N, zd, z0), (zT_o, traj_o, st_o) = _reference(orc, key, make)
    mech, run = _launcher(cclqr, t, cj, K, N, zd, np.array(z0[:n]))
    assert mech.geometry()[0] == lanes and mech.layout_links() == layout
    assert mech.instances_per_wavefront(n, STEPS) == 1
    per_wave = mech.instances_per_wavefront(n, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    assert per_wave == 64 // lanes if n == NINST else per_wave > 1, per_wave
    spread = run(STEPS)
    packed = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    single = run(1, capi.ROLLOUT_PACK_WAVEFRONTS)
    for name, x, y, w in zip(("final state", "trajectory", "multipliers", "status"), spread, packed, single):
        assert np.array_equal(x, y), "packed / spread: " + name
        assert np.array_equal(y, w), "one launch / single steps: " + name      # (a carried status is the worst step of the launches so far: the same number)
    err_traj, err_final = np.abs(packed[1] - traj_o[:n]).max(), np.abs(packed[0] - zT_o[:n]).max()
    print("%s, %d instances (%d per packed wavefront): max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, Newton iterations %s"
          % (key, n, per_wave, err_traj, err_final, packed[3]))
    assert (packed[3] > 0).all() and (spread[3] > 0).all() and (single[3] > 0).all()
    assert err_traj < TOL and err_final < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("n", [NINST, 3])
@pytest.mark.parametrize("nb,lanes,layout", CHAINS)
def test_chain(cclqr, orc, nb, lanes, layout, n):
    _check(cclqr, orc, "%d bodies" % nb, lambda: _chain_problem(cclqr, orc, nb), lanes, layout, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [NINST, 3])
def test_forest_of_two_chains(cclqr, orc, n):
    _check(cclqr, orc, "forest 13 + 3", lambda: _forest_problem(cclqr), 32, 16, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [NINST, 3])
def test_forest_with_a_one_link_chain(cclqr, orc, n):
    _check(cclqr, orc, "forest 5 + 1", lambda: _one_link_forest_problem(cclqr), 16, 8, n)
