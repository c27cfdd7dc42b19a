"""The 32-lane chain kernels that split the Schur rows (16- and 17-link images: bench.py's headline and --links 15) move everything the two halves of a
wavefront exchange in the line search by v_permlane32_swap_b32 instead of ds_bpermute: the partner's search flag comes out of one vote, the trial state
of a lone searcher goes to the helping half by half swaps (rollout_chain.hip halves_pick), so do the helper's two norms on the way back, and the norms
themselves combine their DPP rows by the row swap (group_sum_rows32).  What can go wrong on the device and shows as wrong numbers: the wrong result of
a swap picked on one half (a half evaluates its OWN trial in place of the searcher's, or keeps the partner's), the vote's bits read from the own half,
a half without an instance taking part, the per-instance-plants path (nobody may take the other half's trial) taking one.

Inputs: bench.py's recipe (hanging-equilibrium LQR, y0 ~ U(-0.5, 0.5), phi_i ~ U(-0.2, 0.2), seed 0) on chains of 17 and 16 bodies, 40 steps; the gains
come from the oracle's Riccati recursion, so the reference needs no GPU.  Cases, each on both chains:

  2 instances                one wavefront with both halves
  3 instances                the second wavefront's upper half has no instance
  setpoint + far, far + setpoint   one start AT the setpoint (nothing to solve), one far from it, in both orders: each half is once the lone searcher
                             and once the helper
  3 instances on per-instance plants (every row the mechanism's own numbers, so the reference is the same): the `solo` path

The searches at the noise floor start at Newton iteration 4, so the inputs are checked first, on the CPU and against the oracle alone (its per-step
Newton counts, from a step-by-step replay that is asserted equal to its rollout): in EVERY pair of instances that share a wavefront some step has one
instance beyond iteration 3 while its partner has stopped before that iteration -- the lone-searcher hand-over -- and in every pair of two recipe starts
some step has both beyond iteration 3 -- two searchers.  (An instance that starts at the setpoint stays there and never reaches iteration 4: no such
step can exist in its pairs, which are there for the hand-over.)  test_inputs_reach_both_kinds_of_pass runs in the CPU suite too.

Each case: final state, trajectory, multipliers and status bitwise equal between the packed and the spread launch (an instance's result does not depend
on its partner or its half) and between one launch and carried single-step launches; trajectory and final state within 1e-9 of the oracle, the suite's
tolerance for these kernels."""
import numpy as np
import pytest
import scipy.linalg as sl

from conftest import hanging_setpoint

TOL = 1e-9
STEPS = 40
HORIZON = STEPS + 50
SEARCH_FROM = 4                    # first Newton iteration of a step whose line search runs at the noise floor
BODIES = [17, 16]
# index into the problem's starts: three recipe starts, the setpoint, the far start
PAIR_CASES = {"2 instances": [0, 1], "3 instances": [0, 1, 2], "setpoint + far": [3, 4], "far + setpoint": [4, 3]}

_PROBLEM = {}


def _problem(cclqr, orc, nb):
    """(tables, controlled joints, gains, setpoint, starts [5], the oracle's (final, trajectory, status), its Newton counts [5][STEPS]): made once per
    chain, shared by every test, read-only"""
    if nb in _PROBLEM:
        return _PROBLEM[nb]
    n_links = nb - 1
    ex = cclqr.examples.cartpole_n(n_links)
    t = ex["mech"].tables()
    assert t.nb == nb
    zd = hanging_setpoint(cclqr, n_links)
    rng = np.random.default_rng(0)                                        # bench.py build_workload, three instances
    phi = rng.uniform(-0.2, 0.2, (3, n_links))
    phi[:, 0] += np.pi
    recipe = cclqr.examples.cartpole_states(n_links, rng.uniform(-0.5, 0.5, 3), phi)
    far_phi = np.random.default_rng(77).uniform(-0.6, 0.6, (1, n_links))
    far_phi[:, 0] += np.pi
    far = cclqr.examples.cartpole_states(n_links, [0.5], far_phi)
    z0 = np.concatenate([recipe, zd[None], far])
    Q, R = sl.block_diag(*ex["Q"]) * t.dt, sl.block_diag(*ex["R"]) * t.dt
    A, Bu, Bl, G = orc.linearize(t, zd, [0], np.zeros(1))
    K, _ = orc.riccati(A, Bu, Bl, G, Q, R, HORIZON)
    ctrl = orc.ctrl_desc(t.nb, [0], K=K, N=HORIZON, zd=zd)
    ref = orc.rollout(t, ctrl, z0, STEPS, record=True)
    assert (ref[2] > 0).all(), ref[2]
    # the oracle's Newton count of every step: its rollout replayed step by step (control, then the step with the multipliers carried)
    counts = np.zeros((len(z0), STEPS), dtype=np.int64)
    for i in range(len(z0)):
        z, lam = z0[i].copy(), np.zeros(5 * t.ne)
        for k in range(1, STEPS + 1):
            assert np.array_equal(z, ref[1][i, k - 1]), "the replay left the oracle's rollout"
            z, lam, counts[i, k - 1] = orc.step(t, z, lam, orc.control(t, ctrl, z, k))
        assert np.array_equal(z, ref[0][i]) and counts[i].max() == ref[2][i]
    for a in ref + (z0, counts):
        a.setflags(write=False)
    _PROBLEM[nb] = (t, [0], K, zd, z0, ref, counts)
    return _PROBLEM[nb]


def _wavefront_pairs(ids):
    """the pairs of instances that share a wavefront in a packed launch of `ids` (two per wavefront, in order)"""
    return [(ids[i], ids[i + 1]) for i in range(0, len(ids) - 1, 2)]


def _check_inputs(counts, ids):
    for a, b in _wavefront_pairs(ids):
        ca, cb = counts[a], counts[b]
        lone = ((np.maximum(ca, cb) >= SEARCH_FROM) & (ca != cb)).any()      # beyond iteration 3 while the partner has stopped before that iteration
        both = ((ca >= SEARCH_FROM) & (cb >= SEARCH_FROM)).any()
        print("instances %d and %d: Newton counts per step\n  %s\n  %s" % (a, b, ca, cb))
        assert lone, "no step with a lone searcher: choose another start"
        if a < 3 and b < 3:
            assert both, "no step with two searchers: choose another start"


@pytest.mark.parametrize("nb", BODIES)
def test_inputs_reach_both_kinds_of_pass(cclqr, orc, nb):
    counts = _problem(cclqr, orc, nb)[6]
    for ids in PAIR_CASES.values():
        _check_inputs(counts, ids)
    # each half is once the lone searcher: the instance at the setpoint is done with its first iteration, every step
    assert counts[3].max() < SEARCH_FROM <= counts[4].max(), (counts[3], counts[4])


def _launcher(cclqr, t, cj, K, zd, z0, nominal_plants):
    """run(steps_per_launch, flags) -> (final state, trajectory, multipliers, status) of STEPS steps"""
    import torch
    capi = cclqr._capi
    mech = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(mech, cj, K=K, N=HORIZON, zd=zd)
    dev = torch.device("cuda", 0)
    n = z0.shape[0]
    tile = lambda a: np.tile(a[None], (n,) + (1,) * a.ndim)
    plants = capi.PlantsHandle(mech, tile(t.mass), tile(t.inertia), tile(t.p1), tile(t.p2)) if nominal_plants else None

    def run(per_launch, flags=0):
        z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
        zn = torch.empty_like(z)
        traj = torch.zeros((n, STEPS, t.nb, 13), dtype=torch.float64, device=dev)
        lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
        s = torch.zeros(n, dtype=torch.int32, device=dev)
        if per_launch == STEPS:
            capi.rollout_dev(mech, ctrl, n, STEPS, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zn.data_ptr(), s.data_ptr(), 0, first_instance=0,
                             flags=flags, plants=plants)
            z = zn
        else:       # carried single-step launches: state, multipliers and status round-trip HBM; every launch records its one row
            rows = torch.zeros((STEPS, n, 1, t.nb, 13), dtype=torch.float64, device=dev)
            for k in range(1, STEPS + 1):
                capi.rollout_dev(mech, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, rows[k - 1].data_ptr(), zn.data_ptr(), s.data_ptr(), 0, first_instance=0,
                                 flags=flags | (capi.ROLLOUT_CARRY_STATUS if k > 1 else 0), plants=plants)
                z, zn = zn, z
            traj = rows[:, :, 0].permute(1, 0, 2, 3).contiguous()
        torch.cuda.synchronize()
        return z.cpu().numpy(), traj.cpu().numpy(), lam.cpu().numpy(), s.cpu().numpy()
    return mech, run


def _check(cclqr, orc, nb, ids, nominal_plants=False):
    capi = cclqr._capi
    t, cj, K, zd, z0, (zT_o, traj_o, st_o), counts = _problem(cclqr, orc, nb)
    _check_inputs(counts, ids)
    n = len(ids)
    mech, run = _launcher(cclqr, t, cj, K, zd, np.array(z0[ids]), nominal_plants)
    assert mech.geometry()[0] == 32 and mech.layout_links() == nb
    assert mech.instances_per_wavefront(n, STEPS, capi.ROLLOUT_PACK_WAVEFRONTS) == 2
    spread = run(STEPS)
    packed = run(STEPS, capi.ROLLOUT_PACK_WAVEFRONTS)
    single = run(1, capi.ROLLOUT_PACK_WAVEFRONTS)
    err_traj, err_final = np.abs(packed[1] - traj_o[ids]).max(), np.abs(packed[0] - zT_o[ids]).max()
    print("%d bodies, instances %s%s: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, largest Newton count %s (oracle %s)"
          % (nb, ids, ", per-instance plants" if nominal_plants else "", err_traj, err_final, packed[3], st_o[ids]))
    for name, x, y, w in zip(("final state", "trajectory", "multipliers", "status"), spread, packed, single):
        assert np.array_equal(x, y), "packed / spread: " + name
        assert np.array_equal(y, w), "one launch / single steps: " + name
    assert (packed[3] > 0).all()
    assert err_traj < TOL and err_final < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PAIR_CASES))
@pytest.mark.parametrize("nb", BODIES)
def test_halves_exchange(cclqr, orc, nb, case):
    _check(cclqr, orc, nb, PAIR_CASES[case])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", BODIES)
def test_per_instance_plants_take_no_trial_of_the_other_half(cclqr, orc, nb):
    _check(cclqr, orc, nb, [0, 1, 2], nominal_plants=True)
