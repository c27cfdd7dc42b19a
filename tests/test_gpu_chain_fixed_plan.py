"""A mechanism that is ONE chain of 16 or 17 links from link 0 (the N-link cartpole: bench.py's --links 15 and its headline) runs on
rollout_chain_fixed_kernel<NBP, law, relax> (the kernel text of csrc/rollout_chain.hip compiled with CHAIN_PLAN_FIXED): the plan of the block-tridiagonal solve -- one
chain, the reduction level taken, four sweep steps, the merge step -- is a constant of the kernel instead of being re-derived from the plan word on every
Newton iteration.  Same functions on the same operands in the same order, so the results must be the run-time-plan kernel's BIT FOR BIT;
cclqr_rollout_opts.flags = CCLQR_ROLLOUT_RUNTIME_PLAN launches that kernel on the same mechanism, which is what every case here compares against.  What
can go wrong on the device and shows as different bits: a constant of the plan that is not the run-time value (a front one link short, the merge step in
the wrong pass, a helper flag of the last odd link), a lane taking part that the run-time plan leaves out, a hoisted value that is stale for an instance
that has finished.

Inputs and helpers are those of tests/test_gpu_chain_half_swap.py (bench.py's recipe on chains of 17 and 16 bodies, 40 steps, the oracle's gains; its
reference is computed once and shared).  Cases, each on both chains:

  1, 2, 3 instances                  a lone instance in a wavefront; both halves; a second wavefront whose upper half has no instance
  setpoint + far, far + setpoint     a partner that is done with its first iteration, in either half
  3 instances on per-instance plants (every row the mechanism's own numbers: same reference)
  friction + noise law, 17 bodies    the <17, 1> kernel in one launch (samples from the fill kernel) and the <17, 3> kernel in single steps (samples generated in it)

Each case: final state, trajectory, status and multipliers bitwise equal between the default launch and the launch with ROLLOUT_RUNTIME_PLAN, and between
one launch and carried single-step launches; trajectory and final state within 1e-9 of the oracle.  A 17-body forest of TWO chains never takes the fixed
kernel: the flag changes nothing there.

The inputs are checked first, on the CPU and against the oracle alone (test_inputs_exercise_the_solve runs in the CPU suite): every case contains a step
whose Newton solve goes beyond iteration 3 and a step whose line search halved the step at least once (the oracle's instrumented build counts halvings)."""
import numpy as np
import pytest

from test_gpu_chain_half_swap import BODIES, HORIZON, SEARCH_FROM, STEPS, TOL, _problem

CASES = {"1 instance": [0], "2 instances": [0, 1], "3 instances": [0, 1, 2], "setpoint + far": [3, 4], "far + setpoint": [4, 3]}
FRIC_NOISE = dict(noise_scale=0.5, noise_seed=77)      # + fric = 0.01 on every joint (_law_kw)

_HALVINGS = {}


def _law_kw(t, fric_noise):
    return dict(FRIC_NOISE, fric=np.full(t.ne, 0.01)) if fric_noise else {}


def _halvings(cclqr, orc, nb):
    """halvings of the oracle's line searches over the STEPS steps of each of the problem's five starts (plain law): its instrumented build, replayed step by step"""
    if nb not in _HALVINGS:
        t, cj, K, zd, z0, ref, counts = _problem(cclqr, orc, nb)
        ctrl = orc.ctrl_desc(t.nb, cj, K=K, N=HORIZON, zd=zd)
        out = np.zeros(len(z0))
        for i in range(len(z0)):
            z, lam = z0[i].copy(), np.zeros(5 * t.ne)
            orc.newton_stats(reset=True)
            for k in range(1, STEPS + 1):
                z, lam, _ = orc.step(t, z, lam, orc.control(t, ctrl, z, k), flops=True)
            assert np.array_equal(z, ref[0][i]), "the instrumented replay left the oracle's rollout"
            out[i] = orc.newton_stats(reset=True)[0].sum()
        _HALVINGS[nb] = out
    return _HALVINGS[nb]


@pytest.mark.parametrize("nb", BODIES)
def test_inputs_exercise_the_solve(cclqr, orc, nb):
    counts = _problem(cclqr, orc, nb)[6]
    halvings = _halvings(cclqr, orc, nb)
    print("%d bodies: largest Newton count per start %s, halvings per start %s" % (nb, counts.max(axis=1), halvings))
    for name, ids in CASES.items():
        assert max(counts[i].max() for i in ids) >= SEARCH_FROM, name + ": no step beyond iteration 3"
        assert sum(halvings[i] for i in ids) > 0, name + ": no step with a halved line search"


def _launcher(cclqr, t, cj, z0, ctrl_kw, nominal_plants=False):
    """run(steps_per_launch, flags) -> (final state, trajectory, multipliers, status) of STEPS steps from z0"""
    import torch
    capi = cclqr._capi
    mech = capi.MechHandle(t)
    ctrl = capi.CtrlHandle(mech, cj, **ctrl_kw)
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


NAMES = ("final state", "trajectory", "multipliers", "status")


def _check(cclqr, orc, nb, ids, nominal_plants=False, fric_noise=False):
    capi = cclqr._capi
    t, cj, K, zd, z0, (zT_o, traj_o, st_o), counts = _problem(cclqr, orc, nb)
    kw = dict(K=K, N=HORIZON, zd=zd, **_law_kw(t, fric_noise))
    if fric_noise:      # (the noise stream is keyed by the instance index: the reference of exactly these instances, in this order)
        zT_o, traj_o, st_o = orc.rollout(t, orc.ctrl_desc(t.nb, cj, **kw), z0[ids], STEPS, record=True)
        assert (st_o > 0).all(), st_o
    else:
        zT_o, traj_o, st_o = zT_o[ids], traj_o[ids], st_o[ids]
    mech, run = _launcher(cclqr, t, cj, np.array(z0[ids]), kw, nominal_plants)
    assert mech.geometry()[0] == 32 and mech.layout_links() == nb
    pack = capi.ROLLOUT_PACK_WAVEFRONTS
    fixed = run(STEPS, pack)
    runtime = run(STEPS, pack | capi.ROLLOUT_RUNTIME_PLAN)
    single = run(1, pack)
    single_rt = run(1, pack | capi.ROLLOUT_RUNTIME_PLAN)
    err_traj, err_final = np.abs(fixed[1] - traj_o).max(), np.abs(fixed[0] - zT_o).max()
    print("%d bodies, instances %s%s%s: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, largest Newton count %s (oracle %s)"
          % (nb, ids, ", per-instance plants" if nominal_plants else "", ", friction + noise" if fric_noise else "", err_traj, err_final, fixed[3], st_o))
    for name, f, r, s1, s2 in zip(NAMES, fixed, runtime, single, single_rt):
        assert np.array_equal(f, r), "fixed / run-time plan: " + name
        assert np.array_equal(f, s1), "one launch / single steps: " + name
        assert np.array_equal(s1, s2), "single steps, fixed / run-time plan: " + name
    assert (fixed[3] > 0).all()
    assert err_traj < TOL and err_final < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("nb", BODIES)
def test_fixed_plan_is_the_runtime_plan_bitwise(cclqr, orc, nb, case):
    _check(cclqr, orc, nb, CASES[case])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", BODIES)
def test_per_instance_plants_take_the_fixed_kernel(cclqr, orc, nb):
    _check(cclqr, orc, nb, [0, 1, 2], nominal_plants=True)


@pytest.mark.gpu
def test_friction_and_noise_law(cclqr, orc):
    _check(cclqr, orc, 17, [0, 1, 2], fric_noise=True)


def _two_chain_forest(cclqr):
    """17 bodies in two chains off the origin, 9 and 8 links (examples.tree_mechanism: random 1-DoF joints)"""
    parents = [-1] + list(range(8)) + [-1] + list(range(9, 16))
    return cclqr.examples.tree_mechanism(parents, seed=17, prismatic=(0, 9))


@pytest.mark.gpu
def test_a_forest_of_17_bodies_keeps_the_runtime_kernel(cclqr, orc):
    capi = cclqr._capi
    ex = _two_chain_forest(cclqr)
    t = ex["mech"].tables()
    steps = 20
    rng = np.random.default_rng(5)
    z0 = np.tile(ex["mech"].state(), (3, 1, 1))
    kw = dict(K=rng.normal(size=(steps + 5, 1, 12 * t.nb)) * 0.05, N=steps + 6, zd=z0[0], Fd=np.array([[0.3]]))
    mech = capi.MechHandle(t)
    assert mech.geometry()[0] == 32 and mech.layout_links() == 17
    ctrl = capi.CtrlHandle(mech, [0], **kw)
    a = capi.rollout(mech, ctrl, z0, steps, record=True)
    b = capi.rollout(mech, ctrl, z0, steps, record=True, flags=capi.ROLLOUT_RUNTIME_PLAN)
    assert (a[2] > 0).all(), a[2]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    zo, to, _ = orc.rollout(t, orc.ctrl_desc(t.nb, [0], **kw), z0, steps, record=True)
    err = max(np.abs(a[0] - zo).max(), np.abs(a[1] - to).max())
    print("two-chain forest of 17 bodies: max |state - oracle| = %.3g" % err)
    assert err < TOL
