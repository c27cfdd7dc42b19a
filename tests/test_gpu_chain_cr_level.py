"""The ten fixed-plan chain kernels rollout_chain_fixed_kernel<16 | 17, law, relax> run the reduction level of the block-tridiagonal solve in a form of their
own (cclqr_chain.h cr_level_a / cr_level_b: columns of its own for each pass, no fence between a pass's arithmetic and its stores, z of pass B read back
from LDS) and gather the middle block with 64-bit DPP broadcasts (rollout_chain.hip ck_tri_mid_regs<true>).  Every change is a move, a reload of a value
just stored or a different store site, so the results must be the run-time-plan kernels' BIT FOR BIT -- those keep today's code, and
cclqr_rollout_opts.flags = CCLQR_ROLLOUT_RUNTIME_PLAN launches them on the same mechanism.  What can go wrong on the device and shows as different bits: z
re-read from a slot another lane's store has reached first, a column of pass B stored by a lane that sat the pass out, a broadcast that takes the wrong
lane's dword pair or leaves a lane of the row out, a lane of a `done` half taking part.

Inputs and the reference are those of tests/test_gpu_chain_half_swap.py (bench.py's recipe on chains of 17 and 16 bodies, 40 steps, the oracle's gains;
computed once, shared).  Shapes: 2 instances (one wavefront, both halves), 3 instances (a wavefront with an empty half), a start at the setpoint paired
with a far start in both orders (one half `done` while the other reduces).  Kernels: the plain law on all four shapes; the relaxed-stop kernel, the
friction + noise law with samples from the fill kernel (one launch), the same law with samples generated in the kernel (single-step launches) and the
LQR + PID law on one shape each -- so each of the ten fixed kernels runs.

Each case: final state, trajectory, status and multipliers bitwise equal between the default launch and the launch with ROLLOUT_RUNTIME_PLAN; trajectory
and final state within 1e-9 of the oracle under the same law (the relaxed stop is run with newton_eps_alone = 1e-300, where it never fires ahead of the
exact rule -- the oracle's rule -- while the launch still takes the <NBP, 0, true> kernel).

The inputs are checked first, on the CPU and against the oracle alone (test_inputs_exercise_the_solve runs in the CPU suite): every shape contains a step
whose Newton solve goes beyond iteration 3 and a step whose line search halved the step at least once; under every other law the oracle's largest Newton
count is beyond iteration 3 as well."""
import numpy as np
import pytest

from test_gpu_chain_fixed_plan import _halvings
from test_gpu_chain_half_swap import BODIES, HORIZON, SEARCH_FROM, STEPS, TOL, _problem

SHAPES = {"2 instances": [0, 1], "3 instances": [0, 1, 2], "setpoint + far": [3, 4], "far + setpoint": [4, 3]}
# law -> the shape it runs on (the plain law runs on all four)
LAW_SHAPE = {"relaxed stop": "setpoint + far", "friction + noise": "3 instances", "noise in kernel": "2 instances", "pid": "far + setpoint"}
KERNEL_OF = {"plain": (0, False), "relaxed stop": (0, True), "friction + noise": (1, False), "pid": (2, False), "noise in kernel": (3, False)}
GPU_CASES = [("plain", s) for s in SHAPES] + list(LAW_SHAPE.items())

_REF = {}


def _law_kw(orc, t, zd, law):
    """the controller's arguments beyond K, N, zd -- the same for the library's handle and the oracle's description"""
    if law in ("friction + noise", "noise in kernel"):
        return dict(fric=np.full(t.ne, 0.01), noise_scale=0.5, noise_seed=77)
    if law == "pid":      # a weak PID on the first pendulum joint about its coordinate at the setpoint, next to the LQR on the cart
        return dict(pid=dict(joint=[1], P=[0.4], I=[0.1], D=[0.02], goal=[float(orc.minimal_coordinates(t, zd)[1])]))
    return {}


def _reference(cclqr, orc, nb, law, ids):
    """the oracle's (final, trajectory, status) of instances `ids` under `law`: the shared plain-law reference, or a rollout made once per (chain, law) --
    the noise stream is keyed by the instance index, so that reference is of exactly these instances in this order"""
    t, cj, K, zd, z0, ref, counts = _problem(cclqr, orc, nb)
    if law in ("plain", "relaxed stop"):
        return tuple(a[ids] for a in ref)
    key = (nb, law, tuple(ids))
    if key not in _REF:
        out = orc.rollout(t, orc.ctrl_desc(t.nb, cj, K=K, N=HORIZON, zd=zd, **_law_kw(orc, t, zd, law)), z0[ids], STEPS, record=True)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def test_each_of_the_ten_fixed_kernels_has_a_case():
    """(law, relax) of the cases, each run on both chains: the five instantiations of either image"""
    assert sorted(BODIES) == [16, 17]
    assert {KERNEL_OF[law] for law, _ in GPU_CASES} == {(0, False), (0, True), (1, False), (2, False), (3, False)}
    assert {shape for _, shape in GPU_CASES} == set(SHAPES)


@pytest.mark.parametrize("nb", BODIES)
def test_inputs_exercise_the_solve(cclqr, orc, nb):
    counts = _problem(cclqr, orc, nb)[6]
    halvings = _halvings(cclqr, orc, nb)
    print("%d bodies: largest Newton count per start %s, halvings per start %s" % (nb, counts.max(axis=1), halvings))
    for name, ids in SHAPES.items():
        assert max(counts[i].max() for i in ids) >= SEARCH_FROM, name + ": no step beyond iteration 3"
        assert sum(halvings[i] for i in ids) > 0, name + ": no step with a halved line search"
    for law, shape in LAW_SHAPE.items():
        st = _reference(cclqr, orc, nb, law, SHAPES[shape])[2]
        print("%d bodies, %s on %s: the oracle's largest Newton counts %s" % (nb, law, shape, st))
        assert (st > 0).all() and st.max() >= SEARCH_FROM, law + ": no step beyond iteration 3"


def _run(cclqr, t, cj, ctrl_kw, z0, per_launch, flags, newton_mode, eps_alone):
    """(final state, trajectory, multipliers, status) of STEPS steps from z0, in one launch or in carried single-step launches"""
    import torch
    capi = cclqr._capi
    mech = capi.MechHandle(t)
    assert mech.geometry()[0] == 32 and mech.layout_links() == t.nb
    ctrl = capi.CtrlHandle(mech, cj, **ctrl_kw)
    dev = torch.device("cuda", 0)
    n = z0.shape[0]
    z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
    zn = torch.empty_like(z)
    lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
    s = torch.zeros(n, dtype=torch.int32, device=dev)
    opts = dict(first_instance=0, newton_mode=newton_mode, newton_eps_alone=eps_alone)
    if per_launch == STEPS:
        traj = torch.zeros((n, STEPS, t.nb, 13), dtype=torch.float64, device=dev)
        capi.rollout_dev(mech, ctrl, n, STEPS, 1, z.data_ptr(), lam.data_ptr(), 0, 0, traj.data_ptr(), zn.data_ptr(), s.data_ptr(), 0, flags=flags, **opts)
        z = zn
    else:
        rows = torch.zeros((STEPS, n, 1, t.nb, 13), dtype=torch.float64, device=dev)
        for k in range(1, STEPS + 1):
            capi.rollout_dev(mech, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, rows[k - 1].data_ptr(), zn.data_ptr(), s.data_ptr(), 0,
                             flags=flags | (capi.ROLLOUT_CARRY_STATUS if k > 1 else 0), **opts)
            z, zn = zn, z
        traj = rows[:, :, 0].permute(1, 0, 2, 3).contiguous()
    torch.cuda.synchronize()
    return z.cpu().numpy(), traj.cpu().numpy(), lam.cpu().numpy(), s.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("law,shape", GPU_CASES, ids=["%s, %s" % c for c in GPU_CASES])
@pytest.mark.parametrize("nb", BODIES)
def test_fixed_kernels_are_the_runtime_plan_kernels_bitwise(cclqr, orc, nb, law, shape):
    capi = cclqr._capi
    ids = SHAPES[shape]
    t, cj, K, zd, z0, _, _ = _problem(cclqr, orc, nb)
    zT_o, traj_o, st_o = _reference(cclqr, orc, nb, law, ids)
    kw = dict(K=K, N=HORIZON, zd=zd, **_law_kw(orc, t, zd, law))
    per_launch = 1 if law == "noise in kernel" else STEPS
    mode, eps = (1, 1e-300) if law == "relaxed stop" else (0, 0.0)
    pack = capi.ROLLOUT_PACK_WAVEFRONTS
    fixed = _run(cclqr, t, cj, kw, np.array(z0[ids]), per_launch, pack, mode, eps)
    runtime = _run(cclqr, t, cj, kw, np.array(z0[ids]), per_launch, pack | capi.ROLLOUT_RUNTIME_PLAN, mode, eps)
    err_traj, err_final = np.abs(fixed[1] - traj_o).max(), np.abs(fixed[0] - zT_o).max()
    print("%d bodies, %s, instances %s: max |trajectory - oracle| = %.3g, |final - oracle| = %.3g, largest Newton count %s (oracle %s)"
          % (nb, law, ids, err_traj, err_final, fixed[3], st_o))
    for name, f, r in zip(("final state", "trajectory", "multipliers", "status"), fixed, runtime):
        assert np.array_equal(f, r), "fixed / run-time plan: " + name
    assert (fixed[3] > 0).all()
    assert err_traj < TOL and err_final < TOL
