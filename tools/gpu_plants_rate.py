"""diagnostic (not a test): what per-instance plants cost on the headline workload -- the 17-body chain, 8192 instances x 1000 steps, recorded, exact Newton rule --
with a +-20 % PlantBatch (masses and inertias per body, vertices per joint) against the SAME binary without plants, and with a PlantBatch whose every row is the
mechanism's own plant (the line search without lane lending and the prologue gather alone, on bitwise the same trajectories).  Starts are placed per plant.
python tools/gpu_plants_rate.py [n_inst] [steps] [out.json]"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
links = 16

ex = pkg.examples.cartpole_n(links)
mech = ex["mech"]
t = mech.tables()
nb = t.nb
th0 = np.zeros(nb); th0[1] = np.pi
zd = pkg.joint_position_states(mech, th0[None])[0]
lqr = pkg.LQR(mech, [pkg.getid(b) for b in ex["bodies"]], [pkg.getid(ex["ctrl"][0])], ex["Q"], ex["R"], steps * t.dt, xd=[zd[i, 0:3] for i in range(nb)], qd=[zd[i, 3:7] for i in range(nb)])
mh = mech._cclqr_handle
ctrl = lqr._ctrl_handle(mh)
rng = np.random.default_rng(0)
th = th0[None] + np.concatenate([rng.uniform(-0.5, 0.5, (n, 1)), rng.uniform(-0.2, 0.2, (n, links))], axis=1)
pb = pkg.PlantBatch.scaled(mech, n, mass=(0.8, 1.2), length=(0.8, 1.2), seed=1)
tile = lambda a: np.tile(a[None], (n,) + (1,) * a.ndim)
nominal = pkg.PlantBatch(mech, mass=tile(t.mass), inertia=tile(t.inertia), p1=tile(t.p1), p2=tile(t.p2))


def timed(z0, plants, reps=3):
    z = torch.from_numpy(np.ascontiguousarray(z0)).to(dev)
    zT, st = torch.empty_like(z), torch.zeros(n, dtype=torch.int32, device=dev)
    traj = torch.empty((n, steps, nb, 13), dtype=torch.float64, device=dev)
    ph = None if plants is None else plants.handle(mh)
    ms = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        capi.rollout_dev(mh, ctrl, n, steps, 1, z.data_ptr(), 0, 0, 0, traj.data_ptr(), zT.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream,
                         first_instance=0, plants=ph)
        b.record()
        torch.cuda.synchronize()
        if r:
            ms.append(a.elapsed_time(b))
    s = st.cpu().numpy()
    return dict(ms=[round(x, 2) for x in ms], median_ms=round(float(np.median(ms)), 2), rate=capi.rate_or_refusal(n * steps, np.median(ms) * 1e-3, s),
                newton_worst=int(s.max()), failed=int((s <= 0).sum())), zT.cpu().numpy()


out = {"workload": "%d-body chain, %d x %d, recorded" % (nb, n, steps)}
z_nom = pkg.joint_position_states(mech, th)
out["plain launch (no plants)"], zT0 = timed(z_nom, None)
out["plants, every row the mechanism's own"], zT1 = timed(z_nom, nominal)
out["nominal plants bitwise equal to the plain launch"] = bool(np.array_equal(zT0, zT1))
out["plants +-20 % mass / inertia / vertices"], _ = timed(pkg.joint_position_states(mech, th, plants=pb), pb)
for k, v in out.items():
    print(k, v, flush=True)
if len(sys.argv) > 3:          # the results as JSON as well
    json.dump(out, open(sys.argv[3], "w"), indent=1)
