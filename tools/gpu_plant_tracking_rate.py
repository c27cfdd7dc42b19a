"""diagnostic (not a test): what designing one TrackingLQR per PLANT costs -- the triple cartpole of BASELINE configs[4] (examples.triple_cartpole(), nb 4, mx 48),
N = 1000, plants PlantBatch.scaled(mass=(0.7, 1.3), length=(0.9, 1.1)), every plant's reference its OWN open-loop rollout of tests/golden/triple_cartpole_U.npy,
recorded by cclqr_rollout_plants and left on the device (the constructor reads it there: on_device = 1).
  (a) PlantTrackingLQR(mech, plants, traj_dev, U_dev, ...) for 64, 256 and 1024 plants: host clock around the constructor (it ends in a stream synchronise and the
      copy of the break indices); one warm-up, then the median of 5 (min .. max).  1024 plants once more with a 16 GiB workspace (4 x fewer, 4 x larger chunks).
  (b) the only route before it, on 16 plants, per plant: cclqr_linearize_plants on a table that repeats the plant N - 1 times, cclqr_riccati_tv, cclqr_ctrl_create
      (host pointers throughout: the models and the gains cross the bus twice).  The repeated-plant table and the trajectory's copy to the host are NOT timed.
      One warm-up plant, then all 16; reported per plant.
No ratio is promised anywhere; this prints what it measured.
python tools/gpu_plant_tracking_rate.py [out.txt] [N] [sizes, comma separated]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
sizes = [int(s) for s in sys.argv[3].split(",")] if len(sys.argv) > 3 else [64, 256, 1024]
NBASE = 16

ex = pkg.examples.triple_cartpole()
mech = ex["mech"]
t = mech.tables()
nb = t.nb
eids = [pkg.getid(ex["ctrl"][0])]
cj = [mech.joint_index(e) for e in eids]
U = np.load(os.path.join(g.ROOT, "tests", "golden", "triple_cartpole_U.npy")).reshape(-1, 1)
U = np.ascontiguousarray(np.resize(U, (N, 1)))
td = torch.device("cuda", torch.cuda.current_device())
mh = capi.MechHandle(t)
mech._cclqr_handle = mh
lines = ["triple cartpole (mx 48, mu 1), N = %d, plants mass x U(0.7, 1.3), length x U(0.9, 1.1); milliseconds" % N]


def record(plants, n):
    """every plant's own open-loop rollout from the hanging pose on its own manifold, on the device: (traj [n][N][nb][13], Fd [n][N][1], all converged)"""
    z0 = pkg.joint_position_states(mech, np.zeros((n, t.ne)), plants=plants)
    zd0 = np.zeros((N, nb, 13)); zd0[..., 3] = 1.0
    ol = capi.CtrlHandle(mh, cj, K=None, N=N + 1, zd=zd0, Fd=U)
    dz0, dzT = torch.from_numpy(z0).to(td), torch.empty((n, nb, 13), dtype=torch.float64, device=td)
    traj, st = torch.empty((n, N, nb, 13), dtype=torch.float64, device=td), torch.zeros(n, dtype=torch.int32, device=td)
    capi.rollout_dev(mh, ol, n, N, 1, dz0.data_ptr(), 0, 0, 0, traj.data_ptr(), dzT.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream, first_instance=0,
                     plants=plants.handle(mh))
    torch.cuda.synchronize()
    ol.close()
    return traj, torch.from_numpy(np.ascontiguousarray(np.broadcast_to(U[None], (n, N, 1)))).to(td), bool((st > 0).all().item())


def construct(plants, traj, Fd, **kw):
    t0 = time.perf_counter()
    ctl = pkg.PlantTrackingLQR(mech, plants, traj, Fd, eids, ex["Q"], ex["R"], **kw)
    dt = time.perf_counter() - t0
    kb = ctl.kbreak.copy()
    ctl.close()
    return dt, kb


for n in sizes:
    plants = pkg.PlantBatch.scaled(mech, n, mass=(0.7, 1.3), length=(0.9, 1.1), seed=1)
    traj, Fd, ok = record(plants, n)
    for label, kw in [("default workspace (4 GiB)", {})] + ([("16 GiB workspace", dict(workspace_bytes=16 << 30))] if n >= 512 else []):
        v = [construct(plants, traj, Fd, **kw) for _ in range(6)][1:]
        ts = [x[0] for x in v]
        lines.append("(a) %5d plants, %-26s %10.1f (%.1f .. %.1f)   %.2f per plant; open-loop references converged: %s; kbreak min %d max %d"
                     % (n, label, 1e3 * float(np.median(ts)), 1e3 * min(ts), 1e3 * max(ts), 1e3 * float(np.median(ts)) / n, ok, v[-1][1].min(), v[-1][1].max()))
        print(lines[-1], flush=True)
    del traj, Fd

plants = pkg.PlantBatch.scaled(mech, NBASE, mass=(0.7, 1.3), length=(0.9, 1.1), seed=1)
traj, Fd, ok = record(plants, NBASE)
zh, Q, R = traj.cpu().numpy(), np.array(pkg.lqr._blockdiag(ex["Q"])) * t.dt, np.array(pkg.lqr._blockdiag(ex["R"])) * t.dt
per = []
for i in [0] + list(range(NBASE)):          # the first pass over plant 0 is the warm-up
    rep = capi.PlantsHandle(mh, *[np.repeat(a[i:i + 1], N - 1, axis=0) for a in (plants.mass, plants.inertia, plants.p1, plants.p2)])
    t0 = time.perf_counter()
    lin = capi.linearize(mh, zh[i][:N - 1], cj, U[:N - 1], plants=rep)
    K, kb = capi.riccati_tv(*lin, Q, R, N)
    h = capi.CtrlHandle(mh, cj, K=K, N=N, zd=zh[i], Fd=U)
    per.append(time.perf_counter() - t0)
    h.close(); rep.close()
per = per[1:]
lines.append("(b) the single-problem route, %d plants one after the other: %.1f per plant (median; %.1f .. %.1f), %.1f in all"
             % (NBASE, 1e3 * float(np.median(per)), 1e3 * min(per), 1e3 * max(per), 1e3 * sum(per)))
print(lines[-1], flush=True)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
