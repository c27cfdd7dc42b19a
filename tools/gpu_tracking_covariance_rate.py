"""diagnostic (not a test): what the tracking covariance costs next to policy evaluation with a full gain table on the same shapes and counts --
cclqr_covariance_tracking (a model AND a gain row per knot, the resident kernel) against cclqr_policy_value (one model per problem, a gain row per step) in the same
library, both on their resident kernels (path = 1).  Both make the same two mx^3 products per step on the fp64 matrix pipe; the first streams mx (mx + mu) more doubles per step from HBM and takes the per-knot
moments, the second is the yardstick.

Shapes: triple-cartpole-shaped problems (mx 48, mu 1, ml 20) and Sawyer-shaped ones (mx 84, mu 7, ml 35): seeded synthetic models, one base model per problem with a
knot-dependent perturbation, the Riccati's stationary gain of problem 0 perturbed per knot as the gain table; Wu = 1e-2 ones((mu, mu)), Σ0 = 1e-4 I.

Every number is CALL WALL TIME on the host clock around a call that ends in a device synchronise and the copy of its results, host arrays in and out: the tracking
call uploads N - 1 models per problem (the line "model upload" says how many bytes), the policy call one.  The per-knot models of `count` problems over `N` knots
must fit the host: 64 x 1001 knots is 2.2 GB at mx 48 and 6.9 GB at mx 84; larger batches belong to the controller entry, which linearises on the device in chunks.
Each shape and count: one warm-up call of each, then `reps` rounds that alternate the two, one line each; spread = (max - min) / median.

Part (b), the CONTROLLER entry on the triple cartpole of BASELINE configs[4] (examples.triple_cartpole(), mx 48, mu 1), plants PlantBatch.scaled(mass=(0.7, 1.3),
length=(0.9, 1.1)), every plant's reference its own open-loop rollout left on the device (the setup of tools/gpu_plant_tracking_rate.py): the whole-call time of
TrackingCovariance(mech, ctl, ...) next to the construction of the PlantTrackingLQR `ctl` it evaluates, `--plants` plants at a time; both read the device
trajectories in place, linearise N - 1 knots per plant on the device and run in chunks within the default workspace.  One warm-up of each, then `reps` of each.
Part (c): a device-to-device copy of 1 GiB timed with events, the copy bandwidth the model stream is set against.
KERNEL times are not taken here: run the tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/gpu_tracking_covariance_rate.py ...) and read
ctk_resident_kernel, policy_resident_kernel, ric_project_kernel and linearize_kernel off its statistics; part (a) also calls cclqr_policy_value on `--policy-count`
problems so that the trace holds the yardstick kernel at the large count.

python tools/gpu_tracking_covariance_rate.py [--N 1001] [--plants 64,1024] [--policy-count 1024] [--workspace-gib 0] [--counts 64] [--reps 3] [--shapes cartpole3,sawyer] [--out profiles/r22/tracking_covariance.txt]"""
import argparse, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1001)
ap.add_argument("--counts", default="64")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="cartpole3,sawyer")
ap.add_argument("--plants", default="64,1024")
ap.add_argument("--policy-count", type=int, default=1024)
ap.add_argument("--workspace-gib", type=int, default=0, help="part (b): workspace_bytes of both calls in GiB (0: the library default of 4)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "tracking_covariance.txt"))
a = ap.parse_args()
capi = g.load_package()._capi
SHAPES = dict(cartpole3=(48, 1, 20), sawyer=(84, 7, 35))
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def models(rng, nprob, nk, mx, mu, ml):
    """[nprob][nk][...]: a base model per problem, perturbed per knot"""
    A = rng.normal(size=(mx, mx)) / np.sqrt(mx)
    A *= 0.97 / np.abs(np.linalg.eigvals(A)).max()
    Bu = 2.0 * rng.normal(size=(mx, mu)) / np.sqrt(mx)
    Gr = np.linalg.qr(rng.normal(size=(mx, mx)))[0][:ml]
    Bl = Gr.T + 0.3 * rng.normal(size=(mx, ml)) / np.sqrt(mx)
    pert = lambda M: (M[None, None] + 0.02 * rng.standard_normal(size=(nprob, nk) + M.shape) / np.sqrt(mx))
    return pert(A), pert(Bu), pert(Bl), np.ascontiguousarray(np.broadcast_to(Gr, (nprob, nk, ml, mx)))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


for name in a.shapes.split(","):
    mx, mu, ml = SHAPES[name]
    N = a.N
    for nprob in [int(x) for x in a.counts.split(",")]:
        rng = np.random.default_rng(mx + nprob)
        M = models(rng, nprob, N - 1, mx, mu, ml)
        M0 = tuple(np.ascontiguousarray(x[:, 0]) for x in M)      # the time-invariant models of the policy call: knot 0 of every problem
        Q, R = np.eye(mx), np.eye(mu)
        K0 = capi.riccati(M0[0][:1], M0[1][:1], M0[2][:1], M0[3][:1], Q, R, 400, tol=0.0, keep_last=True)[0][0][0]      # [mu][mx]
        K = K0[None] * (1.0 + 0.01 * rng.standard_normal(size=(N - 1, 1, 1)))                                        # one table of N - 1 rows, shared
        Wu, S0 = 1e-2 * np.ones((mu, mu)), 1e-4 * np.eye(mx)
        up = sum(x.nbytes for x in M)
        calls = {"trk": lambda: capi.covariance_tracking(*M, K, Q, R, Wu, S0, N, path=1),
                 "pol": lambda: capi.policy_value(*M0, K, Q, R, N, tol=0.0, path=1)}
        t = {k: [] for k in calls}
        for k in calls:
            calls[k]()
        for _ in range(a.reps):
            for k in calls:
                dt, out = timed(calls[k])
                assert np.isfinite(out[0]).all()
                t[k].append(dt)
        med = {k: float(np.median(v)) for k, v in t.items()}
        say("%-9s %d x (mx %d, mu %d, ml %d), N = %d: model upload of the tracking call %.2f GB (%d doubles per problem-step)" % (name, nprob, mx, mu, ml, N, up / 1e9,
                                                                                                                              up // 8 // nprob // (N - 1)))
        for k, fn in (("trk", "cclqr_covariance_tracking"), ("pol", "cclqr_policy_value")):
            say("%-9s %d x N = %d  %-28s call wall ms: %s  median %.2f  spread %.1f %%  = %.3f us per problem-step" % (
                name, nprob, N, fn, " / ".join("%.2f" % (1e3 * x) for x in t[k]), 1e3 * med[k], 100 * (max(t[k]) - min(t[k])) / med[k],
                1e6 * med[k] / nprob / (N - 1)))
        say("%-9s %d x N = %d: tracking covariance / policy evaluation = %.2f (call wall, the first including its model upload)" % (name, nprob, N, med["trk"] / med["pol"]))
# ---- the yardstick kernel at the large count (for a kernel trace; its wall time is printed too)
for name in a.shapes.split(","):
    mx, mu, ml = SHAPES[name]
    nprob, N = a.policy_count, a.N
    if nprob < 1:
        continue
    rng = np.random.default_rng(mx + nprob)
    M0 = tuple(np.ascontiguousarray(x[:, 0]) for x in models(rng, nprob, 1, mx, mu, ml))
    Q, R = np.eye(mx), np.eye(mu)
    K = 0.01 * rng.standard_normal(size=(N - 1, mu, mx))
    capi.policy_value(*M0, K, Q, R, N, tol=0.0, path=1)
    ts = [timed(lambda: capi.policy_value(*M0, K, Q, R, N, tol=0.0, path=1))[0] for _ in range(a.reps)]
    say("%-9s %d x N = %d  cclqr_policy_value           call wall ms: %s  = %.3f us per problem-step" % (name, nprob, N, " / ".join("%.2f" % (1e3 * x) for x in ts),
                                                                                                      1e6 * float(np.median(ts)) / nprob / (N - 1)))

# ---- (b) the controller entry beside the constructor of the controller it evaluates
if a.plants:
    import torch
    pkg = g.load_package()
    ex = pkg.examples.triple_cartpole()
    mech = ex["mech"]
    tb = mech.tables()
    nb, N = tb.nb, a.N - 1 if a.N > 2 else a.N
    ids, eids = [pkg.getid(b) for b in mech.bodies], [pkg.getid(ex["ctrl"][0])]
    cj = [mech.joint_index(e) for e in eids]
    U = np.load(os.path.join(g.ROOT, "tests", "golden", "triple_cartpole_U.npy")).reshape(-1, 1)
    U = np.ascontiguousarray(np.resize(U, (N, 1)))
    td = torch.device("cuda", torch.cuda.current_device())
    mh = capi.MechHandle(tb)
    mech._cclqr_handle = mh
    for n in [int(x) for x in a.plants.split(",")]:
        plants = pkg.PlantBatch.scaled(mech, n, mass=(0.7, 1.3), length=(0.9, 1.1), seed=1)
        z0 = pkg.joint_position_states(mech, np.zeros((n, tb.ne)), plants=plants)
        zd0 = np.zeros((N, nb, 13)); zd0[..., 3] = 1.0
        ol = capi.CtrlHandle(mh, cj, K=None, N=N + 1, zd=zd0, Fd=U)
        dz0, dzT = torch.from_numpy(z0).to(td), torch.empty((n, nb, 13), dtype=torch.float64, device=td)
        traj, st = torch.empty((n, N, nb, 13), dtype=torch.float64, device=td), torch.zeros(n, dtype=torch.int32, device=td)
        capi.rollout_dev(mh, ol, n, N, 1, dz0.data_ptr(), 0, 0, 0, traj.data_ptr(), dzT.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream, first_instance=0,
                         plants=plants.handle(mh))
        torch.cuda.synchronize()
        ol.close()
        Fd = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(U[None], (n, N, 1)))).to(td)
        tc_, tv_ = [], []
        ctl = None
        for r in range(a.reps + 1):
            if ctl is not None:
                ctl.close()
            dt, ctl = timed(lambda: pkg.PlantTrackingLQR(mech, plants, traj, Fd, eids, ex["Q"], ex["R"], workspace_bytes=a.workspace_gib << 30))
            tc_.append(dt)
        for r in range(a.reps + 1):
            dt, cov = timed(lambda: pkg.TrackingCovariance(mech, ctl, ids, eids, ex["Q"], ex["R"], noise_scale=2.0, workspace_bytes=a.workspace_gib << 30))
            tv_.append(dt)
            fin = bool(np.isfinite(cov.state_std).all() and np.isfinite(cov.expected_score).all())
            top = float(cov.state_std.max())
            cov.close()
        ctl.close()
        tc_, tv_ = tc_[1:], tv_[1:]
        say("(b) workspace %s GiB, triple cartpole, %4d plants x N = %d, all references converged %s: PlantTrackingLQR construction wall ms %s; TrackingCovariance wall ms %s  = %.3f us per "
            "problem-step; ratio of the medians %.2f; finite %s, largest state std %.3g (noise_scale 2)" % (
                a.workspace_gib or 4, n, N, bool((st > 0).all().item()), " / ".join("%.1f" % (1e3 * x) for x in tc_), " / ".join("%.1f" % (1e3 * x) for x in tv_),
                1e6 * float(np.median(tv_)) / n / (N - 1), float(np.median(tv_)) / float(np.median(tc_)), fin, top))
        del traj, Fd
    # ---- (c) the copy bandwidth
    src, dst = torch.empty(1 << 27, dtype=torch.float64, device=td), torch.empty(1 << 27, dtype=torch.float64, device=td)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    say("(c) device-to-device copy of 1 GiB: %.3f ms = %.0f GB/s read + %.0f GB/s written" % (ms, (1 << 30) / ms / 1e6, (1 << 30) / ms / 1e6))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
