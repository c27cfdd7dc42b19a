"""diagnostic (not a test): what the tracking policy value costs next to its forward dual, the tracking covariance, on the same arrays -- cclqr_policy_value_tracking
against cclqr_covariance_tracking, and TrackingPolicyValue against TrackingCovariance.  Both recursions make the same two mx^3 products per step on the fp64 matrix
pipe and stream the same mx (mx + mu) doubles of model and mu mx of gain per step from HBM; the backward one adds the price pass (mu mx^2 multiply-adds before the
products) and reads Q in its epilogue, the forward one takes the per-knot moments.  The forward kernel is the yardstick; no ratio is fixed in advance.

Part (a), the CALLER entry, seeded synthetic problems (a base model per problem with a problem- and a knot-dependent perturbation, the Riccati's stationary gain of
problem 0 perturbed per knot as the shared gain table, Wu = 1e-2 ones((mu, mu)), Σ0 = 1e-4 I):
    sawyer     1024 problems, mx 84, mu 7, ml 35, N = 200      resident kernels (path 1)
    cartpole3    64 problems, mx 48, mu 1, ml 20, N = 1001     resident kernels (path 1)
    chain17       1 problem,  mx 204, mu 1, ml 85, N = 200     tiled (the only path of that shape)
Every number is CALL WALL TIME on the host clock around a call that ends in a device synchronise and the copy of its results, host arrays in and out; both calls
upload the same N - 1 models per problem (the line "model upload" says how many bytes: 1024 Sawyer problems x 199 knots are 22 GB of host memory).  One warm-up call
of each, then `reps` rounds that alternate the two; spread = (max - min) / median.
Part (b), the CONTROLLER entry on the triple cartpole of examples.triple_cartpole() (mx 48, mu 1), plants PlantBatch.scaled(mass=(0.7, 1.3), length=(0.9, 1.1)),
every plant's reference its own open-loop rollout left on the device (the setup of tools/gpu_tracking_covariance_rate.py): TrackingPolicyValue(mech, ctl, ...,
noise_scale=2) next to TrackingCovariance(mech, ctl, ..., noise_scale=2) on the same PlantTrackingLQR, `--plants` plants at a time, N = 1000.
KERNEL times are not taken here: run the tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/gpu_tracking_policy_rate.py ...) and read
ptk_resident_kernel beside ctk_resident_kernel, and the ptk_* step kernels beside the ctk_* ones, off its statistics.

The output ends with the kernel resources of policy_tracking.hip, compiled and parsed as the test suite does (--resources 0: not).  --cases "" / --plants "" skip a part.

python tools/gpu_tracking_policy_rate.py [--cases sawyer:1024:200,cartpole3:64:1001,chain17:1:200] [--plants 64,1024] [--N 1001] [--reps 3] [--resources 1] [--out profiles/r25/tracking_policy.txt]"""
import argparse, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="sawyer:1024:200,cartpole3:64:1001,chain17:1:200", help="shape:count:N, comma separated")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--plants", default="64,1024")
ap.add_argument("--resources", type=int, default=1, help="1: end with the kernel resources of policy_tracking.hip (a cross-compile, no GPU)")
ap.add_argument("--N", type=int, default=1001, help="part (b): knots + 1, as tools/gpu_tracking_covariance_rate.py counts them")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "tracking_policy.txt"))
a = ap.parse_args()
pkg = g.load_package()
capi = pkg._capi
SHAPES = dict(cartpole3=(48, 1, 20), sawyer=(84, 7, 35), chain17=(204, 1, 85))
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def models(rng, nprob, nk, mx, mu, ml):
    """[nprob][nk][...]: a base model, perturbed per problem and per knot (the sum of the two: 22 GB are written, not drawn)"""
    A = rng.normal(size=(mx, mx)) / np.sqrt(mx)
    A *= 0.97 / np.abs(np.linalg.eigvals(A)).max()
    Bu = 2.0 * rng.normal(size=(mx, mu)) / np.sqrt(mx)
    Gr = np.linalg.qr(rng.normal(size=(mx, mx)))[0][:ml]
    Bl = Gr.T + 0.3 * rng.normal(size=(mx, ml)) / np.sqrt(mx)

    def pert(M):
        out = np.empty((nprob, nk) + M.shape)
        np.add(M + 0.014 * rng.standard_normal(size=(nprob, 1) + M.shape) / np.sqrt(mx), 0.014 * rng.standard_normal(size=(1, nk) + M.shape) / np.sqrt(mx), out=out)
        return out
    return pert(A), pert(Bu), pert(Bl), np.ascontiguousarray(np.broadcast_to(Gr, (nprob, nk, ml, mx)))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


for case in [c for c in a.cases.split(",") if c]:
    name, nprob, N = case.split(":")
    nprob, N = int(nprob), int(N)
    mx, mu, ml = SHAPES[name]
    path = 1 if (mx % 4 == 0 and mx <= 96) else 2
    rng = np.random.default_rng(mx + nprob)
    M = models(rng, nprob, N - 1, mx, mu, ml)
    M0 = tuple(np.ascontiguousarray(x[:1, 0]) for x in M)
    Q, R = np.eye(mx), np.eye(mu)
    K0 = capi.riccati(*M0, Q, R, 400, tol=0.0, keep_last=True)[0][0][0]                                             # [mu][mx]
    K = K0[None] * (1.0 + 0.01 * rng.standard_normal(size=(N - 1, 1, 1)))                                            # one table of N - 1 rows, shared
    Wu, S0 = 1e-2 * np.ones((mu, mu)), 1e-4 * np.eye(mx)
    up = sum(x.nbytes for x in M)
    calls = {"pol": lambda: capi.policy_value_tracking(*M, K, Q, R, Wu, N, path=path),
             "cov": lambda: capi.covariance_tracking(*M, K, Q, R, Wu, S0, N, path=path)}
    t = {k: [] for k in calls}
    outs = {k: calls[k]() for k in calls}
    dual = float(np.sum(outs["pol"][0][0] * S0.T) + outs["pol"][3][0])
    for _ in range(a.reps):
        for k in calls:
            dt, out = timed(calls[k])
            assert np.isfinite(out[0]).all()
            t[k].append(dt)
    med = {k: float(np.median(v)) for k, v in t.items()}
    say("%-9s %d x (mx %d, mu %d, ml %d), N = %d, path %d: model upload of either call %.2f GB (%d doubles per problem-step); problem 0: tr(P_0 Σ_0) + noise_total = %.12g, "
        "covariance total %.12g" % (name, nprob, mx, mu, ml, N, path, up / 1e9, up // 8 // nprob // (N - 1), dual, float(outs["cov"][5][0].sum())))
    for k, fn in (("pol", "cclqr_policy_value_tracking"), ("cov", "cclqr_covariance_tracking")):
        say("%-9s %d x N = %d  %-28s call wall ms: %s  median %.2f  spread %.1f %%  = %.3f us per problem-step" % (
            name, nprob, N, fn, " / ".join("%.2f" % (1e3 * x) for x in t[k]), 1e3 * med[k], 100 * (max(t[k]) - min(t[k])) / med[k], 1e6 * med[k] / nprob / (N - 1)))
    say("%-9s %d x N = %d: tracking policy value / tracking covariance = %.2f (call wall, both including the same model upload)" % (name, nprob, N, med["pol"] / med["cov"]))
    del M, outs

# ---- (b) the controller entry beside its forward dual on the same controller
if a.plants:
    import torch
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
        ctl = pkg.PlantTrackingLQR(mech, plants, traj, Fd, eids, ex["Q"], ex["R"])
        tp_, tv_ = [], []
        for r in range(a.reps + 1):
            dt, v = timed(lambda: pkg.TrackingPolicyValue(mech, ctl, ids, eids, ex["Q"], ex["R"], noise_scale=2.0))
            tp_.append(dt)
            fin = bool(np.isfinite(v.noise_price).all() and np.isfinite(v.P(0)).all())
            ncost, worst = float(v.expected_noise_cost[0]), int(np.argmax(v.noise_price[0]))
            v.close()
            dt, cov = timed(lambda: pkg.TrackingCovariance(mech, ctl, ids, eids, ex["Q"], ex["R"], noise_scale=2.0))
            tv_.append(dt)
            escore = float(cov.expected_score[0].sum())
            cov.close()
        ctl.close()
        tp_, tv_ = tp_[1:], tv_[1:]
        say("(b) triple cartpole, %4d plants x N = %d, all references converged %s: TrackingPolicyValue wall ms %s  = %.3f us per problem-step; TrackingCovariance wall ms %s; "
            "ratio of the medians %.2f; finite %s; plant 0: expected_noise_cost %.9g against sum(expected_score) %.9g (no start covariance: equal), dearest knot %d (noise_scale 2)" % (
                n, N, bool((st > 0).all().item()), " / ".join("%.1f" % (1e3 * x) for x in tp_), 1e6 * float(np.median(tp_)) / n / (N - 1),
                " / ".join("%.1f" % (1e3 * x) for x in tv_), float(np.median(tp_)) / float(np.median(tv_)), fin, ncost, escore, worst))
        del traj, Fd
# ---- the kernel resources of policy_tracking.hip: the test suite's compile and parser (tests/build_common.py), no GPU needed
if a.resources:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from build_common import device_asm
    asm = device_asm("policy_tracking.hip")
    say("kernel resources of policy_tracking.hip (the code object's metadata): VGPRs, scratch bytes, scalar spills, vector spills")
    for kn in asm.kernel_names("_ZN5cclqr"):
        r = asm.kernel(kn).resources
        say("  %-60s vgpr %3d scratch %4d sgpr_spill %3d vgpr_spill %3d" % (kn, r["vgpr"], r["scratch"], r["sgpr_spill"], r["vgpr_spill"]))
    say("LDS of ptk_resident_kernel (ptk_resident_lds_bytes): %d B at (84, 7), %d B at (96, 7) of 163 840" % tuple(
        (2 * mx * mx + 2 * mu * mx + 2 * mu * mu + 8) * 8 for mx, mu in ((84, 7), (96, 7))))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
