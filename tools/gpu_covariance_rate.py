"""diagnostic (not a test): what the closed-loop covariance by doubling costs next to the cost-to-go by doubling of the same gain on the same models --
cclqr_covariance_doubling against cclqr_policy_value_doubling in the same library.  The mx^3 products, the launch shapes and the stop rules are the same kernels, so
the second call is the yardstick: what the covariance adds is its own setup (D Wu D', the trace, the scaled Σ0) and the moments.

Shapes: 1024 Sawyer-shaped problems (mx 84, mu 7, ml 35) and 4096 cartpole-shaped ones (mx 24, mu 1, ml 10): the seeded synthetic models of
tools/gpu_policy_doubling_rate.py, one model per problem, the Riccati's stationary gain of problem 0 shared by all; Wu = 1e-2 ones((mu, mu)) (one sample on every
input, as the rollout applies it), Σ0 = 1e-4 I for the fixed horizon.

Every number is CALL WALL TIME on the host clock around a call that ends in a device synchronise and the copy of its results (the covariance copies Σ and the four
moment arrays, the cost-to-go P).  Each shape: one warm-up call of each, then `reps` rounds that alternate the two calls over N knots and to convergence (N = 0, tol
1e-9: relative to tr W for the covariance, of max|P| for the cost-to-go), one line each; spread = (max - min) / median.

python tools/gpu_covariance_rate.py [--N 1001] [--reps 3] [--shapes sawyer,cartpole] [--out profiles/r21/covariance.txt]"""
import argparse, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1001)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="sawyer,cartpole")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "covariance.txt"))
a = ap.parse_args()
capi = g.load_package()._capi
SHAPES = dict(sawyer=(1024, 84, 7, 35), cartpole=(4096, 24, 1, 10))
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def models(rng, nprob, mx, mu, ml):
    A = rng.normal(size=(mx, mx)) / np.sqrt(mx)
    A *= 0.97 / np.abs(np.linalg.eigvals(A)).max()
    Bu = 2.0 * rng.normal(size=(mx, mu)) / np.sqrt(mx)
    Gr = np.linalg.qr(rng.normal(size=(mx, mx)))[0][:ml]
    Bl = Gr.T + 0.3 * rng.normal(size=(mx, ml)) / np.sqrt(mx)
    pert = lambda M: M[None] + 0.02 * rng.normal(size=(nprob,) + M.shape) / np.sqrt(mx)
    return pert(A), pert(Bu), pert(Bl), np.ascontiguousarray(np.broadcast_to(Gr, (nprob, ml, mx)))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


for name in a.shapes.split(","):
    nprob, mx, mu, ml = SHAPES[name]
    N = a.N
    M = models(np.random.default_rng(mx), nprob, mx, mu, ml)
    Q, R = np.eye(mx), np.eye(mu)
    K0 = capi.riccati(M[0][:1], M[1][:1], M[2][:1], M[3][:1], Q, R, 400, tol=0.0, keep_last=True)[0][0][0]      # [mu][mx]: the stationary gain of problem 0
    Wu, S0 = 1e-2 * np.ones((mu, mu)), 1e-4 * np.eye(mx)
    Pmax = np.abs(capi.policy_value_doubling(*M, K0, Q, R, N)[0]).max()
    calls = {("cov", N): lambda: capi.covariance_doubling(*M, K0, Q, R, Wu, S0, N),
             ("val", N): lambda: capi.policy_value_doubling(*M, K0, Q, R, N),
             ("cov", 0): lambda: capi.covariance_doubling(*M, K0, Q, R, Wu, None, 0, tol=1e-9),
             ("val", 0): lambda: capi.policy_value_doubling(*M, K0, Q, R, 0, tol=1e-9 * Pmax)}
    t = {k: [] for k in calls}
    for k in calls:
        calls[k]()
    for _ in range(a.reps):
        for k in calls:
            dt, out = timed(calls[k])
            assert np.isfinite(out[0]).all()
            t[k].append(dt)
            if k == ("cov", 0) and len(t[k]) == 1:
                say("%-8s covariance to convergence: levels %d .. %d, reasons %s, largest input std %.4g" % (name, out[4].min(), out[4].max(), sorted(set(out[5].tolist())),
                                                                                                            out[3].max() if mu else 0.0))
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in calls:
        say("%-8s %d x (mx %d, mu %d, ml %d)  %-28s %-15s call wall ms: %s  median %.2f  spread %.1f %%" % (
            name, nprob, mx, mu, ml, "cclqr_covariance_doubling" if k[0] == "cov" else "cclqr_policy_value_doubling", "N = %d" % k[1] if k[1] else "to convergence",
            " / ".join("%.2f" % (1e3 * x) for x in t[k]), 1e3 * med[k], 100 * (max(t[k]) - min(t[k])) / med[k]))
    for n in (N, 0):
        say("%-8s %s: covariance / cost-to-go = %.2f (%.2f ms against %.2f ms)" % (name, "N = %d" % n if n else "to convergence", med[("cov", n)] / med[("val", n)],
                                                                                 1e3 * med[("cov", n)], 1e3 * med[("val", n)]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
