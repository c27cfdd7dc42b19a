"""diagnostic (not a test): what a policy evaluation costs next to the Riccati recursion it shares its two mx^3 products with -- cclqr_policy_value against
cclqr_riccati_ex on the same models, the same N and tol = 0 (every backward step runs in both).

Shapes: 1024 Sawyer-shaped problems (mx 84, mu 7, ml 35) and 4096 cartpole-shaped ones (mx 24, mu 1, ml 10): seeded synthetic models (a stable A, G Bλ well conditioned),
one model per problem.  The gains evaluated are the Riccati's own table of problem 0, shared by all problems (n_gains = 1, nK = N - 1); the Riccati call keeps
only its last gain (keep_last), so that neither call moves a table per problem across the bus.

Every number is CALL WALL TIME on the host clock around a call that ends in a device synchronise and the copy of its results: the upload of the models (the same
bytes in both calls), the projection, the sweep, the download.  Each shape: one warm-up call of each, then `reps` rounds that alternate the two calls at N and at
N = 2 (one backward step: the calls' fixed cost), one line each; per-step time = (t(N) - t(2)) / (N - 2) from the medians, and the spread of each call = (max - min) /
median of its runs.  A policy step is a Riccati step minus the gain solve; whether that shows is what this reports.  Kernel times: a separate kernel-trace run.

python tools/gpu_policy_value_rate.py [--N 200] [--reps 3] [--shapes sawyer,cartpole] [--out FILE]"""
import argparse, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="sawyer,cartpole")
ap.add_argument("--out", default=None)
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
    K0 = capi.riccati(M[0][:1], M[1][:1], M[2][:1], M[3][:1], Q, R, N, tol=0.0)[0][0]      # the table evaluated: problem 0's own, [N-1][mu][mx]
    ric = lambda n: capi.riccati(*M, Q, R, n, tol=0.0, keep_last=True)
    pol = lambda n: capi.policy_value(*M, K0[:n - 1], Q, R, n, tol=0.0)
    ric(N); pol(N); ric(2); pol(2)
    t = {("ric", N): [], ("pol", N): [], ("ric", 2): [], ("pol", 2): []}
    for _ in range(a.reps):
        for n in (N, 2):
            dt, (_, kb) = timed(lambda: ric(n))
            assert (kb == (1 if n > 1 else 0)).all()
            t[("ric", n)].append(dt)
            dt, (P, kb, dn) = timed(lambda: pol(n))
            assert (kb == 1).all() and np.isfinite(P).all()
            t[("pol", n)].append(dt)
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    for k in (("ric", N), ("pol", N), ("ric", 2), ("pol", 2)):
        say("%-8s %d x (mx %d, mu %d, ml %d)  %-22s N = %-4d call wall ms: %s  median %.2f  spread %.1f %%" % (
            name, nprob, mx, mu, ml, "cclqr_riccati_ex" if k[0] == "ric" else "cclqr_policy_value", k[1], " / ".join("%.2f" % (1e3 * x) for x in t[k]), 1e3 * med[k],
            100 * spread[k]))
    step = {w: (med[(w, N)] - med[(w, 2)]) / (N - 2) for w in ("ric", "pol")}
    say("%-8s per backward step over the batch: Riccati %.1f us, policy %.1f us (policy / Riccati %.2f); whole call at N = %d: policy / Riccati %.2f, Riccati's own spread %.1f %%" % (
        name, 1e6 * step["ric"], 1e6 * step["pol"], step["pol"] / step["ric"], N, med[("pol", N)] / med[("ric", N)], 100 * spread[("ric", N)]))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
