"""diagnostic (not a test): what the Riccati doubling costs next to the stepped recursion over the same horizon -- cclqr_riccati_doubling against
cclqr_riccati_value (keep_last, tol = 0: every backward step runs) in the same library, on the same models.

Shapes: 1024 Sawyer-shaped problems (mx 84, mu 7, ml 35), 4096 cartpole-shaped ones (mx 24, mu 1, ml 10) and ONE problem of 204 states (mu 1, ml 85: the 17-body
chain's sizes): the seeded synthetic models of tools/gpu_policy_doubling_rate.py, one model per problem.

Every number is CALL WALL TIME on the host clock around a call that ends in a device synchronise and the copy of its results: the upload of the models (the same
bytes in both calls), the projection, the recursion or the compositions, the final step, the download of K and P.  Each shape: one warm-up call of each, then `reps`
rounds that alternate the two calls at N and at N = 2 (one backward step: the calls' fixed cost), one line each; the spread of a call = (max - min) / median of its
runs.  The doubling call counts as faster if the difference of the medians at N exceeds three times the stepping call's own spread (max - min).  Also printed: the
largest relative deviation between the two K and the two P, and one run to convergence (N = 0, tol = 1e-9 of max|P|).

python tools/gpu_riccati_doubling_rate.py [--N 1001] [--reps 3] [--shapes sawyer,cartpole,chain] [--out FILE]"""
import argparse, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1001)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="sawyer,cartpole,chain")
ap.add_argument("--out", default=None)
a = ap.parse_args()
capi = g.load_package()._capi
SHAPES = dict(sawyer=(1024, 84, 7, 35), cartpole=(4096, 24, 1, 10), chain=(1, 204, 1, 85))
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
    step = lambda n: capi.riccati_value(*M, Q, R, n, tol=0.0, keep_last=True)
    dbl = lambda n: capi.riccati_doubling(*M, Q, R, n)
    (Ks, Ps, _), (Kd, Pd, lv, rs, _, _) = step(N), dbl(N)
    step(2); dbl(2)
    say("%-8s %d x (mx %d, mu %d, ml %d)  N = %d: max|K doubling - K stepping| / max|K| = %.3g, max|P doubling - P stepping| / max|P| = %.3g, %d doublings" % (
        name, nprob, mx, mu, ml, N, np.abs(Kd - Ks[:, 0]).max() / np.abs(Ks).max(), np.abs(Pd - Ps).max() / np.abs(Ps).max(), lv.max()))
    t = {("step", N): [], ("dbl", N): [], ("step", 2): [], ("dbl", 2): []}
    for _ in range(a.reps):
        for n in (N, 2):
            dt, (K, P, kb) = timed(lambda: step(n))
            assert (kb == 1).all() and np.isfinite(P).all()
            t[("step", n)].append(dt)
            dt, (K, P, lv, rs, dn, an) = timed(lambda: dbl(n))
            assert np.isfinite(P).all() and (rs == 0).all()
            t[("dbl", n)].append(dt)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in (("step", N), ("dbl", N), ("step", 2), ("dbl", 2)):
        say("%-8s %d x (mx %d, mu %d, ml %d)  %-24s N = %-4d call wall ms: %s  median %.2f  spread %.1f %%" % (
            name, nprob, mx, mu, ml, "cclqr_riccati_value" if k[0] == "step" else "cclqr_riccati_doubling", k[1], " / ".join("%.2f" % (1e3 * x) for x in t[k]),
            1e3 * med[k], 100 * (max(t[k]) - min(t[k])) / med[k]))
    own = max(t[("step", N)]) - min(t[("step", N)])
    gain = med[("step", N)] - med[("dbl", N)]
    say("%-8s whole call at N = %d: stepping / doubling %.2f; beyond the fixed cost (N = 2): %.2f ms against %.2f ms; difference of the medians %.2f ms = %.1f x the stepping call's "
        "own spread of %.3f ms: doubling is %s" % (name, N, med[("step", N)] / med[("dbl", N)], 1e3 * (med[("step", N)] - med[("step", 2)]),
                                                 1e3 * (med[("dbl", N)] - med[("dbl", 2)]), 1e3 * gain, gain / own if own > 0 else float("inf"), 1e3 * own,
                                                 "FASTER" if gain > 3 * own else "NOT faster"))
    dt, (K, P, lv, rs, dn, an) = timed(lambda: capi.riccati_doubling(*M, Q, R, 0, tol=1e-9 * np.abs(Ps).max(), max_levels=40))
    say("%-8s to convergence (tol 1e-9 max|P|): %.2f ms, levels %d .. %d, reasons %s" % (name, 1e3 * dt, lv.min(), lv.max(), sorted(set(rs.tolist()))))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
