"""diagnostic (not a test): what one (Q, R) per controller table costs the batched LQR constructor -- n Sawyer controllers (mx 84, mu 7, ml 35) at n distinct
setpoints, N knots, built in one call.  Every number is CONSTRUCTOR WALL TIME on the host clock around the call: the upload, the batched linearisation, the batched
Riccati recursion, the row permutation, the device synchronise and the copy of the break indices (kernel times: a separate kernel-trace run, never this one).

  shared    cclqr_ctrl_create_lqr_batch with one (Q, R): the path that existed before the weight stride.  Works on any checkout of the project (--tree DIR loads
            the package and its library from DIR), so that a job can alternate this build and its parent: one warm-up call, then `reps` timed calls, one line each.
  weights   this build: (1) n_weights = 1, (2) n_weights = n with the SAME pair replicated -- every table bitwise equal to (1)'s, so the difference is the weights' way
            to the kernels alone: the upload of n pairs and the per-problem fetch --, (3) n_weights = n with Q 10^(p mod 3): distinct problems, reported with the backward steps they executed.  One warm-up round, then
            `reps` rounds that alternate the three.

python tools/gpu_weight_sweep_rate.py shared|weights [--tree DIR] [--n 1024] [--N 200] [--reps 3] [--out FILE]"""
import argparse, importlib.util, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["shared", "weights"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--N", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
tree = os.path.abspath(a.tree)
spec = importlib.util.spec_from_file_location("graft_of_tree", os.path.join(tree, "__graft_entry__.py"))
g = importlib.util.module_from_spec(spec); spec.loader.exec_module(g)
pkg = g.load_package(); capi = pkg._capi
n, N = a.n, a.N

tab = json.load(open(os.path.join(tree, "tests", "golden", "sawyer_arm_tables.json")))
mech = pkg.examples.sawyer(tab)["mech"]
t = mech.tables()
mh = capi.MechHandle(t)
cj = list(range(7))
Q, R = np.eye(84) * 1000.0 * t.dt, np.eye(7) * t.dt
zd = pkg.joint_position_states(mech, np.random.default_rng(45).uniform(-0.8, 0.8, (n, 7)))
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def build(Qa, Ra, n_weights=None, keep=False):
    kw = {} if n_weights is None else dict(n_weights=n_weights)
    t0 = time.perf_counter()
    h = capi.BatchLqrHandle(mh, zd, cj, Qa, Ra, N, **kw)
    dt = time.perf_counter() - t0
    kb = h.kbreak.copy()
    if keep:
        return dt, kb, h
    h.close()
    return dt, kb, None


if a.mode == "shared":
    build(Q, R)
    ts = [build(Q, R)[0] for _ in range(a.reps)]
    say("shared  tree %s  %d Sawyer controllers, N = %d  constructor wall ms: %s  median %.3f" % (
        os.path.relpath(tree), n, N, " / ".join("%.3f" % (1e3 * x) for x in ts), 1e3 * float(np.median(ts))))
else:
    Qn, Rn = np.tile(Q[None], (n, 1, 1)), np.tile(R[None], (n, 1, 1))
    Qd = Qn * (10.0 ** (np.arange(n) % 3))[:, None, None]
    variants = [("1 n_weights = 1", Q, R, 1), ("2 n_weights = n, the same pair replicated", Qn, Rn, n), ("3 n_weights = n, Q 10^(p mod 3)", Qd, Rn, n)]
    # (2) is bitwise (1), table by table
    _, kb1, h1 = build(Q, R, 1, keep=True)
    _, kb2, h2 = build(Qn, Rn, n, keep=True)
    same = bool(np.array_equal(kb1, kb2)) and all(np.array_equal(capi.ctrl_gains(mh, h1, p), capi.ctrl_gains(mh, h2, p)) for p in range(n))
    h1.close(); h2.close()
    assert same, "the replicated pair does not give the shared pair's gains bit for bit"
    say("%d Sawyer controllers, N = %d, one call each; constructor wall time (linearisation included), milliseconds" % (n, N))
    say("gains and break indices of (2) bitwise those of (1), all %d tables: %s" % (n, same))
    times, kbs = {v[0]: [] for v in variants}, {}
    for rnd in range(a.reps + 1):      # round 0 warms every variant up
        for name, Qa, Ra, nw in variants:
            dt, kbs[name], _ = build(Qa, Ra, nw)
            if rnd:
                times[name].append(dt)
    for name, _, _, _ in variants:
        v, kb = times[name], kbs[name]
        say("%-45s %s  median %.3f   executed backward steps %d (kbreak %d .. %d)" % (
            name, " / ".join("%.3f" % (1e3 * x) for x in v), 1e3 * float(np.median(v)), int((N - np.maximum(kb, 1)).sum()), kb.min(), kb.max()))
    m = [float(np.median(times[v[0]])) for v in variants]
    say("(2) - (1), medians: %+.3f ms = %+.2f %%; run-to-run range of (1): %.3f ms" % (
        1e3 * (m[1] - m[0]), 100 * (m[1] - m[0]) / m[0], 1e3 * (max(times[variants[0][0]]) - min(times[variants[0][0]]))))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "a").write("\n".join(lines) + "\n")
