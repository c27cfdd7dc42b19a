"""diagnostic (not a test): what the cost-to-go costs, and what evaluating it yields.

  riccati   the batched Riccati of n Sawyer LQRs (mx 84, mu 7, ml 35; N knots, keep_last: 5 MB of gains come back instead of 1 GB) through the host-pointer
            entry point, HOST WALL TIME around the call: the upload of the models, the recursion, the device synchronise, the download.  Works on any checkout
            of the project (--tree DIR loads the package and its library from DIR), so that a job can alternate this build and its parent (A/B/A/B): one warm-up
            call, then `reps` timed calls.  On a build that has cclqr_riccati_value it also times that entry point with P = NULL and with P emitted, each in a
            block of its own.
  eval      cclqr_value_eval at n instances for the cartpole, the Sawyer and the 17-body chain shapes, with one shared P and with one P per instance: device time
            per launch from events around `reps` launches behind a warm-up, the median; the per-instance form as bytes of P per second.

python tools/gpu_value_rate.py riccati|eval [--tree DIR] [--n N] [--N 200] [--reps 20] [--out FILE]"""
import argparse, importlib.util, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["riccati", "eval"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--n", type=int, default=None)
ap.add_argument("--N", type=int, default=200)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()
tree = os.path.abspath(a.tree)
spec = importlib.util.spec_from_file_location("graft_of_tree", os.path.join(tree, "__graft_entry__.py"))
g = importlib.util.module_from_spec(spec); spec.loader.exec_module(g)
pkg = g.load_package(); capi = pkg._capi
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def fmt(ts):
    ts = 1e3 * np.asarray(ts)
    return "median %.3f  min %.3f  max %.3f ms (%d calls)" % (np.median(ts), ts.min(), ts.max(), ts.size)


def sawyer():
    tab = json.load(open(os.path.join(tree, "tests", "golden", "sawyer_arm_tables.json")))
    return pkg.examples.sawyer(tab)["mech"]


if a.mode == "riccati":
    n = a.n or 1024
    mech = sawyer()
    t = mech.tables()
    mh = capi.MechHandle(t)
    zd = pkg.joint_position_states(mech, np.random.default_rng(45).uniform(-0.05, 0.05, (n, 7)))
    A, Bu, Bl, G = capi.linearize(mh, zd, list(range(7)), np.zeros((n, 7)))
    Q, R = np.eye(84) * 1000.0 * t.dt, np.eye(7) * t.dt
    has_value = hasattr(capi, "riccati_value")
    variants = [("cclqr_riccati_ex", lambda: capi.riccati(A, Bu, Bl, G, Q, R, a.N, keep_last=True))]
    if has_value:
        variants += [("cclqr_riccati_value, P = NULL", lambda: capi.riccati_value(A, Bu, Bl, G, Q, R, a.N, keep_last=True, want_P=False)),
                     ("cclqr_riccati_value, P emitted", lambda: capi.riccati_value(A, Bu, Bl, G, Q, R, a.N, keep_last=True))]
    # one block of calls per variant, a warm-up call in front: a call that follows the 58 MB download of P reads its models from a host cache that download has
    # just emptied, and is 0.75 ms slower for it whatever it runs (seen when the variants alternated call by call)
    times = {v[0]: [] for v in variants}
    for name, call in variants:
        for rnd in range(a.reps + 1):
            t0 = time.perf_counter()
            call()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    say("tree %s: %d Sawyer problems, N = %d, keep_last; host wall time of the call" % (os.path.relpath(tree), n, a.N))
    for name, _ in variants:
        say("  %-34s %s" % (name, fmt(times[name])))
else:
    import torch
    n = a.n or 8192
    stream = torch.cuda.current_stream().cuda_stream
    say("cclqr_value_eval, %d instances, device time per launch (events around %d launches behind a warm-up of 3)" % (n, a.reps))
    for name, mech in (("cartpole", pkg.examples.cartpole_n(1)["mech"]), ("Sawyer", sawyer()), ("17-body chain", pkg.examples.cartpole_n(16)["mech"])):
        t = mech.tables()
        mh = capi.MechHandle(t)
        nb, mx = t.nb, 12 * t.nb
        rng = np.random.default_rng(nb)
        zd = np.zeros((nb, 13)); zd[:, 3] = 1.0
        ctrl1 = capi.CtrlHandle(mh, [0], zd=zd)
        ctrln = capi.CtrlHandle(mh, [0], zd=np.tile(zd, (n, 1, 1)), n_ctrl=n)
        z = zd[None] + 0.1 * rng.normal(size=(n, nb, 13))
        zt = torch.from_numpy(z).cuda()
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        H = rng.normal(size=(mx, mx))
        P1 = H @ H.T / mx
        for label, ctrl, nt in (("one shared P", ctrl1, 1), ("one P per instance", ctrln, n)):
            val = capi.ValueHandle(mh, np.broadcast_to(P1, (nt, mx, mx)))      # (n tables of the Sawyer are 462 MB)
            for _ in range(3):
                capi.value_eval(mh, ctrl, val, n, zt.data_ptr(), out.data_ptr(), stream)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                capi.value_eval(mh, ctrl, val, n, zt.data_ptr(), out.data_ptr(), stream)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            med = float(np.median(ts))
            rate = ""
            if nt > 1:
                rate = "  = %.3f TB/s of P (8 mx^2 = %d bytes per instance)" % (n * 8.0 * mx * mx / med / 1e12, 8 * mx * mx)
            say("  %-14s mx %3d  %-19s %s  %.3g instances/s%s" % (name, mx, label, fmt(ts), n / med, rate))
            val.close()
        ctrl1.close(); ctrln.close(); mh.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "a").write("\n".join(lines) + "\n")
