"""diagnostic (not a test): what designing one LQR per PLANT costs next to one LQR per setpoint -- 256 Sawyer controllers, N = 200 (the shape of
tests/test_gpu_fullsize.py::test_batched_lqr_constructor_keeps_the_gains_on_the_device), built in one call (1) by cclqr_ctrl_create_lqr_batch on the mechanism's
own plant, (2) by cclqr_ctrl_create_lqr_batch_plants on a table whose every row is the mechanism's own plant, (3) by the same on PlantBatch.scaled(mass=(0.7, 1.3),
length=(0.9, 1.1)) with every setpoint placed on its own plant.  Only the linearisation kernel's prologue differs between the three.  Host clock around the
call (it ends in a device synchronise and the copy of the break indices); one warm-up call each, then 5 rounds that alternate the three; median and range.
python tools/gpu_plant_lqr_rate.py [n] [N] [out.txt]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package(); capi = pkg._capi
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200

tab = json.load(open(os.path.join(g.ROOT, "tests", "golden", "sawyer_arm_tables.json")))
mech = pkg.examples.sawyer(tab)["mech"]
t = mech.tables()
mh = capi.MechHandle(t)
cj = list(range(7))
Q, R = np.eye(84) * 1000.0 * t.dt, np.eye(7) * t.dt
ang = np.random.default_rng(45).uniform(-0.8, 0.8, (n, 7))
tile = lambda a: np.tile(a[None], (n,) + (1,) * a.ndim)
nominal = pkg.PlantBatch(mech, mass=tile(t.mass), inertia=tile(t.inertia), p1=tile(t.p1), p2=tile(t.p2))
scaled = pkg.PlantBatch.scaled(mech, n, mass=(0.7, 1.3), length=(0.9, 1.1), seed=1)
zd_nom = pkg.joint_position_states(mech, ang)
variants = [("1 existing constructor, the mechanism's own plant", zd_nom, None),
            ("2 plants, every row the mechanism's own", zd_nom, capi.PlantsHandle(mh, nominal.mass, nominal.inertia, nominal.p1, nominal.p2)),
            ("3 plants, mass x U(0.7, 1.3), length x U(0.9, 1.1)", pkg.joint_position_states(mech, ang, plants=scaled),
             capi.PlantsHandle(mh, scaled.mass, scaled.inertia, scaled.p1, scaled.p2))]


def build(zd, ph):
    t0 = time.perf_counter()
    h = capi.BatchLqrHandle(mh, zd, cj, Q, R, N, plants=ph)
    dt = time.perf_counter() - t0
    kb = h.kbreak.copy()
    h.close()
    return dt, kb


times = {name: [] for name, _, _ in variants}
kbs = {}
for rnd in range(6):          # round 0 warms every variant up
    for name, zd, ph in variants:
        dt, kbs[name] = build(zd, ph)
        if rnd:
            times[name].append(dt)
lines = ["%d Sawyer controllers, N = %d, one call each; milliseconds, median of 5 (min .. max)" % (n, N)]
for name, _, _ in variants:
    v = times[name]
    lines.append("%-55s %.3f (%.3f .. %.3f)" % (name, 1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v)))
a, b = (times[variants[i][0]] for i in (0, 1))
lines.append("(2) - (1), medians: %+.3f ms; run-to-run range of (1): %.3f ms" % (1e3 * float(np.median(b) - np.median(a)), 1e3 * (max(a) - min(a))))
lines.append("break indices of (1) and (2) equal: %s" % bool(np.array_equal(kbs[variants[0][0]], kbs[variants[1][0]])))
print("\n".join(lines), flush=True)
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    open(sys.argv[3], "w").write("\n".join(lines) + "\n")
