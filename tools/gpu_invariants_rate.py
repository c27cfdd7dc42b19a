"""diagnostic (not a test): what the integrator's invariants of a rollout cost on the headline shape -- the 17-body chain, 8192 instances x 1000 steps, the horizon in
chunks of the default length into ONE slab.  Device events, one warm-up round, then `repeats` alternating rounds in one process of
  (a) the chunked recorded rollout alone,
  (b) the same with cclqr_rollout_invariants behind every launch (series [n][steps][6] and the summary [n][8]),
  (c) the invariants launches alone on a resident slab, series and summary,
  (d) the same with the raw rows [n][chunk][ne][5] as well (into a chunk-sized buffer: the whole-horizon array would not fit beside the slab),
  (e) the joints launches alone on the same slab: THE YARDSTICK -- the same read traffic and launch shape, 2 ne doubles written per row where (c) writes 6,
  (f) the score launches alone on the same slab,
and the pass's bytes (from the shapes) over its time as a share of the HBM peak.  The run-to-run spread of (c) and (e) is the largest distance of a repeat from
its median; (c) is expected not to exceed (e) by more than that.
python tools/gpu_invariants_rate.py [n_inst] [steps] [chunk_steps] [out.txt] [repeats]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 5
HBM_PEAK = 8.0e12      # bytes/s, MI355X
links = 16

ex = pkg.examples.cartpole_n(links)
mech = ex["mech"]
t = mech.tables()
nb, ne = t.nb, t.ne
chunk = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else capi.default_chunk_steps(n, nb, steps)
th0 = np.zeros(nb); th0[1] = np.pi
zd = pkg.joint_position_states(mech, th0[None])[0]
ids, eq = [pkg.getid(b) for b in ex["bodies"]], [pkg.getid(ex["ctrl"][0])]
lqr = pkg.LQR(mech, ids, eq, ex["Q"], ex["R"], steps * t.dt, xd=[zd[i, 0:3] for i in range(nb)], qd=[zd[i, 3:7] for i in range(nb)])
mh = mech._cclqr_handle
ctrl = lqr._ctrl_handle(mh)
score = pkg.Score(mech, ids, eq, ex["Q"], ex["R"], settle_tol=1e-4)._handle(mh)
rng = np.random.default_rng(0)
th = th0[None] + np.concatenate([rng.uniform(-0.5, 0.5, (n, 1)), rng.uniform(-0.2, 0.2, (n, links))], axis=1)
z0 = torch.from_numpy(np.ascontiguousarray(pkg.joint_position_states(mech, th))).to(dev)
plan = capi.chunk_plan(steps, chunk)
stream = torch.cuda.current_stream().cuda_stream
f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
slab = f64(n, chunk, nb, 13)
za, zb = torch.empty_like(z0), torch.empty_like(z0)
lam = torch.zeros((n, 5 * ne), dtype=torch.float64, device=dev)
st = torch.zeros(n, dtype=torch.int32, device=dev)
sc = torch.zeros((n, 4), dtype=torch.float64, device=dev)
inv, summ, grow = f64(n, steps, capi.INVARIANTS_LEN), f64(n, capi.INVARIANTS_SUMMARY_LEN), f64(n, chunk, ne, 5)
jth, jrt, jcarry = f64(n, steps, ne), f64(n, steps, ne), f64(n, ne, 2)


def invariants_launch(k0, s, rows=False):
    if rows:      # (the rows of a chunk at the head of a chunk-sized buffer: k0 = 1 there, the summary not carried)
        capi.rollout_invariants(mh, n, s, 1, slab.data_ptr(), chunk, inv.data_ptr() if chunk <= steps else 0, grow.data_ptr(), summ.data_ptr(), stream)
    else:
        capi.rollout_invariants(mh, n, s, k0, slab.data_ptr(), steps, inv.data_ptr(), 0, summ.data_ptr(), stream)


def chunked(with_invariants):
    za.copy_(z0); lam.zero_(); st.zero_()
    z, zn = za, zb
    for k0, s in plan:
        capi.rollout_dev(mh, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0, 0, slab.data_ptr(), zn.data_ptr(), st.data_ptr(), stream, flags=capi.ROLLOUT_CARRY_STATUS)
        if with_invariants:
            invariants_launch(k0, s)
        z, zn = zn, z
    return z


def invariants_alone(rows=False):
    for k0, s in plan:
        invariants_launch(k0, s, rows)


def joints_alone():
    for k0, s in plan:
        capi.rollout_joints(mh, n, s, k0, slab.data_ptr(), capi.JOINTS_CONTINUOUS, steps, jth.data_ptr(), jrt.data_ptr(), jcarry.data_ptr(), stream)


def score_alone():
    for k0, s in plan:
        capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)


work = {"a chunked rollout": lambda: chunked(False), "b chunked rollout + invariants": lambda: chunked(True), "c invariants launches alone": invariants_alone,
        "d invariants + raw rows alone": lambda: invariants_alone(True), "e joints launches alone": joints_alone, "f score launches alone": score_alone}
ms = {k: [] for k in work}
for rep in range(repeats + 1):
    for k, f in work.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        torch.cuda.synchronize()
        if rep:
            ms[k].append(a.elapsed_time(b))
status = st.cpu().numpy()
lines = ["%d-body chain, %d instances x %d steps, %d launches of <= %d steps, slab %.1f MB, invariant series %.3f GB (trajectory %.2f GB), %d repeats after one warm-up"
         % (nb, n, steps, len(plan), chunk, slab.numel() * 8 / 1e6, inv.numel() * 8 / 1e9, n * steps * nb * 13 * 8 / 1e9, repeats)]
med = {k: float(np.median(v)) for k, v in ms.items()}
spread = {k: float(np.max(np.abs(np.asarray(v) - med[k]))) for k, v in ms.items()}
for k, v in ms.items():
    lines.append("%-32s median %9.3f ms  spread %7.3f ms   %s" % (k, med[k], spread[k], [round(v_, 3) for v_ in v]))
lines.append("rate (a) %s, (b) %s" % tuple(capi.rate_or_refusal(n * steps, med[k] * 1e-3, status) for k in ("a chunked rollout", "b chunked rollout + invariants")))
L = len(plan)
per = {k: med[k] / L for k in med}
read = n * chunk * nb * 13 * 8
b_series, b_rows, b_joints = read + n * chunk * 6 * 8, read + n * chunk * (6 + 5 * ne) * 8, read + 2 * n * chunk * ne * 8
share = lambda byts, ms_: (byts / 1e6, byts / ms_ / 1e6, 100 * byts / (ms_ * 1e-3) / HBM_PEAK)
lines.append("invariants pass, series + summary: %.3f ms per slab; %.1f MB per launch -> %.0f GB/s = %.1f %% of the HBM peak" % ((per["c invariants launches alone"],) + share(b_series, per["c invariants launches alone"])))
lines.append("invariants pass with the raw rows:  %.3f ms per slab; %.1f MB per launch -> %.0f GB/s = %.1f %% of the HBM peak" % ((per["d invariants + raw rows alone"],) + share(b_rows, per["d invariants + raw rows alone"])))
lines.append("joints pass (the yardstick):        %.3f ms per slab; %.1f MB per launch -> %.0f GB/s = %.1f %% of the HBM peak" % ((per["e joints launches alone"],) + share(b_joints, per["e joints launches alone"])))
lines.append("score pass:                         %.3f ms per slab" % per["f score launches alone"])
diff, tol = med["c invariants launches alone"] - med["e joints launches alone"], spread["c invariants launches alone"] + spread["e joints launches alone"]
lines.append("invariants - joints = %+.3f ms over %d launches; run-to-run spread of the two %.3f ms: the invariants pass is %s" %
             (diff, L, tol, "within the spread of the joints pass or faster" if diff <= tol else "SLOWER than the joints pass by more than the spread"))
lines.append("the invariants pass adds %.1f %% to the chunked rollout" % (100 * (med["b chunked rollout + invariants"] / med["a chunked rollout"] - 1)))
print("\n".join(lines), flush=True)
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    open(sys.argv[4], "w").write("\n".join(lines) + "\n")
