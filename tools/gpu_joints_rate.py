"""diagnostic (not a test): what the joint coordinates of a rollout cost on the headline shape -- the 17-body chain, 8192 instances x 1000 steps, the horizon in
chunks of the default length into ONE slab.  Device events, one warm-up round, three alternating repeats of
  (a) the chunked recorded rollout alone,
  (b) the same with cclqr_rollout_joints behind every launch (continuous angles and rates into whole-horizon arrays [n][steps][ne]),
  (c) the same followed by cclqr_series_ensemble and cclqr_series_quantiles (five probabilities) over [n][steps][2 ne],
  (d) the joints launches alone on a resident slab,
  (e) the score launches alone on the same slab: the yardstick -- both read the slab once,
  (f) the two series calls alone,
and the joints kernel's bytes (from the shapes) over its time as a share of the HBM peak.
python tools/gpu_joints_rate.py [n_inst] [steps] [chunk_steps] [out.txt]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
HBM_PEAK = 8.0e12      # bytes/s, MI355X
links = 16
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)

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
jth, jrt, jcarry, x = f64(n, steps, ne), f64(n, steps, ne), f64(n, ne, 2), f64(n, steps, 2 * ne)
mean, m2, quant = f64(steps, 2 * ne), f64(steps, 2 * ne), f64(steps, len(PROBS), 2 * ne)
fin = torch.empty((steps, 2 * ne), dtype=torch.int32, device=dev)
wb = capi.series_ensemble_ws_bytes(n, steps, 2 * ne)
ws = f64(wb // 8 + 1)
qb = capi.series_quantiles_ws_bytes(n, steps, 2 * ne)[1] if n <= capi.QUANTILE_MAX_INST else 0
qws = f64(qb // 8 + 1)


def joints_launch(k0, s):
    capi.rollout_joints(mh, n, s, k0, slab.data_ptr(), capi.JOINTS_CONTINUOUS, steps, jth.data_ptr(), jrt.data_ptr(), jcarry.data_ptr(), stream)


def series():
    torch.cat((jth, jrt), dim=2, out=x)
    capi.series_ensemble(n, steps, 2 * ne, x.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), wb, stream)
    if qb:
        capi.series_quantiles(n, steps, 2 * ne, x.data_ptr(), PROBS, quant.data_ptr(), fin.data_ptr(), qws.data_ptr(), qb, stream)


def chunked(joints, stats=False):
    za.copy_(z0); lam.zero_(); st.zero_()
    z, zn = za, zb
    for k0, s in plan:
        capi.rollout_dev(mh, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0, 0, slab.data_ptr(), zn.data_ptr(), st.data_ptr(), stream, flags=capi.ROLLOUT_CARRY_STATUS)
        if joints:
            joints_launch(k0, s)
        z, zn = zn, z
    if stats:
        series()
    return z


def joints_alone():
    for k0, s in plan:
        joints_launch(k0, s)


def score_alone():
    for k0, s in plan:
        capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)


work = {"a chunked rollout": lambda: chunked(False), "b chunked rollout + joints": lambda: chunked(True), "c ... + joints + statistics": lambda: chunked(True, True),
        "d joints launches alone": joints_alone, "e score launches alone": score_alone, "f series statistics alone": series}
ms = {k: [] for k in work}
for rep in range(4):
    for k, f in work.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        torch.cuda.synchronize()
        if rep:
            ms[k].append(a.elapsed_time(b))
status = st.cpu().numpy()
lines = ["%d-body chain, %d instances x %d steps, %d launches of <= %d steps, slab %.1f MB, joint series %.2f GB (trajectory %.2f GB)"
         % (nb, n, steps, len(plan), chunk, slab.numel() * 8 / 1e6, 2 * jth.numel() * 8 / 1e9, n * steps * nb * 13 * 8 / 1e9)]
med = {k: float(np.median(v)) for k, v in ms.items()}
for k, v in ms.items():
    lines.append("%-30s median %9.3f ms   %s" % (k, med[k], [round(v_, 3) for v_ in v]))
lines.append("rate (a) %s, (b) %s, (c) %s" % tuple(capi.rate_or_refusal(n * steps, med[k] * 1e-3, status) for k in ("a chunked rollout", "b chunked rollout + joints",
                                                                                                                   "c ... + joints + statistics")))
per, per_score = med["d joints launches alone"] / len(plan), med["e score launches alone"] / len(plan)
byts = n * chunk * nb * 13 * 8 + 2 * n * chunk * ne * 8
lines.append("joints kernel: %.3f ms per slab = %.2f score passes (%.3f ms); %.1f MB per launch (slab read, theta and rate written) -> %.0f GB/s = %.1f %% of the %.0f TB/s HBM peak"
             % (per, per / per_score, per_score, byts / 1e6, byts / per / 1e6, 100 * byts / (per * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
lines.append("the joints pass adds %.1f %% to the chunked rollout, the joints pass and the statistics %.1f %%"
             % (100 * (med["b chunked rollout + joints"] / med["a chunked rollout"] - 1), 100 * (med["c ... + joints + statistics"] / med["a chunked rollout"] - 1)))
print("\n".join(lines), flush=True)
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    open(sys.argv[4], "w").write("\n".join(lines) + "\n")
