"""diagnostic (not a test): what the ensemble statistics cost on the headline shape -- the 17-body chain, 8192 instances x 1000 steps, the horizon in chunks of the
default length (the largest slab under 1 GiB) into ONE slab.  Device events; one warm-up round, then `reps` alternating timed rounds of
  (a) the chunked recorded rollout alone,
  (b) the same with cclqr_rollout_score behind every launch,
  (c) the same with cclqr_rollout_ensemble (moments only) behind every launch,
  (d) the same with the moments plus one co-moment matrix (one cov_knot) per chunk,
  (e) the score launches alone on a resident slab,
  (f) the moments launches alone on the same slab,
  (g) the moments plus one co-moment matrix per slab alone,
with the median and the spread (min .. max) of every figure, the time per slab, the ensemble's share of the chunked run, the achieved bytes per second of the moments
pass (the slab read once plus the tile partials written and read, from the shapes) and the co-moment kernels' share of the fp64 MFMA peak (2 n 1024 FLOP per lower
32 x 32 tile, 28 tiles at mx = 204: what the tiles compute, the diagonal tiles in full).
python tools/gpu_ensemble_rate.py [n_inst] [steps] [chunk_steps] [reps] [out.txt]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
links = 16
chunk = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else capi.default_chunk_steps(n, links + 1, steps)
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
HBM_PEAK = 8.0e12       # bytes/s, MI355X
MFMA_PEAK = 78.6e12     # fp64 FLOP/s on the matrix cores, MI355X

ex = pkg.examples.cartpole_n(links)
mech = ex["mech"]
t = mech.tables()
nb = t.nb
mx, mu = 12 * nb, 1
nx = mx + mu
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
slab = torch.empty((n, chunk, nb, 13), dtype=torch.float64, device=dev)
za, zb = torch.empty_like(z0), torch.empty_like(z0)
lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
st = torch.zeros(n, dtype=torch.int32, device=dev)
sc = torch.zeros((n, 4), dtype=torch.float64, device=dev)
mean = torch.empty((steps, nx), dtype=torch.float64, device=dev)
m2 = torch.empty((steps, nx), dtype=torch.float64, device=dev)
cov = torch.empty((len(plan), mx, mx), dtype=torch.float64, device=dev)
ws_bytes = capi.rollout_ensemble_ws_bytes(mh, mu, n, chunk, 1)
ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)


def ensemble(ci, k0, s, with_cov):
    capi.rollout_ensemble(mh, ctrl, n, s, k0, slab.data_ptr(), mean[k0 - 1:].data_ptr(), m2[k0 - 1:].data_ptr(), ws.data_ptr(), ws_bytes,
                          cov_steps=[k0 + s // 2] if with_cov else [], cov_ptr=cov[ci:].data_ptr() if with_cov else 0, stream=stream)


def chunked(scored, ens, with_cov=False):
    za.copy_(z0); lam.zero_(); st.zero_()
    z, zn = za, zb
    for ci, (k0, s) in enumerate(plan):
        capi.rollout_dev(mh, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0, 0, slab.data_ptr(), zn.data_ptr(), st.data_ptr(), stream, flags=capi.ROLLOUT_CARRY_STATUS)
        if scored:
            capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)
        if ens:
            ensemble(ci, k0, s, with_cov)
        z, zn = zn, z
    return z


def score_alone():
    for k0, s in plan:
        capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)


def ensemble_alone(with_cov):
    for ci, (k0, s) in enumerate(plan):
        ensemble(ci, k0, s, with_cov)


work = {"a chunked rollout": lambda: chunked(False, False), "b chunked rollout + score": lambda: chunked(True, False),
        "c chunked rollout + moments": lambda: chunked(False, True), "d chunked rollout + moments + cov": lambda: chunked(False, True, True),
        "e score launches alone": score_alone, "f moments launches alone": lambda: ensemble_alone(False), "g moments + cov launches alone": lambda: ensemble_alone(True)}
ms = {k: [] for k in work}
for rep in range(reps + 1):      # round 0 warms every shape up
    for k, f in work.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        torch.cuda.synchronize()
        if rep:
            ms[k].append(a.elapsed_time(b))
status = st.cpu().numpy()
L = len(plan)
lines = ["%d-body chain, %d instances x %d steps, %d launches of <= %d steps, slab %.1f MB, %d timed rounds after one warm-up round"
         % (nb, n, steps, L, chunk, slab.numel() * 8 / 1e6, reps)]
med = {k: float(np.median(v)) for k, v in ms.items()}
for k, v in ms.items():
    lines.append("%-36s median %9.3f ms  (min %9.3f, max %9.3f)   per slab %8.3f ms" % (k, med[k], min(v), max(v), med[k] / L))
lines.append("rate (a) %s" % capi.rate_or_refusal(n * steps, med["a chunked rollout"] * 1e-3, status))
base = med["a chunked rollout"]
lines.append("per slab: rollout alone %.3f ms, with score %.3f ms, with moments %.3f ms, with moments and one co-moment matrix %.3f ms"
             % (base / L, med["b chunked rollout + score"] / L, med["c chunked rollout + moments"] / L, med["d chunked rollout + moments + cov"] / L))
lines.append("on the chunked rollout: score adds %.2f %%, moments add %.2f %%, moments + cov add %.2f %%"
             % tuple(100 * (med[k] / base - 1) for k in ("b chunked rollout + score", "c chunked rollout + moments", "d chunked rollout + moments + cov")))
per_s, per_m, per_c = med["e score launches alone"] / L, med["f moments launches alone"] / L, (med["g moments + cov launches alone"] - med["f moments launches alone"]) / L
tiles = (n + 63) // 64
byts = n * chunk * nb * 13 * 8 + 2 * chunk * tiles * 2 * nx * 8 + 2 * chunk * nx * 8
lines.append("moments pass alone: %.3f ms per slab = %.2f score passes (%.3f ms); %.1f MB per launch (slab once + tile partials written and read + results) -> %.0f GB/s = %.1f %% of the %.0f TB/s HBM peak"
             % (per_m, per_m / per_s, per_s, byts / 1e6, byts / per_m / 1e6, 100 * byts / (per_m * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
flop = 2.0 * n * 1024 * (((mx + 31) // 32) * (((mx + 31) // 32) + 1) // 2)
lines.append("one co-moment matrix (row copy inside the moments kernel + ens_cov_kernel + its finishing sum; g - f): %.3f ms at mx = %d, n = %d; %.2f GFLOP on the lower tiles -> %.2f TFLOP/s = %.1f %% of the fp64 MFMA peak"
             % (per_c, mx, n, flop / 1e9, flop / (per_c * 1e-3) / 1e12, 100 * flop / (per_c * 1e-3) / MFMA_PEAK))
print("\n".join(lines), flush=True)
if len(sys.argv) > 5:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[5])), exist_ok=True)
    open(sys.argv[5], "w").write("\n".join(lines) + "\n")
