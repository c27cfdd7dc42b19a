"""diagnostic (not a test): what the ensemble quantiles cost on the headline shape -- the 17-body chain, 8192 instances x 1000 steps, the horizon in chunks of the
default length (the largest slab under 1 GiB) into ONE slab, the probabilities (0, 0.05, 0.5, 0.95, 1), the workspace of a whole chunk.  Device events; one warm-up
round, then `reps` alternating timed rounds of
  (a) the chunked recorded rollout alone,
  (b) the same with cclqr_rollout_ensemble (moments only) behind every launch,
  (c) the same with the moments and cclqr_rollout_quantiles behind every launch,
  (d) the moments launches alone on a resident slab,
  (e) the quantile launches alone on the same slab (ens_stage_kernel + ens_select_kernel),
  (f) the quantile launches alone with a workspace of ONE row (a launch pair per row),
with the median and the spread (min .. max) of every figure, the time per slab, the shares of the chunked run and the bytes the stage kernel moves.
The split of (e) between the two kernels is not visible to events around the call: run the tool with `only` as the sixth argument under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu_quantile_rate.py 8192 1000 0 5 out.txt only), which times ens_stage_kernel and ens_select_kernel apart.
python tools/gpu_quantile_rate.py [n_inst] [steps] [chunk_steps] [reps] [out.txt] [only]"""
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
only = len(sys.argv) > 6 and sys.argv[6] == "only"
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
HBM_PEAK = 8.0e12       # bytes/s, MI355X

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
rng = np.random.default_rng(0)
th = th0[None] + np.concatenate([rng.uniform(-0.5, 0.5, (n, 1)), rng.uniform(-0.2, 0.2, (n, links))], axis=1)
z0 = torch.from_numpy(np.ascontiguousarray(pkg.joint_position_states(mech, th))).to(dev)
plan = capi.chunk_plan(steps, chunk)
stream = torch.cuda.current_stream().cuda_stream
slab = torch.empty((n, chunk, nb, 13), dtype=torch.float64, device=dev)
za, zb = torch.empty_like(z0), torch.empty_like(z0)
lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
st = torch.zeros(n, dtype=torch.int32, device=dev)
mean = torch.empty((steps, nx), dtype=torch.float64, device=dev)
m2 = torch.empty((steps, nx), dtype=torch.float64, device=dev)
quant = torch.empty((steps, len(PROBS), nx), dtype=torch.float64, device=dev)
fin = torch.empty((steps, nx), dtype=torch.int32, device=dev)
ws_bytes = capi.rollout_ensemble_ws_bytes(mh, mu, n, chunk, 0)
ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
q_min, q_full = capi.rollout_quantiles_ws_bytes(mh, mu, n, chunk)
qws = torch.empty(q_full // 8 + 1, dtype=torch.float64, device=dev)


def moments(k0, s):
    capi.rollout_ensemble(mh, ctrl, n, s, k0, slab.data_ptr(), mean[k0 - 1:].data_ptr(), m2[k0 - 1:].data_ptr(), ws.data_ptr(), ws_bytes, stream=stream)


def quantiles(k0, s, wb):
    capi.rollout_quantiles(mh, ctrl, n, s, k0, slab.data_ptr(), PROBS, quant[k0 - 1:].data_ptr(), fin[k0 - 1:].data_ptr(), qws.data_ptr(), wb, stream=stream)


def chunked(ens, qnt):
    za.copy_(z0); lam.zero_(); st.zero_()
    z, zn = za, zb
    for k0, s in plan:
        capi.rollout_dev(mh, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0, 0, slab.data_ptr(), zn.data_ptr(), st.data_ptr(), stream, flags=capi.ROLLOUT_CARRY_STATUS)
        if ens:
            moments(k0, s)
        if qnt:
            quantiles(k0, s, q_full)
        z, zn = zn, z
    return z


def moments_alone():
    for k0, s in plan:
        moments(k0, s)


def quantiles_alone(wb):
    for k0, s in plan:
        quantiles(k0, s, wb)


work = {"a chunked rollout": lambda: chunked(False, False), "b chunked rollout + moments": lambda: chunked(True, False),
        "c chunked rollout + moments + quantiles": lambda: chunked(True, True), "d moments launches alone": moments_alone,
        "e quantile launches alone": lambda: quantiles_alone(q_full), "f quantile launches alone, one-row workspace": lambda: quantiles_alone(q_min)}
if only:      # (under a kernel trace: one filled slab, then the quantile launches and nothing else)
    chunked(False, False)
    work = {"e quantile launches alone": lambda: quantiles_alone(q_full)}
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
lines = ["%d-body chain, %d instances x %d steps, %d launches of <= %d steps, slab %.1f MB, quantile workspace %.1f MB (one row %.1f MB), %d probabilities, %d timed rounds after one warm-up round"
         % (nb, n, steps, L, chunk, slab.numel() * 8 / 1e6, q_full / 1e6, q_min / 1e6, len(PROBS), reps)]
med = {k: float(np.median(v)) for k, v in ms.items()}
for k, v in ms.items():
    lines.append("%-46s median %9.3f ms  (min %9.3f, max %9.3f)   per slab %8.3f ms" % (k, med[k], min(v), max(v), med[k] / L))
if not only:
    lines.append("rate (a) %s" % capi.rate_or_refusal(n * steps, med["a chunked rollout"] * 1e-3, status))
    base = med["a chunked rollout"]
    lines.append("per slab: rollout alone %.3f ms, with moments %.3f ms, with moments and quantiles %.3f ms"
                 % (base / L, med["b chunked rollout + moments"] / L, med["c chunked rollout + moments + quantiles"] / L))
    lines.append("on the chunked rollout: moments add %.2f %%, moments + quantiles add %.2f %%; the quantile pass alone is %.2f x the rollout of the same chunk, %.1f x the moments pass"
                 % (100 * (med["b chunked rollout + moments"] / base - 1), 100 * (med["c chunked rollout + moments + quantiles"] / base - 1),
                    med["e quantile launches alone"] / base, med["e quantile launches alone"] / med["d moments launches alone"]))
    byts = n * chunk * nb * 13 * 8 + chunk * nx * ((n + 63) // 64 * 64) * 8
    lines.append("stage kernel traffic per full slab: %.1f MB (slab read once + x written transposed); the select kernel reads the %.1f MB of x once"
                 % (byts / 1e6, chunk * nx * ((n + 63) // 64 * 64) * 8 / 1e6))
fq = fin.cpu().numpy()
lines.append("finite_count: min %d max %d of %d; lost instances %d" % (fq.min(), fq.max(), n, int((status <= 0).sum())))
print("\n".join(lines), flush=True)
if len(sys.argv) > 5 and sys.argv[5] != "-":
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[5])), exist_ok=True)
    open(sys.argv[5], "w").write("\n".join(lines) + "\n")
