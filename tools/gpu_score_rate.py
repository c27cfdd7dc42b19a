"""diagnostic (not a test): what scoring a rollout on the device costs on the headline shape -- the 17-body chain, 8192 instances x 1000 steps, horizon in chunks of 50
steps into ONE slab (cclqr_rollout_ex + cclqr_rollout_score per chunk).  Device events, one warm-up round, three alternating repeats of
  (a) the chunked recorded rollout alone,
  (b) the same with cclqr_rollout_score behind every launch,
  (c) a device-to-device copy of one slab (this box's bandwidth yardstick),
  (d) the way without the score: a one-launch recorded rollout plus the copy of its trajectory to the host (staged through one page-locked slab-sized buffer),
  (e) the score launches alone on a resident slab,
and the score kernel's bytes (from the shapes) over its time as a share of the HBM peak.
python tools/gpu_score_rate.py [n_inst] [steps] [chunk_steps] [out.txt]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import torch
pkg = g.load_package(); capi = pkg._capi
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 50
HBM_PEAK = 8.0e12      # bytes/s, MI355X
links = 16

ex = pkg.examples.cartpole_n(links)
mech = ex["mech"]
t = mech.tables()
nb = t.nb
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
slab2 = torch.empty_like(slab)
za, zb = torch.empty_like(z0), torch.empty_like(z0)
lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=dev)
st = torch.zeros(n, dtype=torch.int32, device=dev)
sc = torch.zeros((n, 4), dtype=torch.float64, device=dev)
full = torch.empty((n, steps, nb, 13), dtype=torch.float64, device=dev)
pinned = torch.empty(slab.numel(), dtype=torch.float64, pin_memory=True)


def chunked(scored):
    za.copy_(z0); lam.zero_(); st.zero_()
    z, zn = za, zb
    for k0, s in plan:
        capi.rollout_dev(mh, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0, 0, slab.data_ptr(), zn.data_ptr(), st.data_ptr(), stream, flags=capi.ROLLOUT_CARRY_STATUS)
        if scored:
            capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)
        z, zn = zn, z
    return z


def one_launch_and_copy():
    capi.rollout_dev(mh, ctrl, n, steps, 1, z0.data_ptr(), 0, 0, 0, full.data_ptr(), zb.data_ptr(), st.data_ptr(), stream)
    flat = full.reshape(-1)
    for o in range(0, flat.numel(), pinned.numel()):
        m = min(pinned.numel(), flat.numel() - o)
        pinned[:m].copy_(flat[o:o + m], non_blocking=True)


def score_alone():
    for k0, s in plan:
        capi.rollout_score(mh, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream)


work = {"a chunked rollout": lambda: chunked(False), "b chunked rollout + score": lambda: chunked(True), "c one slab copy d2d": lambda: slab2.copy_(slab),
        "d one launch + copy to host": one_launch_and_copy, "e score launches alone": score_alone}
ms = {k: [] for k in work}
for rep in range(4):
    for k, f in work.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        torch.cuda.synchronize()
        if rep:
            ms[k].append(a.elapsed_time(b))
zT_scored = chunked(True).cpu().numpy(); s_chunked = sc.cpu().numpy(); status = st.cpu().numpy()
capi.rollout_dev(mh, ctrl, n, steps, 1, z0.data_ptr(), 0, 0, 0, full.data_ptr(), zb.data_ptr(), st.data_ptr(), stream)
capi.rollout_score(mh, ctrl, score, n, steps, 1, full.data_ptr(), sc.data_ptr(), stream)
torch.cuda.synchronize()
lines = ["%d-body chain, %d instances x %d steps, %d launches of <= %d steps, slab %.1f MB (trajectory %.2f GB)" % (nb, n, steps, len(plan), chunk, slab.numel() * 8 / 1e6,
                                                                                                                full.numel() * 8 / 1e9)]
med = {k: float(np.median(v)) for k, v in ms.items()}
for k, v in ms.items():
    lines.append("%-28s median %9.3f ms   %s" % (k, med[k], [round(x, 3) for x in v]))
lines.append("rate (a) %s, (b) %s, (d) %s" % tuple(capi.rate_or_refusal(n * steps, med[k] * 1e-3, status) for k in ("a chunked rollout", "b chunked rollout + score", "d one launch + copy to host")))
per = med["e score launches alone"] / len(plan)
byts = n * chunk * nb * 13 * 8 + n * 4 * 8 * 2
lines.append("score kernel: %.3f ms per slab = %.2f slab copies; %.1f MB read per launch (slab + scores; gain and setpoint rows stay in cache) -> %.0f GB/s = %.1f %% of the %.0f TB/s HBM peak"
             % (per, per / med["c one slab copy d2d"], byts / 1e6, byts / per / 1e6, 100 * byts / (per * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
lines.append("scoring adds %.1f %% to the chunked rollout" % (100 * (med["b chunked rollout + score"] / med["a chunked rollout"] - 1)))
lines.append("chunked + scored final states bitwise equal to one launch: %s; chunked score bitwise equal to the one-call score of the recorded trajectory: %s"
             % (bool(np.array_equal(zT_scored, zb.cpu().numpy())), bool(np.array_equal(s_chunked, sc.cpu().numpy()))))
lines.append("score of instance 0: Jx %.6g Ju %.6g peak %.6g last_out %d" % tuple(s_chunked[0][:3].tolist() + [int(s_chunked[0][3])]))
print("\n".join(lines), flush=True)
if len(sys.argv) > 4:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[4])), exist_ok=True)
    open(sys.argv[4], "w").write("\n".join(lines) + "\n")
