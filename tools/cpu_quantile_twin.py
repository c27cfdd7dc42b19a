"""diagnostic (not a test, no GPU): the CPU twin of tests/test_gpu_quantiles.py::test_the_median_lies_where_a_gaussian_samples_median_lies.  chain3, N = 24, the
open-loop trajectory under U_k = 4 sin(2 pi k / 24), one tracking design (the oracle's gains, Q = 10 dt I, R = 0.1 dt), 2048 oracle rollouts from zd[0] under
input noise of scale 1e-3 with the Philox seed 1234; Σ_j by the longdouble recursion tracking_covariance_common.step_tracking on the oracle's linearisation at every
knot; mean and std over the instances in longdouble, the median by the numpy definition of tests/quantile_common.py.  Prints the entries compared and the largest
|median - mean| / (6 sqrt(pi/2 - 1) std / sqrt(n)).
python tools/cpu_quantile_twin.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
from oracle import orc
import ensemble_common as ec
import plants_common as pc
import quantile_common as qc
import tracking_covariance_common as tc
from plant_tracking_common import open_loop

cclqr = g.load_package()
N, N_INST, SIGMA, SEED = 24, 2048, 1e-3, 1234
BOUND = 6.0 * np.sqrt(np.pi / 2.0 - 1.0) / np.sqrt(N_INST)
mech, th0 = pc.mechanism_of(cclqr, ("chain", 2))
t = mech.tables()
nb, cj = t.nb, [0]
U = 4.0 * np.sin(2 * np.pi * np.arange(N) / N)[:, None]
zd = open_loop(orc, t, cj, U, cclqr.joint_position_states(mech, th0[None])[0])
Q, R = np.eye(12 * nb) * 10.0 * t.dt, np.eye(1) * 0.1 * t.dt
K, _ = orc.riccati_tracking(t, cj, zd, U, Q, R, N)
ctrl = orc.ctrl_desc(nb, cj, K=K, N=N, zd=zd, Fd=U, noise_scale=SIGMA, noise_seed=SEED)
zT, traj, st = orc.rollout(t, ctrl, np.tile(zd[0], (N_INST, 1, 1)), N, record=True)
assert (st > 0).all()
models = [orc.linearize(t, zd[j], cj, U[j]) for j in range(N - 1)]
S = tc.step_tracking(*(np.stack([m[i] for m in models]) for i in range(4)), K, np.eye(1) * SIGMA ** 2, None, N, True, True)
var = np.stack([np.diag(s).astype(np.float64) for s in S])
x, xm = ec.rows_of(traj, zd[None], K[None], N)
mean, M2, _, _ = ec.moments_of(x, xm)
mean, std = mean.astype(np.float64)[:, :12 * nb], np.sqrt(M2.astype(np.float64) / N_INST)[:, :12 * nb]
median = qc.quantiles_of(x, (0.5,))[0][:, 0, :12 * nb]
compared, worst, at = 0, 0.0, -1
for j in range(1, N):
    big = var[j] >= 1e-3 * var[j].max()
    ratio = np.abs(median[j, big] - mean[j, big]) / (BOUND * std[j, big])
    compared += int(big.sum())
    assert (ratio <= 1.0).all(), (j, ratio)
    if ratio.max() > worst:
        worst, at = float(ratio.max()), j
print("entries compared %d; largest |median - mean| / bound = %.4f at knot %d (bound = %.4f std); every entry inside the bound" % (compared, worst, at, BOUND))
