"""Shared by tests/test_tracking_policy_reference.py, tests/test_tracking_policy_host.py (CPU) and tests/test_gpu_tracking_policy.py: the cases of the tracking
policy value (cclqr_policy_value_tracking) and their extended-precision references.

The recursion, restated.  Knots are j = 0 .. N-1 as in tests/tracking_covariance_common.py, whose cases and problems these are (CASES, build_case, closed_loop,
call_arrays, SHARINGS are imported from there).  With (Abar_j, D_j) = closed_loop(model of knot j, K_j):
    P_{N-1} = Q,   P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j   j = N-2 .. 0          (lqr_tracking.jl:107-108 with the gain given)
    price_j = tr(Wu D_j' P_{j+1} D_j)   j = 0 .. N-2,   price_{N-1} = 0,   noise_total = the prices summed from j = N-2 down to 0.
nlin = 1 uses model 0 at every knot, nK = 1 gain row 0.

References, in np.longdouble on dlqr_reference.lu_solve, step this on the UNPROJECTED models; they share no code with the product.  A backward recursion's shorter
horizons are not prefixes of the longest, so every (problem, sharing) is stepped once per horizon N in (1, 2, 3, 11), plus 38 on the first case.  e64 of a problem,
sharing and horizon is the largest max|P64_j - Pref_j| / max|Pref_j| over the knots of two float64 twins, the same stepping on the unprojected model and on the
projected pair [A' | D] (np.linalg.solve); the twins must agree with the reference to 1e-9, and the bound is dlqr_reference.tolerance(e64), the suite's own rule.
P_j is held to the bound relative to max|Pref_j|; price_j to bound x its magnitude sum  sum |Wu| .* (|D_j|' |P_{j+1}| |D_j|)';  noise_total to bound x the sum of
those.  The noise is the case's shared Wu (none without inputs: no price exists there)."""
import ctypes as C

import numpy as np

import dlqr_reference as ref
import tracking_covariance_common as tc
from tracking_covariance_common import BY_NAME, CASES, NAMES, NPROB, SHARINGS, build_case, call_arrays, closed_loop, horizons_of      # noqa: F401  (the cases ARE those)

LD = np.longdouble
THREADS, WAVES, TILES, PRE, PRE_S = 512, 8, 5, 18, 2


def resident_lds_bytes(mx, mu):
    """mirror of ptk_resident_lds_bytes (csrc/policy_tracking.hip)"""
    return (2 * mx * mx + 2 * mu * mx + 2 * mu * mu + WAVES) * 8


def resident_fits(mx, mu):
    """mirror of ptk_resident_fits (csrc/policy_tracking.hip)"""
    t16 = (mx + 15) // 16
    return mx % 4 == 0 and t16 * t16 <= TILES * WAVES and mx * mx <= PRE * THREADS and mu * mx <= PRE_S * THREADS and resident_lds_bytes(mx, mu) <= 158 * 1024


def paths_of(name):
    """the paths a case's shape has: 1 (resident) where it fits, and 2 (tiled) always"""
    mx, mu, _ = BY_NAME[name]
    return ((1,) if resident_fits(mx, mu) else ()) + (2,)


def step_policy(A, Bu, Bl, G, K, Q, R, Wu, N, tvA, tvK, dtype=LD, projected=False):
    """one problem -> (P [N] of [mx][mx], price [N], pmag [N]): A .. G [>= N-1][...], K [>= N-1][mu][mx]; tvA / tvK False: index 0 at every knot; Wu None: no price"""
    Q, R = np.asarray(Q, dtype=dtype), np.asarray(R, dtype=dtype)
    P = [None] * N
    price, pmag = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    P[N - 1] = Q
    for j in range(N - 2, -1, -1):
        a, k = (j if tvA else 0), (j if tvK else 0)
        Kj = np.asarray(K[k], dtype=dtype)
        Abar, D = closed_loop(A[a], Bu[a], Bl[a], G[a], Kj, dtype, projected)
        Pn = P[j + 1]
        if Wu is not None:
            W = np.asarray(Wu, dtype=dtype)
            price[j] = np.sum(W * (D.T @ Pn @ D).T)                                      # tr(Wu D' P D)
            pmag[j] = np.sum(np.abs(W) * (np.abs(D).T @ np.abs(Pn) @ np.abs(D)).T)
        P[j] = Q + Kj.T @ R @ Kj + Abar.T @ Pn @ Abar
    return P, price, pmag


_refs = {}


def reference(name, tvA, tvK, N):
    """the references of a case's problems for one sharing and horizon, built once per session and left unchanged: dict(P [nprob][N] longdouble, price [nprob][N],
    pmag [nprob][N], e64 [nprob]); asserts that every knot has a scale and that the twins stay within 1e-9"""
    key = (name, tvA, tvK, N)
    if key in _refs:
        return _refs[key]
    pr = build_case(name)
    out = dict(P=[], price=[], pmag=[], e64=[])
    for p in range(pr["nprob"]):
        one = single_reference(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["K"][p], pr["Q"], pr["R"], pr["Wu"], N, tvA, tvK, "%s problem %d" % (key, p))
        for k in out:
            out[k].append(one[k][0])
    _refs[key] = out
    return out


def single_reference(A, Bu, Bl, G, K, Q, R, Wu, N, tvA=True, tvK=True, what="the problem"):
    """one problem stepped in longdouble and by the two float64 twins, as a reference() of one problem (index 0): what check_horizon takes"""
    args = (A, Bu, Bl, G, K, Q, R, Wu, N, tvA, tvK)
    P, price, pmag = step_policy(*args)
    twins = [step_policy(*args, dtype=np.float64, projected=pj)[0] for pj in (False, True)]
    e64 = 0.0
    for j in range(N):
        scale = float(np.abs(P[j]).max())
        assert np.isfinite(scale) and scale > 0.0, "knot %d of %s has no scale" % (j, what)
        e64 = max(e64, max(float(np.abs(np.asarray(T[j], dtype=LD) - P[j]).max()) / scale for T in twins))
    assert e64 < 1e-9, "the float64 twins of %s lie %.3g apart from the reference" % (what, e64)
    return dict(P=[P], price=[price], pmag=[pmag], e64=[e64])


def check_horizon(r, p, N, P, P_all, price, total, what, Q=None):
    """the acceptance rule of one problem's outputs; prints the figures before it asserts.  P_all, price, total may be None (not asked for, or no noise)"""
    e64 = r["e64"][p]
    bound = ref.tolerance(e64)
    worst = 0.0
    for j in range(N):
        Pj = P_all[j] if P_all is not None else (P if j == 0 else None)
        if Pj is None:
            continue
        Pref = r["P"][p][j]
        err = float(np.abs(Pj - Pref).max() / np.abs(Pref).max())
        worst = max(worst, err)
        assert np.isfinite(Pj).all() and err <= bound, "%s knot %d: max|P - Pref| = %.3g relative, bound %.3g" % (what, j, err, bound)
    perr = terr = 0.0
    tmag = float(np.sum(r["pmag"][p]))
    if price is not None:
        for j in range(N):
            d, m = float(abs(price[j] - r["price"][p][j])), float(r["pmag"][p][j])
            perr = max(perr, d / m if m else 0.0)
            assert d <= bound * m, "%s knot %d: price %.17g, reference %.17g, magnitude sum %.3g, bound %.3g" % (what, j, price[j], float(r["price"][p][j]), m, bound)
        assert price[N - 1] == 0.0, "%s: no noise is priced at the last knot" % what
    if total is not None:
        want = float(np.sum(r["price"][p]))
        terr = abs(float(total) - want)
        assert terr <= bound * tmag, "%s: noise_total %.17g, reference %.17g" % (what, float(total), want)
        if price is not None:
            run = 0.0
            for j in range(N - 2, -1, -1):
                run = run + price[j]
            assert total == run, "%s: noise_total is not the prices summed from N - 2 down" % what
    print("%s: N = %d, e64 %.3g, bound %.3g, P off by at most %.3g relative over the knots, price by %.3g of its magnitude sum, noise_total by %.3g of %.3g"
          % (what, N, e64, bound, worst, perr, terr / tmag if tmag else 0.0, tmag))
    if P_all is not None:
        assert np.array_equal(P, P_all[0]), "%s: P is not knot 0 of P_all" % what
        if Q is not None:
            assert np.array_equal(P_all[N - 1], Q), "%s: P_all[N - 1] is not Q" % what
    return bound


def refusal_call(capi, pr, N0):
    """cclqr_policy_value_tracking through ctypes on sentinel-filled outputs, for tests/test_gpu_tracking_policy.py and tests/test_analysis_refusals_host.py.  pr: nprob,
    mx, mu, ml, the arrays A, Bu, Bl, G [nprob][N0 - 1][...] and K [nprob][N0 - 1][mu][mx] of horizon N0 (call_arrays) and Q, R, Wu.  The call returns
    (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml = pr["nprob"], pr["mx"], pr["mu"], pr["ml"]
    dp = C.POINTER(C.c_double)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    A, Bu, Bl, G, K, Q, R, Wu = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "K", "Q", "R", "Wu"))

    def call(nlin=N0 - 1, n_gains=n, nK=N0 - 1, n_weights=1, n_noise=1, N=N0, path=0, bf16=0, nprob=n, mx_=mx, mu_=mu, A_=A, K_=K, Bl_=Bl, Wu_=Wu, Q_=Q, R_=R,
             price_=True, total_=True):
        P, Pall, price, tot = np.full((n, mx, mx), 7.5), np.full((n, N0, mx, mx), 7.5), np.full((n, N0), 7.5), np.full(n, 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_policy_value_tracking(C.c_int32(nprob), C.c_int32(mx_), C.c_int32(mu_), C.c_int32(ml), C.c_int32(nlin), d(A_), d(Bu), d(Bl_), d(G), C.c_int32(n_gains),
                                           C.c_int32(nK), d(K_), C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), C.c_int32(N), d(P), d(Pall),
                                           d(price) if price_ else None, d(tot) if total_ else None, C.byref(o))
        return rc, bool(all((x == 7.5).all() for x in (P, Pall, price, tot))), L.cclqr_last_error().decode()

    return call


def refusal_cases():
    """what cclqr_policy_value_tracking refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (nprob must not be 2, N0 not 3)"""
    return dict(nprob_0=dict(nprob=0), mx_0=dict(mx_=0), N_0=dict(N=0), nlin_2=dict(nlin=2), nlin_0=dict(nlin=0), n_gains_2=dict(n_gains=2), nK_2=dict(nK=2),
                n_weights_2=dict(n_weights=2), n_weights_0=dict(n_weights=0), n_noise_2=dict(n_noise=2), n_noise_0=dict(n_noise=0),
                price_without_Wu=dict(Wu_=None, total_=False), total_without_Wu=dict(Wu_=None, price_=False), Wu_with_mu_0=dict(mu_=0), without_Q=dict(Q_=None),
                without_R=dict(R_=None), A_null=dict(A_=None), K_null=dict(K_=None), Bl_null=dict(Bl_=None), path_3=dict(path=3), path_neg=dict(path=-1),
                bf16=dict(bf16=1), too_many=dict(nprob=65536, n_gains=1))
