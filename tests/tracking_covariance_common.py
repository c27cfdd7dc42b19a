"""Shared by tests/test_tracking_covariance_reference.py (CPU) and tests/test_gpu_tracking_covariance.py: the cases of the tracking covariance
(cclqr_covariance_tracking) and their extended-precision references.

The recursion, restated.  Knots are j = 0 .. N-1, knot j being the state the law sees at step j + 1.  With (A_j, Bu_j, Bλ_j, G_j) the model of knot j and K_j its gain row
(lqr_tracking.jl:63-65, 88-89), the closed loop of the step is Abar_j = A_j - Bu_j K_j - Bλ_j Kλ_j with Kλ_j = (G_j Bλ_j)⁻¹ G_j (A_j - Bu_j K_j) (lqr_tracking.jl:107),
the noise enters through D_j = Bu_j - Bλ_j (G_j Bλ_j)⁻¹ G_j Bu_j, and
    Σ_0 = Sigma0 (or 0),   Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j'   j = 0 .. N-2
    cx_j = tr(Q Σ_j),  cu_j = tr(R K_j Σ_j K_j') (0 at j = N-1),  zvar_j = diag Σ_j,  uvar_j = diag(K_j Σ_j K_j') (0 at j = N-1),  total = (sum cx_j, sum cu_j).
nlin = 1 uses model 0 at every knot, nK = 1 gain row 0.

References, in np.longdouble on dlqr_reference.lu_solve, step this on the UNPROJECTED models as written above; they share no code with the product.  e64 of a problem
and horizon is the largest max|Σ64_j - Σref_j| / max|Σref_j| over the knots j < N of two float64 twins, the same stepping on the unprojected model and on the projected
pair [A' | D] (np.linalg.solve); the bound is dlqr_reference.tolerance(e64).  A horizon's Σ_j are the first N of the longest horizon's (the recursion does not look
ahead), so every (problem, sharing, variant) is stepped once.  The moments of a knot are held to covariance_common.check_moments: each cost entry within bound x
the larger magnitude sum, zstd² at its own scale |Σref_ii| under the twins' deviation on that entry (entries the twins do not reproduce: bound x max|Σref|), ustd²
within bound x its magnitude sum.  The deviation on entry i is, like e64, the largest over the horizon's knots: a coordinate keeps its conditioning along the
trajectory, a horizon holds N mx such entries per problem, and the two twins are two draws per entry -- knot by knot, ten times the larger of two draws is passed
by a third float64 evaluation on a few entries in a thousand (on the Sawyer's own linearisation, cond(G Bλ) = 4e4: entries 1.6e-8 of max|Σ| where the twins lie
2.0e-13 of the entry apart and their neighbours 1e-12 .. 3.6e-12), pooled over the knots it is not.  Only the TOLERANCE of an entry is pooled: whether the entry is held at its own scale at all is
decided knot by knot, by the twins' deviation at that knot; at the last knot cu and ustd are exact zeros.  total is held to bound x the sum of the knots' cost scales.  A knot whose reference
is exactly zero (Σ_0 without Sigma0) has no scale: the device must return exact zeros there.

A problem's models are dlqr_reference.make_problem(..., tv=True) (a base model with a knot-dependent perturbation), its gain table that problem's time-varying LQR
gains (any table would do: the gains are given); without inputs the same models from dlqr_reference._model and an empty table.  Wu, one Wu per problem and Sigma0
are dlqr_reference._spd.  Variants: full (Wu shared, Sigma0) on all four sharings nlin x nK; nostart (Wu, no Sigma0) and perprob (one Wu per problem, Sigma0) on
nlin = nK = N - 1; without inputs only full."""
import ctypes as C
import zlib

import numpy as np

import covariance_common as cc
import dlqr_reference as ref

LD = np.longdouble
CASES = ((12, 1, 5), (36, 1, 15), (48, 1, 20), (84, 7, 35), (96, 7, 0), (24, 0, 4), (30, 2, 6), (100, 3, 10))
NAMES = tuple("tc_%d_%d_%d" % c for c in CASES)
BY_NAME = dict(zip(NAMES, CASES))
NPROB = 3
SHARINGS = ((True, True), (True, False), (False, True), (False, False))      # (a model per knot?, a gain row per knot?)
THREADS, WAVES, TILES, PRE, PRE_S = 512, 8, 5, 18, 2


def horizons_of(name):
    return (1, 2, 3, 11) + ((38,) if name == NAMES[0] else ())


def resident_lds_bytes(mx, mu):
    return (2 * mx * mx + 2 * mu * mx + 2 * mu * mu + WAVES) * 8


def resident_fits(mx, mu):
    """mirror of ctk_resident_fits (csrc/covariance_tracking.hip)"""
    t16 = (mx + 15) // 16
    return mx % 4 == 0 and t16 * t16 <= TILES * WAVES and mx * mx <= PRE * THREADS and mu * mx <= PRE_S * THREADS and resident_lds_bytes(mx, mu) <= 158 * 1024


def paths_of(name):
    """the paths a case's shape has: 1 (resident) where it fits, and 2 (tiled) always"""
    mx, mu, _ = BY_NAME[name]
    return ((1,) if resident_fits(mx, mu) else ()) + (2,)


def closed_loop(A, Bu, Bl, G, K, dtype=LD, projected=False):
    """(Abar, D) of one knot; projected: through [A' | D] on np.linalg.solve (float64 only)"""
    A, Bu, Bl, G, K = (np.asarray(x, dtype=dtype) for x in (A, Bu, Bl, G, K))
    if not Bl.shape[1]:
        return A - Bu @ K, Bu
    if projected:
        X = np.linalg.solve(G @ Bl, G @ np.hstack([A, Bu]))
        Ap, D = A - Bl @ X[:, :A.shape[1]], Bu - Bl @ X[:, A.shape[1]:]
        return Ap - D @ K, D
    Acl = A - Bu @ K
    return Acl - Bl @ ref.lu_solve(G @ Bl, G @ Acl, dtype), Bu - Bl @ ref.lu_solve(G @ Bl, G @ Bu, dtype)


def step_tracking(A, Bu, Bl, G, K, Wu, S0, N, tvA, tvK, dtype=LD, projected=False):
    """[Σ_0 .. Σ_{N-1}] of one problem: A .. G [>= N-1][...], K [>= N-1][mu][mx]; tvA / tvK False: index 0 at every knot"""
    mx = np.shape(A)[-1]
    S = np.zeros((mx, mx), dtype=dtype) if S0 is None else np.asarray(S0, dtype=dtype)
    out = [S]
    for j in range(N - 1):
        a, k = (j if tvA else 0), (j if tvK else 0)
        Abar, D = closed_loop(A[a], Bu[a], Bl[a], G[a], K[k], dtype, projected)
        S = Abar @ S @ Abar.T + cc.noise(D, Wu, dtype)
        out.append(S)
    return out


def knot_moments(S, Q, R, K, last):
    """the record cc.check_moments takes, without e64 / zdev: at the last knot no gain acts (cu = 0, no ustd)"""
    Kk = np.zeros_like(np.asarray(K, dtype=LD)) if last else K
    cost, zvar, uvar, cmag, umag = cc.moments(S, Q, R, Kk)
    if last:
        uvar, umag = uvar[:0], umag[:0]
    return dict(S=S.astype(np.float64), cost=cost.astype(np.float64), cmag=cmag, zvar=zvar.astype(np.float64), uvar=uvar.astype(np.float64), umag=umag)


def reference_run(A, Bu, Bl, G, K, Wu, S0, N, tvA, tvK, what):
    """one problem stepped in longdouble and by the two float64 twins -> (Σref [N], per knot the twins' relative deviation, per knot and entry their deviation on the
    diagonal); asserts that every knot but a zero start has a scale and that the twins stay within 1e-9"""
    args = (A, Bu, Bl, G, K, Wu, S0, N, tvA, tvK)
    Sref = step_tracking(*args)
    twins = [step_tracking(*args, dtype=np.float64, projected=pj) for pj in (False, True)]
    d = []
    for j in range(N):
        scale = float(np.abs(Sref[j]).max())
        assert np.isfinite(scale) and (scale > 0.0 or (S0 is None and j == 0)), "knot %d of %s has no scale" % (j, what)
        d.append(max(float(np.abs(np.asarray(T[j], dtype=LD) - Sref[j]).max()) / scale for T in twins) if scale > 0.0 else 0.0)
    assert max(d) < 1e-9, "the float64 twins of %s lie %.3g apart from the reference" % (what, max(d))
    return Sref, d, [cc._zdev([T[j] for T in twins], Sref[j]) for j in range(N)]


def single_problem(A, Bu, Bl, G, K, Q, R, Wu, S0, N):
    """one problem of per-knot models and gains (A .. G [N-1][...], K [N-1][mu][mx]) as a case of its own: what records() and check_horizon() take, under the key
    ("full", True, True) and problem 0"""
    S, d, z = reference_run(A, Bu, Bl, G, K, Wu, S0, N, True, True, "the problem")
    return dict(Q=Q, R=R, K=np.asarray(K)[None], runs={("full", True, True): dict(Wu=Wu, Sigma0=S0, S=[S], dev=[d], zdev=[z])})


_built = {}


def build_case(name):
    """the problems of a case and their references, built once per session and left unchanged: dict with mx, mu, ml, nprob, nmax, horizons, paths, A, Bu, Bl, G
    [nprob][nmax-1][...], K [nprob][nmax-1][mu][mx], Q, R, Wu, WuP, Sigma0 and runs = {(variant, tvA, tvK): dict(Wu, Sigma0, S [nprob][nmax] longdouble,
    dev [nprob][nmax] relative twin deviation per knot, zdev [nprob][nmax][mx])}"""
    if name in _built:
        return _built[name]
    mx, mu, ml = BY_NAME[name]
    horizons = horizons_of(name)
    nmax = max(horizons)
    A, Bu, Bl, G, K = [], [], [], [], []
    Q = R = None
    for p in range(NPROB):
        rng = np.random.default_rng(zlib.crc32(("%s_%d" % (name, p)).encode()))
        if mu:
            pr = ref.make_problem(rng, mx, mu, ml, nprob=1, break_at="never", N=nmax, tv=True, Q=Q, R=R)
            Q, R = pr["Q"], pr["R"]
            mods, Kp = (pr["A"], pr["Bu"], pr["Bl"], pr["G"]), pr["ref"][0][0]
        else:
            base = ref._model(rng, mx, mu, ml)
            mods = tuple(np.stack([base[i] + (0.02 * rng.normal(size=base[i].shape) / np.sqrt(mx) if i in (0, 2) else 0.0) for _ in range(nmax - 1)]) for i in range(4))
            Kp = np.zeros((nmax - 1, 0, mx))
            if Q is None:
                Q, R = ref._spd(rng, mx), np.zeros((0, 0))
        assert Kp.shape == (nmax - 1, mu, mx) and np.isfinite(Kp).all() and all(np.isfinite(m).all() for m in mods)
        for lst, m in zip((A, Bu, Bl, G), mods):
            lst.append(m)
        K.append(Kp)
    A, Bu, Bl, G, K = (np.stack(x) for x in (A, Bu, Bl, G, K))
    rng = np.random.default_rng(zlib.crc32(("noise_" + name).encode()))
    Wu = ref._spd(rng, mu) if mu else None
    WuP = np.stack([ref._spd(rng, mu) for _ in range(NPROB)]) if mu else None
    Sigma0 = ref._spd(rng, mx)
    todo = [("full", Wu, Sigma0, s) for s in SHARINGS] + ([("nostart", Wu, None, SHARINGS[0]), ("perprob", WuP, Sigma0, SHARINGS[0])] if mu else [])
    runs = {}
    for vname, wu, s0, (tvA, tvK) in todo:
        S, dev, zdev = [], [], []
        for p in range(NPROB):
            wp = None if wu is None else (wu[p] if wu.ndim == 3 else wu)
            Sp, dp, zp = reference_run(A[p], Bu[p], Bl[p], G[p], K[p], wp, s0, nmax, tvA, tvK, "%s %s" % (name, vname))
            S.append(Sp)
            dev.append(dp)
            zdev.append(zp)
        runs[(vname, tvA, tvK)] = dict(Wu=wu, Sigma0=s0, S=S, dev=dev, zdev=zdev)
    _built[name] = dict(name=name, mx=mx, mu=mu, ml=ml, nprob=NPROB, nmax=nmax, horizons=horizons, paths=paths_of(name), A=A, Bu=Bu, Bl=Bl, G=G, K=K, Q=Q, R=R,
                        Wu=Wu, WuP=WuP, Sigma0=Sigma0, runs=runs)
    return _built[name]


def call_arrays(pr, N, tvA, tvK, sl=slice(None)):
    """(A, Bu, Bl, G, K) as cclqr_covariance_tracking takes them for horizon N: [n][nlin][...] and [n][nK][mu][mx]; N = 1 passes one model and one row (neither is read)"""
    na, nk = (max(N - 1, 1) if tvA else 1), (max(N - 1, 1) if tvK else 1)
    return tuple(np.ascontiguousarray(pr[k][sl, :na]) for k in ("A", "Bu", "Bl", "G")) + (np.ascontiguousarray(pr["K"][sl, :nk]),)


def records(pr, key, N, p):
    """per knot j < N of problem p the record of cc.check_moments (with e64 = the horizon's), and the horizon's e64"""
    run = pr["runs"][key]
    tvK = key[2]
    e64 = max(run["dev"][p][:N])
    zd = np.array(run["zdev"][p][:N])
    seen = np.isfinite(zd)
    zdev = np.where(seen.any(axis=0), np.max(np.where(seen, zd, 0.0), axis=0), np.inf)      # per entry, over the horizon's knots (the docstring above says why)
    out = []
    for j in range(N):
        r = knot_moments(run["S"][p][j], pr["Q"], pr["R"], pr["K"][p][j if tvK and j < N - 1 else 0], j == N - 1)      # (the last knot has no row: none acts there)
        knot_own = 10.0 * zd[j] <= 1e-7      # whether an entry has a scale of its own is decided at THIS knot (cc.check_moments' threshold); only its tolerance is pooled
        r.update(e64=e64, zdev=np.where(knot_own, np.minimum(zdev, 1e-8), zd[j]))
        out.append(r)
    return out, e64


def check_horizon(pr, key, N, p, Sigma, Sigma_all, cost, zstd, ustd, total, what):
    """the acceptance rule of one problem's outputs for horizon N; prints the figures before it asserts.  Sigma_all None (the controller entry returns the last knot's Σ
    only): the knots before the last are held through their moments"""
    recs, e64 = records(pr, key, N, p)
    bound = ref.tolerance(e64)
    worst, tscale = 0.0, 0.0
    for j, r in enumerate(recs):
        scale = float(np.abs(r["S"]).max())
        Sj = Sigma_all[j] if Sigma_all is not None else (Sigma if j == N - 1 else None)
        if scale == 0.0:      # Σ_0 without a start: exact zeros, and nothing derived from them but zeros
            assert (Sj is None or not Sj.any()) and not cost[j].any() and not zstd[j].any() and not ustd[j].any(), "%s knot %d: not exactly zero" % (what, j)
            continue
        if Sj is not None:
            err = float(np.abs(Sj - r["S"]).max()) / scale
            worst = max(worst, err)
            assert np.isfinite(Sj).all() and err <= bound, "%s knot %d: max|Σ - Σref| = %.3g relative, bound %.3g" % (what, j, err, bound)
            assert np.array_equal(zstd[j], np.sqrt(np.maximum(np.diag(Sj), 0.0))), "%s knot %d: zstd is not that of the returned Σ" % (what, j)
        cc.check_moments(cost[j], zstd[j], ustd[j][:len(r["uvar"])], r, "%s knot %d" % (what, j))
        tscale += r["cmag"]
    assert Sigma_all is None or np.array_equal(Sigma, Sigma_all[N - 1]), "%s: Sigma is not the last knot of Sigma_all" % what
    assert not cost[N - 1, 1] and not ustd[N - 1].any(), "%s: no input acts at the last knot" % what
    want = np.sum([r["cost"] for r in recs], axis=0)
    terr = float(np.abs(total - want).max())
    run = [0.0, 0.0]
    for j in range(N):
        run = [run[0] + cost[j, 0], run[1] + cost[j, 1]]
    print("%s: N = %d, e64 %.3g, bound %.3g, Σ off by at most %.3g relative over the knots, total %s (reference %s) off by %.3g of %.3g"
          % (what, N, e64, bound, worst, total, want, terr / tscale if tscale else 0.0, tscale))
    assert terr <= bound * tscale, "%s: total %s, reference %s" % (what, total, want)
    assert np.array_equal(total, np.array(run)), "%s: total is not the costs summed in knot order" % what


def refusal_call(capi, pr, N0):
    """cclqr_covariance_tracking through ctypes on sentinel-filled outputs, for tests/test_gpu_tracking_covariance.py and tests/test_analysis_refusals_host.py.  pr: nprob,
    mx, mu, ml, the arrays A, Bu, Bl, G [nprob][N0 - 1][...] and K [nprob][N0 - 1][mu][mx] of horizon N0 (call_arrays) and Q, R, Wu, Sigma0.  The call returns
    (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml = pr["nprob"], pr["mx"], pr["mu"], pr["ml"]
    dp = C.POINTER(C.c_double)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    A, Bu, Bl, G, K, Q, R, Wu, S0 = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "K", "Q", "R", "Wu", "Sigma0"))

    def call(nlin=N0 - 1, n_gains=n, nK=N0 - 1, n_weights=1, n_noise=1, N=N0, path=0, bf16=0, nprob=n, mx_=mx, mu_=mu, A_=A, K_=K, Bl_=Bl, Wu_=Wu, S0_=S0, Q_=Q, R_=R,
             cost_=True, total_=True):
        S, Sall = np.full((n, mx, mx), 7.5), np.full((n, N0, mx, mx), 7.5)
        cost, zs, us, tot = np.full((n, N0, 2), 7.5), np.full((n, N0, mx), 7.5), np.full((n, N0, mu), 7.5), np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_covariance_tracking(C.c_int32(nprob), C.c_int32(mx_), C.c_int32(mu_), C.c_int32(ml), C.c_int32(nlin), d(A_), d(Bu), d(Bl_), d(G), C.c_int32(n_gains),
                                         C.c_int32(nK), d(K_), C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), d(S0_), C.c_int32(N), d(S), d(Sall),
                                         d(cost) if cost_ else None, d(zs), d(us), d(tot) if total_ else None, C.byref(o))
        return rc, bool(all((x == 7.5).all() for x in (S, Sall, cost, zs, us, tot))), L.cclqr_last_error().decode()

    return call


def refusal_cases():
    """what cclqr_covariance_tracking refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (nprob must not be 2, N0 not 3)"""
    return dict(nprob_0=dict(nprob=0), mx_0=dict(mx_=0), N_0=dict(N=0), nlin_2=dict(nlin=2), nlin_0=dict(nlin=0), n_gains_2=dict(n_gains=2), nK_2=dict(nK=2),
                n_weights_2=dict(n_weights=2), n_weights_0=dict(n_weights=0), n_noise_2=dict(n_noise=2), n_noise_0=dict(n_noise=0), no_source=dict(Wu_=None, S0_=None),
                Wu_with_mu_0=dict(mu_=0), cost_without_Q=dict(Q_=None), total_without_R=dict(R_=None, cost_=False), A_null=dict(A_=None), K_null=dict(K_=None),
                Bl_null=dict(Bl_=None), path_3=dict(path=3), path_neg=dict(path=-1), bf16=dict(bf16=1), too_many=dict(nprob=65536, n_gains=1))
