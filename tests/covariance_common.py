"""Shared by tests/test_covariance_reference.py (CPU) and tests/test_gpu_covariance.py: the cases of the closed-loop covariance by doubling
(cclqr_covariance_doubling) and their extended-precision references.

The covariance, restated.  With the one gain K (LQR{T,Inf}, lqr.jl:40-43) the closed loop is Δz⁺ = Abar Δz + D w with Abar = A - Bu K - Bλ Kλ (lqr.jl:169),
D = Bu - Bλ (G Bλ)⁻¹ G Bu and w ~ (0, Wu), so after n steps from a start of covariance Σ0
    Σ_n = C(n) + M(n) Σ0 M(n)',   C(n) = sum_{i<n} Abar^i W (Abar^i)',   W = D Wu D',   M(n) = Abar^n
which is the pair recursion of policy_doubling_common on (Abar', W) in place of (Abar, Qbar) with Σ0 in place of the terminal Q.  The device runs it on W / w and
Σ0 / w with w = 2^floor(log2 tr W) per problem (1 when tr W = 0), so a run to convergence stops on norm(C(2^j) - C(2^(j-1))) / w < tol.

References, in np.longdouble on dlqr_reference.lu_solve, by STEPPING Σ <- W + Abar Σ Abar' from Σ0 (they share no schedule with the code under test), and the
moments from their definitions: cost = (tr(Q Σ), tr(R K Σ K')), zvar = diag Σ, uvar = diag(K Σ K').
e64 of a problem is the largest relative deviation max|Σ64 - Σref| / max|Σref| of three float64 twins: the stepping recursion on the unprojected and on the projected
model, and pdc.doubling_fixed / pdc.doubling_converge on (Abar64', W64 / w, Σ0 / w); a twin that stops at another level or for another reason counts as deviation 1.
The bound is dlqr_reference.tolerance(e64) and the acceptance rule pdc.check_fixed's / pdc.check_conv's on Σ, levels, reason and the norms (the norms of a run to
convergence under tolerance(e64n), e64n = the larger of e64 and what the float64 doubling twin loses on dnorm and gnorm at the rule's own scale max(|ref|, max|Σref|):
that scale has Σ's units while norm(M) has none, so a weak noise leaves the norms a purely relative bound that a power of Abar does not keep), and for the moments:
each cost entry within bound x the larger of the two magnitude sums sum|Q_ij||Σref_ij| and sum|K'RK|_ij|Σref_ij|; each ustd² within bound x its magnitude sum
sum_kl |K_jk||Σref_kl||K_jl|; each zstd² within bound_i x |Σref_ii|, its own magnitude sum.  bound_i = tolerance(max(e64, zdev_i)) with zdev_i the largest deviation
|Σ64_ii - Σref_ii| / |Σref_ii| of the same three twins ON THAT ENTRY: W = D Wu D' has rank mu, so a diagonal entry can lie orders below the largest one (4e-8 of it on
pd_unstable after one step) and carries the rounding of the projection that formed D at the scale of the whole matrix -- there the float64 stepping twins are
2e-12 of |Σ_ii| apart, more than the whole-matrix e64 allows.  An entry the twins do not reproduce to 1e-8 of itself, or whose reference is exactly 0 (the cartpole's
out-of-plane coordinates: 16 zeros and two entries of 1e-50 max|Σ|), has no scale of its own in float64 and is held to bound x max|Σref| like any entry of Σ.
e64n is wider than e64 only where a weak noise makes max|Σref| small against norm(M): on every pd_* case here e64n = e64, and it differs on the cartpole models of
tests/test_gpu_covariance_noise.py (σ = 1e-3), where Σ and the moments stay under tolerance(e64).

A case takes the models, Q, R, K of pdc._models(name); Wu, one Wu per problem and Σ0 are dlqr_reference._spd under a seed from the case's name.  Variants:
    full      Wu shared and Σ0          fixed horizons
    nostart   Wu shared, Σ0 = None      fixed horizons of at least one step, and to convergence   (not for mu = 0: nothing would be left to propagate)
    perprob   one Wu per problem and Σ0 fixed horizons                      (not for mu = 0)
tol of the run to convergence lies between two consecutive relative increments of problem 0, by the recipe of pdc.build_case; the builder asserts that no longdouble
increment lies within 1e-6 relative of tol, no norm(M) within 1e-6 of 1e50, and tr W of no problem within 1e-6 relative of a power of two."""
import ctypes as C
import zlib

import numpy as np

import dlqr_reference as ref
import policy_doubling_common as pdc

LD = np.longdouble
NAMES = ("pd_12", "pd_30", "pd_84", "pd_mu0", "pd_ml0", "pd_unstable")
STEPS = (0, 1, 2, 9, 37)      # N - 1
MAX_LEVELS = pdc.MAX_LEVELS


def steps_of(name):
    return STEPS + ((1000,) if name == "pd_12" else ())


def input_map(Bu, Bl, G, dtype=LD, projected=False):
    """D = Bu - Bλ (G Bλ)⁻¹ G Bu of one problem; projected: on np.linalg.solve (float64 only), as pdc.closed_loop"""
    Bu, Bl, G = (np.asarray(x, dtype=dtype) for x in (Bu, Bl, G))
    if not Bl.shape[1]:
        return Bu
    if projected:
        return Bu - Bl @ np.linalg.solve(G @ Bl, G @ Bu)
    return Bu - Bl @ ref.lu_solve(G @ Bl, G @ Bu, dtype)


def noise(D, Wu, dtype=LD):
    """W = D Wu D' (zeros when there is no input or no Wu)"""
    mx = D.shape[0]
    if Wu is None or not D.shape[1]:
        return np.zeros((mx, mx), dtype=dtype)
    return D @ np.asarray(Wu, dtype=dtype) @ D.T


def scale_of(W):
    """w = 2^floor(log2 tr W), 1 when the trace is 0; asserts that the trace does not lie within 1e-6 relative of a power of two"""
    tr = float(np.trace(W))
    if tr == 0.0:
        return 1.0
    assert tr > 0.0
    m, e = np.frexp(tr)      # tr = m 2^e, 0.5 <= m < 1
    assert m - 0.5 > 1e-6 and 1.0 - m > 1e-6, "tr W lies within 1e-6 relative of a power of two"
    return float(np.ldexp(1.0, int(e) - 1))


def step_covariance(Abar, W, S0, wanted):
    """Σ and M after every step count in `wanted`, by stepping from Σ0 -> {n: (Σ_n, M(n))}"""
    S, M, out = S0.copy(), np.eye(Abar.shape[0], dtype=Abar.dtype), {}
    with np.errstate(over="ignore", invalid="ignore"):
        for n in range(max(wanted) + 1):
            if n in wanted:
                out[n] = (S, M)
            S, M = W + Abar @ S @ Abar.T, Abar @ M
    return out


def moments(S, Q, R, K):
    """(cost [2], zvar [mx], uvar [mu], cost scale, uvar magnitude sums [mu]) of a covariance, in its dtype"""
    dt = S.dtype
    Q, R, K = (np.asarray(x, dtype=dt) for x in (Q, R, K))
    V = K @ S @ K.T
    cost = np.array([np.sum(Q * S.T), np.sum(R * V.T)], dtype=dt)
    cmag = max(float(np.sum(np.abs(Q) * np.abs(S))), float(np.sum(np.abs(K.T @ R @ K) * np.abs(S))))
    umag = np.array([float(np.abs(K[j]) @ np.abs(S) @ np.abs(K[j])) for j in range(K.shape[0])])
    return cost, np.diag(S).copy(), np.diag(V).copy(), cmag, umag


def _rel(S64, Sref):
    return pdc._rel(S64, Sref)


def _zdev(twins, Sref):
    """per diagonal entry, the largest deviation |Σ64_ii - Σref_ii| / |Σref_ii| of the float64 twins (inf where Σref_ii = 0: such an entry has no scale of its own)"""
    d = np.diag(Sref)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dev = np.max([np.abs(np.diag(np.asarray(T, dtype=LD)) - d) / np.abs(d) for T in twins], axis=0).astype(np.float64)
    return np.where(np.isfinite(dev), dev, np.inf)


def converge_reference(A, Bu, Bl, G, Q, R, K, Wu, tol, max_levels):
    """the reference of a run to convergence on one problem: dict(S float64, levels, reason, dnorm [2] in Σ's units, gnorm [2], e64 and the moments); asserts that no
    longdouble relative increment lies within 1e-6 relative of tol and no longdouble norm(M) within 1e-6 relative of the growth limit"""
    mx = np.shape(A)[0]
    Abar = pdc.closed_loop(A, Bu, Bl, G, Q, R, K)[0]
    W = noise(input_map(Bu, Bl, G), Wu)
    w = scale_of(W)
    Sw, levels, reason, incs, gs = pdc.stepping_converge(Abar.T, W / LD(w), np.zeros((mx, mx), dtype=LD), tol, max_levels)
    for x in incs:
        assert abs(float(x) - tol) > 1e-6 * tol, "a longdouble increment lies within 1e-6 of tol"
    for x in gs:
        assert abs(float(x) - pdc.GROWTH) > 1e-6 * pdc.GROWTH, "a longdouble norm(M) lies within 1e-6 of the growth limit"
    Sref = Sw * LD(w)
    Z64 = np.zeros((mx, mx))
    e64, stepped = 0.0, []
    with np.errstate(over="ignore", invalid="ignore"):
        for pj in (False, True):
            A64 = pdc.closed_loop(A, Bu, Bl, G, Q, R, K, np.float64, pj)[0]
            W64 = noise(input_map(Bu, Bl, G, np.float64, pj), Wu, np.float64)
            stepped.append(step_covariance(A64, W64, Z64, (2 ** levels,))[2 ** levels][0])
            e64 = max(e64, _rel(stepped[-1], Sref))
        Sd, l64, r64, i64, g64 = pdc.doubling_converge(A64.T, W64 / w, Z64, tol, max_levels)      # (the projected model: the last of the loop)
    e64 = max(e64, 1.0 if (l64, r64) != (levels, reason) else _rel(Sd * w, Sref))
    dn, gn = pdc.last_two(incs) * w, pdc.last_two(gs)
    # what the float64 doubling twin loses on the NORMS, on the scale the rule compares them at: norm(M(2^j)) is a power of Abar, and after 2^11 steps of a cartpole
    # the float64 product is 3e-11 relative off whatever the schedule; with a noise of 1e-6 max|Σref| is 2e-9 and gives such a norm no room
    e64n = 1.0
    if (l64, r64) == (levels, reason):
        scale = float(np.abs(Sref).max())
        e64n = max(abs(x - y) / max(abs(y), scale) for x, y in zip(np.r_[pdc.last_two(i64) * w, pdc.last_two(g64)], np.r_[dn, gn]) if not np.isnan(y))
    cost, zvar, uvar, cmag, umag = moments(Sref, Q, R, K)
    return dict(S=Sref.astype(np.float64), levels=levels, reason=reason, dnorm=dn, gnorm=gn, e64=e64, e64n=max(e64, e64n), cost=cost.astype(np.float64),
                cmag=cmag, zvar=zvar.astype(np.float64), zdev=_zdev(stepped + [Sd * w], Sref), uvar=uvar.astype(np.float64), umag=umag, w=w)


_built = {}


def build_case(name):
    """the problems of a case and their references, built once per session and left unchanged: dict with A, Bu, Bl, G, Q, R, K, Wu, WuP, Sigma0, nprob, mx, mu, ml,
    steps, paths, variants = {variant: dict(Wu, Sigma0, w [nprob], fixed = {n: [per problem dict(S, levels, gM, e64, cost, cmag, zvar, uvar, umag)]})}, and for the
    variant "nostart": tol, max_levels, conv = [per problem dict(S, levels, reason, dnorm [2], gnorm [2], e64, cost, ...)]"""
    if name in _built:
        return _built[name]
    c = pdc.BY_NAME[name]
    A, Bu, Bl, G, Q, R, K = pdc._models(name)
    nprob, mx, mu, ml = A.shape[0], A.shape[1], Bu.shape[2], Bl.shape[2]
    rng = np.random.default_rng(zlib.crc32(("cov_" + name).encode()))
    Wu = ref._spd(rng, mu) if mu else None
    WuP = np.stack([ref._spd(rng, mu) for _ in range(nprob)]) if mu else None
    Sigma0 = ref._spd(rng, mx)
    steps = steps_of(name)
    Abar = [pdc.closed_loop(A[p], Bu[p], Bl[p], G[p], Q, R, K)[0] for p in range(nprob)]
    D = [input_map(Bu[p], Bl[p], G[p]) for p in range(nprob)]
    A64 = [[pdc.closed_loop(A[p], Bu[p], Bl[p], G[p], Q, R, K, np.float64, pj)[0] for pj in (False, True)] for p in range(nprob)]
    D64 = [[input_map(Bu[p], Bl[p], G[p], np.float64, pj) for pj in (False, True)] for p in range(nprob)]
    variants = {}
    todo = [("full", Wu, Sigma0)] + ([("nostart", Wu, None), ("perprob", WuP, Sigma0)] if mu else [])
    for vname, wu, s0 in todo:
        wu_of = (lambda p: None) if wu is None else ((lambda p: wu[p]) if wu.ndim == 3 else (lambda p: wu))
        S0 = np.zeros((mx, mx), dtype=LD) if s0 is None else np.asarray(s0, dtype=LD)
        S064 = S0.astype(np.float64)
        W = [noise(D[p], wu_of(p)) for p in range(nprob)]
        w = [scale_of(W[p]) for p in range(nprob)]
        W64 = [[noise(D64[p][k], wu_of(p), np.float64) for k in range(2)] for p in range(nprob)]
        vsteps = steps if s0 is not None else tuple(n for n in steps if n > 0)      # (no start and no step: Σ = 0, nothing to compare against)
        fixed = {n: [] for n in vsteps}
        for p in range(nprob):
            refs = step_covariance(Abar[p], W[p], S0, vsteps)
            twins = [step_covariance(A64[p][k], W64[p][k], S064, vsteps) for k in range(2)]
            for n in vsteps:
                Sref, Mref = refs[n]
                Sd, levels, _, _ = pdc.doubling_fixed(A64[p][1].T, W64[p][1] / w[p], S064 / w[p], n)
                e64 = max(_rel(twins[0][n][0], Sref), _rel(twins[1][n][0], Sref), _rel(Sd * w[p], Sref))
                cost, zvar, uvar, cmag, umag = moments(Sref, Q, R, K)
                fixed[n].append(dict(S=Sref.astype(np.float64), levels=levels, gM=float(pdc.fro(Mref)), e64=e64, cost=cost.astype(np.float64), cmag=cmag,
                                     zvar=zvar.astype(np.float64), zdev=_zdev([twins[0][n][0], twins[1][n][0], Sd * w[p]], Sref), uvar=uvar.astype(np.float64),
                                     umag=umag))
        variants[vname] = dict(Wu=wu, Sigma0=s0, w=w, fixed=fixed)
        if vname != "nostart":
            continue
        # tol between the relative increments of the levels before and at c["level"] of problem 0 (pdc.build_case's recipe), then asserted on every problem
        Z64 = np.zeros((mx, mx))
        _, _, _, incs0, _ = pdc.doubling_converge(A64[0][1].T, W64[0][1] / w[0], Z64, 0.0, c["level"] + 4)
        cand = [j for j in range(c["level"] - 1, len(incs0)) if incs0[j] < min(incs0[:j])]
        assert cand, "the increments of problem 0 never fall to a new minimum: no tol can be placed"
        tol = float(np.sqrt(incs0[cand[0]] * min(incs0[:cand[0]])))
        conv = [converge_reference(A[p], Bu[p], Bl[p], G[p], Q, R, K, wu_of(p), tol, MAX_LEVELS) for p in range(nprob)]
        variants[vname].update(tol=tol, max_levels=MAX_LEVELS, conv=conv)
    _built[name] = dict(name=name, A=A, Bu=Bu, Bl=Bl, G=G, Q=Q, R=R, K=K, Wu=Wu, WuP=WuP, Sigma0=Sigma0, nprob=nprob, mx=mx, mu=mu, ml=ml, steps=steps,
                        paths=c["paths"], variants=variants)
    return _built[name]


def check_moments(cost, zstd, ustd, r, what):
    """the acceptance rule of the moments of one problem against its reference record r; prints every figure before it asserts"""
    bound = ref.tolerance(r["e64"])
    ec = float(np.abs(np.asarray(cost) - r["cost"]).max())
    # zstd² entry by entry at its own scale |Σref_ii|, under the bound the twins' deviation ON THAT ENTRY gives; an entry the twins do not reproduce to 1e-8 of
    # itself (or an exact zero) is rounding residue of the float64 model and is held to what Σ's entries are held to, bound x max|Σref|
    zerr = np.abs(np.asarray(zstd) ** 2 - r["zvar"])
    own = 10.0 * r["zdev"] <= 1e-7
    zb = np.array([ref.tolerance(max(r["e64"], z)) if o else np.nan for z, o in zip(r["zdev"], own)])
    with np.errstate(invalid="ignore", divide="ignore"):
        ez = float(np.max(np.where(own, zerr / np.abs(r["zvar"]) / zb, zerr / (bound * np.abs(r["S"]).max()))))      # in units of each entry's bound
    eu = float(np.max(np.abs(np.asarray(ustd) ** 2 - r["uvar"]) / r["umag"])) if len(r["uvar"]) else 0.0
    print("%s: cost %s (reference %s) off by %.3g of the magnitude sum %.3g; zstd^2 at %.3g of its per-entry bounds (%d of %d entries at their own scale, the largest "
          "of those bounds %.3g), ustd^2 off by %.3g of its magnitude sum; bound %.3g"
          % (what, cost, r["cost"], ec / r["cmag"], r["cmag"], ez, own.sum(), len(own), np.nanmax(zb) if own.any() else 0.0, eu, bound))
    assert np.isfinite(np.asarray(cost)).all() and ec <= bound * r["cmag"], "%s: cost %s, reference %s, bound %.3g of %.3g" % (what, cost, r["cost"], bound, r["cmag"])
    assert ez <= 1.0, "%s: zstd^2 at %.3g of its per-entry bound" % (what, ez)
    assert eu <= bound, "%s: ustd^2 off by %.3g of its magnitude sum, bound %.3g" % (what, eu, bound)


def check_fixed(S, cost, zstd, ustd, levels, gn, dn, r, what):
    """pdc.check_fixed on Σ, levels and the norms, then the moments"""
    pdc.check_fixed(S, levels, gn, dn, (r["S"], r["levels"], r["gM"], r["e64"]), what)
    check_moments(cost, zstd, ustd, r, what)


def check_conv(S, cost, zstd, ustd, levels, reason, dn, gn, r, what):
    """pdc.check_conv on levels, reason and the norms under tolerance(e64n), Σ under tolerance(e64) as for a fixed horizon, then the moments"""
    pdc.check_conv(S, levels, reason, dn, gn, (r["S"], r["levels"], r["reason"], r["dnorm"], r["gnorm"], r["e64n"]), what)
    err, scale, bound = float(np.abs(S - r["S"]).max()), float(np.abs(r["S"]).max()), ref.tolerance(r["e64"])
    assert err <= bound * scale, "%s: max|Σ - Σref| = %.3g relative, bound %.3g" % (what, err / scale, bound)
    check_moments(cost, zstd, ustd, r, what)


def refusal_call(capi, pr):
    """cclqr_covariance_doubling through ctypes on sentinel-filled outputs, for tests/test_gpu_covariance.py and tests/test_analysis_refusals_host.py.  pr: nprob, mx, mu,
    ml and the arrays A, Bu, Bl, G, K, Q, R, Wu, Sigma0.  The call returns (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml = pr["nprob"], pr["mx"], pr["mu"], pr["ml"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    A, Bu, Bl, G, K, Q, R, Wu, S0 = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "K", "Q", "R", "Wu", "Sigma0"))

    def call(n_gains=1, n_weights=1, n_noise=1, N=10, tol=1e-8, max_levels=40, path=0, bf16=0, nprob=n, A_=A, S_=True, K_=K, Bl_=Bl, Wu_=Wu, S0_=S0, Q_=Q, R_=R,
             cost_=True, mu_=mu):
        S = np.full((n, mx, mx), 7.5)
        cost, zs, us = np.full((n, 2), 7.5), np.full((n, mx), 7.5), np.full((n, mu), 7.5)
        lv, rs = np.full(n, -9, dtype=np.int32), np.full(n, -9, dtype=np.int32)
        dn, gn = np.full((n, 2), 7.5), np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_covariance_doubling(C.c_int32(nprob), C.c_int32(mx), C.c_int32(mu_), C.c_int32(ml), d(A_), d(Bu), d(Bl_), d(G), C.c_int32(n_gains), d(K_),
                                         C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), d(S0_), C.c_int32(N), C.c_double(tol), C.c_int32(max_levels),
                                         d(S) if S_ else None, d(cost) if cost_ else None, d(zs), d(us), lv.ctypes.data_as(ip), rs.ctypes.data_as(ip), d(dn), d(gn),
                                         C.byref(o))
        untouched = bool(all((x == 7.5).all() for x in (S, cost, zs, us, dn, gn)) and (lv == -9).all() and (rs == -9).all())
        return rc, untouched, L.cclqr_last_error().decode()

    return call


def refusal_cases():
    """what cclqr_covariance_doubling refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (nprob must not be 2)"""
    return dict(N_neg=dict(N=-1), levels_0=dict(N=0, S0_=None, max_levels=0), levels_61=dict(N=0, S0_=None, max_levels=61), tol_neg=dict(tol=-1e-9),
                tol_nan=dict(tol=float("nan")), n_gains_2=dict(n_gains=2), n_weights_2=dict(n_weights=2), n_weights_0=dict(n_weights=0), path_3=dict(path=3),
                bf16=dict(bf16=2), nprob_0=dict(nprob=0), A_null=dict(A_=None), S_null=dict(S_=False), K_null=dict(K_=None),
                n_noise_2=dict(n_noise=2), n_noise_0=dict(n_noise=0), no_source=dict(Wu_=None, S0_=None), cost_without_Q=dict(Q_=None),
                cost_without_R=dict(R_=None), Wu_with_mu_0=dict(mu_=0), start_with_N_0=dict(N=0))
