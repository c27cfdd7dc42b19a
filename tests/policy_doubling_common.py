"""Shared by tests/test_policy_doubling_reference.py (CPU) and tests/test_gpu_policy_doubling.py: the cases of the doubling evaluation of a stationary gain
(cclqr_policy_value_doubling) and their extended-precision references.

The evaluation, restated.  With the one gain K (LQR{T,Inf}, lqr.jl:40-43), Abar = A - Bu K - Bλ Kλ (lqr.jl:169) and Qbar = Q + K' R K (lqr.jl:170) are constant, and
with S(n) = sum_{i<n} (Abar^i)' Qbar Abar^i, M(n) = Abar^n the cost-to-go after n backward steps is P = S(n) + M(n)' Q M(n).  From S(1) = Qbar, M(1) = Abar:
    doubling    S(2n) = S(n) + M(n)' S(n) M(n),    M(2n) = M(n) M(n)
    accumulate  S(a+n) = S(a) + M(a)' S(n) M(a),   M(a+n) = M(a) M(n),   from S(0) = 0, M(0) = I
Fixed horizon N: n = N - 1, accumulate over the set bits of n from the least significant, double between bits, not after the top bit.
To convergence: level j = 1, 2, .. doubles to 2^j steps; stop after level j, in this order: reason 0 norm(S(2^j) - S(2^(j-1))) < tol, reason 2 norm(M(2^j)) > 1e50,
reason 1 j == max_levels.

References, in np.longdouble on dlqr_reference.lu_solve, both by STEPPING (they share no schedule with the code under test):
    fixed        policy_value_common.policy_sweep(..., K[None], N, 0.0, LD)
    convergence  S <- Qbar + Abar' S Abar and M <- M Abar from S = 0, M = I, with S and norm(M) recorded at the steps 2^j
e64P of a problem is the largest relative deviation max|P64 - Pref| / max|Pref| of three float64 twins: the two stepping twins of policy_value_common.reference (for a
run to convergence: over the 2^levels steps the reference made) and the doubling schedule below in numpy float64 on the projected model; a twin that stops at another
level or for another reason counts as deviation 1.  The bound is dlqr_reference.tolerance(e64P), and the acceptance rule policy_value_common.check's: levels and
reason equal; max|P - Pref| <= bound max|Pref|; every norm of dnorm and gnorm within bound max(|ref|, max|Pref|) of the reference's, NaN where it has none.

A case takes the models, weights and the gain Kfull[0] of a policy_value_common case (or, for the two shapes that has not, the same recipe under its own seed).  tol of
a run to convergence lies between two consecutive longdouble increments of problem 0, and the builder asserts that no longdouble increment of any problem lies within
1e-6 relative of tol and no norm(M) within 1e-6 relative of 1e50.  Large shapes get a tol that converges within three levels, so that the stepping reference stays
cheap."""
import ctypes as C
import zlib

import numpy as np

import dlqr_reference as ref
import policy_value_common as pvc

LD = np.longdouble
GROWTH = 1e50
ALL_STEPS = (0, 1, 2, 7, 8, 9, 37, 1000)      # N - 1: none, one, one doubling, all bits set, one bit, two bits, mixed, the 1001-knot horizon
FEW_STEPS = (9, 37)

#            name           models of        (mx, mu, ml, nprob)  N - 1      level problem 0 converges at   paths
_TABLE = [("pd_12",        "pv_frag_1_3",   None,                ALL_STEPS, 5,                             (0, 1, 2)),
          ("pd_24",        "pv_stationary", None,                ALL_STEPS, 5,                             (0, 1, 2)),
          ("pd_36",        "pv_reg_mu2",    None,                FEW_STEPS, 4,                             (0, 1, 2)),
          ("pd_84",        "pv_frag_7_21",  None,                FEW_STEPS, 3,                             (0, 1, 2)),
          ("pd_96",        None,            (96, 1, 8, 2),       FEW_STEPS, 3,                             (0, 1, 2)),
          ("pd_30",        "pv_tiled_30",   None,                ALL_STEPS, 4,                             (0, 2)),
          ("pd_97",        "pv_tiled_97",   None,                FEW_STEPS, 3,                             (0, 2)),
          ("pd_100",       None,            (100, 2, 10, 2),     (9,),      3,                             (0, 2)),
          ("pd_mu0",       "pv_mu0",        None,                FEW_STEPS, 4,                             (0, 1, 2)),
          ("pd_ml0",       "pv_ml0",        None,                FEW_STEPS, 4,                             (0, 1, 2)),
          ("pd_nonsym",    "pv_nonsym",     None,                FEW_STEPS, 4,                             (0, 1, 2)),
          ("pd_unstable",  "pv_unstable",   None,                (1000,),   5,                             (0, 1, 2))]
CASES = [dict(name=n, source=s, shape=sh, steps=st, level=lv, paths=p) for n, s, sh, st, lv, p in _TABLE]
BY_NAME = {c["name"]: c for c in CASES}
MAX_LEVELS = 40


def closed_loop(A, Bu, Bl, G, Q, R, K, dtype=LD, projected=False):
    """(Abar, Qbar) of one problem; projected: the kernels' form Abar = A' - D K on np.linalg.solve (float64 only)"""
    A, Bu, Bl, G, Q, R, K = (np.asarray(x, dtype=dtype) for x in (A, Bu, Bl, G, Q, R, K))
    ml = Bl.shape[1]
    if projected:
        assert dtype == np.float64
        if ml:
            EF = np.linalg.solve(G @ Bl, G @ np.concatenate([A, Bu], axis=1))
            A, Bu = A - Bl @ EF[:, :A.shape[1]], Bu - Bl @ EF[:, A.shape[1]:]
        Abar = A - Bu @ K
    else:
        Abar = A - Bu @ K
        if ml:
            Abar = Abar - Bl @ ref.lu_solve(G @ Bl, G @ Abar, dtype)
    return Abar, Q + K.T @ R @ K


def fro(X):
    """Frobenius norm, scaled so that the squares of entries of 1e200 (the increments of an unstable closed loop just before the growth stop) do not overflow"""
    m = np.max(np.abs(X))
    if not np.isfinite(m) or m == 0:
        return m
    Y = X / m
    return m * np.sqrt(np.sum(Y * Y))


def doubling_fixed(Abar, Qbar, Q, n):
    """the fixed-horizon schedule as stated -> (P, doublings made, mx^3 products made, norm(M(n))).  The first set bit is a copy: S(0) + I' Sd I = Sd, I Md = Md"""
    Sd, Md, Sa, Ma, products, levels = Qbar, Abar, None, None, 0, 0
    if n == 0:
        return Q.copy(), 0, 0, float(np.sqrt(Q.shape[0]))
    top = n.bit_length() - 1
    for b in range(top + 1):
        if (n >> b) & 1:
            if Sa is None:
                Sa, Ma = Sd, Md
            else:
                Sa, Ma, products = Sa + Ma.T @ Sd @ Ma, Ma @ Md, products + 3
        if b < top:
            Sd, Md, products, levels = Sd + Md.T @ Sd @ Md, Md @ Md, products + 3, levels + 1
    return Sa + Ma.T @ Q @ Ma, levels, products + 2, float(fro(Ma))


def doubling_converge(Abar, Qbar, Q, tol, max_levels):
    """the run to convergence as stated -> (P, levels, reason, increment norms of every level, norm(M) of every level)"""
    Sd, Md, incs, gs, reason = Qbar, Abar, [], [], 1
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(1, max_levels + 1):
            T = Md.T @ Sd @ Md
            Sd, Md = Sd + T, Md @ Md
            incs.append(float(fro(T)))
            gs.append(float(fro(Md)))
            if incs[-1] < tol:
                reason = 0
                break
            if gs[-1] > GROWTH:
                reason = 2
                break
        return Sd + Md.T @ Q @ Md, len(incs), reason, incs, gs


def stepping_converge(Abar, Qbar, Q, tol, max_levels):
    """the reference of a run to convergence: S and M by single steps from S = 0, M = I, looked at after 2^j steps -> as doubling_converge"""
    S, M, incs, gs, reason = Qbar, Abar, [], [], 1      # one step made
    for j in range(1, max_levels + 1):
        S0 = S
        for _ in range(2 ** (j - 1)):
            S, M = Qbar + Abar.T @ S @ Abar, M @ Abar
        incs.append(fro(S - S0))
        gs.append(fro(M))
        if incs[-1] < tol:
            reason = 0
            break
        if gs[-1] > GROWTH:
            reason = 2
            break
    return S + M.T @ Q @ M, len(incs), reason, incs, gs


def last_two(xs):
    return pvc.last_two(xs)


def _rel(P64, Pref):
    return float(np.max(np.abs(np.asarray(P64, dtype=LD) - Pref)) / np.max(np.abs(Pref)))


def _models(name):
    """(A, Bu, Bl, G [nprob][...], Q, R, K [mu][mx]) of a case"""
    c = BY_NAME[name]
    if c["source"]:
        pr = pvc.build_case(c["source"])
        return pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], np.ascontiguousarray(pr["Kfull"][0])
    mx, mu, ml, nprob = c["shape"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A, Bu, Bl, G = ref._model(rng, mx, mu, ml)
    Q, R = ref._spd(rng, mx), ref._spd(rng, mu)
    K = np.ascontiguousarray(ref.dlqr(A, Bu, Bl, G, Q, R, 10, 0.0, np.float64)[0][0])
    As, Bus, Bls = [A], [Bu], [Bl]
    for p in range(1, nprob):
        s = 0.05 * p / np.sqrt(mx)
        As.append(A + s * rng.normal(size=A.shape))
        Bus.append(Bu + s * rng.normal(size=Bu.shape))
        Bls.append(Bl + s * rng.normal(size=Bl.shape))
    return np.stack(As), np.stack(Bus), np.stack(Bls), np.stack([G] * nprob), Q, R, K


def converge_reference(A, Bu, Bl, G, Q, R, K, tol, max_levels):
    """the reference of a run to convergence on one problem: (Pref float64, levels, reason, dnorm [2], gnorm [2], e64P); asserts that no longdouble increment lies
    within 1e-6 relative of tol and no longdouble norm(M) within 1e-6 relative of the growth limit"""
    Abar, Qbar = closed_loop(A, Bu, Bl, G, Q, R, K)
    PLD, levels, reason, incs, gs = stepping_converge(Abar, Qbar, np.asarray(Q, dtype=LD), tol, max_levels)
    for x in incs:
        assert abs(float(x) - tol) > 1e-6 * tol, "a longdouble increment lies within 1e-6 of tol"
    for x in gs:
        assert abs(float(x) - GROWTH) > 1e-6 * GROWTH, "a longdouble norm(M) lies within 1e-6 of the growth limit"
    e64 = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for projected in (False, True):
            P64 = pvc.policy_sweep(A, Bu, Bl, G, Q, R, K[None], 2 ** levels + 1, 0.0, np.float64, projected)[0]
            e64 = max(e64, _rel(P64, PLD))
    A64, Q64 = closed_loop(A, Bu, Bl, G, Q, R, K, np.float64, True)
    P64, l64, r64, _, _ = doubling_converge(A64, Q64, np.asarray(Q, dtype=np.float64), tol, max_levels)
    e64 = max(e64, 1.0 if (l64, r64) != (levels, reason) else _rel(P64, PLD))
    return PLD.astype(np.float64), levels, reason, last_two(incs), last_two(gs), e64


_built = {}


def build_case(name):
    """the problems of a case and their references, built once per session and left unchanged: dict with A, Bu, Bl, G, Q, R, K, nprob, mx, mu, ml, steps, paths,
    fixed = {n: [per problem (Pref float64, levels, gM, e64P)]}, tol, max_levels, conv = [per problem (Pref float64, levels, reason, dnorm [2], gnorm [2], e64P)]"""
    if name in _built:
        return _built[name]
    c = BY_NAME[name]
    A, Bu, Bl, G, Q, R, K = _models(name)
    nprob, mx, mu, ml = A.shape[0], A.shape[1], Bu.shape[2], Bl.shape[2]
    cl = [closed_loop(A[p], Bu[p], Bl[p], G[p], Q, R, K) for p in range(nprob)]
    cl64 = [closed_loop(A[p], Bu[p], Bl[p], G[p], Q, R, K, np.float64, True) for p in range(nprob)]
    Q64 = np.asarray(Q, dtype=np.float64)
    fixed = {}
    for n in c["steps"]:
        rows = []
        for p in range(nprob):
            Pref, _, _, e64, _ = pvc.reference(A[p], Bu[p], Bl[p], G[p], Q, R, K[None], n + 1, 0.0)
            P64, levels, _, _ = doubling_fixed(cl64[p][0], cl64[p][1], Q64, n)      # (against the reference rounded to float64: 1e-16 of its scale)
            MLD = np.eye(mx, dtype=LD)
            for _ in range(n):
                MLD = MLD @ cl[p][0]
            rows.append((Pref, levels, float(fro(MLD)), max(e64, _rel(P64, np.asarray(Pref, dtype=LD)))))
        fixed[n] = rows
    # tol between the increments of the levels before and at c["level"], of problem 0, float64 first (cheap), then asserted on the longdouble norms of every problem
    # (the first level from the wanted one on whose increment is a new minimum: the increments may grow over the first levels, while S still does)
    _, _, _, incs0, _ = doubling_converge(cl64[0][0], cl64[0][1], Q64, 0.0, c["level"] + 4)
    cand = [j for j in range(c["level"] - 1, len(incs0)) if incs0[j] < min(incs0[:j])]
    assert cand, "the increments of problem 0 never fall to a new minimum: no tol can be placed"
    tol = float(np.sqrt(incs0[cand[0]] * min(incs0[:cand[0]])))
    conv = [converge_reference(A[p], Bu[p], Bl[p], G[p], Q, R, K, tol, MAX_LEVELS) for p in range(nprob)]
    _built[name] = dict(c, A=A, Bu=Bu, Bl=Bl, G=G, Q=Q, R=R, K=K, nprob=nprob, mx=mx, mu=mu, ml=ml, fixed=fixed, tol=tol, max_levels=MAX_LEVELS, conv=conv)
    return _built[name]


def check_fixed(P, levels, gn, dn, refp, what):
    """the acceptance rule of a fixed horizon on one problem; prints every figure before it asserts"""
    Pref, lref, gref, e64 = refp
    bound = ref.tolerance(e64)
    scale = float(np.abs(Pref).max())
    err = float(np.abs(P - Pref).max()) if np.isfinite(P).all() else np.inf
    print("%s: levels %d (reference %d), max|P - Pref| = %.3g relative, bound %.3g (e64P %.3g, max|Pref| %.3g), gnorm %s (reference %.6g)"
          % (what, levels, lref, err / scale, bound, e64, scale, gn, gref))
    assert int(levels) == lref, "%s: levels %d, reference %d" % (what, levels, lref)
    assert err <= bound * scale, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, err / scale, bound)
    if gn is not None:
        assert abs(gn[0] - gref) <= bound * max(gref, scale) and np.isnan(gn[1]) and np.isnan(dn).all(), "%s: gnorm %s, dnorm %s, reference norm(M) %.17g" % (what, gn, dn, gref)


def check_conv(P, levels, reason, dn, gn, refp, what):
    """the acceptance rule of a run to convergence on one problem (policy_value_common.check's, with reason beside levels and gnorm beside dnorm)"""
    Pref, lref, rref, dnref, gnref, e64 = refp
    bound = ref.tolerance(e64)
    scale = float(np.abs(Pref).max())
    err = float(np.abs(P - Pref).max()) if np.isfinite(P).all() else np.inf
    print("%s: levels %d reason %d (reference %d, %d), max|P - Pref| = %.3g relative, bound %.3g (e64P %.3g, max|Pref| %.3g), dnorm %s (reference %s), gnorm %s (reference %s)"
          % (what, levels, reason, lref, rref, err / scale, bound, e64, scale, dn, dnref, gn, gnref))
    assert (int(levels), int(reason)) == (lref, rref), "%s: levels %d reason %d, reference %d, %d" % (what, levels, reason, lref, rref)
    assert err <= bound * scale, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, err / scale, bound)
    for name, got, want in (("dnorm", dn, dnref), ("gnorm", gn, gnref)):
        for j in range(2):
            if np.isnan(want[j]):
                assert np.isnan(got[j]), "%s: %s[%d] = %r where no such level ran" % (what, name, j, got[j])
            else:
                assert abs(got[j] - want[j]) <= bound * max(abs(want[j]), scale), "%s: %s[%d] = %.17g, reference %.17g, bound %.3g of max(|ref|, max|Pref| = %.3g)" % (
                    what, name, j, got[j], want[j], bound, scale)


def refusal_call(capi, pr):
    """cclqr_policy_value_doubling through ctypes on sentinel-filled outputs, for tests/test_gpu_policy_doubling.py and tests/test_analysis_refusals_host.py.  pr: nprob,
    mx, mu, ml, tol and the arrays A, Bu, Bl, G, K, Q, R.  The call returns (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml = pr["nprob"], pr["mx"], pr["mu"], pr["ml"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: a.ctypes.data_as(dp)
    A, Bu, Bl, G, K, Q, R = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "K", "Q", "R"))

    def call(n_gains=1, n_weights=1, N=10, tol=pr["tol"], max_levels=40, path=0, bf16=0, nprob=n, A_=A, P_=True, K_=K, Bl_=Bl):
        P = np.full((n, mx, mx), 7.5)
        lv, rs = np.full(n, -9, dtype=np.int32), np.full(n, -9, dtype=np.int32)
        dn, gn = np.full((n, 2), 7.5), np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_policy_value_doubling(C.c_int32(nprob), C.c_int32(mx), C.c_int32(mu), C.c_int32(ml), None if A_ is None else d(A_), d(Bu), d(Bl_), d(G),
                                           C.c_int32(n_gains), None if K_ is None else d(K_), C.c_int32(n_weights), d(Q), d(R), C.c_int32(N), C.c_double(tol),
                                           C.c_int32(max_levels), d(P) if P_ else None, lv.ctypes.data_as(ip), rs.ctypes.data_as(ip), d(dn), d(gn), C.byref(o))
        untouched = bool((P == 7.5).all() and (lv == -9).all() and (rs == -9).all() and (dn == 7.5).all() and (gn == 7.5).all())
        return rc, untouched, L.cclqr_last_error().decode()

    return call


def refusal_cases():
    """what cclqr_policy_value_doubling refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (nprob must not be 2)"""
    return dict(N_neg=dict(N=-1), levels_0=dict(N=0, max_levels=0), levels_61=dict(N=0, max_levels=61), tol_neg=dict(tol=-1e-9), tol_nan=dict(tol=float("nan")),
                tol_nan_conv=dict(N=0, tol=float("nan")), n_gains_2=dict(n_gains=2), n_gains_0=dict(n_gains=0), n_weights_2=dict(n_weights=2),
                n_weights_0=dict(n_weights=0), path_3=dict(path=3), path_neg=dict(path=-1), bf16=dict(bf16=2), nprob_0=dict(nprob=0), A_null=dict(A_=None),
                P_null=dict(P_=False), K_null=dict(K_=None))
