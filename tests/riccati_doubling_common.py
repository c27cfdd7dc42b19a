"""Shared by tests/test_riccati_doubling_reference.py (CPU) and tests/test_gpu_riccati_doubling.py: the cases of the Riccati doubling (cclqr_riccati_doubling) and
their extended-precision references.

The doubling, restated.  With [A' | D] the projected model and G0 = D R^-1 D', n backward steps of lqr.jl:151-170 are the triple (A_n, G_n, H_n) of the map
X -> H_n + A_n' X (I + G_n X)^-1 A_n; H_n is the recursion's Pk after n - 1 steps from Pk = Q.  One step is (A', G0, Q); triple 1 applied after triple 2 is
    W = (I + G1 H2)^-1,   A = A2 W A1,   G = G2 + A2 W G1 A2',   H = H1 + A1' H2 W A1
Fixed horizon N: n = N - 1 single-step triples, accumulated over the set bits of n from the least significant (the first is a copy; an accumulation is 1 = the
accumulated triple, 2 = the doubling one), doubling between bits, not after the top bit.  To convergence: level j = 1, 2, .. doubles to 2^j triples; stop after level
j, in this order: reason 0 norm(H(2^j) - H(2^(j-1))) < tol, reason 2 norm(A(2^j)) > 1e50 or a norm that is not finite, reason 1 j == max_levels.  The final step on
X = H_n is the recursion's own: Ku = (R + D'XD)^-1 D'X A', Abar = A' - D Ku, P = Q + Ku'R Ku + Abar' X Abar.

References, in np.longdouble, by STEPPING dlqr_reference._step (lqr.jl:151-170 statement by statement, the (mu+ml)-square system: no projection, no schedule
shared with the code under test): K = Ku[1] and P = the last Pkp1 of dlqr(.., N, tol = 0); for a run to convergence Pk is looked at after 2^j - 1 steps (= H(2^j)) and
A(n + 1) = A(n) Abar_n, A(1) = the projected A, is carried along.  e64K / e64P of a problem is the worst relative deviation of three float64 twins: the same stepping
in float64, dlqr_reference._step_projected64, and the schedule above in numpy float64; a twin that stops at another level or for another reason counts as deviation
1.  The bounds are dlqr_reference.tolerance(e64K) on max|K - Kref| / max|Kref| and tolerance(e64P) likewise on P.

tol of a run to convergence lies between two consecutive longdouble increments of problem 0; the builder asserts that no longdouble increment of any problem lies
within 1e-6 relative of it and no norm(A) within 1e-6 relative of 1e50."""
import ctypes as C
import zlib

import numpy as np

import dlqr_reference as ref

LD = np.longdouble
GROWTH = 1e50
ALL_STEPS = (1, 2, 7, 8, 9, 37, 1000)      # N - 1: one triple (a copy), one doubling, all bits set, one bit, two bits, mixed, the 1001-knot horizon
FEW_STEPS = (9, 37)
MAX_LEVELS = 12

#          name        (mx, mu, ml, nprob)   N - 1      level problem 0 converges at
_TABLE = [("rd_12",   (12, 1, 3, 3),        ALL_STEPS, 5),
          ("rd_24",   (24, 2, 10, 2),       ALL_STEPS, 5),
          ("rd_30",   (30, 2, 6, 2),        FEW_STEPS, 4),
          ("rd_36",   (36, 2, 12, 2),       FEW_STEPS, 4),
          ("rd_84",   (84, 7, 35, 2),       FEW_STEPS, 3),
          ("rd_97",   (97, 3, 20, 2),       FEW_STEPS, 3),
          ("rd_100",  (100, 2, 10, 2),      FEW_STEPS, 3),
          ("rd_mu0",  (20, 0, 4, 2),        FEW_STEPS, 4),
          ("rd_ml0",  (20, 2, 0, 2),        FEW_STEPS, 4)]
CASES = [dict(name=n, shape=s, steps=st, level=lv) for n, s, st, lv in _TABLE]
BY_NAME = {c["name"]: c for c in CASES}


def fro(X):
    """Frobenius norm, scaled so that the squares of large entries do not overflow"""
    m = np.max(np.abs(X)) if X.size else 0.0
    if not np.isfinite(m) or m == 0:
        return m
    Y = X / m
    return m * np.sqrt(np.sum(Y * Y))


def project(A, Bu, Bl, G):
    """[A' | D] in float64 on LAPACK, as dlqr_reference._step_projected64 forms it"""
    if Bl.shape[1]:
        EF = np.linalg.solve(G @ Bl, G @ np.concatenate([A, Bu], axis=1))
        return A - Bl @ EF[:, :A.shape[1]], Bu - Bl @ EF[:, A.shape[1]:]
    return A.copy(), Bu.copy()


def single_step(Ap, D, Q, R):
    return Ap, (D @ np.linalg.solve(R, D.T) if D.shape[1] else np.zeros_like(Ap)), Q


def compose(one, two):
    """triple `one` applied after triple `two` -> (A, G, H, the increment of H)"""
    A1, G1, H1 = one
    A2, G2, H2 = two
    n = A1.shape[0]
    X = np.linalg.solve(np.eye(n) + G1 @ H2, np.concatenate([A1, G1], axis=1))
    XA, XG = X[:, :n], X[:, n:]
    inc = (A1.T @ H2) @ XA
    return A2 @ XA, G2 + (A2 @ XG) @ A2.T, H1 + inc, inc


def final_step(Ap, D, Q, R, X):
    """the recursion's own step on Pk = X -> (Ku, Pkp1)"""
    Ku = np.linalg.solve(R + D.T @ X @ D, D.T @ X @ Ap) if D.shape[1] else np.zeros((0, Ap.shape[0]))
    Abar = Ap - D @ Ku
    return Ku, Q + Ku.T @ R @ Ku + Abar.T @ X @ Abar


def schedule(n):
    """the operations of a fixed horizon of n >= 1 triples, in order: 'C' copy, 'A' accumulate, 'D' double"""
    ops, top, have = [], n.bit_length() - 1, False
    for b in range(top + 1):
        if (n >> b) & 1:
            ops.append("A" if have else "C")
            have = True
        if b < top:
            ops.append("D")
    return ops


def doubling_fixed(t, n):
    """the fixed-horizon schedule -> (the accumulated triple, doublings made, compositions made)"""
    d, a, levels, comps = t, None, 0, 0
    for op in schedule(n):
        if op == "C":
            a = d
        elif op == "A":
            a, comps = compose(a, d)[:3], comps + 1
        else:
            d, levels, comps = compose(d, d)[:3], levels + 1, comps + 1
    return a, levels, comps


def doubling_converge(t, tol, max_levels):
    """the run to convergence -> (H, levels, reason, increment norms of every level, norm(A) of every level)"""
    d, incs, ans, reason = t, [], [], 1
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(1, max_levels + 1):
            A, G, H, inc = compose(d, d)
            d = (A, G, H)
            incs.append(float(fro(inc)))
            ans.append(float(fro(A)))
            if incs[-1] < tol:
                reason = 0
                break
            if ans[-1] > GROWTH or not (np.isfinite(incs[-1]) and np.isfinite(ans[-1])):
                reason = 2
                break
    return d[2], len(incs), reason, incs, ans


def last_two(xs):
    xs = [float(x) for x in xs]
    return [xs[-1] if xs else np.nan, xs[-2] if len(xs) > 1 else np.nan]


def _step_ld(A, Bu, Bl, G, Q, R, Pk, dtype):
    """dlqr_reference._step with the closed loop it forms handed out as well: (Kuk, Pkp1, Abar)"""
    mu, ml = Bu.shape[1], Bl.shape[1]
    D = Bu - ref._rdiv(Bl, G @ Bl, dtype) @ (G @ Bu) if ml else Bu.copy()       # lqr.jl:151
    DtP = D.T @ Pk
    M = np.zeros((mu + ml, mu + ml), dtype=dtype)
    M[:mu, :mu] = R + DtP @ Bu                                               # lqr.jl:152
    if ml:
        M[:mu, mu:] = DtP @ Bl                                               # lqr.jl:153
        M[mu:, :mu] = G @ Bu                                                 # lqr.jl:154
        M[mu:, mu:] = G @ Bl                                                 # lqr.jl:155
    b = np.concatenate([DtP, G]) @ A                                         # lqr.jl:158
    Kk = ref.lu_solve(M, b, dtype) if mu + ml else np.zeros((0, A.shape[1]), dtype=dtype)   # lqr.jl:160
    Kuk, Klk = Kk[:mu], Kk[mu:]
    Abar = A - Bu @ Kuk - Bl @ Klk                                           # lqr.jl:169
    return Kuk, Q + Kuk.T @ R @ Kuk + Abar.T @ Pk @ Abar, Abar              # lqr.jl:170


def stepping(A, Bu, Bl, G, Q, R, steps, dtype=LD, projected=False):
    """`steps` backward steps from Pk = Q -> (Ku of the last step, its Pkp1): Ku[1] and the last Pkp1 of dlqr(.., N = steps + 1, tol = 0)"""
    A, Bu, Bl, G, Q, R = (np.asarray(x, dtype=dtype) for x in (A, Bu, Bl, G, Q, R))
    Pk = Q
    for _ in range(steps):
        if projected:
            Ku, Pk = ref._step_projected64(A, Bu, Bl, G, Q, R, Pk, dtype)
        else:
            Ku, Pk, _ = _step_ld(A, Bu, Bl, G, Q, R, Pk, dtype)
    return Ku, Pk


def stepping_converge(A, Bu, Bl, G, Q, R, tol, max_levels, dtype=LD):
    """the reference of a run to convergence: Pk and A(n) by single steps, looked at when Pk = H(2^j) -> (Ku, P of the final step, levels, reason, incs, ans)"""
    A, Bu, Bl, G, Q, R = (np.asarray(x, dtype=dtype) for x in (A, Bu, Bl, G, Q, R))
    An = A - Bl @ ref.lu_solve(G @ Bl, G @ A, dtype) if Bl.shape[1] else A      # A(1) = A'
    Pk, n, incs, ans, reason = Q, 1, [], [], 1                                    # Pk = H(n)
    for j in range(1, max_levels + 1):
        H0 = Pk
        while n < 2 ** j:
            _, Pk, Abar = _step_ld(A, Bu, Bl, G, Q, R, Pk, dtype)
            An, n = An @ Abar, n + 1
        incs.append(fro(Pk - H0))
        ans.append(fro(An))
        if incs[-1] < tol:
            reason = 0
            break
        if ans[-1] > GROWTH:
            reason = 2
            break
    Ku, P, _ = _step_ld(A, Bu, Bl, G, Q, R, Pk, dtype)
    return Ku, P, len(incs), reason, incs, ans


def _rel(X64, Xref):
    s = float(np.max(np.abs(Xref))) if Xref.size else 0.0
    return float(np.max(np.abs(np.asarray(X64, dtype=LD) - Xref))) / s if s > 0 else 0.0


def _models(name):
    """(A, Bu, Bl, G [nprob][...], Q, R) of a case: independent models under the case's own seed, one pair of exactly symmetric weights"""
    mx, mu, ml, nprob = BY_NAME[name]["shape"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    mods = [ref._model(rng, mx, mu, ml) for _ in range(nprob)]
    Q, R = ref._spd(rng, mx), ref._spd(rng, mu)
    return tuple(np.stack([m[i] for m in mods]) for i in range(4)) + (Q, R)


_built = {}


def build_case(name):
    """the problems of a case and their references, built once per session and left unchanged: dict with A, Bu, Bl, G, Q, R, nprob, mx, mu, ml, steps,
    fixed = {n: [per problem (Kref, Pref, levels, e64K, e64P, eK of the numpy schedule, eP of it)]}, tol, max_levels,
    conv = [per problem (Kref, Pref, levels, reason, dnorm [2], anorm [2], e64K, e64P, eK, eP)]"""
    if name in _built:
        return _built[name]
    c = BY_NAME[name]
    A, Bu, Bl, G, Q, R = _models(name)
    nprob, mx, mu, ml = A.shape[0], A.shape[1], Bu.shape[2], Bl.shape[2]
    proj = [project(A[p], Bu[p], Bl[p], G[p]) for p in range(nprob)]
    trip = [single_step(proj[p][0], proj[p][1], Q, R) for p in range(nprob)]
    fixed = {}
    for n in c["steps"]:
        rows = []
        for p in range(nprob):
            m = (A[p], Bu[p], Bl[p], G[p], Q, R)
            Kref, Pref = stepping(*m, n)
            a, levels, comps = doubling_fixed(trip[p], n)
            assert comps == bin(n).count("1") - 1 + n.bit_length() - 1
            twins = [stepping(*m, n, np.float64), stepping(*m, n, np.float64, True), final_step(proj[p][0], proj[p][1], Q, R, a[2])]
            eK, eP = [_rel(t[0], Kref) for t in twins], [_rel(t[1], Pref) for t in twins]
            rows.append((Kref.astype(np.float64), Pref.astype(np.float64), levels, max(eK), max(eP), eK[2], eP[2]))
        fixed[n] = rows
    # tol between the increments of the levels before and at c["level"] of problem 0: float64 first (cheap), then asserted on the longdouble norms of every problem
    _, _, _, incs0, _ = doubling_converge(trip[0], 0.0, c["level"] + 3)
    cand = [j for j in range(c["level"] - 1, len(incs0)) if incs0[j] < min(incs0[:j])]
    assert cand, "the increments of problem 0 never fall to a new minimum: no tol can be placed"
    tol = float(np.sqrt(incs0[cand[0]] * min(incs0[:cand[0]])))
    conv = []
    for p in range(nprob):
        m = (A[p], Bu[p], Bl[p], G[p], Q, R)
        Kref, Pref, levels, reason, incs, ans = stepping_converge(*m, tol, MAX_LEVELS)
        for x in incs:
            assert abs(float(x) - tol) > 1e-6 * tol, "a longdouble increment lies within 1e-6 of tol"
        for x in ans:
            assert abs(float(x) - GROWTH) > 1e-6 * GROWTH, "a longdouble norm(A) lies within 1e-6 of the growth limit"
        H, l64, r64, _, _ = doubling_converge(trip[p], tol, MAX_LEVELS)
        twins = [stepping(*m, 2 ** levels, np.float64), stepping(*m, 2 ** levels, np.float64, True), final_step(proj[p][0], proj[p][1], Q, R, H)]
        eK, eP = [_rel(t[0], Kref) for t in twins], [_rel(t[1], Pref) for t in twins]
        if (l64, r64) != (levels, reason):
            eK[2] = eP[2] = 1.0
        conv.append((Kref.astype(np.float64), Pref.astype(np.float64), levels, reason, last_two(incs), last_two(ans), max(eK), max(eP), eK[2], eP[2]))
    _built[name] = dict(c, A=A, Bu=Bu, Bl=Bl, G=G, Q=Q, R=R, nprob=nprob, mx=mx, mu=mu, ml=ml, fixed=fixed, tol=tol, max_levels=MAX_LEVELS, conv=conv)
    return _built[name]


def unstable_problem():
    """one problem with mu = 0, ml = 0 and spectral radius 1.05: H and A grow until norm(A(2^j)) passes 1e50 -> (A, Bu, Bl, G, Q, R, levels, reason of the numpy
    schedule with tol 1e-5 and 40 levels)"""
    rng = np.random.default_rng(zlib.crc32(b"rd_unstable"))
    A, Bu, Bl, G = ref._model(rng, 12, 0, 0, 1.05)
    Q, R = ref._spd(rng, 12), np.zeros((0, 0))
    _, levels, reason, _, ans = doubling_converge(single_step(A, Bu, Q, R), 1e-5, 40)
    assert reason == 2 and abs(ans[-1] - GROWTH) > 1e-6 * GROWTH and ans[-2] < GROWTH * (1 - 1e-6)
    return A, Bu, Bl, G, Q, R, levels, reason


def check(K, P, Kref, Pref, e64K, e64P, what):
    """the acceptance rule on one problem's gain and cost-to-go; prints every figure before it asserts"""
    bK, bP = ref.tolerance(e64K), ref.tolerance(e64P)
    sK, sP = (float(np.abs(Kref).max()) if Kref.size else 0.0), float(np.abs(Pref).max())
    eK = (float(np.abs(K - Kref).max()) if np.isfinite(K).all() else np.inf) if Kref.size else 0.0
    eP = float(np.abs(P - Pref).max()) if np.isfinite(P).all() else np.inf
    print("%s: max|K - Kref| = %.3g relative, bound %.3g (e64K %.3g); max|P - Pref| = %.3g relative, bound %.3g (e64P %.3g)"
          % (what, eK / sK if sK else 0.0, bK, e64K, eP / sP, bP, e64P))
    assert eK <= bK * sK, "%s: max|K - Kref| = %.3g relative, bound %.3g" % (what, eK / sK, bK)
    assert eP <= bP * sP, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, eP / sP, bP)


def check_norms(got, want, bound, scale, name, what):
    for j in range(2):
        if np.isnan(want[j]):
            assert np.isnan(got[j]), "%s: %s[%d] = %r where no such level ran" % (what, name, j, got[j])
        else:
            assert abs(got[j] - want[j]) <= bound * max(abs(want[j]), scale), "%s: %s[%d] = %.17g, reference %.17g, bound %.3g of max(|ref|, %.3g)" % (
                what, name, j, got[j], want[j], bound, scale)


def refusal_call(capi, pr):
    """cclqr_riccati_doubling through ctypes on sentinel-filled outputs, for tests/test_gpu_riccati_doubling.py and tests/test_analysis_refusals_host.py.  pr: nprob, mx,
    mu, ml, tol and the arrays A, Bu, Bl, G, Q, R.  The call returns (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml = pr["nprob"], pr["mx"], pr["mu"], pr["ml"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: a.ctypes.data_as(dp)
    A, Bu, Bl, G, Q, R = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "Q", "R"))

    def call(n_weights=1, N=10, tol=pr["tol"], max_levels=40, bf16=0, nprob=n, A_=A, K_=True, Bl_=Bl, Q_=Q, R_=R, mx_=mx):
        K, P = np.full((n, mu, mx), 7.5), np.full((n, mx, mx), 7.5)
        lv, rs = np.full(n, -9, dtype=np.int32), np.full(n, -9, dtype=np.int32)
        dn, an = np.full((n, 2), 7.5), np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(0, bf16, 1, 0)
        rc = L.cclqr_riccati_doubling(C.c_int32(nprob), C.c_int32(mx_), C.c_int32(mu), C.c_int32(ml), None if A_ is None else d(A_), d(Bu), d(Bl_), d(G),
                                      C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(N), C.c_double(tol), C.c_int32(max_levels), d(K) if K_ else None, d(P),
                                      lv.ctypes.data_as(ip), rs.ctypes.data_as(ip), d(dn), d(an), C.byref(o))
        untouched = bool((K == 7.5).all() and (P == 7.5).all() and (lv == -9).all() and (rs == -9).all() and (dn == 7.5).all() and (an == 7.5).all())
        return rc, untouched, L.cclqr_last_error().decode()

    return call


def refusal_cases(pr):
    """what cclqr_riccati_doubling refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (mu >= 2: a 1 x 1 R cannot fail to be symmetric)"""
    Qn, Rn = np.ascontiguousarray(pr["Q"]).copy(), np.ascontiguousarray(pr["R"]).copy()
    Qn[0, 1] = np.nextafter(Qn[0, 1], np.inf)
    Rn[1, 0] = np.nextafter(Rn[1, 0], np.inf)
    return dict(N_1=dict(N=1), N_neg=dict(N=-1), levels_0=dict(N=0, max_levels=0), levels_61=dict(N=0, max_levels=61), tol_neg=dict(tol=-1e-9),
                tol_nan=dict(tol=float("nan")), tol_nan_conv=dict(N=0, tol=float("nan")), n_weights_2=dict(n_weights=pr["nprob"] + 1), n_weights_0=dict(n_weights=0),
                bf16=dict(bf16=2), nprob_0=dict(nprob=0), mx_0=dict(mx_=0), mx_huge=dict(mx_=20000), A_null=dict(A_=None), K_null=dict(K_=False),
                Q_nonsym=dict(Q_=Qn), R_nonsym=dict(R_=Rn))
