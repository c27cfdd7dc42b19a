"""Shared by tests/test_policy_value_reference.py (CPU), tests/test_gpu_policy_value.py and tests/test_gpu_policy_cost.py: the cases of the policy evaluation
(cclqr_policy_value: dlqr's cost recursion, lqr.jl:147-177, with the gain given) and their extended-precision reference.

The recursion, restated:
    Pk = Q
    for k = N-1:-1:1
        Kuk  = K_t[k]  (nK == N-1)  or  K_t[1]  (nK == 1: a stationary gain)
        Kλk  = (G Bλ) \\ (G (A - Bu Kuk))            second block row of M Kk = b, lqr.jl:154-160
        Abar = A - Bu Kuk - Bλ Kλk                    lqr.jl:169
        Pkp1 = Q + Kuk' R Kuk + Abar' Pk Abar         lqr.jl:170
        norm(Pk - Pkp1) < tol -> break                lqr.jl:172
        Pk = Pkp1
The reference runs it in np.longdouble on dlqr_reference.lu_solve.  e64P of a problem is the larger deviation max|P64 - Pref| / max|Pref| of two float64 twins -- the
form above on lu_solve in float64, and the kernels' projected form Abar = A' - D Kuk on LAPACK solves --; a twin that breaks at another index counts as deviation 1.

The acceptance rule, for every case: kbreak equal; max|P - Pref| <= tolerance(e64P) max|Pref|; each norm of dnorm within the same relative bound of the reference's,
|dnorm - ref| <= tolerance(e64P) max(|ref|, max|Pref|) (a norm the reference does not have -- no such step ran -- must be NaN).  The scale: dnorm is the norm of a
DIFFERENCE of two costs-to-go, each of which is known to tolerance(e64P) max|Pref| per entry, so its absolute error lives on P's scale, not on its own -- a converged
sweep's last norm is 1e-5 of max|P|, and the float64 twins themselves miss it by 1e-11 of ITS size (1e-16 of P's).  No factor for the mx^2 entries a Frobenius norm
sums is granted.

A case: seed crc32(name); base model dlqr_reference._model(rng, mx, mu, ml), Q = _spd, R = _spd; the gain table is the float64 dlqr of the base model at tol = 0;
problem p is the base model with A, Bu, Bλ each perturbed by pert p N(0,1) / sqrt(mx), so problem 0 is the model the table was designed on; tol from
choose_tol(..., "mid") on the float64 norms of every problem."""
import ctypes as C
import zlib

import numpy as np

import dlqr_reference as ref

LD = np.longdouble

#            name            mx  mu  ml  nprob N   paths
_TABLE = [("pv_frag_1_3",    12, 1,  5,  3,   16, (0, 1, 2)),
          ("pv_frag_1_6",    24, 1,  10, 3,   16, (0, 1, 2)),
          ("pv_frag_7_21",   84, 7,  35, 2,   10, (0, 1, 2)),
          ("pv_reg_mu2",     36, 2,  15, 3,   12, (0, 1, 2)),
          ("pv_ldslu_40_8",  40, 8,  10, 2,   10, (0, 1, 2)),
          ("pv_tiled_30",    30, 3,  10, 3,   10, (0, 2)),
          ("pv_tiled_97",    97, 3,  30, 2,   8,  (0, 2)),
          ("pv_mu0",         24, 0,  10, 2,   10, (0, 1, 2)),
          ("pv_ml0",         16, 2,  0,  2,   12, (0, 1, 2)),
          ("pv_nonsym",      24, 1,  10, 3,   10, (0, 1, 2)),
          ("pv_stationary",  24, 1,  10, 3,   40, (0, 1, 2)),
          ("pv_unstable",    24, 1,  10, 3,   40, (0, 1, 2))]
CASES = [dict(name=n, mx=mx, mu=mu, ml=ml, nprob=np_, N=N, paths=paths, nK=1 if n in ("pv_stationary", "pv_unstable") else N - 1,
              pert=0.4 if n == "pv_unstable" else 0.05) for n, mx, mu, ml, np_, N, paths in _TABLE]
BY_NAME = {c["name"]: c for c in CASES}


def policy_sweep(A, Bu, Bl, G, Q, R, Kt, N, tol, dtype=LD, projected=False):
    """the recursion above on one problem; Kt [nK][mu][mx] with nK = N - 1 or 1.  Returns (P = the last Pkp1 computed, Q when N = 1; kbreak = the loop index after the
    loop; [norm(Pk - Pkp1) of every executed step, in step order]).  projected: the kernels' form A' = A - Bλ (G Bλ)^-1 G A, D = Bu - Bλ (G Bλ)^-1 G Bu,
    Abar = A' - D Kuk on np.linalg.solve (float64 only)"""
    A, Bu, Bl, G, Q, R, Kt = (np.asarray(x, dtype=dtype) for x in (A, Bu, Bl, G, Q, R, Kt))
    ml = Bl.shape[1]
    if projected:
        assert dtype == np.float64
        if ml:
            EF = np.linalg.solve(G @ Bl, G @ np.concatenate([A, Bu], axis=1))
            Ap, D = A - Bl @ EF[:, :A.shape[1]], Bu - Bl @ EF[:, A.shape[1]:]
        else:
            Ap, D = A, Bu
    Pk = Q
    P = Q
    norms = []
    k = 0
    for k in range(N - 1, 0, -1):
        Kuk = Kt[k - 1] if Kt.shape[0] > 1 else Kt[0]
        if projected:
            Abar = Ap - D @ Kuk
        else:
            Abar = A - Bu @ Kuk
            if ml:
                Abar = Abar - Bl @ ref.lu_solve(G @ Bl, G @ Abar, dtype)          # Kλk = (G Bλ) \ (G (A - Bu Kuk))
        Pkp1 = Q + Kuk.T @ R @ Kuk + Abar.T @ Pk @ Abar
        P = Pkp1
        nrm = np.sqrt(np.sum((Pk - Pkp1) ** 2))
        norms.append(nrm)
        if nrm < tol:
            break
        Pk = Pkp1
    return P, k, norms


def last_two(norms):
    """dnorm of a sweep: the norm of the last executed step and of the step before it, NaN where no such step ran"""
    return np.array([float(norms[-1]) if len(norms) > 0 else np.nan, float(norms[-2]) if len(norms) > 1 else np.nan])


def reference(A, Bu, Bl, G, Q, R, Kt, N, tol):
    """(P as float64 from the longdouble run, kbreak, dnorm [2], e64P, all longdouble norms as floats)"""
    P, kb, norms = policy_sweep(A, Bu, Bl, G, Q, R, Kt, N, tol, LD)
    scale = float(np.max(np.abs(P)))
    e64 = 0.0
    for projected in (False, True):
        P64, kb64, _ = policy_sweep(A, Bu, Bl, G, Q, R, Kt, N, tol, np.float64, projected)
        e64 = max(e64, 1.0 if kb64 != kb else float(np.max(np.abs(P64.astype(LD) - P))) / scale)
    return P.astype(np.float64), kb, last_two(norms), e64, [float(x) for x in norms]


_built = {}


def build_case(name):
    """the problems of a case and their references, built once per session and left unchanged: dict with A, Bu, Bl, G [nprob][...], Q, R, K [nK][mu][mx] (the table),
    Kfull [N-1][mu][mx], N, nK, tol, ref = [reference(...) per problem]"""
    if name in _built:
        return _built[name]
    c = BY_NAME[name]
    mx, mu, ml, nprob, N = c["mx"], c["mu"], c["ml"], c["nprob"], c["N"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A, Bu, Bl, G = ref._model(rng, mx, mu, ml)
    Q, R = ref._spd(rng, mx), ref._spd(rng, mu)
    if name == "pv_nonsym":
        M = rng.normal(size=(mx, mx))
        Q = Q + 0.3 * (M - M.T) / np.sqrt(mx)
    Kfull = ref.dlqr(A, Bu, Bl, G, Q, R, N, 0.0, np.float64)[0]
    K = np.ascontiguousarray(Kfull[:1] if c["nK"] == 1 else Kfull)
    As, Bus, Bls = [A], [Bu], [Bl]
    for p in range(1, nprob):
        s = c["pert"] * p / np.sqrt(mx)
        As.append(A + s * rng.normal(size=A.shape))
        Bus.append(Bu + s * rng.normal(size=Bu.shape))
        Bls.append(Bl + s * rng.normal(size=Bl.shape))
    As, Bus, Bls, Gs = np.stack(As), np.stack(Bus), np.stack(Bls), np.stack([G] * nprob)
    norm_lists = [policy_sweep(As[p], Bus[p], Bls[p], G, Q, R, K, N, 0.0, np.float64)[2] for p in range(nprob)]
    tol = ref.choose_tol(norm_lists, "mid")
    refs = [reference(As[p], Bus[p], Bls[p], G, Q, R, K, N, tol) for p in range(nprob)]
    for r in refs:
        for x in r[4]:
            assert abs(x - tol) > 1e-6 * tol, "a longdouble norm lies within 1e-6 of tol"
    _built[name] = dict(c, A=As, Bu=Bus, Bl=Bls, G=Gs, Q=Q, R=R, K=K, Kfull=Kfull, tol=tol, ref=refs)
    return _built[name]


def check(P, kb, dn, refp, what):
    """the acceptance rule on one problem; prints every figure before it asserts"""
    Pref, kbref, dnref, e64, _ = refp
    bound = ref.tolerance(e64)
    scale = float(np.abs(Pref).max())
    err = float(np.abs(P - Pref).max()) if np.isfinite(P).all() else np.inf
    print("%s: kbreak %d (reference %d), max|P - Pref| = %.3g relative, bound %.3g (e64P %.3g, max|Pref| %.3g), dnorm %s (reference %s)"
          % (what, kb, kbref, err / scale, bound, e64, scale, dn, dnref))
    assert int(kb) == kbref, "%s: kbreak %d, reference %d" % (what, kb, kbref)
    assert err <= bound * scale, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, err / scale, bound)
    if dn is not None:
        for j in range(2):
            if np.isnan(dnref[j]):
                assert np.isnan(dn[j]), "%s: dnorm[%d] = %r where no such step ran" % (what, j, dn[j])
            else:
                assert abs(dn[j] - dnref[j]) <= bound * max(abs(dnref[j]), scale), "%s: dnorm[%d] = %.17g, reference %.17g, bound %.3g of max(|ref|, max|Pref| = %.3g)" % (
                    what, j, dn[j], dnref[j], bound, scale)


def refusal_call(capi, pr):
    """cclqr_policy_value through ctypes on sentinel-filled outputs, for tests/test_gpu_policy_value.py and tests/test_analysis_refusals_host.py.  pr: nprob, mx, mu, ml,
    N, tol and the contiguous arrays A, Bu, Bl, G, K, Q, R.  The call returns (rc, outputs untouched, cclqr_last_error())"""
    L = capi.lib()
    n, mx, mu, ml, N = pr["nprob"], pr["mx"], pr["mu"], pr["ml"], pr["N"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: a.ctypes.data_as(dp)
    A, Bu, Bl, G, K, Q, R = (np.ascontiguousarray(pr[k]) for k in ("A", "Bu", "Bl", "G", "K", "Q", "R"))

    def call(n_gains=1, nK=N - 1, n_weights=1, N_=N, path=0, bf16=0, nprob=n, A_=A, P_=True, K_=K):
        P = np.full((n, mx, mx), 7.5)
        kb = np.full(n, -9, dtype=np.int32)
        dn = np.full((n, 2), 7.5)
        o = capi.RiccatiOpts(path, bf16, 0, 0)
        rc = L.cclqr_policy_value(C.c_int32(nprob), C.c_int32(mx), C.c_int32(mu), C.c_int32(ml), None if A_ is None else d(A_), d(Bu), d(Bl), d(G), C.c_int32(n_gains),
                                  C.c_int32(nK), None if K_ is None else d(K_), C.c_int32(n_weights), d(Q), d(R), C.c_int32(N_), C.c_double(pr["tol"]),
                                  d(P) if P_ else None, kb.ctypes.data_as(ip), d(dn), C.byref(o))
        return rc, bool((P == 7.5).all() and (kb == -9).all() and (dn == 7.5).all()), L.cclqr_last_error().decode()

    return call


def refusal_cases(pr):
    """what cclqr_policy_value refuses as CCLQR_EINVAL: name -> the arguments of refusal_call's call (nprob must not be 2)"""
    N = pr["N"]
    return dict(n_gains_2=dict(n_gains=2), n_gains_0=dict(n_gains=0), nK_2=dict(nK=2), nK_0=dict(nK=0), nK_N=dict(nK=N), n_weights_2=dict(n_weights=2),
                n_weights_0=dict(n_weights=0), N_0=dict(N_=0), path_3=dict(path=3), path_neg=dict(path=-1), bf16=dict(bf16=2), nprob_0=dict(nprob=0),
                A_null=dict(A_=None), P_null=dict(P_=False), K_null=dict(K_=None))
