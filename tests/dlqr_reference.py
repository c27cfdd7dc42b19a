"""Plain restatement of the reference's dlqr in extended precision: the checker of the Riccati launch-shape sweep
(tests/test_riccati_reference.py on the CPU, tests/test_gpu_riccati_sweep.py on the device).

`dlqr` follows src/control/lqr.jl:141-184 statement by statement -- the (mu+ml)-square system M Kk = b, NOT the projected form the kernels
use -- with its own partially pivoted LU in `dtype` (np.linalg does not take longdouble; on x86-64 that is the 80-bit type, eps 1.1e-19).
`dlqr_tv` is the same recursion on per-knot models, src/control/lqr_tracking.jl:73-122 in the knot convention of cclqr_riccati_tv
(include/cclqr.h: the model of backward step k at index k-1).  Two float64 twins calibrate what "as accurate as fp64 can be" means for a
case: `dlqr` itself with dtype=np.float64, and `dlqr_projected64`, the kernels' form S = R + D'PkD on LAPACK solves.

`riccati_kernels` mirrors the launch-shape choice of csrc/riccati.hip (launch_riccati), so that a test can say which kernels a case runs on.
"""
import numpy as np

LD = np.longdouble


class SingularPivot(ArithmeticError):
    """a factorisation the recursion reaches meets an exact zero pivot (Julia's LAPACK SingularException, lqr.jl:151,160)"""


def lu_solve(M, b, dtype=LD):
    """M \\ b by LU with partial pivoting (first row of largest magnitude, as LAPACK's getrf), all arithmetic in `dtype`"""
    M = np.array(M, dtype=dtype, copy=True)
    x = np.array(b, dtype=dtype, copy=True)
    vec = x.ndim == 1
    if vec:
        x = x[:, None]
    n = M.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if M[p, c] == 0:
            raise SingularPivot("zero pivot in column %d" % c)
        if p != c:
            M[[c, p]] = M[[p, c]]
            x[[c, p]] = x[[p, c]]
        l = M[c + 1:, c] / M[c, c]
        M[c + 1:, c] = l
        M[c + 1:, c + 1:] -= np.outer(l, M[c, c + 1:])
        x[c + 1:] -= np.outer(l, x[c])
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - M[i, i + 1:] @ x[i + 1:]) / M[i, i]
    return x[:, 0] if vec else x


def _rdiv(X, Y, dtype):
    """X / Y (Julia's right division) = (Y' \\ X')'"""
    return lu_solve(Y.T, X.T, dtype).T


def _step(A, Bu, Bl, G, Q, R, Pk, dtype):
    """one backward step of lqr.jl:151-170: returns (Kuk, Pkp1)"""
    mu, ml = Bu.shape[1], Bl.shape[1]
    D = Bu - _rdiv(Bl, G @ Bl, dtype) @ (G @ Bu) if ml else Bu.copy()       # D = Bu - Bλ/(G*Bλ)*G*Bu      lqr.jl:151
    DtP = D.T @ Pk
    M = np.zeros((mu + ml, mu + ml), dtype=dtype)
    M[:mu, :mu] = R + DtP @ Bu                                            # M11 = R + D'*Pk*Bu           lqr.jl:152
    if ml:
        M[:mu, mu:] = DtP @ Bl                                            # M12 = D'*Pk*Bλ               lqr.jl:153
        M[mu:, :mu] = G @ Bu                                              # M21 = G*Bu                   lqr.jl:154
        M[mu:, mu:] = G @ Bl                                              # M22 = G*Bλ                   lqr.jl:155
    b = np.concatenate([DtP, G]) @ A                                      # b = [D'*Pk;G]*A              lqr.jl:158
    Kk = lu_solve(M, b, dtype) if mu + ml else np.zeros((0, A.shape[1]), dtype=dtype)   # Kk = M\b     lqr.jl:160
    Kuk, Klk = Kk[:mu], Kk[mu:]
    Abar = A - Bu @ Kuk - Bl @ Klk                                        #                              lqr.jl:169
    Pkp1 = Q + Kuk.T @ R @ Kuk + Abar.T @ Pk @ Abar                       #                              lqr.jl:170
    return Kuk, Pkp1


def _sweep(model, Q, R, N, tol, dtype, step):
    """for outer k=N-1:-1:1 ... back-fill (lqr.jl:147-181); model(k) -> (A, Bu, Bl, G) of backward step k"""
    Q, R = np.asarray(Q, dtype=dtype), np.asarray(R, dtype=dtype)
    mx = Q.shape[0]
    mu = R.shape[0]
    K = np.zeros((max(N - 1, 0), mu, mx), dtype=dtype)
    norms = []
    Pk = Q
    k = 0
    for k in range(N - 1, 0, -1):
        A, Bu, Bl, G = (np.asarray(x, dtype=dtype) for x in model(k))
        Kuk, Pkp1 = step(A, Bu, Bl, G, Q, R, Pk, dtype)
        K[k - 1] = Kuk                                                    # Ku[k][i] = Kk[i:i,:]          lqr.jl:162-164
        nrm = np.sqrt(np.sum((Pk - Pkp1) ** 2))                           # norm(Pk-Pkp1): Frobenius
        norms.append(nrm)
        if nrm < tol:                                                     #                              lqr.jl:172-174
            break
        Pk = Pkp1
    # `for outer k`: after a completed loop k holds its last value (1); with N = 1 the loop never ran and k is still 0
    for k2 in range(k - 1, 0, -1):                                        # Ku[k2] = Ku[k2+1]            lqr.jl:179-181
        K[k2 - 1] = K[k2]
    return K, k, norms


def dlqr(A, Bu, Bl, G, Q, R, N, tol, dtype=LD):
    """lqr.jl:141-184 on one time-invariant problem: A [mx][mx], Bu [mx][mu], Bl [mx][ml], G [ml][mx].
    Returns (K [N-1][mu][mx] in dtype, kbreak, [norm(Pk - Pkp1) of every executed step, in step order k = N-1, N-2, ...])."""
    return _sweep(lambda k: (A, Bu, Bl, G), Q, R, N, tol, dtype, _step)


def dlqr_tv(A, Bu, Bl, G, Q, R, N, tol, dtype=LD):
    """lqr_tracking.jl:73-122 on caller models: A [N-1][mx][mx] ... with the model of backward step k at index k-1 (cclqr_riccati_tv)"""
    return _sweep(lambda k: (A[k - 1], Bu[k - 1], Bl[k - 1], G[k - 1]), Q, R, N, tol, dtype, _step)


def _step_projected64(A, Bu, Bl, G, Q, R, Pk, dtype):
    """the kernels' projected form in float64 on LAPACK: E = (GBλ)^-1 G Bu, F = (GBλ)^-1 G A, D = Bu - Bλ E, A' = A - Bλ F,
    Ku = (R + D'PkD) \\ D'PkA', Abar = A' - D Ku (riccati.hip, the comment above RIC_MU_REG)"""
    mu, ml = Bu.shape[1], Bl.shape[1]
    if ml:
        try:
            EF = np.linalg.solve(G @ Bl, G @ np.concatenate([A, Bu], axis=1))
        except np.linalg.LinAlgError as e:
            raise SingularPivot(str(e))
        Ap, D = A - Bl @ EF[:, :A.shape[1]], Bu - Bl @ EF[:, A.shape[1]:]
    else:
        Ap, D = A, Bu
    if mu:
        try:
            Kuk = np.linalg.solve(R + D.T @ Pk @ D, D.T @ Pk @ Ap)
        except np.linalg.LinAlgError as e:
            raise SingularPivot(str(e))
    else:
        Kuk = np.zeros((0, A.shape[1]))
    Abar = Ap - D @ Kuk
    return Kuk, Q + Kuk.T @ R @ Kuk + Abar.T @ Pk @ Abar


def dlqr_projected64(A, Bu, Bl, G, Q, R, N, tol):
    return _sweep(lambda k: (A, Bu, Bl, G), Q, R, N, tol, np.float64, _step_projected64)


def dlqr_tv_projected64(A, Bu, Bl, G, Q, R, N, tol):
    return _sweep(lambda k: (A[k - 1], Bu[k - 1], Bl[k - 1], G[k - 1]), Q, R, N, tol, np.float64, _step_projected64)


def reference(A, Bu, Bl, G, Q, R, N, tol, tv=False):
    """the longdouble reference and the error budget of a case: returns (K as float64, kbreak, norms, e64) where e64 is the larger
    relative error max|K64 - Kref| / max|Kref| of the two float64 twins (a twin that breaks at another index counts as error 1)"""
    full, proj = (dlqr_tv, dlqr_tv_projected64) if tv else (dlqr, dlqr_projected64)
    K, kb, norms = full(A, Bu, Bl, G, Q, R, N, tol, LD)
    scale = float(np.max(np.abs(K))) if K.size else 0.0
    e64 = 0.0
    for K64, kb64, _ in (full(A, Bu, Bl, G, Q, R, N, tol, np.float64), proj(A, Bu, Bl, G, Q, R, N, tol)):
        if kb64 != kb:
            e64 = max(e64, 1.0)
        elif scale > 0:
            e64 = max(e64, float(np.max(np.abs(K64.astype(LD) - K))) / scale)
    return K.astype(np.float64), kb, [float(x) for x in norms], e64


def tolerance(e64):
    """the acceptance bound on max|K - Kref| / max|Kref|: ten times what a straightforward fp64 implementation of either formulation
    loses, never tighter than 1e-12 and never looser than the suite's 1e-7"""
    return min(max(10.0 * e64, 1e-12), 1e-7)


# ---------------------------------------------------------------------------------------------------------------------------------
# synthetic problems

def _orth(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def _spd(rng, n, lo=0.5, hi=2.0):
    V = _orth(rng, n)
    S = (V * rng.uniform(lo, hi, n)) @ V.T
    return 0.5 * (S + S.T)          # exactly symmetric (the host routes a Q or R that is not to the kernels that do not assume it)


def _model(rng, mx, mu, ml, rho=0.97):
    """A with spectral radius rho, Bu of unit-size columns, and (G, Bλ) with G Bλ = U diag(1..10) V' (condition number 10)"""
    A = rng.normal(size=(mx, mx)) / np.sqrt(mx)
    A *= rho / np.max(np.abs(np.linalg.eigvals(A)))
    Bu = rng.normal(size=(mx, mu)) / np.sqrt(mx) * 2.0
    if ml:
        O = _orth(rng, mx)
        Gr = O[:ml]                                           # orthonormal rows
        C = (_orth(rng, ml) * np.logspace(0, 1, ml)) @ _orth(rng, ml).T
        Z = rng.normal(size=(mx, ml)) / np.sqrt(mx)
        Bl = Gr.T @ C + (Z - Gr.T @ (Gr @ Z))                 # G Bλ = C up to rounding
        G = 2.0 * Gr
    else:
        Bl, G = np.zeros((mx, 0)), np.zeros((0, mx))
    return A, Bu, Bl, G


def choose_tol(norm_lists, break_at, margin=1e-6):
    """tol such that the first problem's sweep breaks where wanted: 'first' (at the first step), 'mid', or 'never' (tol = 0);
    break_at may also be an int = the number of executed steps before the one that breaks.  Asserts that no executed norm of any
    problem lies within tol (1 +- margin), so that the break index cannot depend on rounding."""
    if break_at == "never":
        return 0.0
    n0 = norm_lists[0]
    if break_at == "first":
        tol = 2.0 * n0[0]
    else:
        j = len(n0) // 2 if break_at == "mid" else int(break_at)
        # the break comes at step j when norm j is a new minimum: tol between it and the smallest norm before it
        cand = [i for i in range(max(j, 1), len(n0)) if n0[i] < min(n0[:i])]
        assert cand, "norms never reach a new minimum: no break can be placed"
        j = cand[0]
        tol = float(np.sqrt(n0[j] * min(n0[:j])))
    for nl in norm_lists:
        for x in nl:
            assert abs(x - tol) > margin * tol, "an executed norm %.17g lies within 1e-6 of tol %.17g" % (x, tol)
    return tol


def make_problem(rng, mx, mu, ml, nprob=1, break_at="mid", N=12, tv=False, R=None, Q=None, rho=0.97, ref_idx=None):
    """synthetic well-conditioned dlqr problems.  Returns a dict: A, Bu, Bl, G ([nprob][...], or [N-1][...] with tv), Q, R, N, tol and
    `ref` = {problem: (K, kbreak, norms, e64)} from the longdouble reference at that tol, for the problems in ref_idx (default: all)."""
    if tv:
        assert nprob == 1
        base = _model(rng, mx, mu, ml, rho)
        # per-knot models: the base model with a knot-dependent perturbation (a trajectory's linearisations drift along it)
        mods = []
        for _ in range(N - 1):
            A, Bu, Bl, G = base
            A = A + 0.02 * rng.normal(size=A.shape) / np.sqrt(mx)
            Bu = Bu + 0.05 * rng.normal(size=Bu.shape) / np.sqrt(mx)
            Bl = Bl + 0.02 * rng.normal(size=Bl.shape) / np.sqrt(mx)
            mods.append((A, Bu, Bl, G))
        models = [tuple(np.stack([m[i] for m in mods]) for i in range(4))]
    else:
        models = [_model(rng, mx, mu, ml, rho) for _ in range(nprob)]
    Q = _spd(rng, mx) if Q is None else np.asarray(Q, dtype=np.float64)
    R = _spd(rng, mu) if R is None else np.asarray(R, dtype=np.float64)
    full = dlqr_tv if tv else dlqr
    # norms at tol = 0 (the whole sweep), in float64: enough to place the break
    ref_idx = list(range(len(models))) if ref_idx is None else list(ref_idx)
    norm_lists = [full(*models[p], Q, R, N, 0.0, np.float64)[2] for p in ref_idx]
    tol = choose_tol(norm_lists, break_at)
    ref = {p: reference(*models[p], Q, R, N, tol, tv=tv) for p in ref_idx}
    for r in ref.values():
        for x in r[2]:
            assert tol == 0.0 or abs(x - tol) > 1e-6 * tol, "a longdouble norm lies within 1e-6 of tol"
    A, Bu, Bl, G = (np.stack([m[i] for m in models]) if not tv else models[0][i] for i in range(4))
    return dict(A=A, Bu=Bu, Bl=Bl, G=G, Q=Q, R=R, N=N, tol=tol, ref=ref, mx=mx, mu=mu, ml=ml, nprob=nprob, tv=tv)


# ---------------------------------------------------------------------------------------------------------------------------------
# mirror of the launch-shape choice in csrc/riccati.hip

RIC_WAVES = 8
RIC_YB = 128
RIC_MU_REG = 7            # riccati.hip: #define RIC_MU_REG
RIC_LDS_M = 96            # riccati.hip: #define RIC_LDS_M
RIC_LU_LANES = 64         # the resident kernel's pivoted LU runs on one wavefront


def ric_resident_is_frag(mx, mu):
    """riccati.hip ric_resident_is_frag"""
    return (mu == 1 and mx in (12, 24, 48)) or (mu == 7 and mx == 84)


def ric_resident_lds_bytes(mx, mu):
    """riccati.hip ric_resident_lds_bytes"""
    na = mx + mu
    return (mx * mx + mx * na + mx * mu + 2 * mu * mx + mu * na + 2 * mu * mu + 2 * RIC_WAVES + 2 +
            (RIC_WAVES * RIC_YB if ric_resident_is_frag(mx, mu) else 0)) * 8 + (mu + 2) * 4


def ric_resident_fits(mx, mu):
    """riccati.hip ric_resident_fits: P and W in one CU's LDS, whole k-groups of four, at most one wavefront per 16-column block of [A'|D],
    and a mu the one-wavefront pivoted LU covers"""
    return ric_resident_lds_bytes(mx, mu) <= 158 * 1024 and mx % 4 == 0 and (mx + mu + 15) // 16 <= RIC_WAVES and mu <= RIC_LU_LANES


def ric_use_tiled(mx, mu, nprob, path):
    """riccati.hip ric_use_tiled (fp64 mode)"""
    if not ric_resident_fits(mx, mu):
        return True
    if path != 0:
        return path == 2
    return mx >= 64 and nprob < 128


def riccati_kernels(mx, mu, ml, nprob, path=0, symmetric=True):
    """the kernels launch_riccati starts for a case: a set of names as rocprofv3 shows them (template arguments included)"""
    ks = {"ric_project_kernel<%s>" % ("true" if 0 < ml <= RIC_LDS_M else "false")}
    if ric_use_tiled(mx, mu, nprob, path):
        return ks | {"ric_pa_kernel", "ric_gain_update_kernel", "ric_pn_kernel", "ric_backfill_kernel"}
    mut = mu if 1 <= mu <= RIC_MU_REG else 0
    ngt = 0
    if symmetric and ric_resident_is_frag(mx, mu):
        ngt = mx // 4
    return ks | {"riccati_resident_kernel<%d, %d, 0>" % (mut, ngt)}
