"""Shared by tests/test_riccati_weights_reference.py (CPU) and tests/test_gpu_riccati_weights.py: the cases of the per-problem-weights Riccati
(cclqr_riccati_weights) and their extended-precision references.

A case is `nprob` synthetic models (dlqr_reference._model), seeded by crc32(name); problem p has its own weights Q_p = _spd(mx) 10^p and R_p = _spd(mu) 10^-p, so
that neighbouring problems' gains differ by orders of magnitude more than any tolerance.  tol is placed by dlqr_reference.choose_tol on the float64 norms of ALL
problems (the first problem breaks mid-sweep, no norm of any problem lies within 1e-6 of tol); the reference of problem p is dlqr_reference.reference on
(model_p, Q_p, R_p).  Every case is built once per session."""
import zlib

import numpy as np

import dlqr_reference as ref


def W(name, mx, mu, ml, nprob, N, paths=(0, 1, 2), nonsym=()):
    return dict(name=name, mx=mx, mu=mu, ml=ml, nprob=nprob, N=N, paths=paths, nonsym=tuple(nonsym))


CASES = [
    W("w_frag_1_3", 12, 1, 5, 3, 16), W("w_frag_1_6", 24, 1, 10, 3, 16), W("w_frag_7_21", 84, 7, 35, 2, 10),      # register-fragment kernels <1,3> <1,6> <7,21>
    W("w_reg_mu2", 36, 2, 15, 3, 12),                # generic register <2,0>
    W("w_ldslu_40_8", 40, 8, 10, 2, 10),             # LDS-LU <0,0>
    W("w_tiled_30", 30, 3, 10, 3, 10, paths=(0, 2)), W("w_tiled_97", 97, 3, 30, 2, 8, paths=(0, 2)),       # the tiled three-launch step, edge tiles
    W("w_mu0", 24, 0, 10, 2, 10),
    W("w_nonsym_one", 24, 1, 10, 3, 10, nonsym=(1,)),      # only problem 1's Q is not symmetric: the whole call runs on the non-mirrored kernels of <1,0>
]
BY_NAME = {c["name"]: c for c in CASES}

_built = {}


def build_case(name):
    """dict(A, Bu, Bl, G [nprob][...], Q [nprob][mx][mx], R [nprob][mu][mu], N, tol, ref = [(K, kbreak, norms, e64)] per problem, symmetric)"""
    if name in _built:
        return _built[name]
    c = BY_NAME[name]
    mx, mu, ml, nprob, N = c["mx"], c["mu"], c["ml"], c["nprob"], c["N"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    models = [ref._model(rng, mx, mu, ml) for _ in range(nprob)]
    Q = np.stack([ref._spd(rng, mx) * 10.0 ** p for p in range(nprob)])
    R = np.stack([ref._spd(rng, mu) * 10.0 ** -p for p in range(nprob)]) if mu else np.zeros((nprob, 0, 0))
    for p in c["nonsym"]:
        M = rng.normal(size=(mx, mx))
        Q[p] += 0.3 * (M - M.T) / np.sqrt(mx)
    norm_lists = [ref.dlqr(*models[p], Q[p], R[p], N, 0.0, np.float64)[2] for p in range(nprob)]
    tol = ref.choose_tol(norm_lists, "mid")
    refs = [ref.reference(*models[p], Q[p], R[p], N, tol) for p in range(nprob)]
    for r in refs:
        for x in r[2]:
            assert abs(x - tol) > 1e-6 * tol, "a longdouble norm lies within 1e-6 of tol"
    A, Bu, Bl, G = (np.stack([m[i] for m in models]) for i in range(4))
    sym = all(np.array_equal(Q[p], Q[p].T) and np.array_equal(R[p], R[p].T) for p in range(nprob))
    assert sym == (not c["nonsym"])
    _built[name] = dict(c, A=A, Bu=Bu, Bl=Bl, G=G, Q=Q, R=R, tol=tol, ref=refs, symmetric=sym)
    return _built[name]


def check_gains(K, kb, refp, what):
    """the acceptance rule of the Riccati launch-shape sweep (tests/test_gpu_riccati_sweep.py check_gains): kbreak equal, max|K - Kref| <= tolerance(e64) max|Kref|,
    the back-filled rows bitwise K[kbreak - 1]"""
    Kref, kbref, norms, e64 = refp
    assert kb == kbref, "%s: kbreak %d, reference %d (norms %s)" % (what, kb, kbref, norms)
    if Kref.size == 0:
        return
    scale = float(np.abs(Kref).max())
    err = float(np.abs(K - Kref).max())
    print("%s: kbreak %d, max|K - Kref| = %.3g relative, bound %.3g" % (what, kb, err / scale, ref.tolerance(e64)))
    assert err <= ref.tolerance(e64) * scale, "%s: max|K - Kref| = %.3g = %.3g relative, bound %.3g (e64 %.3g)" % (what, err, err / scale, ref.tolerance(e64), e64)
    for r in range(kbref - 1):
        assert np.array_equal(K[r], K[kbref - 1]), "%s: back-filled row %d differs from row %d" % (what, r, kbref - 1)
