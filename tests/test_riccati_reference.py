"""The extended-precision dlqr restatement (tests/dlqr_reference.py) pinned to independent answers, and the Riccati sweep's shape table
pinned to the launch-shape choice of csrc/riccati.hip.  CPU only."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sl

import dlqr_reference as ref
import test_gpu_riccati_sweep as sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RICCATI_HIP = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "riccati.hip")


def test_lu_solve_matches_lapack_and_detects_an_exact_zero_pivot():
    rng = np.random.default_rng(0)
    M, b = rng.normal(size=(9, 9)), rng.normal(size=(9, 4))
    x = ref.lu_solve(M, b)
    assert x.dtype == np.longdouble
    assert np.abs(x.astype(np.float64) - np.linalg.solve(M, b)).max() < 1e-12
    # the residual in extended precision is far below what float64 can show
    assert float(np.abs(M.astype(np.longdouble) @ x - b).max()) < 1e-16
    M[:, 3] = 0.0
    with pytest.raises(ref.SingularPivot):
        ref.lu_solve(M, b)


@pytest.mark.parametrize("mx,mu", [(6, 1), (10, 3)])
def test_reference_converges_to_scipy_dare(mx, mu):
    """unconstrained (ml = 0) and iterated to convergence (tol = 0, long horizon): Ku[1] is the DARE gain"""
    rng = np.random.default_rng(mx)
    A, Bu, _, _ = ref._model(rng, mx, mu, 0, rho=0.9)
    Q, R = ref._spd(rng, mx), ref._spd(rng, mu)
    K, kb, norms = ref.dlqr(A, Bu, np.zeros((mx, 0)), np.zeros((0, mx)), Q, R, 300, 0.0)
    assert kb == 1 and len(norms) == 299 and norms[-1] < 1e-13
    P = sl.solve_discrete_are(A, Bu, Q, R)
    Kd = np.linalg.solve(R + Bu.T @ P @ Bu, Bu.T @ P @ A)
    assert np.abs(K[0].astype(np.float64) - Kd).max() < 1e-11 * np.abs(Kd).max()


def test_reference_follows_the_loop_semantics_of_lqr_jl():
    """`for outer k`: the break index, the back-fill, N = 1 (no step, k = 0) and N = 2"""
    rng = np.random.default_rng(1)
    A, Bu, Bl, G = ref._model(rng, 8, 2, 3)
    Q, R = ref._spd(rng, 8), ref._spd(rng, 2)
    K, kb, norms = ref.dlqr(A, Bu, Bl, G, Q, R, 1, 1.0)
    assert K.shape == (0, 2, 8) and kb == 0 and norms == []
    K, kb, norms = ref.dlqr(A, Bu, Bl, G, Q, R, 2, 0.0)
    assert kb == 1 and len(norms) == 1
    K, kb, norms = ref.dlqr(A, Bu, Bl, G, Q, R, 20, 0.0)
    tol = float(np.sqrt(norms[5] * norms[4]))
    K2, kb2, norms2 = ref.dlqr(A, Bu, Bl, G, Q, R, 20, tol)
    assert kb2 == 19 - 5 and len(norms2) == 6
    assert np.array_equal(K2[kb2 - 1], K[kb2 - 1])
    assert all(np.array_equal(K2[r], K2[kb2 - 1]) for r in range(kb2 - 1))
    # the projected float64 twin computes the same recursion
    K3, kb3, _ = ref.dlqr_projected64(A, Bu, Bl, G, Q, R, 20, tol)
    assert kb3 == kb2 and np.abs(K3 - K2.astype(np.float64)).max() < 1e-12 * np.abs(K3).max()


TI_CASES = [c for c in sweep.CASES if c["nprob"] <= 3]


@pytest.mark.parametrize("c", TI_CASES, ids=[c["name"] for c in TI_CASES])
def test_reference_matches_oracle_on_the_sweep_shapes(orc, c):
    """the C oracle the rest of the suite trusts, against the independent restatement, on every time-invariant sweep shape; also that
    each case is well posed (the break where the case wants it, fp64 twins close to the longdouble reference)"""
    pr = sweep.build_case(c)
    N = pr["N"]
    for p, (Kref, kbref, norms, e64) in pr["ref"].items():
        if c["brk"] == "first":
            assert kbref == N - 1
        elif c["brk"] == "never":
            assert kbref == (1 if N > 1 else 0)
        else:
            assert 1 < kbref < N - 1 or (p > 0 and kbref >= 1)
        assert e64 < 1e-12
        if c["mu"] == 0:
            continue            # (the oracle's step needs an input)
        Ko, kbo = orc.riccati(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"], N, tol=pr["tol"])
        assert kbo == kbref
        if Kref.size:
            assert np.abs(Ko - Kref).max() <= ref.tolerance(e64) * np.abs(Kref).max()


def test_reference_tv_matches_oracle_tracking(cclqr, orc):
    """dlqr_tv on the oracle's own linearisations at every knot against the oracle's re-linearising dlqr (lqr_tracking.jl:73-122): the
    knot convention (backward step k uses the model of knot index k-1) and the recursion"""
    t = cclqr.examples.cartpole_n(2)["mech"].tables()
    N = 25
    rng = np.random.default_rng(3)
    zs = np.stack([cclqr.examples.cartpole_states(2, [0.02 * k], rng.uniform(-0.3, 0.3, (1, 2)))[0] for k in range(N)])
    Fd = rng.normal(size=(N, 1))
    mx = 12 * t.nb
    Q, R = np.eye(mx) * 0.01, np.eye(1) * 0.01
    mats = [orc.linearize(t, zs[k], [0], Fd[k]) for k in range(N - 1)]
    A, Bu, Bl, G = (np.stack([m[i] for m in mats]) for i in range(4))
    norms = ref.dlqr_tv(A, Bu, Bl, G, Q, R, N, 0.0, np.float64)[2]
    tol = ref.choose_tol([norms], 2)
    Kref, kb, _, e64 = ref.reference(A, Bu, Bl, G, Q, R, N, tol, tv=True)
    Ko, kbo = orc.riccati_tracking(t, [0], zs, Fd, Q, R, N, tol=tol)
    assert 1 < kb < N - 1 and kbo == kb
    assert np.abs(Ko - Kref).max() <= ref.tolerance(e64) * np.abs(Kref).max()


def test_indefinite_cases_make_the_register_solve_fall_back():
    """R with a negative eigenvalue: S = R + D'PkD is not positive definite at the first step, so gain_in_registers' unpivoted
    factorisation meets a non-positive pivot and the kernel takes the pivoted LDS LU"""
    for c in [c for c in sweep.CASES if c["R"] == "indef"]:
        pr = sweep.build_case(c)
        for p in pr["ref"]:
            A, Bu, Bl, G = pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p]
            D = Bu - Bl @ np.linalg.solve(G @ Bl, G @ Bu)
            S = pr["R"] + D.T @ pr["Q"] @ D
            assert np.linalg.eigvalsh(0.5 * (S + S.T)).min() < 0, c["name"]


def test_dispatch_mirror_matches_riccati_hip():
    """dlqr_reference's mirror of the launch-shape rules states what riccati.hip says: each rule's source text is checked here, so that
    a change of the dispatch shows up as a failure of this test rather than as a sweep that silently stopped covering a kernel"""
    src = open(RICCATI_HIP).read()
    assert "#define RIC_MU_REG %d " % ref.RIC_MU_REG in src
    assert "#define RIC_LDS_M %d " % ref.RIC_LDS_M in src
    assert "#define RIC_WAVES (RIC_THREADS / 64)" in src and "#define RIC_THREADS 512" in src
    assert "#define RIC_YB %d " % ref.RIC_YB in src
    # ric_resident_is_frag
    assert "return (mu == 1 && (mx == 12 || mx == 24 || mx == 48)) || (mu == 7 && mx == 84);" in src
    # ric_resident_lds_bytes
    assert ("return ((size_t)mx * mx + mx * na + (size_t)mx * mu + 2 * (size_t)mu * mx + mu * na + 2 * (size_t)mu * mu + 2 * RIC_WAVES + 2 +\n"
            "            (ric_resident_is_frag(mx, mu) ? (size_t)RIC_WAVES * RIC_YB : 0)) * sizeof(double) + (mu + 2) * sizeof(int);") in src
    # ric_resident_fits
    assert ("return ric_resident_lds_bytes(a.mx, a.mu) <= 158 * 1024 && (a.mx & 3) == 0 && (a.mx + a.mu + 15) / 16 <= RIC_WAVES && "
            "a.mu <= %d;" % ref.RIC_LU_LANES) in src
    # ric_use_tiled (fp64)
    assert "if (path != 0) return path == 2;" in src and "return a.mx >= 64 && a.nprob < 128;" in src
    # the kernel table of launch_riccati: generic by mu, register-fragment by (mu, mx / 4), none of them for a non-symmetric Pk
    assert "ResKernel kern = by_mu[(a.mu >= 1 && a.mu <= RIC_MU_REG) ? a.mu : 0];" in src
    assert "const int ng4 = a.p_rows ? -1 : a.mx >> 2;" in src
    frag = re.findall(r"if \(a\.mu == (\d) && ng4 == (\d+)\) kern = riccati_resident_kernel<(\d), (\d+)>;", src)
    assert sorted((int(a), 4 * int(b)) for a, b, _, _ in frag) == [(1, 12), (1, 24), (1, 48), (7, 84)]
    assert all(ref.ric_resident_is_frag(4 * int(b), int(a)) for a, b, _, _ in frag)
    # ric_project_kernel<LDSM>
    assert "if (ml <= RIC_LDS_M && ml > 0) {" in src
    # the host decides p_rows on exact symmetry of Q and R: the rule is stated once (cclqr_internal.h ric_p_rows) and every p_rows capi.hip hands to the
    # kernels is assigned from it, none from a literal or from a second statement of the rule
    csrc = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc")
    capi, internal = open(os.path.join(csrc, "capi.hip")).read(), open(os.path.join(csrc, "cclqr_internal.h")).read()
    assert internal.count("ric_symmetric(Q, ") == 1 and capi.count("ric_symmetric(") == 0
    assert "return (ric_symmetric(Q, mx) && (mu == 0 || ric_symmetric(R, mu))) ? 0 : 1;" in internal
    assigned = re.findall(r"p_rows\s*=\s*([^;]*);", capi)
    assert len(assigned) == 3 and all(re.fullmatch(r"ric_p_rows\(Q, (\(int\))?mx, R, mu\)", a) for a in assigned), assigned


def _sweep_launches():
    out = []
    for c in sweep.CASES:
        sym = c["Q"] != "nonsym" and c["R"] != "nonsym"
        for path in c["paths"]:
            out.append((c, path, ref.riccati_kernels(c["mx"], c["mu"], c["ml"], c["nprob"], path, sym)))
    for c in sweep.TV_CASES:
        out.append((c, 0, ref.riccati_kernels(c["mx"], c["mu"], c["ml"], 1, 0)))
    return out


def test_sweep_covers_every_launch_shape_and_both_sides_of_every_boundary():
    L = _sweep_launches()
    seen = set().union(*[k for _, _, k in L])
    want = {"riccati_resident_kernel<1, 3, 0>", "riccati_resident_kernel<1, 6, 0>", "riccati_resident_kernel<1, 12, 0>",
            "riccati_resident_kernel<7, 21, 0>", "ric_project_kernel<true>", "ric_project_kernel<false>",
            "ric_pa_kernel", "ric_gain_update_kernel", "ric_pn_kernel", "ric_backfill_kernel"}
    want |= {"riccati_resident_kernel<%d, 0, 0>" % m for m in range(0, ref.RIC_MU_REG + 1)}
    assert want <= seen, sorted(want - seen)
    resident = lambda k: any(x.startswith("riccati_resident_kernel") for x in k)
    lim = 158 * 1024
    fit = [(c["mx"], c["mu"]) for c, p, k in L if p == 1 and resident(k)]
    nofit = [(c["mx"], c["mu"]) for c, p, k in L if p == 1 and not resident(k)]
    # LDS fit: a resident case within 8 KB of the limit, and path-1 cases just past it
    assert any(lim - 8192 < ref.ric_resident_lds_bytes(mx, mu) <= lim for mx, mu in fit)
    assert any(lim < ref.ric_resident_lds_bytes(mx, mu) < lim + 8192 for mx, mu in nofit)
    # the one-wavefront LU: mu 64 resident, mu 65 not (with the LDS fitting)
    assert any(mu == 64 for _, mu in fit)
    assert any(mu == 65 and ref.ric_resident_lds_bytes(mx, mu) <= lim for mx, mu in nofit)
    # whole k-groups of four: an mx that is not a multiple of 4 goes tiled with path 1 although its LDS would fit
    assert any(mx % 4 and ref.ric_resident_lds_bytes(mx, mu) <= lim for mx, mu in nofit)
    # the register solve: mu = 7 in registers, mu = 8 in the LDS LU, mu = 0
    assert {"riccati_resident_kernel<7, 0, 0>"} <= seen and any(c["mu"] == 8 and resident(k) for c, p, k in L)
    assert any(c["mu"] == 0 and resident(k) for c, p, k in L) and any(c["mu"] == 0 and not resident(k) for c, p, k in L)
    # G Bλ in LDS up to ml = 96, in global memory from 97 (and for ml = 0)
    assert {c["ml"] for c, p, k in L if "ric_project_kernel<true>" in k} >= {1, 96}
    assert {c["ml"] for c, p, k in L if "ric_project_kernel<false>" in k} >= {0, 97}
    # the automatic crossover: mx >= 64 with 127 problems tiled, 128 resident
    auto = {c["nprob"]: resident(k) for c, p, k in L if p == 0 and c["mx"] >= 64 and c["nprob"] in (127, 128)}
    assert auto == {127: False, 128: True}
    # a frag shape with a non-symmetric weight runs on the generic kernel
    assert any(c["Q"] == "nonsym" and ref.ric_resident_is_frag(c["mx"], c["mu"]) and "riccati_resident_kernel<1, 0, 0>" in k for c, p, k in L)
    # horizons
    assert {1, 2, 3} <= {c["N"] for c in sweep.CASES}
    # the time-varying cases run resident generic and tiled
    tv = [k for c, p, k in L if c in sweep.TV_CASES]
    assert any("riccati_resident_kernel<3, 0, 0>" in k for k in tv) and any(not resident(k) for k in tv)
