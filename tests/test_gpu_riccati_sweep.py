"""Every launch shape of csrc/riccati.hip against the extended-precision restatement of lqr.jl's dlqr (tests/dlqr_reference.py).

launch_riccati picks among the register-fragment resident kernels <1,3> <1,6> <1,12> <7,21>, the generic resident kernels <1..7,0> (S solved in
registers) and <0,0> (pivoted LU in LDS), the tiled three-launch step, and ric_project_kernel<true / false>, by (mx, mu, ml, nprob, path).  CASES
holds at least one shape for each of them and both sides of every boundary between them (tests/test_riccati_reference.py checks that on the
CPU through the mirror of the dispatch rules, dlqr_reference.riccati_kernels).  Each case runs on every path it lists and must give
  * kbreak equal to the reference's (the break placed so that no norm lies within 1e-6 of tol: the index cannot depend on rounding),
  * max|K - Kref| <= tolerance(e64) max|Kref|, e64 = the larger error of the two float64 twins (dlqr_reference.reference),
  * the back-filled rows (lqr.jl:179-181) bitwise equal to K[kbreak-1],
  * with keep_last, bitwise row 0 of the full table of the same path.
"""
import zlib

import numpy as np
import pytest

import dlqr_reference as ref


def C(name, mx, mu, ml, nprob=2, N=12, brk="mid", paths=(0, 1, 2), Q=None, R=None, ref_idx=None):
    return dict(name=name, mx=mx, mu=mu, ml=ml, nprob=nprob, N=N, brk=brk, paths=paths, Q=Q, R=R, ref_idx=ref_idx)


CASES = [
    # register-fragment resident kernels, synthetic data (the suite's other tests feed them mechanisms only)
    C("frag_1_3", 12, 1, 5, nprob=3, N=16), C("frag_1_6", 24, 1, 10, nprob=3, N=16), C("frag_1_12", 48, 1, 20, nprob=3, N=16),
    C("frag_7_21", 84, 7, 35, N=12),
    # generic resident kernels, S in registers
    C("reg_mu2", 36, 2, 15), C("reg_mu3", 60, 3, 25), C("reg_mu4", 48, 4, 20, N=10), C("reg_mu5", 72, 5, 30),
    C("reg_mu6", 60, 6, 25, N=10), C("reg_mu7", 88, 7, 40, N=10),
    # <0,0>: pivoted LU in LDS on one wavefront; mu 65 / 72 exceed its 64 lanes and must go tiled
    C("ldslu_40_8", 40, 8, 10, N=10), C("ldslu_64_12", 64, 12, 20, nprob=1, N=10), C("ldslu_48_16_ml0", 48, 16, 0, N=10),
    C("ldslu_84_8", 84, 8, 35, nprob=1, N=10), C("ldslu_12_64", 12, 64, 4, N=8), C("mu65_12", 12, 65, 4, N=8), C("mu72_8", 8, 72, 2, N=8),
    # the LDS-fit boundary: the first two fit, the others go tiled even with path = 1
    C("fit_96_1", 96, 1, 40, nprob=1, N=8), C("fit_96_2", 96, 2, 40, nprob=1, N=8), C("nofit_92_7", 92, 7, 40, nprob=1, N=8),
    C("nofit_96_6", 96, 6, 40, nprob=1, N=8), C("nofit_100_1", 100, 1, 40, nprob=1, N=8),
    # tiled only: edge tiles (mx not a multiple of 4 / 16 / 32), mu up to 17
    C("tiled_5", 5, 1, 2, nprob=3, N=10), C("tiled_30", 30, 3, 10, nprob=3, N=10), C("tiled_33", 33, 17, 8, nprob=1, N=10),
    C("tiled_97", 97, 3, 30, nprob=3, N=8), C("tiled_130", 130, 1, 40, nprob=1, N=8), C("tiled_204", 204, 17, 60, nprob=1, N=6),
    C("tiled_252", 252, 3, 80, nprob=1, N=6),
    # projection: G Bλ in LDS (ml <= 96) or in global memory (<false>: ml > 96, and ml = 0)
    C("proj_ml0", 120, 2, 0, nprob=1, N=8), C("proj_ml1", 120, 2, 1, nprob=1, N=8), C("proj_ml96", 120, 2, 96, nprob=1, N=8),
    C("proj_ml97", 120, 2, 97, nprob=1, N=8), C("proj_ml110", 120, 2, 110, nprob=1, N=8), C("proj_ml0_frag", 48, 1, 0, nprob=1, N=8),
    # degenerate
    C("mu0", 24, 0, 10, N=10), C("N1", 24, 1, 10, N=1, brk="never"), C("N2", 24, 1, 10, N=2, brk="first"), C("N3", 36, 2, 15, N=3, brk="never"),
    C("nobreak", 36, 2, 15, N=12, brk="never"), C("break_first", 36, 2, 15, N=12, brk="first"),
    # automatic crossover: 127 problems of 64 states go tiled, 128 resident (a sample against the reference)
    C("auto_127", 64, 2, 20, nprob=127, N=8, paths=(0,), ref_idx=(0, 1, 63, 126)),
    C("auto_128", 64, 2, 20, nprob=128, N=8, paths=(0,), ref_idx=(0, 64, 127)),
    # R with one negative eigenvalue: S indefinite, the register solve falls back to the pivoted LDS LU
    C("indef_mu1", 24, 1, 10, N=6, brk="never", paths=(1, 2), R="indef"), C("indef_mu3", 36, 3, 15, N=6, brk="never", paths=(1, 2), R="indef"),
    C("indef_mu7", 84, 7, 35, nprob=1, N=6, brk="never", paths=(1, 2), R="indef"),
    # Q / R not symmetric: lqr.jl:152-170 keeps D'*Pk and Abar'*Pk*Abar as written
    C("nonsym_frag", 24, 1, 10, N=10, Q="nonsym"), C("nonsym_reg", 36, 2, 15, N=10, Q="nonsym", R="nonsym"),
]
# time-varying models (cclqr_riccati_tv, automatic path)
TV_CASES = [C("tv_24_1", 24, 1, 10, nprob=1, N=12), C("tv_36_2", 36, 2, 15, nprob=1, N=12), C("tv_60_3", 60, 3, 0, nprob=1, N=12),
            C("tv_130_3", 130, 3, 40, nprob=1, N=8)]


def _weights(rng, c):
    mx, mu = c["mx"], c["mu"]
    Q = R = None
    if c["Q"] == "nonsym":
        M = rng.normal(size=(mx, mx))
        Q = ref._spd(rng, mx) + 0.3 * (M - M.T) / np.sqrt(mx)
    if c["R"] == "indef":
        V = ref._orth(rng, mu)
        R = (V * np.concatenate([[-40.0], np.linspace(1.0, 2.0, mu - 1)])) @ V.T
        R = 0.5 * (R + R.T)
    elif c["R"] == "nonsym":
        M = rng.normal(size=(mu, mu))
        R = ref._spd(rng, mu) + 0.3 * (M - M.T)
    elif mu == 0:
        R = np.zeros((0, 0))
    return Q, R


def build_case(c, tv=False):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    Q, R = _weights(rng, c)
    pr = ref.make_problem(rng, c["mx"], c["mu"], c["ml"], nprob=c["nprob"], break_at=c["brk"], N=c["N"], tv=tv, Q=Q, R=R,
                          ref_idx=c["ref_idx"])
    # the kernel a case runs on depends on EXACT symmetry of the weights (cclqr_internal.h ric_p_rows)
    assert np.array_equal(pr["Q"], pr["Q"].T) == (c["Q"] != "nonsym") and np.array_equal(pr["R"], pr["R"].T) == (c["R"] != "nonsym")
    return pr


def check_gains(K, kb, p, refp, what):
    Kref, kbref, norms, e64 = refp
    assert kb == kbref, "%s: kbreak %d, reference %d (norms %s)" % (what, kb, kbref, norms)
    if Kref.size == 0:
        return
    scale = float(np.abs(Kref).max())
    err = float(np.abs(K - Kref).max())
    assert err <= ref.tolerance(e64) * scale, "%s: max|K - Kref| = %.3g = %.3g relative, bound %.3g (e64 %.3g)" % (
        what, err, err / scale, ref.tolerance(e64), e64)
    for r in range(kbref - 1):          # Ku[k2] = Ku[k2+1] below the break: copies of row kbreak-1 (lqr.jl:179-181)
        assert np.array_equal(K[r], K[kbref - 1]), "%s: back-filled row %d differs from row %d" % (what, r, kbref - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_riccati_sweep_against_extended_precision(cclqr, c):
    capi = cclqr._capi
    pr = build_case(c)
    args = (pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"])
    for path in c["paths"]:
        K, kb = capi.riccati(*args, tol=pr["tol"], path=path)
        for p, refp in pr["ref"].items():
            check_gains(K[p], int(kb[p]), p, refp, "%s path %d problem %d" % (c["name"], path, p))
        Kl, kbl = capi.riccati(*args, tol=pr["tol"], path=path, keep_last=True)
        assert np.array_equal(kbl, kb), "%s path %d: keep_last kbreak %s vs %s" % (c["name"], path, kbl, kb)
        if pr["N"] > 1:
            assert np.array_equal(Kl[:, 0], K[:, 0]), "%s path %d: keep_last gain differs from row 0 of the full table" % (c["name"], path)


@pytest.mark.gpu
@pytest.mark.parametrize("c", TV_CASES, ids=[c["name"] for c in TV_CASES])
def test_riccati_tv_sweep_against_extended_precision(cclqr, c):
    pr = build_case(c, tv=True)
    K, kb = cclqr._capi.riccati_tv(pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"])
    check_gains(K, kb, 0, pr["ref"][0], c["name"])


def _singular_knot(Bl, knot):
    """zero one column of Bλ: G Bλ gets an exact zero column, so every partially pivoted LU meets an exact zero pivot"""
    Bl[knot][:, 0] = 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 2])
def test_riccati_singular_projection_at_a_reached_knot_raises(cclqr, path):
    """G Bλ singular in a problem whose sweep runs: CCLQR_ESINGULAR, as the reference's LAPACK exception (lqr.jl:151)"""
    capi = cclqr._capi
    c = C("sing_reached", 24 if path == 1 else 33, 1, 10, N=6, brk="never")
    pr = build_case(c)
    _singular_knot(pr["Bl"], 1)
    with pytest.raises(ref.SingularPivot):
        ref.dlqr(pr["A"][1], pr["Bu"][1], pr["Bl"][1], pr["G"][1], pr["Q"], pr["R"], pr["N"], pr["tol"])
    with pytest.raises(capi.CclqrError) as e:
        capi.riccati(pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path)
    assert e.value.code == capi.ESINGULAR
    # time-varying: the first step's own knot
    t = C("sing_reached_tv", 24 if path == 1 else 130, 1, 10, nprob=1, N=8, brk="never")
    pt = build_case(t, tv=True)
    _singular_knot(pt["Bl"], pt["N"] - 2)
    with pytest.raises(capi.CclqrError) as e:
        capi.riccati_tv(pt["A"], pt["Bu"], pt["Bl"], pt["G"], pt["Q"], pt["R"], pt["N"], tol=pt["tol"])
    assert e.value.code == capi.ESINGULAR


@pytest.mark.gpu
@pytest.mark.parametrize("mx", [24, 130])
def test_riccati_tv_singular_knot_below_the_break_is_not_reached(cclqr, mx):
    """lqr_tracking.jl:87-116 factors G Bλ inside the step: a singular knot the sweep never reaches (below kbreak) is no error there,
    and the gains are those of the reference (resident path at mx 24, tiled at mx 130)"""
    c = C("sing_below_%d" % mx, mx, 1 if mx == 24 else 3, 10 if mx == 24 else 40, nprob=1, N=12 if mx == 24 else 8)
    pr = build_case(c, tv=True)
    kb0 = pr["ref"][0][1]
    assert kb0 > 1
    _singular_knot(pr["Bl"], 0)                   # knot of backward step 1: below the break
    r = ref.reference(pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"], pr["tol"], tv=True)
    assert r[1] == kb0
    K, kb = cclqr._capi.riccati_tv(pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], pr["N"], tol=pr["tol"])
    check_gains(K, kb, 0, r, c["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", [1, 2])
def test_riccati_singular_projection_with_N1_is_not_reached(cclqr, path):
    """dlqr with N = 1 runs no backward step and factors nothing (lqr.jl:150): kbreak 0, no error, whatever G Bλ is"""
    capi = cclqr._capi
    c = C("sing_N1", 24, 1, 10, N=1, brk="never")
    pr = build_case(c)
    _singular_knot(pr["Bl"], 0)
    K, kb, _ = ref.dlqr(pr["A"][0], pr["Bu"][0], pr["Bl"][0], pr["G"][0], pr["Q"], pr["R"], 1, 0.0)
    assert kb == 0 and K.shape[0] == 0
    K, kb = capi.riccati(pr["A"], pr["Bu"], pr["Bl"], pr["G"], pr["Q"], pr["R"], 1, tol=0.0, path=path)
    assert list(kb) == [0, 0] and K.shape[1] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# per-instance gain tables written by the Riccati kernels themselves (kpad = the zero pad behind every instance's table)

def _gain_row_overrun(mh):
    """cclqr_internal.h gain_row_overrun for a chain: doubles the rollout kernel's control phase reads past the end of a gain row"""
    G, _ = mh.geometry()
    over = -(-12 * mh.layout_links() // G) * G - 12 * mh.tables.nb
    return (over + 1) & ~1 if over > 0 else 0


def _chain_batch(cclqr, links, n, seed):
    rng = np.random.default_rng(seed)
    y = rng.uniform(-0.5, 0.5, n)
    zd = cclqr.examples.cartpole_states(links, y, np.zeros((n, links)))
    z0 = cclqr.examples.cartpole_states(links, y + rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, (n, links)))
    return zd, z0


@pytest.mark.gpu
@pytest.mark.parametrize("links,inf", [(4, False), (4, True), (8, False), (8, True)])
def test_batch_lqr_tables_with_row_overrun_match_the_host_tables(cclqr, links, inf):
    """cclqr_ctrl_create_lqr_batch has the Riccati kernels write every instance's table straight into the controller, kpad doubles apart
    (nb 5: mx 60, resident; nb 9: mx 108, tiled).  The rollout it drives is bitwise the rollout of linearize -> riccati (kpad = 0) ->
    a caller-gain controller, statuses included"""
    capi = cclqr._capi
    t = cclqr.examples.cartpole_n(links)["mech"].tables()
    mh = capi.MechHandle(t)
    assert _gain_row_overrun(mh) > 0
    n, N, mx = 6, 30, 12 * t.nb
    zd, z0 = _chain_batch(cclqr, links, n, links)
    Q, R = np.eye(mx) * t.dt, np.eye(1) * t.dt
    dev = capi.BatchLqrHandle(mh, zd, [0], Q, R, N, infinite_horizon=inf)
    A, Bu, Bl, G = capi.linearize(mh, zd, [0], np.zeros((n, 1)))
    K, kb = capi.riccati(A, Bu, Bl, G, Q, R, N, keep_last=inf)
    assert np.array_equal(dev.kbreak, kb)
    host = capi.CtrlHandle(mh, [0], K=K, N=0 if inf else N, zd=zd[:, None], n_ctrl=n)
    zT_h, tr_h, st_h = capi.rollout(mh, host, z0, N - 1, record=True)
    zT_d, tr_d, st_d = capi.rollout(mh, dev, z0, N - 1, record=True)
    assert np.array_equal(st_h, st_d) and (st_h > 0).all()
    assert np.array_equal(tr_h, tr_d) and np.array_equal(zT_h, zT_d)


@pytest.mark.gpu
@pytest.mark.parametrize("links", [4, 8])
def test_caller_gain_tables_do_not_read_the_next_instances_table(cclqr, links):
    """per-instance caller gains with table i+1 full of NaN and +-Inf: instance i's trajectory is bitwise the one it has with its table
    alone (the row overrun of the control phase meets the table's own zero pad, never the neighbour's entries)"""
    capi = cclqr._capi
    t = cclqr.examples.cartpole_n(links)["mech"].tables()
    mh = capi.MechHandle(t)
    assert _gain_row_overrun(mh) > 0
    n, N, mx = 3, 20, 12 * t.nb
    zd, z0 = _chain_batch(cclqr, links, n, 10 + links)
    A, Bu, Bl, G = capi.linearize(mh, zd, [0], np.zeros((n, 1)))
    K, _ = capi.riccati(A, Bu, Bl, G, np.eye(mx) * t.dt, np.eye(1) * t.dt, N)
    bad = np.full_like(K[2], np.nan)
    bad[..., 0::3], bad[..., 1::3] = np.inf, -np.inf
    Kb = K.copy()
    Kb[2] = bad
    both = capi.CtrlHandle(mh, [0], K=Kb, N=N, zd=zd[:, None], n_ctrl=n)
    _, tr, st = capi.rollout(mh, both, z0, N - 1, record=True)
    for i in (0, 1):
        lone = capi.CtrlHandle(mh, [0], K=K[i], N=N, zd=zd[i])
        _, tr1, st1 = capi.rollout(mh, lone, z0[i:i + 1], N - 1, record=True)
        assert st1[0] > 0 and st[i] == st1[0]
        assert np.array_equal(tr[i], tr1[0]), "instance %d differs from its lone run: %.3g" % (i, np.abs(tr[i] - tr1[0]).max())
