"""CPU tests of the rollout score (cclqr_rollout_score): the kernel's row functions (csrc/cclqr_score.h) emulated lane by lane against the numpy restatement of the
definition, the chunk plan, the packing of Score(...)'s weights, the Python-side refusals and the additive C ABI (header, binding, Julia shim, version 202)."""
import math
import os
import re

import numpy as np
import pytest

import score_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    return sc.emu_score()


@pytest.mark.parametrize("kind", ["inf", "gated", "tracking"])
@pytest.mark.parametrize("nb", [1, 2, 5, 8, 9, 17, 33, 64])
def test_row_functions_match_the_numpy_definition(emu, nb, kind):
    """every lane-group size and its first overflow, every horizon kind, one and several controller tables (first_instance 2), k0 1 and 4, a permuted
    link order; Jx, Ju, peak within 1e-10 A, last_out exact"""
    for mu in sorted({min(m, nb) for m in (1, 3, 7)}):
        for n_ctrl, first in ((1, 0), (7, 2)):
            for k0 in (1, 4):
                n_inst, steps = 5, 8
                case = sc.synthetic_case(nb, mu, kind, n_ctrl, n_inst, steps, seed=1000 * nb + 10 * mu + n_ctrl + k0)
                perm = np.random.default_rng(nb).permutation(nb)
                cx, cu, Ax, Au = sc.stage_costs(case["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"], k0=k0, first_instance=first)
                tol = sc.settle_tol_between(cx)
                init = None
                if k0 > 1:
                    init = np.abs(np.random.default_rng(7).normal(size=(n_inst, 4)))
                    init[:, 3] = [0, 1, 2, 3, 3]
                ref, A = sc.score_of(cx, cu, Ax, Au, tol, k0=k0, init=init)
                got = sc.emu_score_run(emu, case, perm, tol, k0=k0, first_instance=first, init=init)
                sc.assert_score(got, ref, A, "nb %d mu %d %s n_ctrl %d k0 %d" % (nb, mu, kind, n_ctrl, k0))
                assert (ref[:, 3] >= k0).any(), "the threshold separates nothing"


def test_a_nan_in_one_row_is_that_instance_alone(emu):
    case = sc.synthetic_case(5, 3, "gated", 1, 5, 8, seed=3)
    clean = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    case["traj"][2, 3, 1, 8] = np.nan
    perm = np.arange(5)
    cx, cu, Ax, Au = sc.stage_costs(clean["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"])
    tol = sc.settle_tol_between(cx)
    ref0, _ = sc.score_of(cx, cu, Ax, Au, tol)
    cxn, cun, Axn, Aun = sc.stage_costs(case["traj"], case["zd"], case["K"], case["N"], case["Qb"], case["R"])
    ref, A = sc.score_of(cxn, cun, Axn, Aun, tol)
    assert np.isnan(ref[2, 0]) and np.isnan(ref[2, 2]) and np.isnan(ref[2, 1]) and ref[2, 3] >= 4      # step 4 (k < N = 5: the feedback is on)
    got = sc.emu_score_run(emu, case, perm, tol)
    got0 = sc.emu_score_run(emu, clean, perm, tol)
    sc.assert_score(got, ref, A, "planted NaN")
    others = [0, 1, 3, 4]
    assert np.array_equal(got[others], got0[others]) and np.array_equal(ref[others], ref0[others])


def test_emulated_chunks_are_bitwise_one_call(emu):
    case = sc.synthetic_case(9, 3, "tracking", 1, 3, 23, seed=5)
    perm = np.random.default_rng(2).permutation(9)
    whole = sc.emu_score_run(emu, case, perm, 0.5)
    for plan in ([1] * 23, [7, 7, 7, 2], [20, 3]):
        s, k0 = None, 1
        for n in plan:
            part = dict(case, traj=np.ascontiguousarray(case["traj"][:, k0 - 1:k0 - 1 + n]))
            s = sc.emu_score_run(emu, part, perm, 0.5, k0=k0, init=s)
            k0 += n
        assert np.array_equal(s, whole), plan


@pytest.mark.parametrize("steps", [1, 7, 50, 51])
@pytest.mark.parametrize("chunk", [1, 7, 50])
def test_chunk_plan_covers_the_horizon_exactly_once(cclqr, steps, chunk):
    plan = cclqr._capi.chunk_plan(steps, chunk)
    assert len(plan) == math.ceil(steps / chunk)
    covered = [k for k0, n in plan for k in range(k0, k0 + n)]
    assert covered == list(range(1, steps + 1))
    assert all(1 <= n <= chunk for _, n in plan)
    with pytest.raises(ValueError):
        cclqr._capi.chunk_plan(steps, 0)


def test_default_chunk_keeps_the_slab_under_one_gib(cclqr):
    c = cclqr._capi.default_chunk_steps(8192, 17, 1000)
    assert 8192 * c * 17 * 13 * 8 <= 1 << 30 < 8192 * (c + 1) * 17 * 13 * 8
    assert cclqr._capi.default_chunk_steps(4, 2, 30) == 30 and cclqr._capi.default_chunk_steps(10 ** 9, 64, 30) == 1


def test_score_packs_and_scales_its_weights_as_lqr_does(cclqr):
    ex = cclqr.examples.cartpole_n(2)
    mech = ex["mech"]
    ids = [cclqr.getid(b) for b in ex["bodies"]]
    rng = np.random.default_rng(0)
    Q = [rng.normal(size=(12, 12)) for _ in ids]
    R = [np.array([[0.3]])]
    eq = [cclqr.getid(ex["ctrl"][0])]
    s = cclqr.Score(mech, ids, eq, Q, R, settle_tol=1e-3)
    Qm, Rm, _, _ = cclqr.lqr._weights_and_horizon(Q, R, math.inf, mech.Δt)
    assert np.array_equal(s.Q, Qm) and np.array_equal(s.R, Rm) and s.settle_tol == 1e-3
    assert np.array_equal(s.Qb, np.stack(Q) * mech.Δt)
    # blocks follow bodyids: a permuted listing is brought back to the mechanism's body order
    order = [2, 0, 1]
    sp = cclqr.Score(mech, [ids[i] for i in order], eq, [Q[i] for i in order], R)
    assert np.array_equal(sp.Qb, s.Qb)


def test_python_side_refusals(cclqr):
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids = [cclqr.getid(b) for b in ex["bodies"]]
    eq = [cclqr.getid(ex["ctrl"][0])]
    with pytest.raises(AssertionError, match="bodies"):
        cclqr.Score(mech, ids, eq, ex["Q"][:1], ex["R"])
    with pytest.raises(AssertionError, match="constraints"):
        cclqr.Score(mech, ids, eq, ex["Q"], [])
    with pytest.raises(ValueError, match="settle_tol"):
        cclqr.Score(mech, ids, eq, ex["Q"], ex["R"], settle_tol=math.nan)
    with pytest.raises(ValueError, match="finite"):
        cclqr.Score(mech, ids, eq, [np.eye(12) * math.inf, np.eye(12)], ex["R"])
    with pytest.raises(ValueError, match="12 x 12"):
        cclqr.Score(mech, ids, eq, [np.eye(6), np.eye(12)], ex["R"])
    score = cclqr.Score(mech, ids, eq, ex["Q"], ex["R"])

    class Closure(cclqr.Controller):
        controlfunction = staticmethod(lambda batch, c, k: None)

    with pytest.raises(ValueError, match="controlfunction"):
        cclqr.simulate(mech, 0.1, Closure(), score=score)
    with pytest.raises(ValueError, match="chunk_steps"):
        cclqr.simulate(mech, 0.1, Closure(), chunk_steps=3)
    with pytest.raises(ValueError, match="chunk_steps"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), score=score, chunk_steps=0)
    with pytest.raises(TypeError, match="Score"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), score=np.eye(3))
    other = cclqr.examples.cartpole_n(1)["mech"]
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.simulate(other, 0.1, cclqr.Controller(), score=score)


def test_the_three_entry_points_are_declared_cited_and_listed(cclqr):
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    for name in ("cclqr_score_create", "cclqr_score_destroy", "cclqr_rollout_score"):
        i = hdr.index("int %s(" % name)
        assert re.search(r"lqr\.jl:\d+", hdr[max(0, i - 3500):i]), name
        assert name in cclqr._capi.EXPORTS and ":" + name in jl
    assert "#define CCLQR_SCORE_LEN 4" in hdr and cclqr._capi.SCORE_LEN == 4
    assert "typedef struct cclqr_score cclqr_score;" in hdr
    assert "#define CCLQR_ABI_VERSION 202" in hdr and cclqr._capi.ABI_VERSION == 202
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(cclqr._capi.mirrored_layout()) == 48
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    assert "score.hip" in mk and "cclqr_score.h" in mk
