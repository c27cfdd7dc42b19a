"""CPU tests of the ensemble statistics (cclqr_rollout_ensemble): the kernel's row and tile functions (csrc/cclqr_ensemble.h) emulated lane by lane against the
numpy restatement of the definition in longdouble, the cancellation case |mean| >> spread, EnsembleStats.merge, the Python-side refusals and the additive C ABI
(header, binding, Julia shim, INTEGRATION.md, Makefile; version 202)."""
import os
import re

import numpy as np
import pytest

import ensemble_common as ec
import score_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_rollout_ensemble_ws_bytes", "cclqr_rollout_ensemble")


@pytest.fixture(scope="module")
def emu():
    return ec.emu_ensemble()


@pytest.mark.parametrize("kind", ["inf", "gated", "tracking"])
@pytest.mark.parametrize("nb", [1, 2, 5, 8, 9, 17, 33, 64])
def test_row_and_tile_functions_match_the_numpy_definition(emu, nb, kind):
    """every lane-group size and its first overflow, every horizon kind, a permuted link order; n_inst 1, 2, one under and one over a tile of 64 (and so over a
    multiple of every pass), 257 = four tiles and one instance; one table and a shard at first_instance 2 of n_inst + 2 tables; k0 1 and 4 (an 8-step window crosses
    N = 5 / 6).  mean and M2 within 1e-10 A of the longdouble two-pass"""
    perm = np.random.default_rng(nb).permutation(nb)
    mu = min(3, nb)
    for n_inst in (1, 2, 63, 65, 257):
        for multi, k0 in ((False, 1), (True, 4)):
            n_ctrl, first = (n_inst + 2, 2) if multi else (1, 0)
            steps = 8 if n_inst < 257 else 3
            case = sc.synthetic_case(nb, mu, kind, n_ctrl, n_inst, steps, seed=100000 * nb + 10 * n_inst + k0)
            mean, M2 = ec.emu_ensemble_run(emu, case, perm, k0=k0, first_instance=first)
            ec.assert_moments(mean, M2, case, k0=k0, first_instance=first, what="nb %d %s n_inst %d n_ctrl %d k0 %d" % (nb, kind, n_inst, n_ctrl, k0))
            if n_inst == 1:
                assert (M2 == 0.0).all()
            if kind == "gated" and k0 == 4:
                assert (mean[1:, 12 * nb:] == 0.0).all() and (M2[1:, 12 * nb:] == 0.0).all() and (mean[0, 12 * nb:] != 0.0).all()      # the gate closes at k = N = 5


def test_a_controller_without_gains_commands_nothing(emu):
    case = dict(sc.synthetic_case(5, 2, "inf", 1, 9, 4, seed=2), K=None)
    mean, M2 = ec.emu_ensemble_run(emu, case, np.arange(5))
    assert mean.shape == (4, 60)
    ec.assert_moments(mean, M2, case, what="no gains")


@pytest.mark.parametrize("nb", [2, 9, 17, 33])
def test_centred_sums_survive_a_mean_far_above_the_spread(emu, nb):
    """z = 1 + 1e-6 g, n = 257: every centred variance within 1e-8 relative of the longdouble two-pass; S2 / n - mean^2 in float64 would leave about 2e-4"""
    case = ec.cancellation_case(nb, 257, seed=nb)
    mean, M2 = ec.emu_ensemble_run(emu, case, np.random.default_rng(1).permutation(nb))
    worst = ec.assert_cancellation(M2, case)
    x, _ = ec.rows_of(case["traj"], case["zd"], None, 0)
    naive = (x ** 2).sum(axis=1) - x.sum(axis=1) ** 2 / 257
    ref = ec.moments_of(x, x)[1]
    assert float((np.abs(naive - ref) / ref).max()) > 100 * max(worst, 1e-10)      # (the case does tell the two schemes apart)


def test_equal_instances_have_no_spread_at_all(emu):
    """every instance at the same state: the mean is that state's error, bit for bit, and M2 is exactly zero, whatever the count (3 x is not 3 times x in floating point)"""
    case = sc.synthetic_case(5, 2, "inf", 1, 1, 2, seed=4)
    for n in (3, 67, 131):
        many = dict(case, traj=np.ascontiguousarray(np.repeat(case["traj"], n, axis=0)))
        mean, M2 = ec.emu_ensemble_run(emu, many, np.arange(5))
        one = ec.emu_ensemble_run(emu, case, np.arange(5))[0]
        assert (M2 == 0.0).all() and np.array_equal(mean, one)


def test_a_nan_in_one_body_is_that_bodys_coordinates_alone(emu):
    case = sc.synthetic_case(5, 3, "gated", 1, 70, 8, seed=3)
    clean = dict(case, traj=case["traj"].copy())
    case["traj"][66, 3, 1, 8] = np.inf           # body 1, step 4 (k < N = 5: the feedback reads it); step 7 lies behind the gate
    case["traj"][2, 6, 1, 8] = np.nan
    perm = np.array([3, 1, 4, 0, 2])
    mean, M2 = ec.emu_ensemble_run(emu, case, perm)
    m0, q0 = ec.emu_ensemble_run(emu, clean, perm)
    bad = np.zeros(mean.shape, dtype=bool)
    bad[3, 12:24] = bad[6, 12:24] = True
    bad[3, 60:] = True
    hit = bad.copy()
    hit[3, 12:24] = hit[6, 12:24] = False
    hit[3, 12 + 4] = hit[6, 12 + 4] = True       # entry 8 of the state is v_y: coordinate 4 of the body's error
    assert np.isnan(mean[hit]).all() and np.isnan(M2[hit]).all()
    keep = ~bad
    assert np.array_equal(mean[keep], m0[keep]) and np.array_equal(M2[keep], q0[keep])
    others = bad & ~hit
    assert np.array_equal(mean[others], m0[others]) and np.array_equal(M2[others], q0[others])      # the body's other coordinates keep their bits too


def test_emulated_chunks_are_bitwise_one_call(emu):
    case = sc.synthetic_case(9, 3, "tracking", 1, 70, 23, seed=5)
    perm = np.random.default_rng(2).permutation(9)
    whole = ec.emu_ensemble_run(emu, case, perm)
    for plan in ([1] * 23, [7, 7, 7, 2], [20, 3]):
        k0, rows = 1, []
        for n in plan:
            rows.append(ec.emu_ensemble_run(emu, dict(case, traj=np.ascontiguousarray(case["traj"][:, k0 - 1:k0 - 1 + n])), perm, k0=k0))
            k0 += n
        assert np.array_equal(np.concatenate([r[0] for r in rows]), whole[0]) and np.array_equal(np.concatenate([r[1] for r in rows]), whole[1]), plan


def _stats(cclqr, x, mx, knots):
    mean, M2, _, _ = ec.moments_of(x, np.abs(x))
    C = {j: ec.comoment_of(x[j], np.abs(x[j]), mx)[0].astype(np.float64) for j in knots}
    mean, M2 = mean.astype(np.float64), M2.astype(np.float64)
    return cclqr.EnsembleStats(x.shape[1], mean[:, :mx], M2[:, :mx], mean[:, mx:], M2[:, mx:], C)


def test_merging_two_halves_gives_the_whole(cclqr):
    """Chan's merge on (count, mean, M2, C): two uneven shards against the statistics of the whole batch, within the bound of the whole; an empty shard is the identity"""
    rng = np.random.default_rng(0)
    steps, n, mx, mu = 5, 200, 24, 2
    x = 3.0 + rng.normal(size=(steps, n, mx + mu))
    xm = np.abs(x)
    whole, a, b = _stats(cclqr, x, mx, (0, 3)), _stats(cclqr, x[:, :77], mx, (0, 3)), _stats(cclqr, x[:, 77:], mx, (0, 3))
    m = a.merge(b)
    mean, M2, Amean, AM2 = ec.moments_of(x, xm)
    assert m.count == n
    ec.assert_close(np.hstack([m.mean, m.input_mean]), mean, Amean, "merged mean")
    ec.assert_close(np.hstack([m.M2, m.input_M2]), M2, AM2, "merged M2")
    for j in (0, 3):
        Cref, AC = ec.comoment_of(x[j], xm[j], mx)
        ec.assert_close(m.C[j], Cref, AC, "merged C[%d]" % j)
        assert np.array_equal(m.C[j], m.C[j].T)
        assert np.allclose(m.cov(j), np.cov(x[j, :, :mx].T, bias=True), rtol=1e-9, atol=1e-12)
        assert np.allclose(m.second_moment(j), x[j, :, :mx].T @ x[j, :, :mx] / n, rtol=1e-9)
    assert np.allclose(m.rms ** 2, (x[:, :, :mx] ** 2).mean(axis=1), rtol=1e-12) and np.allclose(m.std, x[:, :, :mx].std(axis=1), rtol=1e-9)
    assert np.allclose(m.var(ddof=1), x[:, :, :mx].var(axis=1, ddof=1), rtol=1e-9) and np.allclose(m.input_rms ** 2, (x[:, :, mx:] ** 2).mean(axis=1), rtol=1e-12)
    empty = cclqr.EnsembleStats.empty(steps, mx, mu, (0, 3))
    for e in (whole.merge(empty), empty.merge(whole)):
        assert e.count == n and np.array_equal(e.mean, whole.mean) and np.array_equal(e.M2, whole.M2) and np.array_equal(e.input_M2, whole.input_M2)
        assert all(np.array_equal(e.C[j], whole.C[j]) for j in (0, 3))
    with pytest.raises(KeyError, match="cov_knots"):
        whole.cov(1)
    with pytest.raises(KeyError, match="cov_knots"):
        whole.second_moment(4)


def test_python_side_refusals(cclqr):
    """they raise before any device call: no GPU is touched here"""
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ens = cclqr.Ensemble(mech, cov_knots=(0, 5))
    assert ens.cov_knots == (0, 5)

    class Closure(cclqr.Controller):
        controlfunction = staticmethod(lambda batch, c, k: None)

    with pytest.raises(ValueError, match="controlfunction"):
        cclqr.simulate(mech, 0.1, Closure(), ensemble=ens)
    with pytest.raises(TypeError, match="Ensemble"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), ensemble=np.eye(3))
    other = cclqr.examples.cartpole_n(1)["mech"]
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.simulate(other, 0.1, cclqr.Controller(), ensemble=ens)
    with pytest.raises(ValueError, match="at least one step"):
        cclqr.simulate(mech, 0.0, cclqr.Controller(), ensemble=ens)
    with pytest.raises(ValueError, match="chunk_steps"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), ensemble=ens, chunk_steps=0)
    with pytest.raises(ValueError, match="cov_knots"):
        cclqr.simulate(mech, cclqr.Storage(5, len(mech.bodies)), cclqr.Controller(), ensemble=ens)      # knot 5 of a 5-step run
    with pytest.raises(ValueError, match="cov_knots"):
        cclqr.Ensemble(mech, cov_knots=(-1,))
    with pytest.raises(TypeError, match="Ensemble"):
        cclqr.Ensemble("mech")
    with pytest.raises(ValueError, match="chunk_steps"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), chunk_steps=3)      # still an option of score= / ensemble= only


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name) and "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name in jl and name in integ
        i = hdr.index("int %s(" % name)
        assert re.search(r"\.jl:\d+", hdr[max(0, i - 3500):i]), name
    assert re.search(r"Still 202[^\n]*cclqr_rollout_ensemble_ws_bytes, cclqr_rollout_ensemble", hdr[:hdr.index("#define CCLQR_ABI_VERSION")])
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    assert "ensemble.hip" in mk and "cclqr_ensemble.h" in mk
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202 and all(hasattr(L, n) for n in NAMES)
