"""One TrackingLQR per plant, the parts that need no GPU: the chunk rule and the knot -> (plant, setpoint row) map of cclqr_ctrl_create_tracking_batch_plants
through their host twin, PlantTrackingLQR's validation, and the oracle facts the GPU tests' fixtures rest on."""
import ctypes as C
import os

import numpy as np
import pytest

from plants_common import ROOT
from plant_tracking_common import BREAK_TOL, CASES, HANGING, SMALL, _rel, case, emu_tracking_plan, oracle_gains, oracle_nominal


@pytest.fixture(scope="module")
def plan():
    return emu_tracking_plan()


def _chunks(plan, n, per, fixed, budget):
    pc = plan.emu_tracking_chunk_problems(n, per, fixed, budget)
    if pc < 1:
        return pc, []
    cnt = plan.emu_tracking_chunk_count(n, pc)
    return pc, [(i * pc, min(n, (i + 1) * pc)) for i in range(cnt)]


def test_chunks_cover_every_problem_once_within_the_budget(plan):
    """tracking_chunk_problems / tracking_chunk_count: the chunks are consecutive, cover [0, n_ctrl) exactly once, none is empty, each fits the budget next to
    the fixed part, and no budget that holds one more problem per chunk would have been left unused by more than the evening-out allows"""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        n = int(rng.integers(1, 5000))
        per = int(rng.integers(1, 1 << 27))
        fixed = int(rng.integers(0, 1 << 20))
        budget = fixed + int(rng.integers(per, 64 * per + 1)) if rng.random() < 0.9 else fixed + per
        pc, ch = _chunks(plan, n, per, fixed, budget)
        assert pc >= 1 and ch
        assert ch[0][0] == 0 and ch[-1][1] == n and all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and all(hi > lo for lo, hi in ch)
        assert all(fixed + (hi - lo) * per <= budget for lo, hi in ch)
        fit = min((budget - fixed) // per, n)
        assert len(ch) == -(-n // fit)          # as few chunks as the budget allows; evening out changes their sizes, not their number
        assert max(hi - lo for lo, hi in ch) - min(hi - lo for lo, hi in ch) <= len(ch) - 1 or len(ch) == 1


def test_one_chunk_when_everything_fits_and_refusal_when_one_problem_does_not(plan):
    per, fixed = 64 << 20, 4096
    assert _chunks(plan, 7, per, fixed, fixed + 7 * per) == (7, [(0, 7)])
    assert _chunks(plan, 7, per, fixed, fixed + 700 * per) == (7, [(0, 7)])
    assert _chunks(plan, 7, per, fixed, fixed + 7 * per - 1)[0] == 4          # two chunks, evened out: 4 + 3
    assert _chunks(plan, 7, per, fixed, fixed + per)[0] == 1
    for budget in (fixed + per - 1, fixed, 1):
        assert plan.emu_tracking_chunk_problems(7, per, fixed, budget) == 0
    # <= 0 is the default budget, a few GiB: 64 MB problems run 63 to a chunk next to the fixed part, evened out over 1024 / 63 -> 17 chunks
    default = plan.emu_tracking_default_budget()
    assert 1 << 30 <= default <= 8 << 30
    for b in (0, -5):
        assert plan.emu_tracking_chunk_problems(1024, per, fixed, b) == plan.emu_tracking_chunk_problems(1024, per, fixed, default) == 61
    # a launch never holds more problems than the grids' y extent
    cap = plan.emu_tracking_max_chunk()
    assert cap <= 65535 and plan.emu_tracking_chunk_problems(10 * cap, 8, 0, 1 << 40) == cap


def test_problem_bytes_are_the_issue_arithmetic(plan):
    """triple cartpole (mx 48, mu 1, ml 20), per knot: A 2304 + Bu 48 + Bl 960 + G 960 doubles of model; [A'|D] 2352 and the projection scratch (ml^2 + ml na = 1380) are
    the recursion's share, passed in"""
    N, ric = 1000, 999 * (2352 + 1382 + 22) + 12345
    got = plan.emu_tracking_problem_bytes(48, 1, 20, N, ric)
    assert got == 8 * (999 * (2304 + 48 + 960 + 960) + ric) + 4 * 1000
    assert 60e6 < got < 70e6                       # "about 64 KB per knot"


def test_knot_to_row_and_plant(plan):
    """lin_knot_rows, the function linearize_kernel calls: rows_per_plant = 0 is the one-knot-per-plant map of cclqr_linearize_plants; with N rows and N - 1 knots
    per problem, knot q belongs to problem q / (N - 1) and reads row problem * N + q % (N - 1): every trajectory's last row is skipped, nothing else is"""
    out = (C.c_longlong * 2)()
    for q in (0, 1, 17, 123456):
        for kpp in (0, 1, 9):
            plan.emu_lin_knot_rows(q, kpp, 0, out)
            assert tuple(out) == (q, q)
    for N in (2, 3, 24, 1000):
        seen = []
        for q in range(5 * (N - 1)):
            plan.emu_lin_knot_rows(q, N - 1, N, out)
            assert out[0] == q // (N - 1) and out[1] == out[0] * N + q % (N - 1)
            seen.append(out[1])
        assert seen == [r for r in range(5 * N) if r % N != N - 1]
    plan.emu_lin_knot_rows(1023 * 999 + 998, 999, 1000, out)
    assert tuple(out) == (1023, 1023 * 1000 + 998)


def test_python_side_validation(cclqr, orc):
    """shape errors of storage and Fτ, a PlantBatch of another mechanism, plants out of range, a controlfunction: ValueError before any device call"""
    c = case(cclqr, orc, "chain3")
    mech, nb, n, N = c["mech"], c["t"].nb, c["n"], c["N"]
    eids = [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
    Q, R = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1]
    mk = lambda storage=c["zd"], F=c["U"], plants=c["plants"], **kw: cclqr.PlantTrackingLQR(mech, plants, storage, F, eids, Q, R, **kw)
    with pytest.raises(ValueError, match=r"storage must be \[n\]\[N\]\[nb\]\[13\]"):
        mk(storage=c["zd"][0])
    with pytest.raises(ValueError, match=r"storage must be \[n\]\[N\]\[nb\]\[13\]"):
        mk(storage=c["zd"][:, :, :2])
    with pytest.raises(ValueError, match="at least two steps"):
        mk(storage=c["zd"][:, :1])
    with pytest.raises(ValueError, match="Fτ must be"):
        mk(F=c["U"][:-1])
    with pytest.raises(ValueError, match="Fτ must be"):
        mk(F=np.zeros((n - 1, N, 1)))
    other = case(cclqr, orc, "chain4")
    with pytest.raises(ValueError, match="another mechanism"):
        mk(plants=other["plants"])
    with pytest.raises(ValueError, match="are not all among the plants 0 .. 4"):
        mk(first_plant=1)
    with pytest.raises(ValueError, match="are not all among the plants 0 .. 4"):
        mk(storage=np.concatenate([c["zd"], c["zd"][:1]]))
    with pytest.raises(ValueError, match="no controlfunction"):
        mk(controlfunction=lambda *a: None)
    with pytest.raises(AssertionError, match="Missmatched length for constraints"):
        cclqr.PlantTrackingLQR(mech, c["plants"], c["zd"], c["U"], eids, Q, R + R)


@pytest.mark.parametrize("name", SMALL + ("tree-slider-128",))
def test_oracle_facts_of_the_fixtures(cclqr, orc, name):
    """what the GPU tests rely on, so that the fixtures cannot drift: every oracle solve converges on a non-singular model (orc.riccati_tracking raises otherwise),
    all gains are finite, kbreak = 1 everywhere, and the gains differ by more than 1e-2 between plants (and, on the hanging mechanisms, from the nominal plant's)"""
    c = case(cclqr, orc, name)
    assert c["zd"].shape == (c["n"], c["N"], c["t"].nb, 13) and (c["n"], c["N"]) == CASES[name][:2]
    og = oracle_gains(orc, c)
    ks = list(c["check"])
    assert all(np.isfinite(og[i][0]).all() and og[i][1] == 1 for i in ks)
    assert all(_rel(og[i][0], og[ks[0]][0]) > 1e-2 for i in ks[1:])
    if name in HANGING:
        Kn, _ = oracle_nominal(orc, c)
        assert all(_rel(og[i][0], Kn) > 1e-2 for i in ks)
    assert max(_rel(og[i][0][0], og[i][0][-1]) for i in ks) > 1e-2          # the gains vary along a trajectory: a time-invariant solve would not pass


def test_oracle_facts_of_the_break_case(cclqr, orc):
    """rest trajectories at the hanging pose with tol = 2.0: every plant's recursion breaks, at least three distinct knots, none at knot 1 -- and none of the breaks
    is marginal: the same knots at tol (1 -+ 1e-3), i.e. | ||Pk - Pkp1|| - tol | > 2e-3 at every break, four orders above the 1e-7 the gains are held to"""
    c = case(cclqr, orc, "break")
    kb = [oracle_gains(orc, c)[i][1] for i in c["check"]]
    assert kb == [45, 43, 41, 80, 39]
    assert len(set(kb)) >= 3 and min(kb) > 1
    for f in (1 - 1e-3, 1 + 1e-3):
        assert [oracle_gains(orc, c, tol=BREAK_TOL * f)[i][1] for i in c["check"]] == kb


def test_the_entry_points_are_declared_everywhere(cclqr):
    """additive over ABI 202: the two symbols are in the header, the binding's export list and the Julia shim; the version and the struct layout are untouched"""
    header = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    for name in ("cclqr_ctrl_create_tracking_batch_plants", "cclqr_ctrl_get_gains"):
        assert "int %s(" % name in header and name in cclqr._capi.EXPORTS and ":" + name in jl
    assert "#define CCLQR_ABI_VERSION 202" in header and cclqr._capi.ABI_VERSION == 202 and "#define CCLQR_ABI_LAYOUT_LEN 48" in header
    assert hasattr(cclqr, "PlantTrackingLQR") and hasattr(cclqr._capi, "BatchTrackingHandle") and hasattr(cclqr._capi, "ctrl_gains")
