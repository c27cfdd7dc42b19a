"""One LQR per plant (cclqr_linearize_plants, cclqr_ctrl_create_lqr_batch_plants, PlantLQR), the parts that need no GPU: the linearisation kernel's body on a
plant record, run serially on the CPU (tests/emu/emu_lin_plants.cpp), the fixtures the GPU tests share, and the surface."""
import os
import re

import numpy as np
import pytest

from plant_lqr_common import CASES, SLIDERS, _rel, case, emu_lin_plants, emu_linearize_on, oracle_gains, oracle_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(ms):
    return [np.ascontiguousarray(m).view(np.uint64) for m in ms]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("name", CASES[:3])
def test_fixtures_are_what_the_gpu_tests_assume(cclqr, orc, name):
    """the shared cases, stated with the oracle alone: every plant's setpoint lies on its own constraint manifold (5e-16), every recursion runs all N - 1 steps
    with finite gains of the stated size, and the plants matter -- each plant's gains differ from the nominal plant's by at least 5.3e-2 relative, its A and Bu
    by at least 5.6e-2 (the smallest, Bu of plant 0 of the tree-slider, is 5.69e-2).  (A table that the device silently ignored would therefore miss the GPU tests' 1e-10 / 1e-7 by orders of magnitude.)"""
    c = case(cclqr, name)
    assert c["n"] == 6 and c["N"] == 40
    for i in range(c["n"]):
        assert np.abs(orc.constraints(c["plants"].tables(i), c["zd"][i])).max() <= 5e-16
    per, nom = oracle_models(orc, c)
    K, kb, (Kn, kbn) = oracle_gains(orc, c)
    assert kb == [1] * c["n"] and int(kbn) == 1
    for i in range(c["n"]):
        assert np.isfinite(K[i]).all() and 138 <= np.abs(K[i]).max() <= 401
        assert _rel(K[i], Kn) >= 5.3e-2
        assert _rel(per[i][0], nom[0]) >= 5.6e-2 and _rel(per[i][1], nom[1]) >= 5.6e-2


@pytest.mark.parametrize("name", CASES[:3])
def test_kernel_body_on_a_plant_record(cclqr, orc, emu, name):
    """the serial twin of linearize_kernel for one knot, on link-order records: on record i of PlantBatch.link_records() its A, Bu, Bl, G equal BIT FOR BIT what
    the existing twin (emu_linearize) gives on a mechanism built from plant i's own tables, on the mechanism's own records (given, or defaulted) what it gives
    on the mechanism; and they agree with the oracle on plant i's tables to 1e-10.  On the slider mechanisms plant i's Bu column of the slider joint differs
    from the nominal one in the PARENT body's rows: the child joint's vertex p1 is read from the record."""
    c = case(cclqr, name)
    t, cj, plants = c["t"], c["cj"], c["plants"]
    L = emu_lin_plants()
    rec = plants.link_records()
    per, _ = oracle_models(orc, c)
    own = cclqr.PlantBatch(c["mech"], mass=t.mass[None], inertia=t.inertia[None], p1=t.p1[None], p2=t.p2[None]).link_records()[0]
    base = emu_linearize_on(emu, "emu_linearize", orc, t, c["zd_nominal"], cj, c["Fd"][0])
    assert _same_bits(emu_linearize_on(L, "emu_lin_plants", orc, t, c["zd_nominal"], cj, c["Fd"][0], records=own), base)
    assert _same_bits(emu_linearize_on(L, "emu_lin_plants", orc, t, c["zd_nominal"], cj, c["Fd"][0], records=None), base)
    for i in range(c["n"]):
        got = emu_linearize_on(L, "emu_lin_plants", orc, t, c["zd"][i], cj, c["Fd"][i], records=rec[i])
        assert _same_bits(got, emu_linearize_on(emu, "emu_linearize", orc, plants.tables(i), c["zd"][i], cj, c["Fd"][i]))
        for a, b in zip(got, per[i]):
            assert _rel(a, b) < 1e-10
        assert not _same_bits(got[:2], base[:2])
        if name in SLIDERS:
            col = cj.index(c["slider"])
            pa = int(t.parent[c["slider"]])                        # the slider's parent body: its ω rows carry -2 D_R^-1 (p1 x axis)
            rows = slice(12 * pa + 9, 12 * pa + 12)
            assert np.abs(got[1][rows, col]).max() > 1e-3 and np.abs(got[1][rows, col] - base[1][rows, col]).max() > 1e-4 * np.abs(base[1][rows, col]).max()
    if name in SLIDERS:
        # the evidence that the child-p1 sites are reached: a record that differs from the mechanism's in the SLIDER's p1 alone changes the parent's rows
        sl = int(np.flatnonzero(cclqr.link_order(t)[1] == c["slider"])[0])
        r2 = own.copy()
        r2[sl, 10:13] *= 1.05
        z2 = cclqr.joint_position_states(c["mech"], c["th"][:1], plants=cclqr.PlantBatch(c["mech"], p1=np.where(np.arange(t.ne)[:, None] == c["slider"], 1.05, 1.0)[None] * t.p1[None]))[0]
        got = emu_linearize_on(L, "emu_lin_plants", orc, t, z2, cj, c["Fd"][0], records=r2)
        col, pa = cj.index(c["slider"]), int(t.parent[c["slider"]])
        assert np.abs(got[1][12 * pa + 9:12 * pa + 12, col] - base[1][12 * pa + 9:12 * pa + 12, col]).max() > 1e-6


def test_surface(cclqr):
    """include/cclqr.h declares both entry points under a comment that cites the reference lines they stand for, the binding lists them (the ABI stays 202: additive, the layout vector unchanged),
    the Julia shim has their ccall stubs, and the package exports PlantLQR"""
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    for name in ("cclqr_linearize_plants", "cclqr_ctrl_create_lqr_batch_plants"):
        i = hdr.index("int " + name + "(")
        assert re.search(r"\.jl:\d+", hdr[max(0, i - 1500):i][hdr[max(0, i - 1500):i].rindex("/*"):]), name
        assert name in cclqr._capi.EXPORTS
        assert ":" + name in open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    assert "lqr.jl:63" in hdr[hdr.index("/* cclqr_linearize on per-instance plants"):hdr.index("int cclqr_linearize_plants(")]
    assert "lqr.jl:141-184" in hdr[hdr.index("/* cclqr_ctrl_create_lqr_batch with one plant"):hdr.index("int cclqr_ctrl_create_lqr_batch_plants(")]
    assert cclqr._capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr
    assert issubclass(cclqr.PlantLQR, cclqr.Controller)
    if os.path.exists(cclqr._capi.LIB_PATH):
        L = cclqr._capi.lib()
        assert L.cclqr_version() == 202
        # the argument checks that precede any device work
        assert L.cclqr_linearize_plants(None, None, 0, 1, None, 0, None, None, None, None, None, None) == cclqr._capi.EINVAL
        assert L.cclqr_ctrl_create_lqr_batch_plants(None, None, 0, 1, None, 1, None, None, None, None, 2, 0, 0, None, None) == cclqr._capi.EINVAL


def test_plantlqr_refusals_need_no_library(cclqr, monkeypatch):
    """PlantLQR refuses, on the host, a PlantBatch of another mechanism, setpoints that do not match the plants' rows, and what the batched constructor does not
    carry (controlfunction, friction, noise) -- before the library is touched"""
    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(cclqr._capi, "lib", no_library)
    monkeypatch.setattr(cclqr._capi, "MechHandle", no_library)
    c = case(cclqr, "chain2")
    mech, plants, t = c["mech"], c["plants"], c["t"]
    ids, eids = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[0])]
    Q, R = [np.eye(12) * 10.0] * t.nb, [np.eye(1) * 0.1]
    other = case(cclqr, "chain-slider")
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.PlantLQR(mech, other["plants"], ids, eids, Q, R, 0.4, c["zd"])
    with pytest.raises(ValueError, match=r"zd must be \[n\]\[nb\]\[13\]"):
        cclqr.PlantLQR(mech, plants, ids, eids, Q, R, 0.4, c["zd"][:, :2])
    with pytest.raises(ValueError, match="not all among the plants 0 .. 5"):
        cclqr.PlantLQR(mech, plants, ids, eids, Q, R, 0.4, np.concatenate([c["zd"], c["zd"][:1]]))
    with pytest.raises(ValueError, match="not all among the plants 0 .. 5"):
        cclqr.PlantLQR(mech, plants, ids, eids, Q, R, 0.4, c["zd"][:2], first_plant=5)
    with pytest.raises(ValueError, match="one holding input per plant"):
        cclqr.PlantLQR(mech, plants, ids, eids, Q, R, 0.4, c["zd"], Fτd=np.zeros((3, 1)))
    with pytest.raises(ValueError, match="controlfunction"):
        cclqr.PlantLQR(mech, plants, ids, eids, Q, R, 0.4, c["zd"], controlfunction=lambda batch, ctl, k: None)
    # friction and noise reach a controller through simulate -> _ctrl_handle: refused there, whatever the controller holds
    blank = cclqr.PlantLQR.__new__(cclqr.PlantLQR)
    for kw in (dict(fric=np.ones(t.ne)), dict(noise_scale=1.0), dict(noise_seed=7)):
        with pytest.raises(ValueError, match="neither joint friction nor noise"):
            blank._ctrl_handle(None, **kw)
