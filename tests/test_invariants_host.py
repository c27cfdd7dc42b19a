"""CPU tests of the invariants feature's host side: the additive C ABI (header with the definition, binding, Julia shim, INTEGRATION.md, Makefile; version 202), the
resources of csrc/invariants.hip as compiled for gfx950 against the joints kernel's, the cross-lane rule on its source, the Python-side refusals of Invariants /
simulate(invariants=) and the InvariantSeries accessors."""
import os
import re

import numpy as np
import pytest

import invariants_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cclqr_rollout_invariants"


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "int %s(" % NAME in hdr and NAME in capi.EXPORTS and ":" + NAME in jl and NAME in integ
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*" + NAME, head)
    assert "#define CCLQR_INVARIANTS_LEN 6" in hdr and "#define CCLQR_INVARIANTS_SUMMARY_LEN 8" in hdr
    assert (capi.INVARIANTS_LEN, capi.INVARIANTS_SUMMARY_LEN) == (ic.LEN, ic.SUMMARY_LEN) == (6, 8)
    assert len(cclqr.InvariantSeries.NAMES) == capi.INVARIANTS_LEN
    doc = hdr[hdr.index("The integrator's own invariants"):hdr.index("int %s(" % NAME)]
    for stated in ("xor butterfly", "link order", "PROPAGATES a NaN", "never Inf", "CCLQR_FIXED_ORIENTATION", "read and merged when k0 > 1", "CCLQR_EINVAL"):
        assert stated in doc, stated      # the summation order and the NaN rule are part of the contract
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    srcs, hdrs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split(), re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    assert "invariants.hip" in srcs and "cclqr_invariants.h" in hdrs
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202 and hasattr(L, NAME)


def test_invariants_kernel_resources():
    """csrc/invariants.hip cross-compiled for gfx950: no kernel touches scratch memory or spills a vector register, all LDS is dynamic, and every instantiation has at
    least the occupancy of the joints kernel of the same shape (512 vector registers to a SIMD lane, allocated in blocks of 8)"""
    from build_common import device_asm
    inv, jnt = device_asm("invariants.hip"), device_asm("joints.hip")
    names = inv.kernel_names("_ZN5cclqr17invariants_kernel")
    assert len(names) == 5 and names == inv.kernel_names(), inv.kernel_names()      # four lane-group sizes and the closed-loop form, nothing else
    waves = lambda k: 512 // (-(-(k["vgpr"] + k["agpr"]) // 8) * 8)
    for name in names:
        k = inv.kernel(name).resources
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, dict(k))
        twin = name.replace("17invariants_kernel", "13joints_kernel").replace("NS_7InvArgsE", "NS_10JointsArgsE")
        assert waves(k) >= min(waves(jnt.kernel(twin).resources), 8), (name, dict(k), dict(jnt.kernel(twin).resources))


def test_the_kernel_source_keeps_the_cross_lane_rule():
    """invariants.hip under the scanner of test_static_kernel_rules: every cross-lane operation of the kernel sits directly in the step loop, whose bounds are launch
    arguments -- under no lane predicate --, the header holds none, and there is neither an atomic nor inline assembly"""
    import test_static_kernel_rules as rules
    txt = rules.strip_comments(open(os.path.join(rules.CSRC, "cclqr_invariants.h")).read())
    assert not rules.CROSS.search(txt) and not re.search(r"\basm\b", txt)
    txt = rules.strip_comments(open(os.path.join(rules.CSRC, "invariants.hip")).read())
    body = txt[txt.index("void invariants_kernel("):txt.index("hipError_t launch_invariants")]
    seen = 0
    for m in re.finditer(r"\binv_wave_sync\(\)|\binv_group_(sum|max)<G>\(", body):
        seen += 1
        hdrs = rules.enclosing_headers(body, m.start())
        assert [(kw, cond) for kw, cond in hdrs] == [("for", "int kk = 0; kk < steps; kk++")], hdrs
    assert seen == 7      # the two wave syncs and the five butterflies
    assert not rules.CROSS.search(re.sub(r"inv_group_(sum|max)", "", body))      # and no other cross-lane operation in the kernel body
    assert not re.search(r"\batomic\w*\(", txt) and not re.search(r"\basm\b", txt) and "__syncthreads" not in txt


def test_python_side_refusals(cclqr):
    """they raise before any device call: no GPU is touched here"""
    mech = cclqr.examples.cartpole_n(1)["mech"]
    nb = len(mech.bodies)
    v = cclqr.Invariants(mech)
    assert v.mechanism is mech and v.keep and not v.rows and v.quantiles == ()
    v = cclqr.Invariants(mech, keep=False, rows=True, quantiles=(0, 0.5, 1))
    assert (v.keep, v.rows, v.quantiles) == (False, True, (0.0, 0.5, 1.0))
    with pytest.raises(TypeError, match="Invariants\\(mechanism"):
        cclqr.Invariants("cartpole")
    for kw in ("keep", "rows"):
        with pytest.raises(TypeError, match=kw):
            cclqr.Invariants(mech, **{kw: 1})
    for bad in ((1.5,), (-0.1,), (0.5, float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cclqr.Invariants(mech, quantiles=bad)
    with pytest.raises(ValueError, match="at most 16"):
        cclqr.Invariants(mech, quantiles=tuple(np.linspace(0, 1, 17)))
    z0 = np.zeros((2, nb, 13))
    with pytest.raises(TypeError, match="invariants= takes an Invariants"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), invariants=cclqr.Joints(mech), z0=z0)
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), invariants=cclqr.Invariants(cclqr.examples.cartpole_n(1)["mech"]), z0=z0)
    with pytest.raises(ValueError, match="16384"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), invariants=cclqr.Invariants(mech, quantiles=(0.5,)), z0=np.zeros((16385, nb, 13)))
    closure = cclqr.Controller()
    closure.controlfunction = lambda *a: None
    with pytest.raises(ValueError, match="custom controlfunction"):
        cclqr.simulate(mech, 0.1, closure, invariants=cclqr.Invariants(mech), z0=z0)
    with pytest.raises(ValueError, match="chunk_steps is an option"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), chunk_steps=3, z0=z0)
    assert cclqr.Storage(3, nb).invariants is None


def test_invariant_series_accessors(cclqr):
    rng = np.random.default_rng(0)
    n, steps = 7, 5
    x = rng.normal(size=(n, steps, 6))
    g = rng.normal(size=(n, steps, 2, 5))
    summ = ic.summary_of(x)
    mean, M2 = x.mean(axis=0), ((x - x.mean(axis=0)) ** 2).sum(axis=0)
    q, fin = rng.normal(size=(steps, 3, 6)), np.full((steps, 6), n, dtype=np.int32)
    s = cclqr.InvariantSeries(n, summ, mean, M2, x, g, probs=(0.0, 0.5, 1.0), quantiles=q, finite_count=fin)
    assert s.count == n and s.NAMES == ("kinetic", "potential", "energy", "gap", "twist", "quat")
    for c, name in enumerate(s.NAMES):
        assert np.array_equal(getattr(s, name), x[:, :, c])
    assert np.array_equal(s.g, g)
    assert np.array_equal(s.energy_first, x[:, 0, 2]) and np.array_equal(s.energy_min, x[:, :, 2].min(axis=1)) and np.array_equal(s.energy_max, x[:, :, 2].max(axis=1))
    assert np.array_equal(s.gap_max, x[:, :, 3].max(axis=1)) and np.array_equal(s.gap_step, x[:, :, 3].argmax(axis=1) + 1) and s.gap_step.dtype == np.int64
    assert np.array_equal(s.twist_max, x[:, :, 4].max(axis=1)) and np.array_equal(s.quat_max, x[:, :, 5].max(axis=1))
    assert np.array_equal(s.bad_rows, np.zeros(n, dtype=np.int64))
    # energy_drift = max(E_max - E_1, E_1 - E_min), in that arithmetic
    E = x[:, :, 2]
    assert np.array_equal(s.energy_drift, np.maximum(E.max(axis=1) - E[:, 0], E[:, 0] - E.min(axis=1))) and (s.energy_drift >= 0).all()
    one = cclqr.InvariantSeries(1, [[2.0, 1.5, 4.0, 0, 0, 0, 0, 0]], mean, M2)
    assert one.energy_drift[0] == 2.0      # max(4 - 2, 2 - 1.5)
    assert np.allclose(s.std, x.std(axis=0)) and np.allclose(s.var(ddof=1), x.var(axis=0, ddof=1))
    assert np.array_equal(s.quantile(0.5), q[:, 1]) and np.array_equal(s.median, q[:, 1]) and np.array_equal(s.min, q[:, 0]) and np.array_equal(s.max, q[:, 2])
    assert np.array_equal(s.finite_count, fin)
    with pytest.raises(KeyError, match=r"0\.25.*\[0\.0, 0\.5, 1\.0\]"):
        s.quantile(0.25)
    bare = cclqr.InvariantSeries(n, summ, mean, M2)
    assert bare.energy is None and bare.gap is None and bare.g is None and bare.finite_count is None and bare.probs is None
    assert np.array_equal(bare.gap_max, s.gap_max)      # the summary is always there
    with pytest.raises(KeyError, match="not asked for"):
        bare.median
    with pytest.raises(ValueError):
        cclqr.InvariantSeries(n, summ[:, :7], mean, M2)      # a summary has eight entries
    # rows that are not finite are left out of the summary and counted
    y = x.copy()
    y[0, 0, 2] = np.nan
    y[1, :, :] = np.nan
    t = cclqr.InvariantSeries(n, ic.summary_of(y), mean, M2, y)
    assert t.energy_first[0] == y[0, 1, 2] and t.bad_rows[0] == 1 and t.bad_rows[1] == steps and np.isnan(t.energy_drift[1]) and t.gap_step[1] == 0
