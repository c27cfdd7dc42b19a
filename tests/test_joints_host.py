"""CPU tests of the joint-coordinate feature's host side: the additive C ABI (header with its citations, binding, Julia shim, INTEGRATION.md, Makefile; version 202,
layout 48), the resources of csrc/joints.hip as compiled for gfx950, the Python-side refusals of Joints / simulate(joints=) and the JointSeries accessors."""
import ctypes
import os
import re

import numpy as np
import pytest

import joints_common as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_rollout_joints", "cclqr_series_ensemble_ws_bytes", "cclqr_series_ensemble", "cclqr_series_quantiles_ws_bytes", "cclqr_series_quantiles")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name) and "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name in jl and name in integ
        i = hdr.index("int %s(" % name)
        assert re.search(r"\.jl:\d+", hdr[max(0, i - 4500):i]), name
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_rollout_joints,\n[^\n]*cclqr_series_ensemble_ws_bytes, cclqr_series_ensemble, cclqr_series_quantiles_ws_bytes, cclqr_series_quantiles", head)
    assert "pid.jl:43-57" in hdr and "trackingLQR_triple_cartpole.jl:98-101" in hdr
    assert "#define CCLQR_JOINTS_RAW 0" in hdr and "#define CCLQR_JOINTS_CONTINUOUS 1" in hdr and "#define CCLQR_SERIES_MAX_COORDS 1024" in hdr
    assert (capi.JOINTS_RAW, capi.JOINTS_CONTINUOUS, capi.SERIES_MAX_COORDS) == (jc.RAW, jc.CONTINUOUS, 1024)
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    srcs, hdrs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split(), re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    assert "joints.hip" in srcs and "cclqr_joints.h" in hdrs
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202 and all(hasattr(L, n) for n in NAMES)


def test_joint_kernel_resources():
    """csrc/joints.hip cross-compiled for gfx950: no kernel touches scratch memory or spills a vector register, all their LDS is dynamic, and the joints kernel's at
    nb = 64 (one 13 nb row per instance, four wavefronts) and the tile-moments kernel's stay within 160 KB"""
    from build_common import device_asm
    asm = device_asm("joints.hip")
    joints, moments, stage = (asm.kernel_names("_ZN5cclqr" + k) for k in ("13joints_kernel", "21series_moments_kernel", "19series_stage_kernel"))
    assert len(joints) == 5 and len(moments) == 1 and len(stage) == 1, asm.kernel_names()      # four lane-group sizes and the closed-loop form
    for name in joints + moments + stage:
        k = asm.kernel(name).resources
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, dict(k))
        assert k["vgpr"] <= 256, (name, dict(k))      # 256 threads to a workgroup: at least two wavefronts to a SIMD
    emu = jc.emu_joints()
    emu.emu_joints_lds.restype = emu.emu_series_moments_lds.restype = ctypes.c_longlong
    assert emu.emu_joints_lds(ctypes.c_int(64)) == 8 * 4 * 833 <= 160 * 1024
    assert all(emu.emu_joints_lds(ctypes.c_int(nb)) <= 160 * 1024 for nb in range(1, 65))
    assert emu.emu_joints_lds(ctypes.c_int(17)) == 8 * 4 * 2 * 221      # the headline's 17-body chain: two instances to a wavefront
    assert emu.emu_series_moments_lds() == 64 * 1024


def test_the_kernel_source_keeps_the_cross_lane_rule():
    """joints.hip under the scanner of test_static_kernel_rules: every cross-lane operation sits under control flow on launch arguments; the header holds none"""
    import test_static_kernel_rules as rules
    txt = rules.strip_comments(open(os.path.join(rules.CSRC, "cclqr_joints.h")).read())
    assert not rules.CROSS.search(txt)
    txt = rules.strip_comments(open(os.path.join(rules.CSRC, "joints.hip")).read())
    seen = 0
    for m in re.finditer(r"\bjnt_wave_sync\(\)|__syncthreads\(\)|__shfl\w*", txt):
        if "void jnt_wave_sync" in txt[max(0, m.start() - 40):m.end()]:
            continue
        seen += 1
        for kw, cond in rules.enclosing_headers(txt, m.start()):
            assert kw == "for" and re.fullmatch(r"int kk = 0; kk < steps; kk\+\+", cond), (kw, cond)
    assert seen == 3      # the two wave syncs of the step loop and the stage kernel's one workgroup barrier
    assert not re.search(r"\batomic\w*\(", txt)


def test_python_side_refusals(cclqr):
    """they raise before any device call: no GPU is touched here"""
    mech = cclqr.examples.cartpole_n(1)["mech"]
    nb = len(mech.bodies)
    j = cclqr.Joints(mech)
    assert j.mechanism is mech and j.continuous and j.rates and j.keep and j.quantiles == ()
    j = cclqr.Joints(mech, continuous=False, rates=False, keep=False, quantiles=(0, 0.5, 1))
    assert (j.continuous, j.rates, j.keep, j.quantiles) == (False, False, False, (0.0, 0.5, 1.0))
    with pytest.raises(TypeError, match="Joints\\(mechanism"):
        cclqr.Joints("cartpole")
    for kw in ("continuous", "rates", "keep"):
        with pytest.raises(TypeError, match=kw):
            cclqr.Joints(mech, **{kw: 1})
    for bad in ((1.5,), (-0.1,), (0.5, float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cclqr.Joints(mech, quantiles=bad)
    with pytest.raises(ValueError, match="at most 16"):
        cclqr.Joints(mech, quantiles=tuple(np.linspace(0, 1, 17)))
    z0 = np.zeros((2, nb, 13))
    with pytest.raises(TypeError, match="joints= takes a Joints"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), joints=cclqr.Ensemble(mech), z0=z0)
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), joints=cclqr.Joints(cclqr.examples.cartpole_n(1)["mech"]), z0=z0)
    with pytest.raises(ValueError, match="16384"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), joints=cclqr.Joints(mech, quantiles=(0.5,)), z0=np.zeros((16385, nb, 13)))
    closure = cclqr.Controller()
    closure.controlfunction = lambda *a: None
    with pytest.raises(ValueError, match="custom controlfunction"):
        cclqr.simulate(mech, 0.1, closure, joints=cclqr.Joints(mech), z0=z0)
    with pytest.raises(ValueError, match="chunk_steps is an option"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), chunk_steps=3, z0=z0)
    assert cclqr.Storage(3, nb).joints is None


def test_joint_series_accessors():
    import __graft_entry__ as g
    cclqr = g.load_package()
    rng = np.random.default_rng(0)
    n, steps, ne = 9, 4, 3
    th, rt = rng.normal(size=(n, steps, ne)), rng.normal(size=(n, steps, ne))
    x = np.concatenate([th, rt], axis=2)
    mean, M2 = x.mean(axis=0), ((x - x.mean(axis=0)) ** 2).sum(axis=0)
    q, fin = rng.normal(size=(steps, 3, 2 * ne)), np.full((steps, 2 * ne), n, dtype=np.int32)
    s = cclqr.JointSeries(n, mean[:, :ne], M2[:, :ne], mean[:, ne:], M2[:, ne:], th, rt, probs=(0.0, 0.5, 1.0), quantiles=q, finite_count=fin)
    assert s.count == n and s.continuous and s.theta is not None and s.mean.shape == (steps, ne)
    assert np.allclose(s.std, x[..., :ne].std(axis=0)) and np.allclose(s.rate_std, x[..., ne:].std(axis=0)) and np.allclose(s.var(ddof=1), x[..., :ne].var(axis=0, ddof=1))
    assert np.array_equal(s.quantile(0.5), q[:, 1, :ne]) and np.array_equal(s.rate_quantile(1), q[:, 2, ne:]) and np.array_equal(s.median, q[:, 1, :ne])
    assert np.array_equal(s.min, q[:, 0, :ne]) and np.array_equal(s.max, q[:, 2, :ne]) and np.array_equal(s.finite_count, fin)
    with pytest.raises(KeyError, match=r"0\.25.*\[0\.0, 0\.5, 1\.0\]"):
        s.quantile(0.25)
    bare = cclqr.JointSeries(n, mean[:, :ne], M2[:, :ne])
    assert bare.theta is None and bare.rate is None and bare.finite_count is None and bare.probs is None
    with pytest.raises(KeyError, match="not asked for"):
        bare.median
    with pytest.raises(KeyError, match="rates=False"):
        bare.rate_quantile(0.5)
    with pytest.raises(KeyError, match="rates=False"):
        bare.rate_std
