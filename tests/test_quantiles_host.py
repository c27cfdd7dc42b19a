"""CPU tests of the ensemble quantiles (cclqr_rollout_quantiles): the select kernel's per-lane functions (csrc/cclqr_quantiles.h: key map, bitonic network, count and
formula) emulated lane by lane against the numpy restatement of the definition, bit for bit; the Python-side refusals; the additive C ABI (header, binding, Julia
shim, INTEGRATION.md, Makefile; version 202); and the kernels' resources as compiled for gfx950."""
import ctypes
import os
import re

import numpy as np
import pytest

import quantile_common as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_rollout_quantiles_ws_bytes", "cclqr_rollout_quantiles")
DENORMAL = 4.9406564584124654e-324


@pytest.fixture(scope="module")
def emu():
    return qc.emu_quantiles()


def _check(emu, v, what):
    got, cnt = qc.emu_quantiles_run(emu, v, qc.PROBS)
    s = qc.sorted_finite(v)
    ref = np.array([qc.quantile_of_sorted(s, p) for p in qc.PROBS])
    assert cnt == len(s), what
    assert qc.same_bits(got, ref), "%s: got %s, definition %s" % (what, got, ref)
    return got


def _batches(n, rng):
    """random values; heavy ties; signed zeros among small values; infinities, NaN and denormals planted"""
    yield "random", rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    yield "ties", rng.integers(-2, 3, size=n).astype(np.float64)
    z = rng.choice(np.array([0.0, -0.0, DENORMAL, -DENORMAL, 3 * DENORMAL, 1e-310, -1e-310]), size=n)
    yield "zeros and denormals", z
    v = rng.normal(size=n)
    bad = rng.random(n) < 0.3
    v[bad] = rng.choice(np.array([np.inf, -np.inf, np.nan]), size=int(bad.sum()))
    v[rng.random(n) < 0.2] = -0.0
    yield "planted", v


@pytest.mark.parametrize("block", range(0, 130, 10))
def test_network_and_formula_are_the_definition_bit_for_bit(emu, block):
    """every batch size 1 .. 130 (ten per case): below and above a wavefront's 128 keys, every pad to a power of two"""
    for n in range(block + 1, block + 11):
        rng = np.random.default_rng(n)
        for what, v in _batches(n, rng):
            _check(emu, v, "n %d %s" % (n, what))


@pytest.mark.parametrize("n", [1024, 1025])
def test_a_power_of_two_and_its_first_overflow_of_the_pad(emu, n):
    """1024 keys: the steps j >= 128 that meet at a workgroup barrier on the device; 1025 pads to 2048, where a thread takes two pairs per step"""
    rng = np.random.default_rng(n)
    for what, v in _batches(n, rng):
        got = _check(emu, v, "n %d %s" % (n, what))
        s = qc.sorted_finite(v)
        if len(s):
            assert qc.same_bits(got[:2], np.array([s[0], s[-1]]))      # p = 0, 1: the extremes themselves


def test_signed_zeros_extremes_and_an_empty_column(emu):
    got, cnt = qc.emu_quantiles_run(emu, [0.0, -0.0, 0.0, -0.0], (0.0, 1.0, 1.0 / 3.0, 0.5))
    assert cnt == 4 and np.signbit(got[0]) and not np.signbit(got[1]) and np.signbit(got[2]) and (got == 0.0).all()      # -0.0, -0.0 | +0.0, +0.0; h = 1 at p = 1/3
    got, cnt = qc.emu_quantiles_run(emu, [np.nan, np.inf, -np.inf], qc.PROBS)
    assert cnt == 0 and np.isnan(got).all()
    got, cnt = qc.emu_quantiles_run(emu, [np.inf, 2.5, np.nan], qc.PROBS)
    assert cnt == 1 and (got == 2.5).all()
    big = 1.7976931348623157e308
    got, cnt = qc.emu_quantiles_run(emu, [-big, big, np.inf], (0.0, 1.0))
    assert cnt == 2 and got[0] == -big and got[1] == big      # (g = 0: the order statistic itself, whatever s_hi - s_lo would overflow to)
    assert qc.same_bits(qc.emu_quantiles_run(emu, [DENORMAL, 3 * DENORMAL], (0.5,))[0], [2 * DENORMAL])


def test_the_key_map_orders_as_numbers_and_inverts(emu):
    import ctypes as C
    v = np.array([-np.inf, -1.7976931348623157e308, -1.0, -1e-310, -DENORMAL, -0.0, 0.0, DENORMAL, 1e-310, 1.0, 1.7976931348623157e308, np.inf, np.nan, -np.nan])
    key, back = np.zeros(len(v), dtype=np.uint64), np.zeros(len(v))
    emu.emu_quantile_keys.restype = None
    emu.emu_quantile_keys(C.c_longlong(len(v)), v.ctypes.data_as(C.POINTER(C.c_double)), key.ctypes.data_as(C.POINTER(C.c_uint64)), back.ctypes.data_as(C.POINTER(C.c_double)))
    fin = np.isfinite(v)
    assert (np.diff(key[fin].astype(object)) > 0).all() and qc.same_bits(back[fin], v[fin])
    assert (key[~fin] == np.uint64(0xffffffffffffffff)).all() and (key[fin] < np.uint64(0xffffffffffffffff)).all()


def test_python_side_refusals(cclqr):
    """they raise before any device call: no GPU is touched here"""
    mech = cclqr.examples.cartpole_n(1)["mech"]
    nb = len(mech.bodies)
    plain, knots = cclqr.Ensemble(mech), cclqr.Ensemble(mech, cov_knots=(5, 0))
    assert plain.mechanism is mech and plain.cov_knots == () and plain.quantiles == ()
    assert knots.cov_knots == (0, 5) and knots.quantiles == ()
    ens = cclqr.Ensemble(mech, quantiles=(0, 0.05, 0.5, 0.95, 1))
    assert ens.quantiles == (0.0, 0.05, 0.5, 0.95, 1.0) and ens.cov_knots == ()
    for bad in ((1.5,), (-0.1,), (0.5, float("nan"))):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            cclqr.Ensemble(mech, quantiles=bad)
    with pytest.raises(ValueError, match="at most 16"):
        cclqr.Ensemble(mech, quantiles=tuple(np.linspace(0, 1, 17)))
    assert len(cclqr.Ensemble(mech, quantiles=tuple(np.linspace(0, 1, 16))).quantiles) == 16
    with pytest.raises(ValueError, match="16384"):
        cclqr.simulate(mech, 0.1, cclqr.Controller(), ensemble=ens, z0=np.zeros((16385, nb, 13)))
    steps, mx, mu, n = 3, 12 * nb, 1, 9
    rng = np.random.default_rng(0)
    q, fin = rng.normal(size=(steps, 3, mx + mu)), np.full((steps, mx + mu), n, dtype=np.int32)
    z = np.zeros((steps, mx)), np.zeros((steps, mx)), np.zeros((steps, mu)), np.zeros((steps, mu))
    e = cclqr.EnsembleStats(n, *z, probs=(0.0, 0.5, 1.0), quantiles=q, finite_count=fin)
    assert np.array_equal(e.quantile(0.5), q[:, 1, :mx]) and np.array_equal(e.input_quantile(1), q[:, 2, mx:]) and e.quantile(0.5).shape == (steps, mx)
    assert np.array_equal(e.median, q[:, 1, :mx]) and np.array_equal(e.min, q[:, 0, :mx]) and np.array_equal(e.max, q[:, 2, :mx]) and np.array_equal(e.finite_count, fin)
    with pytest.raises(KeyError, match=r"0\.25.*\[0\.0, 0\.5, 1\.0\]"):
        e.quantile(0.25)
    old = cclqr.EnsembleStats(n, *z)      # the six positional arguments, as before
    assert old.finite_count is None and old.probs is None
    with pytest.raises(KeyError, match="not asked for"):
        old.median
    m = e.merge(cclqr.EnsembleStats(n, *z, probs=(0.0, 0.5, 1.0), quantiles=q, finite_count=fin))
    assert m.count == 2 * n and m.finite_count is None
    for f in (lambda: m.quantile(0.5), lambda: m.input_quantile(0.5), lambda: m.max, lambda: e.merge(cclqr.EnsembleStats.empty(steps, mx, mu)).median):
        with pytest.raises(KeyError, match="do not combine"):
            f()


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name) and "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name in jl and name in integ
        i = hdr.index("int %s(" % name)
        assert re.search(r"\.jl:\d+", hdr[max(0, i - 3500):i]), name
    assert re.search(r"Still 202[^\n]*cclqr_rollout_quantiles_ws_bytes, cclqr_rollout_quantiles", hdr[:hdr.index("#define CCLQR_ABI_VERSION")])
    assert "#define CCLQR_QUANTILE_MAX_INST  16384" in hdr and "#define CCLQR_QUANTILE_MAX_PROBS 16" in hdr
    assert capi.QUANTILE_MAX_INST == qc.MAX_INST == 16384 and capi.QUANTILE_MAX_PROBS == qc.MAX_PROBS == 16
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    srcs, hdrs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split(), re.search(r"^HDRS = (.*)$", mk, re.M).group(1).split()
    assert "quantiles.hip" in srcs and "cclqr_quantiles.h" in hdrs
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202 and all(hasattr(L, n) for n in NAMES)


def test_quantile_kernel_resources():
    """csrc/quantiles.hip cross-compiled for gfx950: no kernel touches scratch memory or spills a vector register; all their LDS is dynamic, and the select kernel's
    at the largest batch (16384 keys of 8 bytes) stays within 160 KB, the stage kernel's window within its budget for every mechanism size"""
    from build_common import device_asm
    asm = device_asm("quantiles.hip")
    stage, select = asm.kernel_names("_ZN5cclqr16ens_stage_kernel"), asm.kernel_names("_ZN5cclqr17ens_select_kernel")
    assert len(stage) == 4 and len(select) == 1, asm.kernel_names()
    for name in stage + select:
        k = asm.kernel(name).resources
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, (name, dict(k))
    assert asm.kernel(select[0]).resources["vgpr"] <= 64      # 1024 threads to a workgroup
    emu = qc.emu_quantiles()      # the launch's own arithmetic (launch_quantiles: qnt_pow2, qnt_stage_window, qnt_stage_lds_bytes)
    emu.emu_quantile_select_lds.restype = emu.emu_quantile_stage_lds.restype = ctypes.c_longlong
    assert emu.emu_quantile_select_lds(ctypes.c_longlong(qc.MAX_INST)) == 128 * 1024 <= 160 * 1024
    assert emu.emu_quantile_select_lds(ctypes.c_longlong(8192)) == 64 * 1024 and emu.emu_quantile_select_lds(ctypes.c_longlong(1)) == 8
    for nb in range(1, 65):
        for mu in (0, 1, min(nb, 7), nb):
            W = ctypes.c_int(0)
            lds = emu.emu_quantile_stage_lds(ctypes.c_int(nb), ctypes.c_int(mu), ctypes.byref(W))
            P = 4 * (64 // (8 if nb <= 8 else 16 if nb <= 16 else 32 if nb <= 32 else 64))
            assert lds <= 144 * 1024 and W.value in (4, 8, 16, 32, 64) and W.value >= P and W.value % P == 0, (nb, mu, lds, W.value)
            if nb <= 12 or (nb == 17 and mu <= 7):
                assert W.value == 64, (nb, mu)      # small mechanisms and the headline's 17-body chain collect a whole tile: 512-byte runs
