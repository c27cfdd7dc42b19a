"""The Riccati doubling without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; the new source is built; its
kernels keep the resource rules of policy_doubling.hip; the bit schedule and the workspace size of cclqr_internal.h, compiled for the host, are those of
square-and-multiply; cclqr.StationaryLQR exists and refuses, before any device is asked, a zd of the wrong shape, weight lists of the wrong length, non-symmetric
weights, a max_levels or tol out of range, a closed-loop mechanism, a controlfunction, and friction or noise on top."""
import ctypes
import os
import re

import numpy as np
import pytest

from build_common import host_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_riccati_doubling", "cclqr_ctrl_create_lqr_batch_doubling")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name + "," in jl and "`%s`" % name in integ, name
        i = hdr.index("int %s(" % name)
        above = hdr[max(0, i - 5000):i]
        assert re.search(r"lqr\.jl:25-27, 39-43", above) and re.search(r"lqr\.jl:141-184", above) and "Still 202" in above, name
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_riccati_doubling, cclqr_ctrl_create_lqr_batch_doubling", head)
    assert re.search(r"Still 202[^\n]*cclqr_policy_value_doubling, cclqr_value_create_policy_doubling", head), "the earlier lines stay"
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.riccati_doubling) and callable(capi.ctrl_create_lqr_batch_doubling)
    declared = set(re.findall(r"^(?:int|const char \*)\s*(cclqr_\w+)\(", hdr, re.M))
    assert set(NAMES) <= declared and set(NAMES) <= set(capi.EXPORTS)


def test_library_exports_the_entry_points(cclqr):
    import __graft_entry__ as graft
    if not os.path.exists(cclqr._capi.LIB_PATH):
        graft.build()
    lib = ctypes.CDLL(cclqr._capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in NAMES)
    assert cclqr._capi.lib().cclqr_version() == 202


def test_the_new_source_is_built():
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\briccati_doubling\.hip\b", mk, re.M) and re.search(r"^SRCS = .*\bpolicy_doubling\.hip\b", mk, re.M)


def test_doubling_kernel_resources():
    """csrc/riccati_doubling.hip: no scratch memory, no vector-register spill, at most 256 registers per lane (two wavefronts per SIMD for the 512-thread LU and
    substitution workgroups), a bounded number of scalar spills; and the product kernel runs on the fp64 matrix cores"""
    from build_common import device_asm
    asm = device_asm("riccati_doubling.hip")
    names = asm.kernel_names("_ZN5cclqr")
    for k in ("rdb_setup_kernel", "rdb_product_kernel", "rdb_level_kernel", "rdb_gain_kernel", "rdb_fixed_out_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    for k in ("rdb_lu_kernel", "rdb_solve_kernel"):
        assert sum(k in n for n in names) == 2, (k, names)      # M in LDS, M in global memory
    for n in names:
        r = asm.kernel(n).resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))
        if "rdb_product_kernel" in n:
            start = next(i for i, l in enumerate(asm.lines) if l.startswith(n + ":"))
            end = next(i for i in range(start + 1, len(asm.lines)) if asm.lines[i].startswith(".Lfunc_end"))
            assert sum("v_mfma_f64_16x16x4" in l for l in asm.lines[start:end]) >= 8, n


@pytest.fixture(scope="module")
def emu_rdb():
    lib = host_library("libemu_riccati_doubling.so", ["emu/emu_riccati_doubling.cpp"])
    lib.emu_rdb_work_doubles.restype = ctypes.c_longlong
    lib.emu_rdb_work_doubles.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return lib


def test_the_bit_schedule_of_the_header(emu_rdb):
    import riccati_doubling_common as rdc
    cap = emu_rdb.emu_rdb_max_ops()
    for n in (1, 2, 7, 8, 9, 37, 1000, 2 ** 31 - 1):
        ops = (ctypes.c_ubyte * cap)()
        count = emu_rdb.emu_rdb_fixed_schedule(ctypes.c_uint(n), ops)
        got = ["CAD"[ops[i]] for i in range(count)]
        assert count <= cap and got == rdc.schedule(n), (n, got)
        assert got.count("A") + got.count("D") == bin(n).count("1") - 1 + n.bit_length() - 1


def test_the_workspace_size_of_the_header(emu_rdb):
    for nprob, mx in ((1, 1), (3, 12), (2, 97), (1024, 84), (1, 204)):
        tm = (mx + 31) // 32
        want = 11 * nprob * mx * mx + 4 * nprob * tm * tm + (nprob * mx + 1) // 2 + 8
        assert emu_rdb.emu_rdb_work_doubles(nprob, mx) == want


def test_python_side_refusals(cclqr):
    """what StationaryLQR refuses before the library is asked (no device here)"""
    SL = cclqr.StationaryLQR
    assert SL is cclqr.lqr.StationaryLQR and issubclass(SL, cclqr.PlantLQR) and issubclass(SL, cclqr.Controller)
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    zd = np.zeros((2, 2, 13))
    zd[:, :, 3] = 1.0
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SL(mech, ids, eids, ex["Q"], ex["R"], np.zeros((2, 3, 13)))
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SL(mech, ids, eids, ex["Q"], ex["R"], zd[0])
    with pytest.raises(ValueError, match="one pair per table, 2 .got 3 and 3"):
        SL(mech, ids, eids, [ex["Q"]] * 3, [ex["R"]] * 3, zd)
    with pytest.raises(ValueError, match="one pair per table, 2 .got 2 and 3"):
        SL(mech, ids, eids, [ex["Q"]] * 2, [ex["R"]] * 3, zd)
    Qn = [np.array(q, dtype=np.float64) for q in ex["Q"]]
    Qn[1][0, 1] += 1e-9
    with pytest.raises(ValueError, match="not symmetric"):
        SL(mech, ids, eids, Qn, ex["R"], zd)
    for bad in (0, 61, -1):
        with pytest.raises(ValueError, match="max_levels = %d" % bad):
            SL(mech, ids, eids, ex["Q"], ex["R"], zd, max_levels=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            SL(mech, ids, eids, ex["Q"], ex["R"], zd, tol=bad)
    with pytest.raises(ValueError, match="controlfunction"):
        SL(mech, ids, eids, ex["Q"], ex["R"], zd, controlfunction=lambda *a: None)
    with pytest.raises(ValueError, match="Fτd"):
        SL(mech, ids, eids, ex["Q"], ex["R"], zd, Fτd=np.zeros((3, 1)))
    loop = cclqr.examples.fourbar()
    lm = loop["mech"]
    with pytest.raises(ValueError, match="closed loops"):
        SL(lm, [cclqr.getid(b) for b in loop["bodies"]], loop["eqcids"], [np.eye(12)] * 3, [np.eye(1)], np.zeros((1, len(lm.bodies), 13)))
    # friction or noise on top are refused by the handle it would hand simulate, as PlantLQR's
    sl = SL.__new__(SL)
    sl.first_plant = 0
    for law in (dict(fric=np.zeros(2)), dict(noise_scale=0.1), dict(noise_seed=3)):
        with pytest.raises(ValueError, match="neither joint friction nor noise"):
            sl._ctrl_handle(None, **law)
    # the binding refuses outputs of the wrong shape before the library is asked
    with pytest.raises(ValueError, match=r"\[nprob\]\[mu\]\[mx\]"):
        cclqr._capi.riccati_doubling(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.eye(4), np.eye(1), 4, K=np.zeros((2, 2, 4)))
