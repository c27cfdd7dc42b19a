"""The doubling evaluation without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; the new source is built; its
kernels keep the resource rules of policy.hip; cclqr.StationaryPolicyValue exists and refuses, before any device is asked, a zd of the wrong shape, weight lists of the
wrong length, a controller of another mechanism, a controller with a table of several rows and a max_levels out of range."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_policy_value_doubling", "cclqr_value_create_policy_doubling")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name + "," in jl and "`%s`" % name in integ, name
        assert re.fullmatch(r"[a-z_]+", name)
        i = hdr.index("int %s(" % name)
        above = hdr[max(0, i - 4000):i]
        assert re.search(r"lqr\.jl:\d+", above) and "Still 202" in above, name
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_policy_value_doubling, cclqr_value_create_policy_doubling", head)
    assert re.search(r"Still 202[^\n]*cclqr_policy_value, cclqr_value_create_policy;", head), "the earlier lines stay"
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.policy_value_doubling) and callable(capi.value_create_policy_doubling)
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
    assert re.search(r"^SRCS = .*\bpolicy_doubling\.hip\b", mk, re.M) and re.search(r"^SRCS = .*\bpolicy\.hip\b", mk, re.M)


def test_doubling_kernel_resources():
    """csrc/policy_doubling.hip obeys what test_policy_value_host.py demands of policy.hip: no scratch memory, no vector-register spill, at most 256 registers per
    lane (two wavefronts per SIMD for the 512-thread resident workgroup), a bounded number of scalar spills; and the kernels that form mx^3 products -- the resident
    kernel and the tiled product kernel -- run them on the fp64 matrix cores"""
    from build_common import device_asm
    asm = device_asm("policy_doubling.hip")
    names = asm.kernel_names("_ZN5cclqr")
    assert sum("dbl_resident_kernel" in n for n in names) == 1 and sum("dbl_product_kernel" in n for n in names) == 1 and sum("dbl_setup_kernel" in n for n in names) == 1, names
    for n in names:
        r = asm.kernel(n).resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))
        if any(x in n for x in ("dbl_resident_kernel", "dbl_product_kernel")):
            # (the whole function, not Kernel.body: both return early for a problem that has nothing to do, and the body ends at the first s_endpgm)
            start = next(i for i, l in enumerate(asm.lines) if l.startswith(n + ":"))
            end = next(i for i in range(start + 1, len(asm.lines)) if asm.lines[i].startswith(".Lfunc_end"))
            assert sum("v_mfma_f64_16x16x4" in l for l in asm.lines[start:end]) >= 8, n


def test_python_side_refusals(cclqr):
    """what StationaryPolicyValue refuses before the library is asked (no device here)"""
    SPV = cclqr.StationaryPolicyValue
    assert SPV is cclqr.lqr.StationaryPolicyValue and not issubclass(SPV, cclqr.Controller) and cclqr.PolicyValue is not SPV
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism, lqr.N = mech, 0
    zd = np.zeros((2, 2, 13))
    zd[:, :, 3] = 1.0
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SPV(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, np.zeros((2, 3, 13)))
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SPV(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd[0])
    with pytest.raises(ValueError, match="one pair per model, 2 .got 3 and 3"):
        SPV(mech, lqr, ids, eids, [ex["Q"]] * 3, [ex["R"]] * 3, 0.4, zd)
    with pytest.raises(ValueError, match="one pair per model, 2 .got 2 and 3"):
        SPV(mech, lqr, ids, eids, [ex["Q"]] * 2, [ex["R"]] * 3, None, zd)
    other = cclqr.LQR.__new__(cclqr.LQR)
    other.mechanism, other.N = cclqr.examples.cartpole_n(1)["mech"], 0
    with pytest.raises(ValueError, match="another mechanism"):
        SPV(mech, other, ids, eids, ex["Q"], ex["R"], 0.4, zd)
    table = cclqr.LQR.__new__(cclqr.LQR)
    table.mechanism, table.N = mech, 40      # a finite horizon of 40 steps: 39 gain rows
    with pytest.raises(ValueError, match="39 gain rows"):
        SPV(mech, table, ids, eids, ex["Q"], ex["R"], 0.4, zd)
    with pytest.raises(ValueError, match="LQR, PlantLQR or LQRSweep"):
        SPV(mech, cclqr.OpenLoop.__new__(cclqr.OpenLoop), ids, eids, ex["Q"], ex["R"], 0.4, zd)
    for bad in (0, 61, -1):
        with pytest.raises(ValueError, match="max_levels = %d" % bad):
            SPV(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd, max_levels=bad)
    with pytest.raises(ValueError, match="tol"):
        SPV(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd, tol=-1.0)
    # the binding refuses a gain that is not [..][mu][mx] before the library is asked
    with pytest.raises(ValueError, match=r"\[mu\]\[mx\]"):
        cclqr._capi.policy_value_doubling(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.zeros((3, 2, 4)), np.eye(4), np.eye(1), 4)
