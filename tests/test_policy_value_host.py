"""Policy evaluation without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; cclqr.PolicyValue exists and
refuses, before any device is asked, weight lists of the wrong length, a zd of the wrong shape and a controller of another mechanism."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_policy_value", "cclqr_value_create_policy")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name in jl and name in integ, name
        i = hdr.index("int %s(" % name)
        above = hdr[max(0, i - 4000):i]
        assert re.search(r"lqr\.jl:\d+", above) and "Still 202" in above, name
    assert re.search(r"Still 202[^\n]*cclqr_policy_value, cclqr_value_create_policy", hdr[:hdr.index("#define CCLQR_ABI_VERSION")])
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.policy_value) and callable(capi.value_create_policy)


def test_library_exports_the_entry_points(cclqr):
    import __graft_entry__ as graft
    if not os.path.exists(cclqr._capi.LIB_PATH):
        graft.build()
    lib = ctypes.CDLL(cclqr._capi.LIB_PATH)
    assert all(hasattr(lib, n) for n in NAMES)
    assert cclqr._capi.lib().cclqr_version() == 202


def test_the_new_source_is_built(cclqr):
    mk = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpolicy\.hip\b", mk, re.M) and "cclqr_riccati_dev.h" in mk


def test_python_side_refusals(cclqr):
    """what PolicyValue refuses before the library is asked (no device here)"""
    assert cclqr.PolicyValue is cclqr.lqr.PolicyValue and not issubclass(cclqr.PolicyValue, cclqr.Controller)
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism = mech
    zd = np.zeros((2, 2, 13))
    zd[:, :, 3] = 1.0
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        cclqr.PolicyValue(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, np.zeros((2, 3, 13)))
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        cclqr.PolicyValue(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, zd[0])
    with pytest.raises(ValueError, match="one pair per model, 2 .got 3 and 3"):
        cclqr.PolicyValue(mech, lqr, ids, eids, [ex["Q"]] * 3, [ex["R"]] * 3, 0.4, zd)
    with pytest.raises(ValueError, match="one pair per model, 2 .got 2 and 3"):
        cclqr.PolicyValue(mech, lqr, ids, eids, [ex["Q"]] * 2, [ex["R"]] * 3, 0.4, zd)
    other = cclqr.LQR.__new__(cclqr.LQR)
    other.mechanism = cclqr.examples.cartpole_n(1)["mech"]
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.PolicyValue(mech, other, ids, eids, ex["Q"], ex["R"], 0.4, zd)
    with pytest.raises(TypeError, match="LQR, PlantLQR or LQRSweep"):
        cclqr.PolicyValue(mech, cclqr.OpenLoop.__new__(cclqr.OpenLoop), ids, eids, ex["Q"], ex["R"], 0.4, zd)
    # the binding refuses a gain table that is not [..][mu][mx] before the library is asked
    with pytest.raises(ValueError, match=r"\[nK\]\[mu\]\[mx\]"):
        cclqr._capi.policy_value(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.zeros((3, 2, 4)), np.eye(4), np.eye(1), 4)


def test_policy_kernel_resources():
    """csrc/policy.hip obeys what test_host.py demands of riccati.hip's kernels: no scratch memory, no vector-register spill, at most 256 registers per lane (two
    wavefronts per SIMD for the 512-thread resident workgroup); the scalar spills the compiler makes today (6 in the resident kernel, to VGPR lanes) are an upper
    bound with a margin; and the mx^3 products of both launch shapes run on the fp64 matrix cores"""
    from build_common import device_asm
    asm = device_asm("policy.hip")
    names = asm.kernel_names("_ZN5cclqr")
    assert len(names) == 5 and sum("policy_resident_kernel" in n for n in names) == 1, names
    for n in names:
        k = asm.kernel(n)
        r = k.resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))
        if any(x in n for x in ("policy_resident_kernel", "pol_v_kernel", "pol_pn_kernel")):
            # (the whole function, not Kernel.body: the tiled kernels return early for a stopped problem, and the body ends at the first s_endpgm)
            start = next(i for i, l in enumerate(asm.lines) if l.startswith(n + ":"))
            end = next(i for i in range(start + 1, len(asm.lines)) if asm.lines[i].startswith(".Lfunc_end"))
            assert sum("v_mfma_f64_16x16x4" in l for l in asm.lines[start:end]) >= 8, n
