"""The covariance by doubling without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; the new source is built;
its kernels keep the resource rules of policy_doubling.hip, whose own three kernels are still one each; cclqr.StationaryCovariance exists and refuses, before any
device is asked, what StationaryPolicyValue refuses and besides: no source of covariance, noise_scale together with Wu, Sigma0 with horizon=None."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_covariance_doubling", "cclqr_value_create_covariance_doubling")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name + "," in jl and "`%s`" % name in integ, name
        assert re.fullmatch(r"[a-z_]+", name)
        i = hdr.index("int %s(" % name)
        above = hdr[max(0, i - 5000):i]
        assert re.search(r"lqr\.jl:40-43", above) and re.search(r"lqr\.jl:169-170", above) and "trackingLQR_triple_cartpole.jl:98" in above and "Still 202" in above, name
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_covariance_doubling, cclqr_value_create_covariance_doubling", head)
    assert re.search(r"Still 202[^\n]*cclqr_policy_value_doubling, cclqr_value_create_policy_doubling", head), "the earlier lines stay"
    assert re.search(r"Still 202[^\n]*cclqr_riccati_doubling, cclqr_ctrl_create_lqr_batch_doubling", head), "the earlier lines stay"
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.covariance_doubling) and callable(capi.value_create_covariance_doubling)
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
    assert re.search(r"^SRCS = .*\bcovariance_doubling\.hip\b", mk, re.M) and re.search(r"^SRCS = .*\bpolicy_doubling\.hip\b", mk, re.M)


def test_covariance_kernel_resources():
    """csrc/covariance_doubling.hip obeys what test_policy_doubling_host.py demands of policy_doubling.hip: no scratch memory, no vector-register spill, at most 256
    registers per lane, a bounded number of scalar spills (its kernels are vector code: the mx^3 products stay in policy_doubling.hip); and that file still holds
    one setup, one resident and one product kernel -- the covariance added none to it"""
    from build_common import device_asm
    asm = device_asm("covariance_doubling.hip")
    names = asm.kernel_names("_ZN5cclqr")
    assert sum("cov_setup_kernel" in n for n in names) == 1 and sum("cov_moments_kernel" in n for n in names) == 1 and len(names) == 2, names
    for n in names:
        r = asm.kernel(n).resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))
    old = device_asm("policy_doubling.hip").kernel_names("_ZN5cclqr")
    assert sum("dbl_resident_kernel" in n for n in old) == 1 and sum("dbl_product_kernel" in n for n in old) == 1 and sum("dbl_setup_kernel" in n for n in old) == 1, old
    assert not any("cov_" in n for n in old)


def test_python_side_refusals(cclqr):
    """what StationaryCovariance refuses before the library is asked (no device here)"""
    SC = cclqr.StationaryCovariance
    assert SC is cclqr.lqr.StationaryCovariance and not issubclass(SC, cclqr.Controller) and not hasattr(SC, "_value_handle")
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism, lqr.N = mech, 0
    zd = np.zeros((2, 2, 13))
    zd[:, :, 3] = 1.0
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, np.zeros((2, 3, 13)), noise_scale=1.0)
    with pytest.raises(ValueError, match=r"\[n\]\[2\]\[13\]"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd[0], noise_scale=1.0)
    with pytest.raises(ValueError, match="one pair per model, 2 .got 3 and 3"):
        SC(mech, lqr, ids, eids, [ex["Q"]] * 3, [ex["R"]] * 3, 0.4, zd, noise_scale=1.0)
    with pytest.raises(ValueError, match="one pair per model, 2 .got 2 and 3"):
        SC(mech, lqr, ids, eids, [ex["Q"]] * 2, [ex["R"]] * 3, None, zd, noise_scale=1.0)
    other = cclqr.LQR.__new__(cclqr.LQR)
    other.mechanism, other.N = cclqr.examples.cartpole_n(1)["mech"], 0
    with pytest.raises(ValueError, match="another mechanism"):
        SC(mech, other, ids, eids, ex["Q"], ex["R"], 0.4, zd, noise_scale=1.0)
    table = cclqr.LQR.__new__(cclqr.LQR)
    table.mechanism, table.N = mech, 40      # a finite horizon of 40 steps: 39 gain rows
    with pytest.raises(ValueError, match="39 gain rows"):
        SC(mech, table, ids, eids, ex["Q"], ex["R"], 0.4, zd, noise_scale=1.0)
    with pytest.raises(ValueError, match="LQR, PlantLQR or LQRSweep"):
        SC(mech, cclqr.OpenLoop.__new__(cclqr.OpenLoop), ids, eids, ex["Q"], ex["R"], 0.4, zd, noise_scale=1.0)
    for bad in (0, 61, -1):
        with pytest.raises(ValueError, match="max_levels = %d" % bad):
            SC(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd, noise_scale=1.0, max_levels=bad)
    with pytest.raises(ValueError, match="tol"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd, noise_scale=1.0, tol=-1.0)
    with pytest.raises(ValueError, match="none of noise_scale, Wu and Sigma0"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, zd)
    with pytest.raises(ValueError, match="noise_scale and Wu are both given"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, zd, noise_scale=1.0, Wu=np.ones((1, 1)))
    with pytest.raises(ValueError, match="Sigma0 with horizon=None"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], None, zd, noise_scale=1.0, Sigma0=np.eye(24))
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, zd, Wu=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"Sigma0 must be \[12 nb\]\[12 nb\]"):
        SC(mech, lqr, ids, eids, ex["Q"], ex["R"], 0.4, zd, Sigma0=np.eye(12))
    with pytest.raises(TypeError, match="not a Controller"):
        cclqr.simulate(mech, 0.1, SC.__new__(SC))
    with pytest.raises(TypeError, match="keep_value"):
        cclqr.predicted_cost(mech, SC.__new__(SC), zd)
    # the binding refuses noise of the wrong shape before the library is asked
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        cclqr._capi.covariance_doubling(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.zeros((1, 4)), np.eye(4), np.eye(1),
                                        np.eye(2), None, 4)
