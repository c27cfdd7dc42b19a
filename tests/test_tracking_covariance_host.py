"""The tracking covariance without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; the new source is built; its
kernels keep the resource rule of the sibling files, whose own kernel sets are what they were; the resident kernel's fit rule is the one the tests mirror; the
workspace plan is pure arithmetic next to the tracking one; cclqr.TrackingCovariance exists and refuses, before any device is asked, what its docstring lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import tracking_covariance_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_covariance_tracking", "cclqr_value_create_covariance_tracking")


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name + "," in jl and "`%s`" % name in integ, name
        assert re.fullmatch(r"[a-z_]+", name)
        i = hdr.index("int %s(" % name)
        above = hdr[max(0, i - 6000):i]
        for cite in (r"lqr_tracking\.jl:63", r"lqr_tracking\.jl:88", r"lqr_tracking\.jl:107", r"trackingLQR_triple_cartpole\.jl:98", "Still 202"):
            assert re.search(cite, above), (name, cite)
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_covariance_tracking, cclqr_value_create_covariance_tracking", head)
    assert re.search(r"Still 202[^\n]*cclqr_covariance_doubling, cclqr_value_create_covariance_doubling", head), "the earlier lines stay"
    assert re.search(r"Still 202[^\n]*cclqr_policy_value_doubling, cclqr_value_create_policy_doubling", head), "the earlier lines stay"
    assert re.search(r"Still 202[^\n]*cclqr_riccati_doubling, cclqr_ctrl_create_lqr_batch_doubling", head), "the earlier lines stay"
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.covariance_tracking) and callable(capi.value_create_covariance_tracking)
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
    assert re.search(r"^SRCS = .*\bcovariance_tracking\.hip\b", mk, re.M) and re.search(r"^SRCS = .*\bcovariance_doubling\.hip\b", mk, re.M)


def test_tracking_covariance_kernel_resources():
    """csrc/covariance_tracking.hip obeys the rule of its siblings: no scratch memory, no vector-register spill, at most 256 registers per lane, at most 16 scalar
    spills; it holds one resident kernel and the tiled step's kernels; and policy.hip, policy_doubling.hip and covariance_doubling.hip hold the kernels they held"""
    from build_common import device_asm
    asm = device_asm("covariance_tracking.hip")
    names = asm.kernel_names("_ZN5cclqr")
    for k in ("ctk_init_kernel", "ctk_resident_kernel", "ctk_moments_kernel", "ctk_abar_kernel", "ctk_t_kernel", "ctk_next_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) == 6, names
    for n in names:
        r = asm.kernel(n).resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))
    pol = device_asm("policy.hip").kernel_names("_ZN5cclqr")
    for k in ("policy_resident_kernel", "pol_abar_kernel", "pol_v_kernel", "pol_pn_kernel", "pol_finish_kernel"):
        assert sum(k in n for n in pol) == 1, (k, pol)
    assert len(pol) == 5 and not any("ctk_" in n for n in pol), pol
    dbl = device_asm("policy_doubling.hip").kernel_names("_ZN5cclqr")
    assert sum("dbl_resident_kernel" in n for n in dbl) == 1 and sum("dbl_product_kernel" in n for n in dbl) == 1 and sum("dbl_setup_kernel" in n for n in dbl) == 1, dbl
    assert not any("ctk_" in n for n in dbl)
    cov = device_asm("covariance_doubling.hip").kernel_names("_ZN5cclqr")
    assert sum("cov_setup_kernel" in n for n in cov) == 1 and sum("cov_moments_kernel" in n for n in cov) == 1 and len(cov) == 2, cov


def test_the_fit_rule_is_the_one_the_tests_mirror():
    """ctk_resident_fits, read from the source: the constants and the LDS formula of tests/tracking_covariance_common.py; the shapes policy_resident_kernel serves"""
    src = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "covariance_tracking.hip")).read()
    for name, val in (("CTK_THREADS", tc.THREADS), ("CTK_TILES", tc.TILES), ("CTK_PRE", tc.PRE), ("CTK_PRE_S", tc.PRE_S)):
        assert re.search(r"#define %s %d\b" % (name, val), src), name
    assert "2 * (size_t)mx * mx + 2 * (size_t)mu * mx + 2 * (size_t)mu * mu + CTK_WAVES" in src and "158 * 1024" in src
    assert src.count("bool ctk_resident_fits(") == 1
    for mx, mu, fits in ((12, 1, True), (48, 1, True), (84, 7, True), (96, 7, True), (96, 11, False), (100, 3, False), (30, 2, False), (24, 0, True), (204, 1, False)):
        assert tc.resident_fits(mx, mu) == fits, (mx, mu)
    assert tc.resident_lds_bytes(84, 7) == 123152 and tc.resident_lds_bytes(96, 7) == 159056
    assert [tc.paths_of(n) for n in tc.NAMES] == [(1, 2)] * 6 + [(2,)] * 2


def test_the_shared_blocks_are_defined_once():
    """across csrc/ the five-slot tile struct, the (mid, big) sum of squares and its per-tile total are each defined exactly once, and tile_mfma_splitk is called
    from riccati.hip and from the shared header only: the order of every sum the bitwise tests rest on is written in one place"""
    csrc = os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc")
    code = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            code[f] = "\n".join(l.split("//")[0] for l in open(os.path.join(csrc, f)).read().splitlines())      # without comments
    count = lambda pat: {f: len(re.findall(pat, s)) for f, s in code.items() if re.search(pat, s)}
    assert count(r"void put\(int t, v4d r\)") == {"cclqr_riccati_dev.h": 1}
    assert count(r"struct \w+ \{\s*double mid, big;") == {"cclqr_riccati_dev.h": 1}
    assert count(r"v \* 0x1p-600") == {"cclqr_riccati_dev.h": 1}
    assert count(r"double \w*tile_total\(const double\* part, int ntile\)") == {"cclqr_riccati_dev.h": 1}
    assert set(count(r"\+= part\[2 \* t\]")) == {"cclqr_riccati_dev.h"}
    assert set(count(r"\btile_mfma_splitk\(")) == {"cclqr_riccati_dev.h", "riccati.hip"}


def test_the_workspace_plan_is_new_arithmetic_next_to_the_tracking_one():
    hdr = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "cclqr_internal.h")).read()
    assert "inline long long tracking_cov_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles)" in hdr
    assert "inline long long tracking_cov_fixed_bytes(" in hdr
    i, j = hdr.index("inline long long tracking_chunk_count("), hdr.index("inline long long tracking_cov_problem_bytes(")
    assert i < j, "the plan stands next to the tracking one"
    # the three the tracking constructor's plan is pinned to are as they were
    assert "inline long long tracking_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) {" in hdr
    assert "return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles) + 4 * ((nk + 1) & ~1LL);" in hdr


def test_python_side_refusals(cclqr):
    """what TrackingCovariance refuses before the library is asked (no device here)"""
    TC = cclqr.TrackingCovariance
    assert TC is cclqr.lqr.TrackingCovariance and not issubclass(TC, cclqr.Controller) and not hasattr(TC, "_value_handle")
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(j) for j in ex["ctrl"]]
    N = 6
    trk = cclqr.TrackingLQR.__new__(cclqr.TrackingLQR)
    trk.mechanism, trk.N, trk.eqcids, trk.controlfunction = mech, N, [int(e) for e in eids], None
    trk.zd = np.zeros((N, 2, 13))
    trk.zd[..., 3] = 1.0
    trk.Fd = np.zeros((N, 1))
    Q, R = ex["Q"], ex["R"]
    with pytest.raises(ValueError, match="none of noise_scale, Wu and Sigma0"):
        TC(mech, trk, ids, eids, Q, R)
    with pytest.raises(ValueError, match="noise_scale and Wu are both given"):
        TC(mech, trk, ids, eids, Q, R, noise_scale=1.0, Wu=np.ones((1, 1)))
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        TC(mech, trk, ids, eids, Q, R, Wu=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"Sigma0 must be \[12 nb\]\[12 nb\]"):
        TC(mech, trk, ids, eids, Q, R, Sigma0=np.eye(12))
    with pytest.raises(ValueError, match=r"storage must be \[n\]\[N\]\[nb\]\[13\] = \[n\]\[6\]\[2\]\[13\]"):
        TC(mech, trk, ids, eids, Q, R, noise_scale=1.0, storage=np.zeros((3, 5, 2, 13)))
    with pytest.raises(ValueError, match=r"Fτ must be \[N\]\[mu\]"):
        TC(mech, trk, ids, eids, Q, R, noise_scale=1.0, Fτ=np.zeros((2, 4, 1)))
    with pytest.raises(ValueError, match="one pair per model, 2 .got 3 and 3"):
        TC(mech, trk, ids, eids, [Q] * 3, [R] * 3, noise_scale=1.0, storage=np.tile(trk.zd, (2, 1, 1, 1)))
    other = cclqr.TrackingLQR.__new__(cclqr.TrackingLQR)
    other.mechanism, other.N, other.eqcids, other.controlfunction = cclqr.examples.cartpole_n(1)["mech"], N, [int(e) for e in eids], None
    with pytest.raises(ValueError, match="another mechanism"):
        TC(mech, other, ids, eids, Q, R, noise_scale=1.0)
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism, lqr.N = mech, 0
    with pytest.raises(ValueError, match="TrackingLQR or PlantTrackingLQR"):
        TC(mech, lqr, ids, eids, Q, R, noise_scale=1.0)
    with pytest.raises(ValueError, match="TrackingLQR or PlantTrackingLQR"):
        TC(mech, cclqr.OpenLoop.__new__(cclqr.OpenLoop), ids, eids, Q, R, noise_scale=1.0)
    trk.controlfunction = lambda batch, lqr, k: None
    with pytest.raises(ValueError, match="controlfunction"):
        TC(mech, trk, ids, eids, Q, R, noise_scale=1.0)
    with pytest.raises(TypeError, match="not a Controller"):
        cclqr.simulate(mech, 0.1, TC.__new__(TC))
    with pytest.raises(TypeError, match="keep_value"):
        cclqr.predicted_cost(mech, TC.__new__(TC), trk.zd[:1])
    # the binding refuses arrays of the wrong shape before the library is asked
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        cclqr._capi.covariance_tracking(np.zeros((2, 1, 4, 4)), np.zeros((2, 1, 4, 1)), np.zeros((2, 1, 4, 0)), np.zeros((2, 1, 0, 4)), np.zeros((1, 4)), np.eye(4),
                                        np.eye(1), np.eye(2), None, 4)
    with pytest.raises(ValueError, match=r"A must be \[nprob\]\[nlin\]\[mx\]\[mx\]"):
        cclqr._capi.covariance_tracking(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.zeros((1, 4)), np.eye(4), np.eye(1),
                                        np.eye(1), None, 4)
