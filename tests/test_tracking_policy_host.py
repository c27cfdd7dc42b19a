"""The tracking policy value without a GPU: the two entry points are declared, cited, listed and exported, additively at ABI 202 / layout 48; the new source is built;
its kernels are the named set and keep the resource rule of the sibling files; the resident kernel's fit rule and LDS formula are the ones the tests mirror, and
serve the shapes the tracking covariance's resident kernel serves; the workspace plan is pure arithmetic next to the tracking ones; cclqr.TrackingPolicyValue exists
and refuses, before any device is asked, what its docstring lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import tracking_covariance_common as tc
import tracking_policy_common as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_policy_value_tracking", "cclqr_value_create_policy_tracking")
KERNELS = ("ptk_resident_kernel", "ptk_init_kernel", "ptk_abar_kernel", "ptk_price_kernel", "ptk_v_kernel", "ptk_pn_kernel")


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
        for cite in (r"lqr_tracking\.jl:63", r"lqr_tracking\.jl:88", r"lqr_tracking\.jl:107", r"lqr_tracking\.jl:108|107, 108", r"trackingLQR_triple_cartpole\.jl:98", "Still 202"):
            assert re.search(cite, above), (name, cite)
    head = hdr[:hdr.index("#define CCLQR_ABI_VERSION")]
    assert re.search(r"Still 202[^\n]*cclqr_policy_value_tracking, cclqr_value_create_policy_tracking", head)
    assert re.search(r"Still 202[^\n]*cclqr_covariance_tracking, cclqr_value_create_covariance_tracking", head), "the earlier lines stay"
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    assert callable(capi.policy_value_tracking) and callable(capi.value_create_policy_tracking)
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
    assert re.search(r"^SRCS = .*\bpolicy_tracking\.hip\b", mk, re.M) and re.search(r"^SRCS = .*\bcovariance_tracking\.hip\b", mk, re.M)


def test_tracking_policy_kernel_set_and_resources():
    """csrc/policy_tracking.hip holds exactly the named kernels -- one resident, the init and the tiled step's four --, each without scratch memory or vector-register
    spill, within 256 registers per lane and 16 scalar spills"""
    from build_common import device_asm
    asm = device_asm("policy_tracking.hip")
    names = asm.kernel_names("_ZN5cclqr")
    for k in KERNELS:
        assert sum(k in n for n in names) == 1, (k, names)
    assert len(names) == len(KERNELS), names
    for n in names:
        r = asm.kernel(n).resources
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 256 and r["sgpr_spill"] <= 16, (n, dict(r))


def test_the_fit_rule_and_the_lds_formula_are_the_ones_the_tests_mirror():
    """ptk_resident_fits and ptk_resident_lds_bytes, read from the source: the constants and the formula of tests/tracking_policy_common.py; the verdicts of the
    tracking covariance's resident kernel on the shapes its own test lists; the path by shape and opts->path alone"""
    src = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "policy_tracking.hip")).read()
    for name, val in (("PTK_THREADS", tp.THREADS), ("PTK_TILES", tp.TILES), ("PTK_PRE", tp.PRE), ("PTK_PRE_S", tp.PRE_S)):
        assert re.search(r"#define %s %d\b" % (name, val), src), name
    assert "#define PTK_WAVES (PTK_THREADS / 64)" in src and tp.WAVES == tp.THREADS // 64
    assert src.count("size_t ptk_resident_lds_bytes(int mx, int mu) {") == 1
    assert "return (2 * (size_t)mx * mx + 2 * (size_t)mu * mx + 2 * (size_t)mu * mu + PTK_WAVES) * sizeof(double);" in src
    assert src.count("bool ptk_resident_fits(int mx, int mu) {") == 1
    assert ("return res_tiles_serve(mx, PTK_WAVES) && mx * mx <= PTK_PRE * PTK_THREADS && mu * mx <= PTK_PRE_S * PTK_THREADS && "
            "ptk_resident_lds_bytes(mx, mu) <= 158 * 1024;") in src
    assert "int ptk_chosen_path(int mx, int mu, int path) { return (path != 2 && ptk_resident_fits(mx, mu)) ? 1 : 2; }" in src
    assert src.count("ptk_resident_lds_bytes(a.mx, a.mu)") == 1, "the launch takes its LDS size from the one formula"
    for mx, mu, fits in ((12, 1, True), (48, 1, True), (84, 7, True), (96, 7, True), (96, 11, False), (100, 3, False), (30, 2, False), (24, 0, True), (204, 1, False)):
        assert tp.resident_fits(mx, mu) == fits == tc.resident_fits(mx, mu), (mx, mu)
    assert tp.resident_lds_bytes(84, 7) == 123152 and tp.resident_lds_bytes(96, 7) == 159056
    assert 8 * (2 * 96 * 96 + 3 * 7 * 96 + 2 * 49 + 8) == 164432 > 163840, "a third mu mx panel would not fit at (96, 7): the kernel has two"
    assert [tp.paths_of(n) for n in tp.NAMES] == [(1, 2)] * 6 + [(2,)] * 2


def test_the_workspace_plan_is_new_arithmetic_next_to_the_tracking_ones():
    hdr = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "cclqr_internal.h")).read()
    assert "inline long long tracking_pol_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles)" in hdr
    assert "inline long long tracking_pol_fixed_bytes(int mx, int mu, long long ric_fixed, int n_weights, int n_noise)" in hdr
    i, j, k = (hdr.index("inline long long %s(" % f) for f in ("tracking_chunk_count", "tracking_cov_problem_bytes", "tracking_pol_problem_bytes"))
    assert i < j < k, "the plan stands next to the tracking ones"
    # the lines the earlier plans are pinned to are as they were
    assert "inline long long tracking_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) {" in hdr
    assert "return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles) + 4 * ((nk + 1) & ~1LL);" in hdr
    assert "ric_doubles + (long long)N * (2 + mx + mu) + 2) + 4 * ((nk + 1) & ~1LL) + 8;" in hdr
    # the policy's own: the models, the recursion's share, N prices and a total, the Newton statuses, status and knot
    assert "return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles + (long long)N + 1) + 4 * ((nk + 1) & ~1LL) + 8;" in hdr
    capi_src = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "csrc", "capi.hip")).read()
    assert capi_src.count("tracking_pol_problem_bytes(") == 1 and capi_src.count("tracking_cov_problem_bytes(") == 1
    assert capi_src.count("tracking_value_on_plants(") == 3, "the two controller entries share ONE host sequence: defined once, called twice"


def test_python_side_refusals(cclqr):
    """what TrackingPolicyValue refuses before the library is asked (no device here)"""
    TPV = cclqr.TrackingPolicyValue
    assert TPV is cclqr.lqr.TrackingPolicyValue and not issubclass(TPV, cclqr.Controller) and hasattr(TPV, "_value_handle") and hasattr(TPV, "_ctrl_handle")
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
    with pytest.raises(ValueError, match="noise_scale and Wu are both given"):
        TPV(mech, trk, ids, eids, Q, R, noise_scale=1.0, Wu=np.ones((1, 1)))
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        TPV(mech, trk, ids, eids, Q, R, Wu=np.ones((2, 2)))
    for knot in (-1, N, 2.5):
        with pytest.raises(ValueError, match=r"knot must be a knot of the controller's trajectory, 0 \.\. N-1 = 5"):
            TPV(mech, trk, ids, eids, Q, R, knot=knot)
    with pytest.raises(ValueError, match=r"storage must be \[n\]\[N\]\[nb\]\[13\] = \[n\]\[6\]\[2\]\[13\]"):
        TPV(mech, trk, ids, eids, Q, R, storage=np.zeros((3, 5, 2, 13)))
    with pytest.raises(ValueError, match=r"Fτ must be \[N\]\[mu\]"):
        TPV(mech, trk, ids, eids, Q, R, Fτ=np.zeros((2, 4, 1)))
    with pytest.raises(ValueError, match="one pair per model, 2 .got 3 and 3"):
        TPV(mech, trk, ids, eids, [Q] * 3, [R] * 3, storage=np.tile(trk.zd, (2, 1, 1, 1)))
    other = cclqr.TrackingLQR.__new__(cclqr.TrackingLQR)
    other.mechanism, other.N, other.eqcids, other.controlfunction = cclqr.examples.cartpole_n(1)["mech"], N, [int(e) for e in eids], None
    with pytest.raises(ValueError, match="another mechanism"):
        TPV(mech, other, ids, eids, Q, R)
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism, lqr.N = mech, 0
    with pytest.raises(ValueError, match="TrackingPolicyValue evaluates the gain rows of a TrackingLQR or PlantTrackingLQR"):
        TPV(mech, lqr, ids, eids, Q, R)
    with pytest.raises(ValueError, match="TrackingLQR or PlantTrackingLQR"):
        TPV(mech, cclqr.OpenLoop.__new__(cclqr.OpenLoop), ids, eids, Q, R)
    trk.controlfunction = lambda batch, lqr, k: None
    with pytest.raises(ValueError, match="controlfunction"):
        TPV(mech, trk, ids, eids, Q, R)
    with pytest.raises(TypeError, match="not a Controller"):
        cclqr.simulate(mech, 0.1, TPV.__new__(TPV))
    with pytest.raises(TypeError, match="TrackingPolicyValue"):
        cclqr.predicted_cost(mech, trk, trk.zd[:1])
    # TrackingCovariance shares these checks and keeps its own refusal of an empty question
    src = open(os.path.join(ROOT, "constrainedcontrol.jl_amd", "lqr.py")).read()
    assert src.count("one trajectory of the controller's N knots per model") == 1 and src.count("def _tracking_arguments(") == 1 and src.count("_tracking_arguments(self,") == 3
    # the binding refuses arrays of the wrong shape before the library is asked
    with pytest.raises(ValueError, match=r"Wu must be \[mu\]\[mu\]"):
        cclqr._capi.policy_value_tracking(np.zeros((2, 1, 4, 4)), np.zeros((2, 1, 4, 1)), np.zeros((2, 1, 4, 0)), np.zeros((2, 1, 0, 4)), np.zeros((1, 4)), np.eye(4),
                                          np.eye(1), np.eye(2), 4)
    with pytest.raises(ValueError, match=r"A must be \[nprob\]\[nlin\]\[mx\]\[mx\]"):
        cclqr._capi.policy_value_tracking(np.zeros((2, 4, 4)), np.zeros((2, 4, 1)), np.zeros((2, 4, 0)), np.zeros((2, 0, 4)), np.zeros((1, 4)), np.eye(4), np.eye(1),
                                          np.eye(1), 4)
