"""One LQR per weight candidate (cclqr_riccati_weights, cclqr_ctrl_create_lqr_batch_weights, LQRSweep), the parts that need no GPU: the surface, the host rule
that picks the kernels of a batch of weights (tests/emu/emu_weights_host.cpp), and LQRSweep's argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dlqr_reference as ref
from build_common import host_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cclqr_riccati_weights", "cclqr_ctrl_create_lqr_batch_weights")


def emu_weights_host():
    """compiled for the host the way capi_host_common.emu_capi_host compiles its source"""
    lib = host_library("libemu_weights_host.so", ["emu/emu_weights_host.cpp"])
    lib.emu_ric_p_rows_batch.restype = C.c_int
    lib.emu_ric_p_rows_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong]
    lib.emu_ric_per_problem_weights.restype = None
    lib.emu_ric_per_problem_weights.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    return lib


def test_surface(cclqr):
    """include/cclqr.h declares both entry points under a comment that cites the reference lines they stand for, the binding lists them, the Julia shim has their
    ccall stubs, INTEGRATION.md names them, the ABI stays 202 (additive: looked up by name), and the package exports LQRSweep"""
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        i = hdr.index("int " + name + "(")
        head = hdr[max(0, i - 2500):i]
        assert re.search(r"lqr\.jl:\d+", head[head.rindex("/*"):]), name
        assert name in capi.EXPORTS and ":" + name in jl and name in integ
    assert re.search(r"Still 202[^\n]*cclqr_riccati_weights and cclqr_ctrl_create_lqr_batch_weights", hdr[:hdr.index("#define CCLQR_ABI_VERSION")])
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert issubclass(cclqr.LQRSweep, cclqr.Controller) and callable(capi.riccati_weights)
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202
        # the argument checks that precede any device work: null arguments, then a count that is neither 1 nor the problem count (both numbers named)
        assert L.cclqr_riccati_weights(1, 4, 0, 0, None, None, None, None, 1, None, None, 2, C.c_double(0.0), None, None, None) == capi.EINVAL
        x = np.zeros(3 * 16)
        p = x.ctypes.data_as(C.POINTER(C.c_double))
        assert L.cclqr_riccati_weights(3, 4, 0, 0, p, None, None, None, 2, p, None, 2, C.c_double(0.0), p, None, None) == capi.EINVAL
        msg = L.cclqr_last_error().decode()
        assert "n_weights = 2" in msg and "(3)" in msg, msg
        assert L.cclqr_ctrl_create_lqr_batch_weights(None, None, 0, 1, None, 1, None, None, 1, None, None, 2, 0, C.c_double(0.0), None, None) == capi.EINVAL


def test_batch_symmetry_rule():
    """ric_p_rows_batch: 0 only if EVERY problem's Q and R are exactly symmetric -- one asymmetric R in the LAST problem sends the batch to the kernels that do not
    assume a symmetric Pk, mu = 0 never looks at R; ric_per_problem_weights leaves a shared pair alone (stride 0) and gives a batch the strides mx^2 / mu^2"""
    L = emu_weights_host()
    rng = np.random.default_rng(7)
    mx, mu, n = 12, 3, 4
    Q = np.stack([ref._spd(rng, mx) for _ in range(n)])
    R = np.stack([ref._spd(rng, mu) for _ in range(n)])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.emu_ric_p_rows_batch(vp(Q), mx, vp(R), mu, n) == 0
    Rn = R.copy()
    Rn[n - 1, 0, 1] = np.nextafter(Rn[n - 1, 0, 1], 1e9)        # one unit in the last place, last problem
    assert L.emu_ric_p_rows_batch(vp(Q), mx, vp(Rn), mu, n) == 1
    assert L.emu_ric_p_rows_batch(vp(Q), mx, vp(Rn), mu, n - 1) == 0
    Qn = Q.copy()
    Qn[1, 2, 5] += 1e-9
    assert L.emu_ric_p_rows_batch(vp(Qn), mx, vp(R), mu, n) == 1 and L.emu_ric_p_rows_batch(vp(Qn), mx, vp(R), mu, 1) == 0
    # mu == 0: R is not looked at (a null pointer, or garbage)
    assert L.emu_ric_p_rows_batch(vp(Q), mx, None, 0, n) == 0 and L.emu_ric_p_rows_batch(vp(Qn), mx, None, 0, n) == 1
    out = (C.c_longlong * 3)()
    for p0 in (0, 1):
        L.emu_ric_per_problem_weights(n, mx, mu, p0, vp(Q), vp(R), 1, out)
        assert list(out) == [0, 0, p0]
    L.emu_ric_per_problem_weights(n, mx, mu, 0, vp(Q), vp(R), n, out)
    assert list(out) == [mx * mx, mu * mu, 0]
    L.emu_ric_per_problem_weights(n, mx, mu, 0, vp(Q), vp(Rn), n, out)
    assert list(out) == [mx * mx, mu * mu, 1]


def test_lqrsweep_validates_before_any_device_call(cclqr, monkeypatch):
    """mismatched candidate counts, bodyids that are no permutation, bad zd / Fτd shapes, blocks of the wrong size, another mechanism's plants, a plant range
    outside the table and a controlfunction are refused on the host -- before the library is touched; friction and noise are refused at rollout"""
    def no_library(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(cclqr._capi, "lib", no_library)
    monkeypatch.setattr(cclqr._capi, "MechHandle", no_library)
    ex = cclqr.examples.cartpole_n(1)
    mech = ex["mech"]
    nb = len(mech.bodies)
    ids, eids = [cclqr.getid(b) for b in ex["bodies"]], [cclqr.getid(ex["ctrl"][0])]
    zd = cclqr.examples.cartpole_states(1, [0.0], [[0.0]])[0]
    Qs = [[np.eye(12) * w] * nb for w in (1.0, 10.0, 100.0)]
    Rs = [[np.eye(1) * w] for w in (1.0, 0.1, 0.01)]
    S = cclqr.LQRSweep
    with pytest.raises(ValueError, match=r"got 3 and 2"):
        S(mech, ids, eids, Qs, Rs[:2], 1.0, zd)
    with pytest.raises(ValueError, match=r"got 0 and 3"):
        S(mech, ids, eids, [], Rs, 1.0, zd)
    with pytest.raises(ValueError, match="bodyids must name every body exactly once"):
        S(mech, [ids[0], ids[0]], eids, Qs, Rs, 1.0, zd)
    with pytest.raises(AssertionError, match="Missmatched length for bodies"):
        S(mech, ids, eids, [Qs[0][:1]] + Qs[1:], Rs, 1.0, zd)
    with pytest.raises(AssertionError, match="Missmatched length for constraints"):
        S(mech, ids, eids, Qs, [Rs[0] * 2] + Rs[1:], 1.0, zd)
    with pytest.raises(ValueError, match=r"zd must be \[nb\]\[13\]"):
        S(mech, ids, eids, Qs, Rs, 1.0, np.tile(zd[None], (2, 1, 1)))
    with pytest.raises(ValueError, match=r"zd must be \[nb\]\[13\]"):
        S(mech, ids, eids, Qs, Rs, 1.0, zd[:, :12])
    with pytest.raises(ValueError, match=r"Fτd must be \[mu\]"):
        S(mech, ids, eids, Qs, Rs, 1.0, zd, Fτd=np.zeros((2, 1)))
    with pytest.raises(ValueError, match="every Q block must be 12 x 12"):
        S(mech, ids, eids, [[np.eye(12), np.eye(6)]] * 3, Rs, 1.0, zd)
    with pytest.raises(ValueError, match="controlfunction"):
        S(mech, ids, eids, Qs, Rs, 1.0, zd, controlfunction=lambda batch, ctl, k: None)
    other = cclqr.examples.cartpole_n(1)["mech"]
    ones = lambda m: cclqr.PlantBatch(m, mass=np.tile(m.tables().mass[None], (3, 1)))
    with pytest.raises(ValueError, match="another mechanism"):
        S(mech, ids, eids, Qs, Rs, 1.0, zd, plants=ones(other))
    with pytest.raises(ValueError, match="not all among the plants 0 .. 2"):
        S(mech, ids, eids, Qs, Rs, 1.0, zd, plants=ones(mech), first_plant=1)
    with pytest.raises(TypeError):
        S(object(), ids, eids, Qs, Rs, 1.0, zd)
    # valid arguments reach the device handle -- and nothing before it did
    with pytest.raises(AssertionError, match="the library was called"):
        S(mech, ids, eids, Qs, Rs[:1], math.inf, zd)
    blank = S.__new__(S)
    for kw in (dict(fric=np.ones(2)), dict(noise_scale=1.0), dict(noise_seed=7)):
        with pytest.raises(ValueError, match="neither joint friction nor noise"):
            blank._ctrl_handle(None, **kw)
    blank.first_plant = 2
    with pytest.raises(ValueError, match="starts at plant 0"):
        blank._ctrl_handle(None)
