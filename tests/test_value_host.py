"""cclqr_value_eval without a GPU: the row functions of csrc/cclqr_value.h, run lane by lane (tests/emu/emu_value.cpp), against the definition restated in numpy;
the header, the binding and the Julia shim are additive at ABI 202 / layout 48; the Python layer's refusals."""
import os
import re

import numpy as np
import pytest

from value_common import assert_value, emu_value, emu_value_run, synthetic_case, value_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cclqr_riccati_value", "cclqr_ctrl_create_lqr_batch_value", "cclqr_value_create", "cclqr_value_get", "cclqr_value_destroy", "cclqr_value_eval")


@pytest.mark.parametrize("nb", [1, 2, 3, 4, 17])
@pytest.mark.parametrize("n_ctrl,n_tables", [(1, 1), (16, 1), (16, 16), (1, 16)])
def test_row_functions_against_numpy(nb, n_ctrl, n_tables):
    """every lane-group width (16, 32, 64 lanes; mx = 204 = 3 x 64 + 12 at 17 bodies), a link order that differs from the body order, a non-symmetric P, a shard with
    first_instance > 0: |got - ref| <= RTOL A with A = |dz|' |P| |dz| (mx^2 2^-53 = 5e-12 at mx = 204)"""
    lib = emu_value()
    case = synthetic_case(nb, n_ctrl, n_tables, 13, seed=1000 * nb + 10 * n_ctrl + n_tables)
    perm = np.random.default_rng(nb).permutation(nb)
    V, A = value_of(case["z"], case["zd"], case["P"])
    got = emu_value_run(lib, case, perm)
    assert_value(got, V, A, "nb %d tables %d / %d" % (nb, n_ctrl, n_tables))
    # the same instance alone and in a shard: the same bits
    part = emu_value_run(lib, case, perm, first_instance=3, z=case["z"][3:8])
    assert np.array_equal(part, got[3:8])
    # a NaN in one body's state is a NaN cost, of that instance alone
    z = case["z"].copy()
    z[5, nb - 1, 8] = np.nan
    bad = emu_value_run(lib, case, perm, z=z)
    assert np.isnan(bad[5]) and np.array_equal(np.delete(bad, 5), np.delete(got, 5))
    if n_tables > 1 and nb > 1:
        assert not np.allclose(got, value_of(case["z"], case["zd"], case["P"][:1])[0], rtol=1e-3)


def test_strided_states_equal_the_packed_ones():
    """states read at a stride -- step 2 of a recorded slab [n][4][nb][13] -- give the bits of the packed call"""
    lib = emu_value()
    case = synthetic_case(2, 1, 1, 6, seed=5)
    slab = np.full((6, 4, 2, 13), 3.25)
    slab[:, 2] = case["z"]
    import ctypes as C
    flat = np.ascontiguousarray(slab.reshape(-1)[2 * 26:])
    packed = emu_value_run(lib, case, [1, 0])
    dp = C.POINTER(C.c_double)
    out = np.zeros(6)
    zl = np.ascontiguousarray(case["zd"][:, :, [1, 0]])
    perm = np.array([1, 0], dtype=np.int32)
    assert lib.emu_value(C.c_int(2), C.c_int64(6), C.c_int64(0), perm.ctypes.data_as(C.POINTER(C.c_int32)), flat.ctypes.data_as(dp), C.c_int64(4 * 26),
                         zl.ctypes.data_as(dp), C.c_int(1), C.c_int(1), case["P"].ctypes.data_as(dp), C.c_int64(1), out.ctypes.data_as(dp)) == 0
    assert np.array_equal(out, packed)


def test_abi_is_additive_at_202(cclqr):
    capi = cclqr._capi
    hdr = open(os.path.join(ROOT, "include", "cclqr.h")).read()
    jl = open(os.path.join(ROOT, "julia", "CCLQR.jl")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.fullmatch(r"[a-z_]+", name) and "int %s(" % name in hdr and name in capi.EXPORTS and ":" + name in jl and name in integ
        i = hdr.index("int %s(" % name)
        assert re.search(r"\.jl:\d+", hdr[max(0, i - 2500):i]), name
    assert re.search(r"Still 202[^\n]*cclqr_riccati_value, cclqr_ctrl_create_lqr_batch_value", hdr[:hdr.index("#define CCLQR_ABI_VERSION")])
    assert capi.ABI_VERSION == 202 and "#define CCLQR_ABI_VERSION 202" in hdr and "ABI_VERSION = 202" in jl
    assert "#define CCLQR_ABI_LAYOUT_LEN 48" in hdr and len(capi.mirrored_layout()) == 48
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        assert L.cclqr_version() == 202 and all(hasattr(L, n) for n in NAMES)


def test_python_side_refusals(cclqr):
    """what the Python layer refuses before the library is asked: a controller without keep_value, a P of the wrong shape, models that are not N - 1 per problem"""
    capi = cclqr._capi
    ex = cclqr.examples.cartpole_n(1)

    class Fake:
        tables = ex["mech"].tables()
    with pytest.raises(ValueError, match=r"\[24\]\[24\]"):
        capi.ValueHandle(Fake, np.zeros((3, 12, 12)))
    with pytest.raises(ValueError, match="N - 1 = 4"):
        capi.riccati_value(np.zeros((6, 4, 4)), np.zeros((6, 4, 1)), np.zeros((6, 4, 0)), np.zeros((6, 0, 4)), np.eye(4), np.eye(1), 5, time_varying=True)
    with pytest.raises(TypeError, match="keep_value"):
        cclqr.predicted_cost(ex["mech"], cclqr.OpenLoop.__new__(cclqr.OpenLoop), np.zeros((1, 2, 13)))
    lqr = cclqr.LQR.__new__(cclqr.LQR)
    lqr.mechanism, lqr.P = ex["mech"], None
    with pytest.raises(ValueError, match="without keep_value=True"):
        lqr._value_handle(None)
    lqr.mechanism = cclqr.examples.cartpole_n(1)["mech"]
    with pytest.raises(ValueError, match="another mechanism"):
        cclqr.predicted_cost(ex["mech"], lqr, np.zeros((1, 2, 13)))
