"""cclqr_value_eval on the device (csrc/value.hip): synthetic cost-to-go tables and setpoints against the numpy restatement of the definition
(tests/value_common.py: |got - ref| <= RTOL A, A = |dz|' |P| |dz|) on every lane-group width and topology, the bit-for-bit invariances the header promises, and
the refusals of the C ABI."""
import numpy as np
import pytest

import value_common as vc
from conftest import long_and_short_chain_forest

pytestmark = pytest.mark.gpu

TREE14_PARENTS = [-1, 0, 1, 2, 3, 2, 5, 6, 1, 8, 8, 10, 0, 12]      # the branching tree of the benchmark


def _tables(cclqr, name):
    ex = cclqr.examples
    if name == "pendulum":
        return ex.pendulum()["mech"].tables()                       # 1 body: 16 lanes
    if name == "cartpole":
        return ex.cartpole_n(1)["mech"].tables()                    # 2 bodies: 32 lanes
    if name == "triple_cartpole":
        return ex.cartpole_n(3)["mech"].tables()                    # 4 bodies: 64 lanes, 48 columns
    if name == "chain17":
        return ex.cartpole_n(16)["mech"].tables()                   # mx 204 = 3 x 64 + 12 columns
    if name == "tree14":
        return ex.tree_mechanism(TREE14_PARENTS, seed=4, prismatic=(0, 5))["mech"].tables()
    if name == "forest":
        return long_and_short_chain_forest(cclqr)[0]                # a 13-link and a 3-link chain interleaved: the link order differs from the body order
    return ex.deltabot()["mech"].tables()                           # closed loops: 7 joints on 5 bodies


_MECH = {}


def _mech(cclqr, name):
    if name not in _MECH:
        _MECH[name] = cclqr._capi.MechHandle(_tables(cclqr, name))
    return _MECH[name]


def gpu_value(cclqr, mech, case, first_instance=0, z=None, z_stride=None, n_inst=None, offset=0):
    """controller (setpoints only) and value object of `case` on the device, one cclqr_value_eval launch; returns V [n].  z: the device array to read (default: the
    case's states, packed), from double `offset` on"""
    import torch
    capi = cclqr._capi
    nb = mech.tables.nb
    n_ctrl = case["zd"].shape[0]
    ctrl = capi.CtrlHandle(mech, [0], zd=case["zd"].reshape(-1, nb, 13), n_ctrl=n_ctrl if n_ctrl > 1 else 0)
    val = capi.ValueHandle(mech, case["P"])
    try:
        zdev = torch.from_numpy(np.ascontiguousarray(case["z"] if z is None else z)).cuda()
        n = case["z"].shape[0] if n_inst is None else n_inst
        out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        capi.value_eval(mech, ctrl, val, n, zdev.data_ptr() + 8 * offset, out.data_ptr(), torch.cuda.current_stream().cuda_stream, first_instance=first_instance,
                        z_stride=z_stride)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        val.close()
        ctrl.close()


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "triple_cartpole", "chain17", "tree14", "forest", "deltabot"])
def test_synthetic_tables_match_the_definition(cclqr, name):
    """one table, one per instance, and one P shared by per-instance setpoints; thirteen instances (a prime count: the last wavefront is not full) of a shard that
    starts at table 2 of 15"""
    mech = _mech(cclqr, name)
    nb = mech.tables.nb
    if name == "forest":
        assert list(cclqr.link_order(mech.tables)[0]) != list(range(nb))
    for seed, (n_ctrl, n_tables) in enumerate(((1, 1), (15, 15), (15, 1))):
        first = 2 if max(n_ctrl, n_tables) > 1 else 0
        case = vc.synthetic_case(nb, n_ctrl, n_tables, 13, seed=100 * nb + seed)
        V, A = vc.value_of(case["z"], case["zd"], case["P"], first_instance=first)
        got = gpu_value(cclqr, mech, case, first_instance=first)
        vc.assert_value(got, V, A, "%s tables %d / %d" % (name, n_ctrl, n_tables))


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "chain17"])
def test_an_instance_has_the_same_bits_wherever_it_runs(cclqr, name):
    """alone, in the batch, and in a shard with first_instance > 0; read at a stride out of a recorded slab; a NaN state is a NaN cost of that instance alone"""
    mech = _mech(cclqr, name)
    nb = mech.tables.nb
    case = vc.synthetic_case(nb, 13, 13, 13, seed=7 + nb)
    whole = gpu_value(cclqr, mech, case)
    for i in (0, 5, 12):
        assert np.array_equal(gpu_value(cclqr, mech, case, first_instance=i, z=case["z"][i:i + 1], n_inst=1), whole[i:i + 1]), i
    assert np.array_equal(gpu_value(cclqr, mech, case, first_instance=4, z=case["z"][4:11], n_inst=7), whole[4:11])
    slab = np.full((13, 5, nb, 13), 3.25)
    slab[:, 3] = case["z"]
    assert np.array_equal(gpu_value(cclqr, mech, case, z=slab, z_stride=5 * 13 * nb, offset=3 * 13 * nb), whole)
    z = case["z"].copy()
    z[6, nb - 1, 4] = np.nan
    bad = gpu_value(cclqr, mech, case, z=z)
    assert np.isnan(bad[6]) and np.array_equal(np.delete(bad, 6), np.delete(whole, 6))


def test_value_object_round_trip(cclqr):
    mech = _mech(cclqr, "cartpole")
    P = np.random.default_rng(1).normal(size=(3, 24, 24))
    val = cclqr._capi.ValueHandle(mech, P)
    try:
        assert all(np.array_equal(val.get(t), P[t]) for t in range(3))
        with pytest.raises(cclqr._capi.CclqrError, match="table 3"):
            val.get(3)
    finally:
        val.close()


def test_refusals_come_before_the_launch(cclqr):
    """every refusal of cclqr_value_eval a caller can reach: CCLQR_EINVAL, the output untouched (a controller without a setpoint table is refused too, but
    cclqr_ctrl_create makes none)"""
    import torch
    capi = cclqr._capi
    mech, other = _mech(cclqr, "cartpole"), capi.MechHandle(_tables(cclqr, "cartpole"))
    pend = _mech(cclqr, "pendulum")
    case = vc.synthetic_case(2, 5, 5, 4, seed=3)
    ctrl5 = capi.CtrlHandle(mech, [0], zd=case["zd"].reshape(-1, 2, 13), n_ctrl=5)
    ctrl1 = capi.CtrlHandle(mech, [0], zd=case["zd"][0])
    ctrl_p = capi.CtrlHandle(pend, [0])
    val5, val1, val3 = capi.ValueHandle(mech, case["P"]), capi.ValueHandle(mech, case["P"][:1]), capi.ValueHandle(mech, case["P"][:3])
    val_o = capi.ValueHandle(other, case["P"])
    z = torch.from_numpy(case["z"]).cuda()
    out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")

    def refused(match, ctrl, val, n=4, first=0, stride=None, m=mech):
        with pytest.raises(capi.CclqrError, match=match) as e:
            capi.value_eval(m, ctrl, val, n, z.data_ptr(), out.data_ptr(), first_instance=first, z_stride=stride)
        assert e.value.code == capi.EINVAL
    try:
        refused("value object was created for another mechanism", ctrl5, val_o)
        refused("controller was created for another mechanism", ctrl_p, val5)
        refused("holds 3 tables", ctrl5, val3)
        refused("holds 5 tables", ctrl1, val5)
        refused("exceeds the 5 tables", ctrl5, val5, first=2)
        refused("exceeds the 5 tables", ctrl5, val1, first=2)
        refused("z_stride = 25", ctrl5, val5, stride=25)
        refused("negative", ctrl5, val5, n=-1)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all()
        capi.value_eval(mech, ctrl5, val1, 4, z.data_ptr(), out.data_ptr(), first_instance=1)      # (and the accepted call right behind them)
        torch.cuda.synchronize()
        assert np.isfinite(out.cpu().numpy()).all()
    finally:
        for h in (ctrl5, ctrl1, ctrl_p, val5, val1, val3, val_o, other):
            h.close()
