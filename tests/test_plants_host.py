"""Per-instance plants (PlantBatch, cclqr_plants_create / cclqr_rollout_plants), the parts that need no GPU: the link-order packing, the
placement of every instance on its own plant's constraint manifold, the kernels' record loader on the CPU, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import long_and_short_chain_forest
from plants_common import TREE14, emu_plants, mechanism_of, patched_copy, random_plants, starts


def _desc(orc, t):
    return orc.mech_desc(t)


def test_packing_order_on_a_permuted_forest(cclqr, orc):
    """the 13 + 3-link forest with permuted body numbers: the link-order records PlantBatch states equal a numpy restatement from the perm / jperm
    tables the library's own table builder (cclqr_tables.h build_mech_tables, compiled for the host) produces"""
    t2 = long_and_short_chain_forest(cclqr)[0]
    nb = t2.nb
    rng = np.random.default_rng(3)
    n = 3
    mass = rng.uniform(0.5, 2.0, (n, nb))
    A = rng.normal(size=(n, nb, 3, 3))
    inertia = A @ A.transpose(0, 1, 3, 2) + 0.5 * np.eye(3)
    p1, p2 = rng.normal(size=(n, nb, 3)), rng.normal(size=(n, nb, 3))
    pb = cclqr.PlantBatch(t2, mass=mass, inertia=inertia, p1=p1, p2=p2)
    L = emu_plants()
    perm, jperm, parent = (np.zeros(nb, dtype=np.int32) for _ in range(3))
    ip = C.POINTER(C.c_int32)
    assert L.emu_plants_link_order(C.byref(_desc(orc, t2).desc), perm.ctypes.data_as(ip), jperm.ctypes.data_as(ip), parent.ctypes.data_as(ip)) == 0
    assert sorted(perm) == list(range(nb)) and not np.array_equal(perm, np.arange(nb))      # (the numbering really is permuted)
    lp, lj = cclqr.link_order(t2)
    assert np.array_equal(lp, perm) and np.array_equal(lj, jperm)
    want = np.concatenate([mass[:, perm, None], inertia.reshape(n, nb, 9)[:, perm], p1[:, jperm], p2[:, jperm]], axis=2)
    rec = pb.link_records()
    assert rec.shape == (n, nb, 16) and np.array_equal(rec, want)
    # an array that is not given is the mechanism's own value
    rec2 = cclqr.PlantBatch(t2, mass=mass).link_records()
    assert np.array_equal(rec2[:, :, 0], mass[:, perm]) and np.array_equal(rec2[1, :, 1:10], t2.inertia[perm]) and np.array_equal(rec2[2, :, 13:16], t2.p2[jperm])
    for i in range(n):
        ti = pb.tables(i)
        assert np.array_equal(ti.mass, mass[i]) and np.array_equal(ti.p1, p1[i]) and np.array_equal(ti.parent, t2.parent) and np.array_equal(ti.axis, t2.axis)


@pytest.mark.parametrize("case", [("chain", 1), ("chain", 3), ("chain", 16), ("tree", TREE14)], ids=["2b", "4b", "17b", "tree14"])
def test_placement_on_each_plants_manifold(cclqr, orc, case):
    """joint_position_states(mech, theta, plants=) places instance i with plant i's vertices: the placement on a deep copy of the mechanism with that
    plant's numbers patched in, and on plant i's constraint manifold"""
    mech, th0 = mechanism_of(cclqr, case)
    n = 5
    pb = random_plants(cclqr, mech, n, seed=21)
    z, th = starts(cclqr, mech, th0, n, seed=22, plants=pb)
    z_nom = cclqr.joint_position_states(mech, th)
    assert np.abs(z - z_nom).max() > 1e-3          # (the plants' vertices matter)
    for i in range(n):
        ti = pb.tables(i)
        zi = cclqr.joint_position_states(patched_copy(mech, ti), th[i:i + 1])[0]
        assert np.array_equal(z[i], zi)
        assert np.abs(orc.constraints(ti, z[i])).max() < 1e-12
    # a shard of the batch places the same states
    shard = random_plants(cclqr, mech, 2, seed=21, first_index=2)
    assert np.array_equal(shard.mass, pb.mass[2:4]) and np.array_equal(shard.p2, pb.p2[2:4])
    assert np.array_equal(cclqr.joint_position_states(mech, th[2:4], plants=shard, first_instance=2), z[2:4])
    # scaled(): inertia follows the mass, p1 and p2 share one factor per joint
    t = mech.tables()
    f = pb.mass / t.mass[None]
    assert f.min() >= 0.7 and f.max() <= 1.3 and f.std() > 0.05 and np.allclose(pb.inertia, t.inertia[None] * f[:, :, None], rtol=1e-15)
    nz = np.abs(t.p2).max(axis=1) > 0
    g = np.linalg.norm(pb.p2[:, nz], axis=2) / np.linalg.norm(t.p2[nz], axis=1)[None]
    assert g.min() >= 0.9 - 1e-12 and g.max() <= 1.1 + 1e-12 and g.std() > 0.01


@pytest.mark.parametrize("which", ["chain4", "forest"])
def test_record_loader_equals_a_mechanism_of_the_plant(cclqr, orc, which):
    """cclqr_chain.h link_load_consts_rec on the CPU: the lane constants from the nominal MechDev plus plant i's records equal, bit for bit and in every
    field (dtm, sxb, sxa included), those link_load_consts fills from a MechDev built from plant i's own tables -- on a chain with an
    origin-attached (the cart) and link-attached joints, and on the permuted two-chain forest; lanes without a link included"""
    if which == "chain4":
        t = cclqr.examples.cartpole_n(3)["mech"].tables()
        lanes = 8
    else:
        t = long_and_short_chain_forest(cclqr)[0]
        lanes = 32
    pb = cclqr.PlantBatch.scaled(t, 3, mass=(0.7, 1.3), length=(0.9, 1.1), seed=5)
    L = emu_plants()
    dp = C.POINTER(C.c_double)
    seen_sxa = False
    for i in range(3):
        ti = pb.tables(i)
        a, b = np.full((lanes, 40), -1.0), np.full((lanes, 40), -2.0)
        per = L.emu_plants_link_consts(C.byref(_desc(orc, t).desc), C.byref(_desc(orc, ti).desc), C.c_int(lanes), a.ctypes.data_as(dp), b.ctypes.data_as(dp))
        assert per == 34
        a, b = a.reshape(-1)[:lanes * per].reshape(lanes, per), b.reshape(-1)[:lanes * per].reshape(lanes, per)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        nom = np.full((lanes, 40), -3.0)
        L.emu_plants_link_consts(C.byref(_desc(orc, t).desc), C.byref(_desc(orc, t).desc), C.c_int(lanes), nom.ctypes.data_as(dp), b.ctypes.data_as(dp))
        nom = nom.reshape(-1)[:lanes * per].reshape(lanes, per)
        assert not np.array_equal(a[:t.nb, 0], nom[:t.nb, 0]) and not np.array_equal(a[:t.nb, 31], nom[:t.nb, 31])      # (mass and sxa differ from the nominal plant's)
        seen_sxa = seen_sxa or ((a[:t.nb, 31] == 0).any() and (a[:t.nb, 31] > 0).any())      # origin-attached: 0; link-attached: dt^2 / parent mass
        assert np.array_equal(a[:, 16:29], nom[:, 16:29]) and np.array_equal(a[:, 32:], nom[:, 32:])      # topology, friction, flags: the mechanism's
    assert seen_sxa


def test_refusals(cclqr):
    """mass 0, a NaN, an indefinite inertia, and an index range that does not cover the launch are each refused, naming the first offending
    (plant, body); through the library where its argument checks come before any device work"""
    mech = cclqr.examples.cartpole_n(3)["mech"]
    t = mech.tables()
    good = cclqr.PlantBatch.scaled(mech, 4, mass=(0.8, 1.2), length=(0.95, 1.05), seed=1)
    m = good.mass.copy(); m[2, 1] = 0.0
    with pytest.raises(ValueError, match=r"plant 2, body 1: mass must be positive"):
        cclqr.PlantBatch(mech, mass=m)
    m = good.mass.copy(); m[3, 0] = -1.0; m[1, 2] = -2.0
    with pytest.raises(ValueError, match=r"plant 1, body 2"):
        cclqr.PlantBatch(mech, mass=m)
    p = good.p1.copy(); p[1, 3, 2] = np.nan
    with pytest.raises(ValueError, match=r"plant 1, body 3: a non-finite value in p1"):
        cclqr.PlantBatch(mech, p1=p)
    J = good.inertia.copy().reshape(4, 4, 3, 3); J[0, 2] = np.diag([1.0, -0.1, 1.0])
    with pytest.raises(ValueError, match=r"plant 0, body 2: inertia must be symmetric positive definite"):
        cclqr.PlantBatch(mech, inertia=J)
    J = good.inertia.copy().reshape(4, 4, 3, 3); J[3, 3, 0, 1] += 0.01
    with pytest.raises(ValueError, match=r"plant 3, body 3: inertia"):
        cclqr.PlantBatch(mech, inertia=J)
    with pytest.raises(ValueError):
        cclqr.PlantBatch(mech)                          # nothing given
    with pytest.raises(ValueError):
        cclqr.PlantBatch(mech, mass=good.mass, p1=good.p1[:3])
    with pytest.raises(ValueError, match="closed loops"):
        cclqr.PlantBatch(cclqr.examples.fourbar()["mech"], mass=np.ones((2, len(cclqr.examples.fourbar()["mech"].bodies))))
    # the index range: plants 2 .. 5 do not cover instances 0 .. 3, nor 4 .. 7
    shard = cclqr.PlantBatch(mech, mass=good.mass, first_index=2)
    assert list(shard.rows_for(3, 2)) == [1, 2]
    for first, n in ((0, 4), (4, 4), (1, 1), (6, 1)):
        with pytest.raises(ValueError, match="not all among the plants 2 .. 5"):
            shard.rows_for(first, n)
    th = np.zeros((4, 4))
    with pytest.raises(ValueError, match="not all among"):
        cclqr.joint_position_states(mech, th, plants=shard)
    pid = cclqr.PID(mech, cclqr.getid(mech.eqconstraints[0]), 0.0, P=1.0)
    with pytest.raises(ValueError, match="not all among"):
        cclqr.simulate(mech, 0.1, pid, z0=np.tile(mech.state(), (4, 1, 1)), plants=shard)
    hosted = cclqr.PID(mech, cclqr.getid(mech.eqconstraints[0]), 0.0, P=1.0, controlfunction=lambda batch, c, k: None)
    with pytest.raises(ValueError, match="not supported yet"):
        cclqr.simulate(mech, 0.1, hosted, z0=np.tile(mech.state(), (2, 1, 1)), plants=good)
    # the library's own argument checks that precede any device work
    capi = cclqr._capi
    if os.path.exists(capi.LIB_PATH):
        L = capi.lib()
        out = C.c_void_p()
        assert L.cclqr_plants_create(None, C.c_int64(1), C.c_int64(0), None, None, None, None, C.c_int32(0), None, C.byref(out)) == capi.EINVAL
        assert L.cclqr_plants_destroy(None) == capi.OK
        assert L.cclqr_rollout_plants(None, None, None, C.c_int64(1), C.c_int32(1), C.c_int32(1), None, None, None, C.c_int64(0), None, None, None, None, None) == capi.EINVAL
        assert set(("cclqr_plants_create", "cclqr_plants_destroy", "cclqr_rollout_plants")) <= set(capi.EXPORTS) and capi.ABI_VERSION == 202
