"""One LQR per plant on the GPU (cclqr_linearize_plants, cclqr_ctrl_create_lqr_batch_plants, PlantLQR): the linearisation kernel on a plant record bit for
bit against the same kernel on a mechanism built from that plant, and against the CPU oracle; the batched constructor against the host path on the same
plants; permutation, sharding, the infinite horizon, simulate, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from plant_lqr_common import CASES, _rel, case, oracle_gains, oracle_models
from plants_common import random_plants, starts

pytestmark = pytest.mark.gpu
TOL_LIN, TOL_GAIN, TOL_TRAJ = 1e-10, 1e-7, 1e-9          # the project's tolerances (tests/test_gpu_setup.py)
_dev, _runs = {}, {}


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a, b))


def dev_case(cclqr, name):
    """the case on the device, once per session: the mechanism's handle (the one PlantLQR and simulate use), the plants' handle, the linearisation of every
    plant at its setpoint, and the starts of the rollouts (each on its own plant's manifold)"""
    if name in _dev:
        return _dev[name]
    capi = cclqr._capi
    c = dict(case(cclqr, name))
    if getattr(c["mech"], "_cclqr_handle", None) is None or not c["mech"]._cclqr_handle.ptr:
        c["mech"]._cclqr_handle = capi.MechHandle(c["t"])
    c["mh"] = c["mech"]._cclqr_handle
    c["ph"] = c["plants"].handle(c["mh"])
    c["lin"] = capi.linearize(c["mh"], c["zd"], c["cj"], c["Fd"], plants=c["ph"])
    if name == "sawyer":
        c["z0"] = cclqr.joint_position_states(c["mech"], c["th"] + np.random.default_rng(48).uniform(-0.002, 0.002, c["th"].shape), plants=c["plants"])
    else:
        c["z0"] = starts(cclqr, c["mech"], c["th0"], c["n"], seed=5, plants=c["plants"])[0]
    _dev[name] = c
    return c


def dev_runs(cclqr, name):
    """both ways to one controller per plant and the rollouts they drive, once per session: the host path (linearize(plants=) -> riccati, nprob = n -> CtrlHandle,
    n_ctrl = n) and the batched constructor on the same plants"""
    if name in _runs:
        return _runs[name]
    capi = cclqr._capi
    c = dev_case(cclqr, name)
    n, N = c["n"], c["N"]
    K, kb = capi.riccati(*c["lin"], c["Q"], c["R"], N)
    host = capi.CtrlHandle(c["mh"], c["cj"], K=K, N=N, zd=c["zd"][:, None], Fd=c["Fd"][:, None], n_ctrl=n)
    dev = capi.BatchLqrHandle(c["mh"], c["zd"], c["cj"], c["Q"], c["R"], N, Fd=c["Fd"], plants=c["ph"])
    r = dict(K=K, kb=np.atleast_1d(kb), dev=dev, host_run=capi.rollout(c["mh"], host, c["z0"], N - 1, record=True, plants=c["ph"]),
             dev_run=capi.rollout(c["mh"], dev, c["z0"], N - 1, record=True, plants=c["ph"]))
    host.close()
    _runs[name] = r
    return r


@pytest.mark.parametrize("name", CASES)
def test_linearize_on_plants(cclqr, orc, name):
    """cclqr_linearize_plants: row i is BITWISE what cclqr_linearize gives on a mechanism handle built from plant i's own tables at zd[i], and within 1e-10 of the
    oracle on those tables; plants = NULL and a table that repeats the mechanism's own numbers are both bitwise the plain call"""
    capi = cclqr._capi
    c = dev_case(cclqr, name)
    per, _ = oracle_models(orc, c)
    t, n = c["t"], c["n"]
    for i in range(n):
        hi = capi.MechHandle(c["plants"].tables(i))
        own = capi.linearize(hi, c["zd"][i:i + 1], c["cj"], c["Fd"][i:i + 1])
        hi.close()
        assert _same([m[i] for m in c["lin"]], [m[0] for m in own]), i
        for got, want in zip(c["lin"], per[i]):
            assert _rel(got[i], want) < TOL_LIN
    zn = np.tile(c["zd_nominal"][None], (n, 1, 1))
    plain = capi.linearize(c["mh"], zn, c["cj"], c["Fd"])
    assert _same(plain, capi.linearize(c["mh"], zn, c["cj"], c["Fd"], plants=None))
    rep = cclqr.PlantBatch(c["mech"], mass=np.tile(t.mass[None], (n, 1)), inertia=np.tile(t.inertia[None], (n, 1, 1)), p1=np.tile(t.p1[None], (n, 1, 1)),
                           p2=np.tile(t.p2[None], (n, 1, 1)))
    rh = capi.PlantsHandle(c["mh"], rep.mass, rep.inertia, rep.p1, rep.p2)
    assert _same(plain, capi.linearize(c["mh"], zn, c["cj"], c["Fd"], plants=rh))
    # the entry point itself with plants = NULL
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cj = np.ascontiguousarray(c["cj"], dtype=np.int32)
    out = [np.zeros_like(m) for m in plain]
    capi.check(capi.lib().cclqr_linearize_plants(c["mh"].ptr, None, C.c_int64(0), C.c_int32(n), zn.ctypes.data_as(dp), C.c_int32(len(cj)), cj.ctypes.data_as(ip),
                                                 c["Fd"].ctypes.data_as(dp), *[o.ctypes.data_as(dp) for o in out]))
    assert _same(plain, out)
    rh.close()


@pytest.mark.parametrize("name", CASES[:3])
def test_permutation_and_sharding(cclqr, name):
    """knot k is linearised on the plant with GLOBAL index first_plant + k: the plants and setpoints reversed give the rows reversed, first_plant = 2 with three
    knots gives rows 2 .. 4 of the full call, and so does a handle created with first_index = 2 that holds only those plants -- all bitwise"""
    capi = cclqr._capi
    c = dev_case(cclqr, name)
    pb, lin = c["plants"], c["lin"]
    rv = capi.PlantsHandle(c["mh"], pb.mass[::-1], pb.inertia[::-1], pb.p1[::-1], pb.p2[::-1])
    assert _same(capi.linearize(c["mh"], c["zd"][::-1], c["cj"], c["Fd"][::-1], plants=rv), [m[::-1] for m in lin])
    rv.close()
    want = [m[2:5] for m in lin]
    assert _same(capi.linearize(c["mh"], c["zd"][2:5], c["cj"], c["Fd"][2:5], plants=c["ph"], first_plant=2), want)
    shard = random_plants(cclqr, c["mech"], 3, seed=3, first_index=2)
    assert np.array_equal(shard.mass, pb.mass[2:5]) and shard.first_index == 2
    assert _same(capi.linearize(c["mh"], c["zd"][2:5], c["cj"], c["Fd"][2:5], plants=shard.handle(c["mh"]), first_plant=2), want)


@pytest.mark.parametrize("name", CASES)
def test_batched_constructor_against_the_host_path(cclqr, orc, name):
    """cclqr_ctrl_create_lqr_batch_plants against linearize(plants=) -> riccati -> CtrlHandle on the same plants: equal break indices, and the two controllers
    drive cclqr_rollout_plants for N - 1 recorded steps to bit-identical trajectories and statuses, all converged.  The host path's gains are within 1e-7 of the
    oracle's dlqr on the oracle's linearisation of each plant, the trajectories within 1e-9 of the oracle's rollout on each plant's tables under those gains;
    and (hanging mechanisms) every plant's gains differ from the nominal plant's by more than 1e-2: a table that was ignored fails here."""
    capi = cclqr._capi
    c, r = dev_case(cclqr, name), dev_runs(cclqr, name)
    n, N, nb = c["n"], c["N"], c["t"].nb
    assert np.array_equal(r["dev"].kbreak, r["kb"]) and r["dev"].n_ctrl == n and r["dev"].plants is c["ph"]
    (zT_h, tr_h, st_h), (zT_d, tr_d, st_d) = r["host_run"], r["dev_run"]
    print(name, "status", st_h, "kbreak", r["kb"])
    assert (st_h > 0).all() and np.array_equal(st_h, st_d)
    assert _same((tr_h, zT_h), (tr_d, zT_d))
    Ko, kbo, (Kn_o, _) = oracle_gains(orc, c)
    for i in range(n):
        print(name, i, "gain err", _rel(r["K"][i], Ko[i]))
        assert int(r["kb"][i]) == kbo[i] and _rel(r["K"][i], Ko[i]) < TOL_GAIN
        oc = orc.ctrl_desc(nb, c["cj"], K=r["K"][i], N=N, zd=c["zd"][i][None], Fd=c["Fd"][i][None])
        zo, tro, sto = orc.rollout(c["plants"].tables(i), oc, c["z0"][i:i + 1], N - 1, record=True)
        print(name, i, "trajectory err", np.abs(tro[0] - tr_d[i]).max())
        assert (sto > 0).all() and np.abs(tro[0] - tr_d[i]).max() < TOL_TRAJ and np.abs(zo[0] - zT_d[i]).max() < TOL_TRAJ
    if name != "sawyer":
        Kn, _ = capi.riccati(*capi.linearize(c["mh"], c["zd_nominal"][None], c["cj"], c["Fd"][:1]), c["Q"], c["R"], N)
        assert _rel(Kn[0], Kn_o) < TOL_GAIN
        for i in range(n):
            assert _rel(r["K"][i], Kn[0]) > 1e-2


def test_infinite_horizon_keeps_one_gain_per_plant(cclqr):
    """infinite_horizon on per-plant tables (LQR{T,Inf}, lqr.jl:25-27, 40-43): one gain per plant, Ku[1] of the finite run at the same N -- the rollout it drives
    equals the one driven by a host-built ungated table of row 0 of the finite gains, and differs from the finite (gated) controller's once k >= N"""
    capi = cclqr._capi
    c, r = dev_case(cclqr, "chain2"), dev_runs(cclqr, "chain2")
    n, N = c["n"], c["N"]
    dev = capi.BatchLqrHandle(c["mh"], c["zd"], c["cj"], c["Q"], c["R"], N, Fd=c["Fd"], infinite_horizon=True, plants=c["ph"])
    assert dev.N == 0 and np.array_equal(dev.kbreak, r["kb"])
    host = capi.CtrlHandle(c["mh"], c["cj"], K=np.ascontiguousarray(r["K"][:, :1]), N=0, zd=c["zd"][:, None], Fd=c["Fd"][:, None], n_ctrl=n)
    steps = N + 10
    zT_h, tr_h, st_h = capi.rollout(c["mh"], host, c["z0"], steps, record=True, plants=c["ph"])
    zT_d, tr_d, st_d = capi.rollout(c["mh"], dev, c["z0"], steps, record=True, plants=c["ph"])
    assert (st_h > 0).all() and np.array_equal(st_h, st_d) and _same((tr_h, zT_h), (tr_d, zT_d))
    fin = capi.rollout(c["mh"], r["dev"], c["z0"], steps, record=True, plants=c["ph"])[1]
    assert np.array_equal(fin[:, :2], tr_d[:, :2]) and not np.array_equal(fin, tr_d)       # (step 1 applies Ku[1] either way; later steps Ku[k], and none once k >= N)
    host.close(); dev.close()


@pytest.mark.parametrize("name", CASES)
def test_simulate_with_plantlqr(cclqr, name):
    """simulate(mech, Storage, PlantLQR, z0=, plants=): instance i reads table i and runs on plant i -- bitwise the batched constructor's rollout; an instance
    simulated alone (first_instance = i) equals its row; friction and noise are refused"""
    c, r = dev_case(cclqr, name), dev_runs(cclqr, name)
    mech, n, N, nb = c["mech"], c["n"], c["N"], c["t"].nb
    ids, eids = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
    ctl = cclqr.PlantLQR(mech, c["plants"], ids, eids, [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1] * len(eids), (N - 0.5) * c["t"].dt, c["zd"], Fτd=c["Fd"])
    assert ctl.N == N and np.array_equal(ctl.Q, c["Q"]) and np.array_equal(ctl.R, c["R"])
    assert np.array_equal(ctl.kbreak, r["kb"]) and ctl.converged.shape == (n,) and ctl.converged.all()
    zT_d, tr_d, st_d = r["dev_run"]
    st = cclqr.simulate(mech, cclqr.Storage(N - 1, nb), ctl, z0=c["z0"], plants=c["plants"])
    assert _same((st.z, st.zT), (tr_d, zT_d)) and np.array_equal(st.status, st_d)
    i = n - 2
    one = cclqr.simulate(mech, cclqr.Storage(N - 1, nb), ctl, z0=c["z0"][i:i + 1], plants=c["plants"], first_instance=i)
    assert _same((one.z[0], one.zT[0]), (tr_d[i], zT_d[i]))
    with pytest.raises(ValueError, match="neither joint friction nor noise"):
        cclqr.simulate(mech, cclqr.Storage(2, nb), ctl, z0=c["z0"], plants=c["plants"], fric=np.ones(c["t"].ne))
    with pytest.raises(ValueError, match="neither joint friction nor noise"):
        cclqr.simulate(mech, cclqr.Storage(2, nb), ctl, z0=c["z0"], plants=c["plants"], noise_seed=3)
    ctl.close()


def test_refusals(cclqr):
    """another mechanism's plants, a range outside the table and a closed-loop mechanism are refused with the stated code and message before anything is
    launched: the outputs of the preceding successful call are untouched, and no controller is handed out"""
    capi = cclqr._capi
    c, o = dev_case(cclqr, "chain2"), dev_case(cclqr, "chain-slider")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    cj = np.ascontiguousarray(c["cj"], dtype=np.int32)
    L = capi.lib()

    def raw_lin(mh, ph, first, nk, out):
        return L.cclqr_linearize_plants(mh.ptr, ph.ptr, C.c_int64(first), C.c_int32(nk), c["zd"].ctypes.data_as(dp), C.c_int32(1), cj.ctypes.data_as(ip),
                                        c["Fd"].ctypes.data_as(dp), *[a.ctypes.data_as(dp) for a in out])

    out = [np.zeros_like(m) for m in c["lin"]]
    assert raw_lin(c["mh"], c["ph"], 0, c["n"], out) == capi.OK and _same(out, c["lin"])
    keep = [a.copy() for a in out]
    assert raw_lin(c["mh"], o["ph"], 0, 3, out) == capi.EINVAL and "the plants were created for another mechanism" in L.cclqr_last_error().decode()
    for first, nk in ((4, 3), (6, 1)):
        assert raw_lin(c["mh"], c["ph"], first, nk, out) == capi.EINVAL
        msg = L.cclqr_last_error().decode()
        assert "plants %d .. %d" % (first, first + nk - 1) in msg and "plants 0 .. 5" in msg
    assert _same(out, keep)
    shard = random_plants(cclqr, c["mech"], 3, seed=3, first_index=2).handle(c["mh"])
    with pytest.raises(capi.CclqrError) as e:
        capi.linearize(c["mh"], c["zd"][:2], c["cj"], c["Fd"][:2], plants=shard, first_plant=1)
    assert e.value.code == capi.EINVAL and "plants 1 .. 2" in str(e.value) and "plants 2 .. 4" in str(e.value)
    for ph, first, n, code, text in ((o["ph"], 0, 3, capi.EINVAL, "another mechanism"), (c["ph"], 5, 2, capi.EINVAL, "plants 5 .. 6 of the call are not all among the plants 0 .. 5")):
        with pytest.raises(capi.CclqrError) as e:
            capi.BatchLqrHandle(c["mh"], c["zd"][:n], c["cj"], c["Q"], c["R"], c["N"], plants=ph, first_plant=first)
        assert e.value.code == code and text in str(e.value)
    # closed loops have no plants
    ex = cclqr.examples.deltabot()
    db = ex["mech"].tables()
    hd = capi.MechHandle(db)
    zdb = ex["mech"].state()[None]
    with pytest.raises(capi.CclqrError) as e:
        capi.linearize(hd, zdb, [0], plants=c["ph"])
    assert e.value.code == capi.EUNSUPPORTED and "closed-loop" in str(e.value)
    with pytest.raises(capi.CclqrError) as e:
        capi.BatchLqrHandle(hd, zdb, [0], np.eye(12 * db.nb), np.eye(1), 10, plants=c["ph"])
    assert e.value.code == capi.EUNSUPPORTED
    hd.close()
