"""One TrackingLQR per plant on the GPU (cclqr_ctrl_create_tracking_batch_plants, cclqr_ctrl_get_gains, PlantTrackingLQR): the batched time-varying recursion
against the CPU oracle on every plant's own tables and trajectory, against the device's own single-problem route, across chunkings, with device pointers, under
the friction / noise law, and its refusals."""
import ctypes as C
import re

import numpy as np
import pytest

from plant_tracking_common import HANGING, _rel, case, open_loop, oracle_gains, oracle_nominal
from plants_common import random_plants, starts

pytestmark = pytest.mark.gpu
TOL_GAIN, TOL_TRAJ = 1e-7, 1e-9          # the project's tolerances (README, tests/test_gpu_plant_lqr.py)
ALL = ("chain3", "chain4", "tree-slider", "sawyer", "tree-slider-128", "break")
_dev = {}


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a, b))


def build(cclqr, c, zd=None, Fd=None, **kw):
    """the batched constructor on the case's plants (keywords override)"""
    kw.setdefault("plants", c["ph"])
    kw.setdefault("tol", c["tol"])
    return cclqr._capi.BatchTrackingHandle(c["mh"], c["zd"] if zd is None else zd, c["cj"], c["Q"], c["R"], Fd=c["Fd"] if Fd is None else Fd, **kw)


def all_gains(cclqr, c, h, tables=None):
    return [cclqr._capi.ctrl_gains(c["mh"], h, i) for i in (range(h.n_ctrl) if tables is None else tables)]


def dev_case(cclqr, orc, name):
    """the case on the device, once per session: mechanism and plants handles, the batched controller `ctl` with the gains of its checked tables read back, and
    the perturbed starts of the rollouts (each on its own plant's manifold)"""
    if name in _dev:
        return _dev[name]
    capi = cclqr._capi
    c = dict(case(cclqr, orc, name))
    if getattr(c["mech"], "_cclqr_handle", None) is None or not c["mech"]._cclqr_handle.ptr:
        c["mech"]._cclqr_handle = capi.MechHandle(c["t"])
    c["mh"] = c["mech"]._cclqr_handle
    c["ph"] = c["plants"].handle(c["mh"])
    c["ctl"] = build(cclqr, c)
    c["K"] = dict(zip(c["check"], all_gains(cclqr, c, c["ctl"], c["check"])))
    if name == "sawyer":
        c["z0"] = cclqr.joint_position_states(c["mech"], c["th"] + np.random.default_rng(48).uniform(-0.002, 0.002, c["th"].shape), plants=c["plants"])
    else:
        c["z0"] = starts(cclqr, c["mech"], c["th0"], c["n"], seed=5, plants=c["plants"])[0]
    _dev[name] = c
    return c


@pytest.mark.parametrize("name", ALL)
def test_gains_against_the_oracle(cclqr, orc, name):
    """.gains(i) of every (checked) plant within 1e-7 relative of orc.riccati_tracking on that plant's tables and trajectory, kbreak equal -- `break` included: five
    problems of one launch break at five different knots and back-fill on their own; on the hanging mechanisms every plant's gains differ from the nominal plant's
    by more than 1e-2, so an ignored plant table or a shifted knot-to-plant map fails here"""
    c = dev_case(cclqr, orc, name)
    og = oracle_gains(orc, c)
    assert c["ctl"].n_ctrl == c["n"] and c["ctl"].kbreak.shape == (c["n"],)
    print(name, "kbreak", c["ctl"].kbreak[list(c["check"])], "oracle", [og[i][1] for i in c["check"]])
    for i in c["check"]:
        K = c["K"][i]
        print(name, i, "gain err", _rel(K, og[i][0]))
        assert K.shape == (c["N"] - 1, len(c["cj"]), 12 * c["t"].nb) and np.isfinite(K).all()
        assert int(c["ctl"].kbreak[i]) == og[i][1] and _rel(K, og[i][0]) < TOL_GAIN
    if name in HANGING or name == "break":
        Kn, _ = oracle_nominal(orc, c)
        for i in c["check"]:
            assert _rel(c["K"][i], Kn) > 1e-2


def _single_route(cclqr, c, i):
    """the parent's route for plant i: cclqr_linearize_plants on a table that repeats the plant N - 1 times, then cclqr_riccati_tv -> (K [N-1][mu][mx], kbreak)"""
    capi, pb, nk = cclqr._capi, c["plants"], c["N"] - 1
    rep = capi.PlantsHandle(c["mh"], *[np.repeat(a[i:i + 1], nk, axis=0) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)])
    lin = capi.linearize(c["mh"], c["zd"][i][:nk], c["cj"], c["Fd"][i][:nk], plants=rep)
    rep.close()
    return capi.riccati_tv(*lin, c["Q"], c["R"], c["N"], tol=c["tol"])


@pytest.mark.parametrize("name", ALL)
def test_against_the_single_problem_route(cclqr, orc, name):
    """per plant, linearize(plants=) on a repeated-plant table -> riccati_tv -> CtrlHandle(n_ctrl = n): where one Riccati path serves both routes (every case but
    tree-slider-128, whose 128 problems take the resident kernel while one problem of 72 states takes the tiled one) gains, break knots and the N - 1 recorded steps
    of cclqr_rollout_plants from perturbed starts are BITWISE equal, statuses included.  Every case: the trajectories under the batched controller are within 1e-9
    of the oracle's rollout on each plant's tables under the same gains."""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    n, N, nb = c["n"], c["N"], c["t"].nb
    zT_d, tr_d, st_d = capi.rollout(c["mh"], c["ctl"], c["z0"], N - 1, record=True, plants=c["ph"])
    print(name, "status", st_d[list(c["check"])])
    assert (st_d > 0).all()
    if name != "tree-slider-128":
        single = [_single_route(cclqr, c, i) for i in range(n)]
        Ks, kbs = np.stack([s[0] for s in single]), [s[1] for s in single]
        print(name, "single route: max gain difference", max(_rel(c["K"][i], Ks[i]) for i in range(n)), "kbreak", kbs)
        assert kbs == [int(k) for k in c["ctl"].kbreak]
        assert _same([c["K"][i] for i in range(n)], list(Ks))
        host = capi.CtrlHandle(c["mh"], c["cj"], K=Ks, N=N, zd=c["zd"].reshape(n * N, nb, 13), Fd=c["Fd"].reshape(n * N, -1), n_ctrl=n)
        zT_h, tr_h, st_h = capi.rollout(c["mh"], host, c["z0"], N - 1, record=True, plants=c["ph"])
        host.close()
        assert np.array_equal(st_h, st_d) and _same((tr_h, zT_h), (tr_d, zT_d))
    for i in c["check"]:
        oc = orc.ctrl_desc(nb, c["cj"], K=c["K"][i], N=N, zd=c["zd"][i], Fd=c["Fd"][i])
        zo, tro, sto = orc.rollout(c["plants"].tables(i), oc, c["z0"][i:i + 1], N - 1, record=True)
        print(name, i, "trajectory err", np.abs(tro[0] - tr_d[i]).max())
        assert (sto > 0).all() and np.abs(tro[0] - tr_d[i]).max() < TOL_TRAJ and np.abs(zo[0] - zT_d[i]).max() < TOL_TRAJ


@pytest.mark.parametrize("name", ("chain4", "sawyer"))
def test_chunking_changes_nothing(cclqr, orc, name):
    """a workspace budget that holds exactly one problem (the bytes are the ones the refusal of a smaller budget names) runs one problem per chunk: gains and
    kbreak bitwise those of the default call.  The Sawyer's four problems take the tiled path in the default call, so its chunks of one must too."""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    with pytest.raises(capi.CclqrError) as e:
        build(cclqr, c, workspace_bytes=1000)
    assert e.value.code == capi.EINVAL
    m = re.search(r"workspace_bytes = 1000 does not hold one problem.* need (\d+) bytes", str(e.value))
    assert m, str(e.value)
    one = int(m.group(1))
    assert 8 * (c["N"] - 1) * (12 * c["t"].nb) ** 2 < one < (1 << 30)
    with pytest.raises(capi.CclqrError):
        build(cclqr, c, workspace_bytes=one - 1)
    for budget in (one, 2 * one + one // 2):
        h = build(cclqr, c, workspace_bytes=budget)
        assert np.array_equal(h.kbreak, c["ctl"].kbreak)
        assert _same(all_gains(cclqr, c, h, c["check"]), [c["K"][i] for i in c["check"]])
        h.close()


def test_device_pointers(cclqr, orc):
    """zd and Fd as torch device tensors, the trajectories recorded by cclqr_rollout_plants and never copied to the host (on_device = 1): gains bitwise those of
    the host-pointer call on the same numbers; the device's recording is within 1e-9 of the oracle's rollouts the other tests use"""
    import torch
    capi = cclqr._capi
    c = dev_case(cclqr, orc, "chain4")
    n, N, nb, mu = c["n"], c["N"], c["t"].nb, len(c["cj"])
    td = torch.device("cuda", torch.cuda.current_device())
    zd0 = np.zeros((N, nb, 13)); zd0[..., 3] = 1.0
    ol = capi.CtrlHandle(c["mh"], c["cj"], K=None, N=N + 1, zd=zd0, Fd=c["U"])
    dz0, dzT = torch.from_numpy(np.array(c["z_start"])).to(td), torch.empty((n, nb, 13), dtype=torch.float64, device=td)
    dtraj, dst = torch.empty((n, N, nb, 13), dtype=torch.float64, device=td), torch.zeros(n, dtype=torch.int32, device=td)
    dFd = torch.from_numpy(np.array(c["Fd"])).to(td)
    stream = torch.cuda.current_stream().cuda_stream
    capi.rollout_dev(c["mh"], ol, n, N, 1, dz0.data_ptr(), 0, 0, 0, dtraj.data_ptr(), dzT.data_ptr(), dst.data_ptr(), stream, first_instance=0, plants=c["ph"])
    h = build(cclqr, c, zd=dtraj.data_ptr(), Fd=dFd.data_ptr(), n_ctrl=n, N=N, on_device=True, stream=stream)
    traj = dtraj.cpu().numpy()
    assert (dst.cpu().numpy() > 0).all() and np.abs(traj - c["zd"]).max() < TOL_TRAJ
    hh = build(cclqr, c, zd=traj)
    assert np.array_equal(h.kbreak, hh.kbreak) and _same(all_gains(cclqr, c, h), all_gains(cclqr, c, hh))
    assert _same([dtraj.cpu().numpy()], [traj])          # the caller's trajectories are read, not written
    # the rollouts the two controllers drive agree bitwise as well (setpoints and feed-forward rows went to link order on the device in one case, through the host in the other)
    ra, rb = (capi.rollout(c["mh"], x, c["z0"], N - 1, record=True, plants=c["ph"]) for x in (h, hh))
    assert _same(ra[:2], rb[:2]) and np.array_equal(ra[2], rb[2])
    h.close(); hh.close(); ol.close()


@pytest.mark.parametrize("name", ("chain3", "tree-slider"))
def test_permutation_slicing_and_the_mechanisms_own_plant(cclqr, orc, name):
    """table k is designed on the plant with GLOBAL index first_plant + k: plants and trajectories reversed give the tables reversed, first_plant = 2 with three
    tables gives tables 2 .. 4 (tree-slider: 1 .. 3), and so does a handle created with that first_index -- all bitwise.  plants = NULL on n copies of the nominal
    trajectory: n bitwise equal tables, within 1e-7 of cclqr_riccati_tracking on that trajectory."""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    pb, n, N = c["plants"], c["n"], c["N"]
    full = [c["K"][i] for i in range(n)]
    rv = capi.PlantsHandle(c["mh"], pb.mass[::-1], pb.inertia[::-1], pb.p1[::-1], pb.p2[::-1])
    h = build(cclqr, c, zd=c["zd"][::-1], Fd=c["Fd"][::-1], plants=rv)
    assert _same(all_gains(cclqr, c, h), full[::-1]) and np.array_equal(h.kbreak, c["ctl"].kbreak[::-1])
    h.close(); rv.close()
    lo = 2 if n >= 5 else 1
    h = build(cclqr, c, zd=c["zd"][lo:lo + 3], Fd=c["Fd"][lo:lo + 3], first_plant=lo)
    assert h.n_ctrl == 3 and _same(all_gains(cclqr, c, h), full[lo:lo + 3])
    h.close()
    shard = random_plants(cclqr, c["mech"], 3, seed=3, first_index=lo)
    assert np.array_equal(shard.mass, pb.mass[lo:lo + 3])
    h = build(cclqr, c, zd=c["zd"][lo:lo + 3], Fd=c["Fd"][lo:lo + 3], plants=shard.handle(c["mh"]), first_plant=lo)
    assert _same(all_gains(cclqr, c, h), full[lo:lo + 3])
    h.close()
    zn = open_loop(orc, c["t"], c["cj"], c["U"], c["z_nominal"])
    h = build(cclqr, c, zd=np.tile(zn[None], (n, 1, 1, 1)), plants=None)
    got = all_gains(cclqr, c, h)
    Kt, kbt = capi.riccati_tracking(c["mh"], c["cj"], zn, c["Fd"][0], c["Q"], c["R"], N)
    assert _same(got[1:], [got[0]] * (n - 1)) and (h.kbreak == kbt).all() and _rel(got[0], Kt) < TOL_GAIN
    h.close()


def test_the_law_and_simulate(cclqr, orc):
    """PlantTrackingLQR(..., fric=, noise_scale=, noise_seed=) simulated on its plants: bitwise the rollout under a CtrlHandle that carries the same law and the
    gains of every table read back; an instance simulated alone (first_instance = i) equals its row; the law cannot be changed on top, and a controller designed
    for a slice that does not start at plant 0 is not rolled out"""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, "chain4")
    mech, n, N, nb = c["mech"], c["n"], c["N"], c["t"].nb
    eids = [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
    Qb, Rb = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1] * len(eids)
    fric, scale, seed = np.array([0.0, 0.1, 0.1, 0.1]), 0.5, 1234
    ctl = cclqr.PlantTrackingLQR(mech, c["plants"], c["zd"], c["U"], eids, Qb, Rb, fric=fric, noise_scale=scale, noise_seed=seed)
    assert ctl.N == N and np.array_equal(ctl.Q, c["Q"]) and np.array_equal(ctl.R, c["R"]) and np.array_equal(ctl.kbreak, c["ctl"].kbreak)
    K = np.stack([ctl.gains(i) for i in range(n)])
    assert _same(list(K), [c["K"][i] for i in range(n)])           # the law does not enter the design
    st = cclqr.simulate(mech, cclqr.Storage(N - 1, nb), ctl, z0=c["z0"], plants=c["plants"])
    host = capi.CtrlHandle(c["mh"], c["cj"], K=K, N=N, zd=c["zd"].reshape(n * N, nb, 13), Fd=c["Fd"].reshape(n * N, -1), fric=fric, noise_scale=scale, noise_seed=seed,
                           n_ctrl=n)
    zT_h, tr_h, st_h = capi.rollout(c["mh"], host, c["z0"], N - 1, record=True, plants=c["ph"])
    host.close()
    assert (st_h > 0).all() and np.array_equal(st.status, st_h) and _same((st.z, st.zT), (tr_h, zT_h))
    plain = capi.rollout(c["mh"], c["ctl"], c["z0"], N - 1, record=True, plants=c["ph"])[1]
    assert not np.array_equal(plain, tr_h)                           # friction and noise did act
    i = n - 2
    one = cclqr.simulate(mech, cclqr.Storage(N - 1, nb), ctl, z0=c["z0"][i:i + 1], plants=c["plants"], first_instance=i)
    assert _same((one.z[0], one.zT[0]), (tr_h[i], zT_h[i]))
    for kw in (dict(fric=np.ones(nb)), dict(noise_seed=3), dict(noise_scale=2.0), dict(noise=np.zeros((n, 2)))):
        with pytest.raises(ValueError, match="fixed at construction"):
            cclqr.simulate(mech, cclqr.Storage(2, nb), ctl, z0=c["z0"], plants=c["plants"], **kw)
    ctl.close()
    shard = random_plants(cclqr, mech, 3, seed=3, first_index=2)
    sl = cclqr.PlantTrackingLQR(mech, shard, c["zd"][2:5], c["U"], eids, Qb, Rb)
    assert sl.first_plant == 2 and _same([sl.gains(k) for k in range(3)], [c["K"][k] for k in range(2, 5)])
    with pytest.raises(ValueError, match="starts at plant 0"):
        cclqr.simulate(mech, cclqr.Storage(2, nb), sl, z0=c["z0"][2:5], plants=shard, first_instance=2)
    sl.close()


@pytest.mark.parametrize("name", ("chain3", "tree-slider"))
def test_gains_read_back_what_was_uploaded(cclqr, orc, name):
    """cclqr_ctrl_get_gains on a controller built from host gains (cclqr_ctrl_create, n_ctrl tables): every table comes back bit for bit in the caller's body
    order -- the tree's link order differs from it --; PlantLQR.gains goes through the same call"""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    n, nb, mu = 3, c["t"].nb, len(c["cj"])
    K = np.random.default_rng(9).normal(size=(n, 7, mu, 12 * nb))
    h = capi.CtrlHandle(c["mh"], c["cj"], K=K, N=8, zd=c["zd"][:n, 0], n_ctrl=n)
    assert _same([capi.ctrl_gains(c["mh"], h, i) for i in range(n)], list(K))
    h.close()
    one = capi.CtrlHandle(c["mh"], c["cj"], K=K[1], N=8, zd=c["zd"][0, 0])
    assert _same([capi.ctrl_gains(c["mh"], one, 0)], [K[1]])
    one.close()
    if name == "chain3":
        mech = c["mech"]
        ids, eids = [cclqr.getid(b) for b in mech.bodies], [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
        zs = np.array(c["z_start"])
        pl = cclqr.PlantLQR(mech, c["plants"], ids, eids, [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1], 9.5 * c["t"].dt, zs)
        lin = capi.linearize(c["mh"], zs, c["cj"], plants=c["ph"])
        Kh, _ = capi.riccati(*lin, c["Q"], c["R"], 10)
        for i in range(c["n"]):
            assert pl.gains(i).shape == Kh[i].shape and _rel(pl.gains(i), Kh[i]) < TOL_GAIN
        pl.close()


def test_refusals(cclqr, orc):
    """another mechanism's plants, a plant range outside the table, a closed-loop mechanism, N < 2 and a controlled joint out of range are refused with their
    code and message and hand out no controller; a controller built before still rolls out bitwise as before; cclqr_ctrl_get_gains refuses a table out of
    range and a controller without gains"""
    capi = cclqr._capi
    c, o = dev_case(cclqr, orc, "chain3"), dev_case(cclqr, orc, "chain4")
    N = c["N"]
    before = capi.rollout(c["mh"], c["ctl"], c["z0"], N - 1, record=True, plants=c["ph"])
    L = capi.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def raw(mh, ph, first, n, N_, cj):
        out = C.c_void_p()
        cja = np.ascontiguousarray(cj, dtype=np.int32)
        zd, Fd = np.ascontiguousarray(c["zd"][:n]), np.ascontiguousarray(c["Fd"][:n])
        rc = L.cclqr_ctrl_create_tracking_batch_plants(mh.ptr, None if ph is None else ph.ptr, C.c_int64(first), C.c_int32(n), C.c_int32(N_), zd.ctypes.data_as(dp),
                                                       Fd.ctypes.data_as(dp), C.c_int32(0), C.c_int32(len(cja)), cja.ctypes.data_as(ip), c["Q"].ctypes.data_as(dp),
                                                       c["R"].ctypes.data_as(dp), C.c_double(1e-5), None, C.c_int64(0), None, None, C.byref(out))
        assert not out.value
        return rc, L.cclqr_last_error().decode()

    rc, msg = raw(c["mh"], o["ph"], 0, 3, N, c["cj"])
    assert rc == capi.EINVAL and "the plants were created for another mechanism" in msg
    for first, n in ((3, 3), (5, 1)):
        rc, msg = raw(c["mh"], c["ph"], first, n, N, c["cj"])
        assert rc == capi.EINVAL and "plants %d .. %d of the call are not all among the plants 0 .. 4" % (first, first + n - 1) in msg
    rc, msg = raw(c["mh"], c["ph"], 0, 3, 1, c["cj"])
    assert rc == capi.EINVAL and "bad sizes" in msg
    for cj in ([3], [-1]):
        rc, msg = raw(c["mh"], c["ph"], 0, 3, N, cj)
        assert rc == capi.EINVAL and "controlled joint out of range" in msg
    ex = cclqr.examples.deltabot()
    db = ex["mech"].tables()
    hd = capi.MechHandle(db)
    zdb = np.tile(ex["mech"].state()[None, None], (2, 4, 1, 1))
    for ph in (None, c["ph"]):
        with pytest.raises(capi.CclqrError) as e:
            capi.BatchTrackingHandle(hd, zdb, [0], np.eye(12 * db.nb), np.eye(1), plants=ph)
        assert e.value.code == capi.EUNSUPPORTED and "closed-loop" in str(e.value)
    hd.close()
    after = capi.rollout(c["mh"], c["ctl"], c["z0"], N - 1, record=True, plants=c["ph"])
    assert _same(before[:2], after[:2]) and np.array_equal(before[2], after[2])
    # the inspector
    for table in (-1, c["n"]):
        with pytest.raises(capi.CclqrError) as e:
            capi.ctrl_gains(c["mh"], c["ctl"], table)
        assert e.value.code == capi.EINVAL and "is not among the controller's tables 0 .. 4" in str(e.value)
    zd0 = np.zeros((N, c["t"].nb, 13)); zd0[..., 3] = 1.0
    ol = capi.CtrlHandle(c["mh"], c["cj"], K=None, N=N + 1, zd=zd0, Fd=c["U"])
    with pytest.raises(capi.CclqrError) as e:
        capi.ctrl_gains(c["mh"], ol, 0)
    assert e.value.code == capi.EINVAL and "has no gains" in str(e.value)
    ol.close()
