"""TrackingCovariance / cclqr_value_create_covariance_tracking on the chain3, tree-slider and sawyer cases of tests/plant_tracking_common.py (5 / 4 / 4 plants, 24 / 16 /
12 knots), one PlantTrackingLQR per case:
  * against the longdouble recursion of tests/tracking_covariance_common.py run on the device's OWN per-knot linearisation (linearize(..., plants=) on a table that
    repeats the plant) and the gains read back with .gains(i), under the same acceptance rule;
  * a plain TrackingLQR on its own trajectory, and as ONE table shared by every plant along the plants' own trajectories (storage=, Fτ=, plants=), against the same;
  * one stationary gain row in one table through the C entry, values against the same;
  * one problem per chunk (the budget the refusal of a smaller one names) gives bitwise the default call's result;
  * device tensors for the trajectories give bitwise the host arrays' result;
  * reversed bodyids permute Q, Sigma0 and state_std;
  * the refusals of the C entry leave the outputs and *out untouched; a closed-loop mechanism is CCLQR_EUNSUPPORTED; simulate and predicted_cost raise TypeError."""
import ctypes as C
import re

import numpy as np
import pytest

import dlqr_reference as ref
import tracking_covariance_common as tc
from plant_tracking_common import case, open_loop

pytestmark = pytest.mark.gpu
NAMES = ("chain3", "tree-slider", "sawyer")
SIGMA = 0.3
_dev = {}


def dev_case(cclqr, orc, name):
    """the case with its PlantTrackingLQR, the noise and the default call's TrackingCovariance, once per session"""
    if name in _dev:
        return _dev[name]
    c = dict(case(cclqr, orc, name))
    mech, nb, mu = c["mech"], c["t"].nb, len(c["cj"])
    c["ids"] = [cclqr.getid(b) for b in mech.bodies]
    c["eids"] = [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
    c["Qb"], c["Rb"] = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1] * mu
    c["ctl"] = cclqr.PlantTrackingLQR(mech, c["plants"], c["zd"], c["U"], c["eids"], c["Qb"], c["Rb"])
    c["S0"] = 1e-4 * ref._spd(np.random.default_rng(11), 12 * nb)
    c["cov"] = cclqr.TrackingCovariance(mech, c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"])
    _dev[name] = c
    return c


def _outputs(cov):
    return [cov.stage_cost, cov.state_std, cov.input_std, cov.expected_score] + [cov.Sigma(i) for i in range(cov.n_models)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_against_extended_precision_on_the_devices_own_linearisation(cclqr, orc, name):
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    cov, n, N, mu = c["cov"], c["n"], c["N"], len(c["cj"])
    assert cov.N == N and cov.n_models == n and cov.state_std.shape == (n, N, 12 * c["t"].nb) and cov.input_std.shape == (n, N, mu)
    assert cov.stage_cost.shape == (n, N, 2) and cov.expected_score.shape == (n, 2)
    assert c["ids"] == sorted(c["ids"])      # the mechanism's own order: state_std needs no permutation here
    mh, pb, nk = cclqr.lqr._device_mech(c["mech"]), c["plants"], N - 1
    Wu = SIGMA ** 2 * np.ones((mu, mu))
    for i in range(n):
        rep = capi.PlantsHandle(mh, *[np.repeat(a[i:i + 1], nk, axis=0) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)])
        A, Bu, Bl, G = capi.linearize(mh, c["zd"][i][:nk], c["cj"], c["Fd"][i][:nk], plants=rep)
        rep.close()
        pr = tc.single_problem(A, Bu, Bl, G, c["ctl"].gains(i), cov.Q[0], cov.R[0], Wu, c["S0"], N)
        tc.check_horizon(pr, ("full", True, True), N, 0, cov.Sigma(i), None, cov.stage_cost[i], cov.state_std[i], cov.input_std[i], cov.expected_score[i],
                         "%s plant %d" % (name, i))
    if name != "sawyer":      # the plants differ: so do their spreads (an ignored plant table or a shifted trajectory-to-plant map fails above, and here)
        assert np.abs(cov.state_std[1] - cov.state_std[0]).max() > 1e-3 * np.abs(cov.state_std[0]).max()
    with pytest.raises(TypeError, match="not a Controller"):
        cclqr.simulate(c["mech"], cclqr.Storage(2, c["t"].nb), cov)
    with pytest.raises(TypeError, match="keep_value"):
        cclqr.predicted_cost(c["mech"], cov, c["z_start"])


@pytest.mark.parametrize("name", ("chain3", "tree-slider"))
def test_a_plain_tracking_lqr_alone_and_as_one_table_shared_by_every_plant(cclqr, orc, name):
    """a TrackingLQR designed on the mechanism's own plant along its own open-loop rollout: (a) its covariance along that trajectory, one model; (b) storage= / Fτ= /
    plants=: the NOMINAL table, one shared by all, along every perturbed plant's own trajectory on that plant -- both against the longdouble recursion on the device's
    own linearisation with the table's rows, so a table read per problem where it is shared, or a row shifted by a knot, fails here"""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, name)
    mech, n, N, nb, mu = c["mech"], c["n"], c["N"], c["t"].nb, len(c["cj"])
    zn = open_loop(orc, c["t"], c["cj"], c["U"], c["z_nominal"])
    trk = cclqr.TrackingLQR(mech, cclqr.Storage(N, nb, 1, z=np.ascontiguousarray(zn[None])), c["U"], c["eids"], c["Qb"], c["Rb"])
    assert trk.K.shape == (N - 1, mu, 12 * nb)
    mh, pb, nk = cclqr.lqr._device_mech(mech), c["plants"], N - 1
    Wu = SIGMA ** 2 * np.ones((mu, mu))
    own = cclqr.TrackingCovariance(mech, trk, c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"])
    shared = cclqr.TrackingCovariance(mech, trk, c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"], storage=c["zd"], Fτ=c["Fd"], plants=c["plants"])
    try:
        assert own.n_models == 1 and own.N == N and shared.n_models == n
        A, Bu, Bl, G = capi.linearize(mh, zn[:nk], c["cj"], c["U"][:nk])
        pr = tc.single_problem(A, Bu, Bl, G, trk.K, own.Q[0], own.R[0], Wu, c["S0"], N)
        tc.check_horizon(pr, ("full", True, True), N, 0, own.Sigma(0), None, own.stage_cost[0], own.state_std[0], own.input_std[0], own.expected_score[0],
                         "%s, the TrackingLQR on its own trajectory" % name)
        for i in range(n):
            rep = capi.PlantsHandle(mh, *[np.repeat(a[i:i + 1], nk, axis=0) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)])
            A, Bu, Bl, G = capi.linearize(mh, c["zd"][i][:nk], c["cj"], c["Fd"][i][:nk], plants=rep)
            rep.close()
            pr = tc.single_problem(A, Bu, Bl, G, trk.K, shared.Q[0], shared.R[0], Wu, c["S0"], N)
            tc.check_horizon(pr, ("full", True, True), N, 0, shared.Sigma(i), None, shared.stage_cost[i], shared.state_std[i], shared.input_std[i],
                             shared.expected_score[i], "%s, the nominal table on plant %d" % (name, i))
        assert not np.array_equal(shared.stage_cost[0], c["cov"].stage_cost[0])      # another table than the plant's own: another cost
    finally:
        own.close()
        shared.close()


@pytest.mark.parametrize("name", ("chain3", "sawyer"))
def test_one_problem_per_chunk_changes_nothing(cclqr, orc, name):
    c = dev_case(cclqr, orc, name)
    make = lambda wb: cclqr.TrackingCovariance(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"], workspace_bytes=wb)
    with pytest.raises(cclqr._capi.CclqrError) as e:
        make(1000)
    assert e.value.code == cclqr._capi.EINVAL
    m = re.search(r"workspace_bytes = 1000 does not hold one problem.* need (\d+) bytes", str(e.value))
    assert m, str(e.value)
    one = int(m.group(1))
    assert 8 * (c["N"] - 1) * (12 * c["t"].nb) ** 2 < one < (1 << 30)
    with pytest.raises(cclqr._capi.CclqrError):
        make(one - 1)
    for budget in (one, 2 * one + one // 2):
        cov = make(budget)
        try:
            assert _same(_outputs(cov), _outputs(c["cov"])), budget
        finally:
            cov.close()


def test_one_stationary_row_shared_by_every_plant_has_the_references_values(cclqr, orc):
    """a controller of ONE gain row and one table through the C entry (nK = 1, n_gains = 1): the row acts at every knot of every plant's trajectory"""
    capi = cclqr._capi
    c = dev_case(cclqr, orc, "chain3")
    dev = cclqr.lqr._device_mech(c["mech"])
    n, N, nb, mu = c["n"], c["N"], c["t"].nb, len(c["cj"])
    pb, nk = c["plants"], N - 1
    K1 = np.ascontiguousarray(c["ctl"].gains(0)[N // 2][None])      # [1][mu][mx]: some stabilising row
    ctrl = capi.CtrlHandle(dev, c["cj"], K=K1, N=0, zd=c["zd"][0][0])
    Wu, Q, R = SIGMA ** 2 * np.ones((mu, mu)), c["cov"].Q[0], c["cov"].R[0]
    try:
        v, cost, zstd, ustd, total = capi.value_create_covariance_tracking(dev, ctrl, c["zd"], n, N, c["cj"], Q, R, Wu, c["S0"], Fd=c["Fd"], plants=pb.handle(dev))
        try:
            for i in range(n):
                rep = capi.PlantsHandle(dev, *[np.repeat(a[i:i + 1], nk, axis=0) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)])
                A, Bu, Bl, G = capi.linearize(dev, c["zd"][i][:nk], c["cj"], c["Fd"][i][:nk], plants=rep)
                rep.close()
                pr = tc.single_problem(A, Bu, Bl, G, np.repeat(K1, nk, axis=0), Q, R, Wu, c["S0"], N)
                tc.check_horizon(pr, ("full", True, True), N, 0, v.get(i), None, cost[i], zstd[i], ustd[i], total[i], "one row, plant %d" % i)
        finally:
            v.close()
    finally:
        ctrl.close()


def test_device_tensors_give_the_host_arrays_bits(cclqr, orc):
    import torch
    c = dev_case(cclqr, orc, "tree-slider")
    z, F = torch.from_numpy(np.ascontiguousarray(c["zd"])).cuda(), torch.from_numpy(np.ascontiguousarray(c["Fd"])).cuda()
    cov = cclqr.TrackingCovariance(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"], storage=z, Fτ=F)
    try:
        assert _same(_outputs(cov), _outputs(c["cov"]))
    finally:
        cov.close()
    # the controller's own trajectories as host arrays, passed explicitly: the same again
    cov = cclqr.TrackingCovariance(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=c["S0"], storage=c["zd"], Fτ=c["U"])
    try:
        assert _same(_outputs(cov), _outputs(c["cov"]))
    finally:
        cov.close()


def test_reversed_bodyids_permute_q_sigma0_and_state_std(cclqr, orc):
    c = dev_case(cclqr, orc, "chain3")
    nb = c["t"].nb
    ids = list(reversed(c["ids"]))
    assert ids != c["ids"]
    Qb = [np.eye(12) * (10.0 + 3.0 * k) for k in range(nb)]                                            # in the mechanism's order: body k weighs 10 + 3 k
    place = np.concatenate([12 * ids.index(b) + np.arange(12) for b in sorted(ids)])                  # where each coordinate of the mechanism's order lies in the order of ids
    S0m = c["S0"]
    S0r = np.empty_like(S0m)
    S0r[np.ix_(place, place)] = S0m                                                                   # the same start, written in the order of ids
    a = cclqr.TrackingCovariance(c["mech"], c["ctl"], c["ids"], c["eids"], Qb, c["Rb"], noise_scale=SIGMA, Sigma0=S0m)
    b = cclqr.TrackingCovariance(c["mech"], c["ctl"], ids, c["eids"], list(reversed(Qb)), c["Rb"], noise_scale=SIGMA, Sigma0=S0r)
    try:
        assert np.array_equal(a.Q, b.Q) and np.array_equal(a.Sigma0, b.Sigma0)
        assert _same([a.stage_cost, a.input_std, a.expected_score, a.Sigma(0)], [b.stage_cost, b.input_std, b.expected_score, b.Sigma(0)])
        assert np.array_equal(b.state_std[..., place], a.state_std) and not np.array_equal(b.state_std, a.state_std)
        assert not np.array_equal(a.stage_cost, c["cov"].stage_cost)      # the weights are read: another Q, another cost
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_outputs_untouched_and_loops_are_unsupported(cclqr, orc):
    capi = cclqr._capi
    L = capi.lib()
    c = dev_case(cclqr, orc, "chain3")
    dev = cclqr.lqr._device_mech(c["mech"])
    n, N, nb, mu = c["n"], c["N"], c["t"].nb, len(c["cj"])
    mx = 12 * nb
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    cj = np.ascontiguousarray(c["cj"], dtype=np.int32)
    zd, Fd = np.ascontiguousarray(c["zd"]), np.ascontiguousarray(c["Fd"])
    Q, R = np.ascontiguousarray(c["cov"].Q), np.ascontiguousarray(c["cov"].R)
    W3, S1 = np.ones((3, mu, mu)), np.ascontiguousarray(np.eye(mx))
    SENTINEL = 0x5A5A
    ph = c["plants"].handle(dev)
    one_row = capi.CtrlHandle(dev, c["cj"], K=np.zeros((1, mu, mx)), N=0, zd=c["zd"][0][0])
    open_loop = capi.CtrlHandle(dev, c["cj"], K=None, N=0, zd=c["zd"][0][0])      # setpoints only: no gains
    loop_dev = cclqr.lqr._device_mech(cclqr.examples.fourbar()["mech"])
    f = L.cclqr_value_create_covariance_tracking

    def call(mech=dev, plants=ph, first=0, n_=n, N_=N, mu_=mu, ctrl=c["ctl"]._handle, n_weights=1, Q_=Q, R_=R, n_noise=1, Wu_=W3, S0_=S1, wb=0, zd_=zd):
        cost, zs, us, tot = np.full((n, N, 2), 7.5), np.full((n, N, mx), 7.5), np.full((n, N, mu), 7.5), np.full((n, 2), 7.5)
        out = C.c_void_p(SENTINEL)
        rc = f(mech.ptr, None if plants is None else plants.ptr, C.c_int64(first), C.c_int32(n_), C.c_int32(N_), d(zd_), d(Fd), C.c_int32(0), C.c_int32(mu_),
               cj.ctypes.data_as(ip), ctrl.ptr, C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), d(S0_), C.c_int64(wb), d(cost), d(zs), d(us), d(tot),
               None, C.byref(out))
        untouched = bool(all((x == 7.5).all() for x in (cost, zs, us, tot)) and out.value == SENTINEL)
        if rc == capi.OK:
            capi.check(L.cclqr_value_destroy(out))
        return rc, untouched

    try:
        rc, untouched = call()
        assert rc == capi.OK and not untouched
        assert call(ctrl=one_row)[0] == capi.OK      # one stationary row, one table: accepted
        refused = dict(cost_without_Q=call(Q_=None), cost_without_R=call(R_=None), n_noise_3=call(n_noise=3), no_source=call(Wu_=None, S0_=None),
                       n_weights_3=call(n_weights=3), rows_not_N_minus_1=call(N_=N - 2), tables_not_n=call(n_=n - 1), no_models=call(n_=0), N_0=call(N_=0),
                       other_joints=call(mu_=0), no_gains=call(ctrl=open_loop), plants_out_of_range=call(first=2), small_workspace=call(wb=1000), zd_null=call(zd_=None))
        for what, (rc, untouched) in refused.items():
            assert rc == capi.EINVAL and untouched, (what, rc, untouched, L.cclqr_last_error().decode())
        rc, untouched = call(mech=loop_dev, plants=None)
        assert rc == capi.EUNSUPPORTED and untouched
    finally:
        one_row.close()
        open_loop.close()
