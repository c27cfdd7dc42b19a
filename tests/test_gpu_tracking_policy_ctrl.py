"""TrackingPolicyValue / cclqr_value_create_policy_tracking on the chain3 case of tests/plant_tracking_common.py (5 plants, 24 knots), set up as
tests/test_gpu_tracking_covariance_ctrl.py sets it up:
  * a PlantTrackingLQR, one table per plant, against the longdouble recursion of tests/tracking_policy_common.py run on the device's OWN per-knot linearisation
    (linearize(..., plants=) on a table that repeats the plant) with the gains read back, at knot = 0, N // 2 and N - 1 (the last: Q exactly, every price zero);
  * a plain TrackingLQR on its own trajectory, and as ONE table shared by every plant along the plants' own trajectories (storage=, Fτ=, plants=), against the same;
  * one problem per chunk gives bitwise the default call's result; device tensors give bitwise the host arrays' result;
  * reversed bodyids permute Q and nothing else;
  * duality with TrackingCovariance on the device: Sigma0 = δδ' and noise_scale = σ give sum(expected_score) = δ' P(0) δ + expected_noise_cost;
  * the refusals of the C entry leave the outputs and *out untouched; a closed-loop mechanism is CCLQR_EUNSUPPORTED; simulate raises TypeError."""
import ctypes as C
import re

import numpy as np
import pytest

import dlqr_reference as ref
import tracking_policy_common as tp
from plant_tracking_common import case, open_loop

pytestmark = pytest.mark.gpu
SIGMA = 0.3
_dev = {}


def dev_case(cclqr, orc):
    """chain3 with its PlantTrackingLQR, the default call's TrackingPolicyValue at knot 0, the device's own linearisation of every plant's trajectory and the
    longdouble reference on it, once per session"""
    if _dev:
        return _dev
    capi = cclqr._capi
    c = dict(case(cclqr, orc, "chain3"))
    mech, nb, mu, n, N = c["mech"], c["t"].nb, len(c["cj"]), c["n"], c["N"]
    c["ids"] = [cclqr.getid(b) for b in mech.bodies]
    c["eids"] = [cclqr.getid(mech.eqconstraints[j]) for j in c["cj"]]
    assert c["ids"] == sorted(c["ids"])      # the mechanism's own order: P needs no permutation here
    c["Qb"], c["Rb"] = [np.eye(12) * 10.0] * nb, [np.eye(1) * 0.1] * mu
    c["ctl"] = cclqr.PlantTrackingLQR(mech, c["plants"], c["zd"], c["U"], c["eids"], c["Qb"], c["Rb"])
    c["tpv"] = cclqr.TrackingPolicyValue(mech, c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA)
    c["Wu"] = SIGMA ** 2 * np.ones((mu, mu))
    mh, pb, nk = cclqr.lqr._device_mech(mech), c["plants"], N - 1
    c["lin"] = []
    for i in range(n):
        rep = capi.PlantsHandle(mh, *[np.repeat(a[i:i + 1], nk, axis=0) for a in (pb.mass, pb.inertia, pb.p1, pb.p2)])
        c["lin"].append(capi.linearize(mh, c["zd"][i][:nk], c["cj"], c["Fd"][i][:nk], plants=rep))
        rep.close()
    c["ref"] = [tp.single_reference(*c["lin"][i], c["ctl"].gains(i), c["tpv"].Q[0], c["tpv"].R[0], c["Wu"], N, what="chain3 plant %d" % i) for i in range(n)]
    _dev.update(c)
    return _dev


def check_knot(r, N, knot, P, price, total, what):
    """P_knot, the prices of the knots j >= knot (zeros below, and at N - 1) and their sum against the reference r of the whole horizon; returns the bound"""
    bound = ref.tolerance(r["e64"][0])
    Pref = r["P"][0][knot]
    err = float(np.abs(P - Pref).max() / np.abs(Pref).max())
    assert np.isfinite(P).all() and err <= bound, "%s: max|P - Pref| = %.3g relative, bound %.3g" % (what, err, bound)
    assert price.shape == (N,) and not price[:knot].any() and price[N - 1] == 0.0, "%s: prices below the knot and at the last knot are zero" % what
    perr = 0.0
    for j in range(knot, N):
        d, m = float(abs(price[j] - r["price"][0][j])), float(r["pmag"][0][j])
        perr = max(perr, d / m if m else 0.0)
        assert d <= bound * m, "%s knot %d: price %.17g, reference %.17g" % (what, j, price[j], float(r["price"][0][j]))
    want, tmag = float(np.sum(r["price"][0][knot:])), float(np.sum(r["pmag"][0][knot:]))
    assert abs(float(total) - want) <= bound * tmag, "%s: expected_noise_cost %.17g, reference %.17g" % (what, float(total), want)
    run = 0.0
    for j in range(N - 2, knot - 1, -1):
        run = run + price[j]
    assert total == run, "%s: expected_noise_cost is not the prices summed from N - 2 down to the knot" % what
    print("%s: knot %d, bound %.3g, P off by %.3g relative, prices by at most %.3g of their magnitude sums, total %.17g (reference %.17g)"
          % (what, knot, bound, err, perr, float(total), want))
    return bound


def _outputs(v):
    return [v.noise_price, v.expected_noise_cost] + [v.P(i) for i in range(v.n_models)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_one_table_per_plant_at_three_knots_against_extended_precision(cclqr, orc):
    c = dev_case(cclqr, orc)
    mech, n, N, nb = c["mech"], c["n"], c["N"], c["t"].nb
    for knot in (0, N // 2, N - 1):
        v = c["tpv"] if knot == 0 else cclqr.TrackingPolicyValue(mech, c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, knot=knot)
        try:
            assert v.N == N and v.n_models == n and v.knot == knot and v.noise_price.shape == (n, N) and v.expected_noise_cost.shape == (n,)
            for i in range(n):
                check_knot(c["ref"][i], N, knot, v.P(i), v.noise_price[i], v.expected_noise_cost[i], "chain3 plant %d" % i)
            if knot == N - 1:
                assert all(np.array_equal(v.P(i), v.Q[0]) for i in range(n)) and not v.noise_price.any() and not v.expected_noise_cost.any()
            else:      # the plants differ: so do their costs-to-go (an ignored plant table or a shifted trajectory-to-plant map fails above, and here)
                assert np.abs(v.P(1) - v.P(0)).max() > 1e-6 * np.abs(v.P(0)).max()
        finally:
            if knot:
                v.close()
    with pytest.raises(TypeError, match="not a Controller"):
        cclqr.simulate(mech, cclqr.Storage(2, nb), c["tpv"])
    quiet = cclqr.TrackingPolicyValue(mech, c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"])      # no noise: the same P, no price
    try:
        assert _same([quiet.P(i) for i in range(n)], [c["tpv"].P(i) for i in range(n)]) and not quiet.noise_price.any() and not quiet.expected_noise_cost.any()
    finally:
        quiet.close()


def test_a_plain_tracking_lqr_alone_and_as_one_table_shared_by_every_plant(cclqr, orc):
    """a TrackingLQR designed on the mechanism's own plant along its own open-loop rollout: (a) its cost-to-go along that trajectory, one model; (b) storage= / Fτ= /
    plants=: the NOMINAL table, one shared by all, along every perturbed plant's own trajectory on that plant -- a table read per problem where it is shared, or a
    row shifted by a knot, fails here"""
    capi = cclqr._capi
    c = dev_case(cclqr, orc)
    mech, n, N, nb, mu = c["mech"], c["n"], c["N"], c["t"].nb, len(c["cj"])
    zn = open_loop(orc, c["t"], c["cj"], c["U"], c["z_nominal"])
    trk = cclqr.TrackingLQR(mech, cclqr.Storage(N, nb, 1, z=np.ascontiguousarray(zn[None])), c["U"], c["eids"], c["Qb"], c["Rb"])
    mh, nk = cclqr.lqr._device_mech(mech), N - 1
    knot = N // 2
    own = cclqr.TrackingPolicyValue(mech, trk, c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA)
    shared = cclqr.TrackingPolicyValue(mech, trk, c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, storage=c["zd"], Fτ=c["Fd"], plants=c["plants"], knot=knot)
    try:
        assert own.n_models == 1 and own.N == N and own.knot == 0 and shared.n_models == n and shared.knot == knot
        A, Bu, Bl, G = capi.linearize(mh, zn[:nk], c["cj"], c["U"][:nk])
        r = tp.single_reference(A, Bu, Bl, G, trk.K, own.Q[0], own.R[0], c["Wu"], N, what="the TrackingLQR on its own trajectory")
        check_knot(r, N, 0, own.P(0), own.noise_price[0], own.expected_noise_cost[0], "chain3, the TrackingLQR on its own trajectory")
        for i in range(n):
            r = tp.single_reference(*c["lin"][i], trk.K, shared.Q[0], shared.R[0], c["Wu"], N, what="the nominal table on plant %d" % i)
            check_knot(r, N, knot, shared.P(i), shared.noise_price[i], shared.expected_noise_cost[i], "chain3, the nominal table on plant %d" % i)
        assert not np.array_equal(shared.noise_price[0], c["tpv"].noise_price[0])      # another table than the plant's own: another price
        assert np.array_equal(shared.zd, c["zd"][:, knot]) and np.array_equal(own.zd, zn[None, 0])      # the setpoints predicted_cost measures about
    finally:
        own.close()
        shared.close()


def test_one_problem_per_chunk_changes_nothing(cclqr, orc):
    c = dev_case(cclqr, orc)
    make = lambda wb: cclqr.TrackingPolicyValue(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, workspace_bytes=wb)
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
        v = make(budget)
        try:
            assert _same(_outputs(v), _outputs(c["tpv"])), budget
        finally:
            v.close()


def test_device_tensors_give_the_host_arrays_bits(cclqr, orc):
    import torch
    c = dev_case(cclqr, orc)
    z, F = torch.from_numpy(np.ascontiguousarray(c["zd"])).cuda(), torch.from_numpy(np.ascontiguousarray(c["Fd"])).cuda()
    knot = 5
    host = cclqr.TrackingPolicyValue(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, storage=c["zd"], Fτ=c["U"], knot=knot)
    v = cclqr.TrackingPolicyValue(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, storage=z, Fτ=F, knot=knot)
    try:
        assert _same(_outputs(v), _outputs(host)) and np.array_equal(v.zd, host.zd) and np.array_equal(v.zd, c["zd"][:, knot])
    finally:
        v.close()
        host.close()


def test_reversed_bodyids_permute_q_and_nothing_else(cclqr, orc):
    c = dev_case(cclqr, orc)
    nb = c["t"].nb
    ids = list(reversed(c["ids"]))
    assert ids != c["ids"]
    Qb = [np.eye(12) * (10.0 + 3.0 * k) for k in range(nb)]      # in the mechanism's order: body k weighs 10 + 3 k
    a = cclqr.TrackingPolicyValue(c["mech"], c["ctl"], c["ids"], c["eids"], Qb, c["Rb"], noise_scale=SIGMA)
    b = cclqr.TrackingPolicyValue(c["mech"], c["ctl"], ids, c["eids"], list(reversed(Qb)), c["Rb"], noise_scale=SIGMA)
    try:
        assert np.array_equal(a.Q, b.Q) and _same(_outputs(a), _outputs(b))
        assert not np.array_equal(a.P(0), c["tpv"].P(0))      # the weights are read: another Q, another cost-to-go
    finally:
        a.close()
        b.close()


def test_duality_with_the_tracking_covariance_on_the_device(cclqr, orc):
    """Sigma0 = δδ' and noise_scale = σ: sum(expected_score) of TrackingCovariance = δ' P(0) δ + expected_noise_cost within the bound of the policy recursion,
    dlqr_reference.tolerance(e64), times the cost's magnitude sum |δ|' |P_0| |δ| + the prices' magnitude sums"""
    c = dev_case(cclqr, orc)
    n, nb = c["n"], c["t"].nb
    delta = 1e-2 * np.random.default_rng(5).normal(size=12 * nb)
    S0 = np.outer(delta, delta)
    cov = cclqr.TrackingCovariance(c["mech"], c["ctl"], c["ids"], c["eids"], c["Qb"], c["Rb"], noise_scale=SIGMA, Sigma0=S0)
    try:
        for i in range(n):
            r = c["ref"][i]
            bound = ref.tolerance(r["e64"][0])
            P0 = c["tpv"].P(i)
            dual = float(delta @ P0 @ delta) + float(c["tpv"].expected_noise_cost[i])
            scale = float(np.abs(delta) @ np.abs(np.asarray(r["P"][0][0], dtype=np.float64)) @ np.abs(delta)) + float(np.sum(r["pmag"][0]))
            got = float(cov.expected_score[i].sum())
            print("chain3 plant %d: δ'P(0)δ + expected_noise_cost = %.17g, sum(expected_score) = %.17g, off by %.3g of the cost scale %.3g (bound %.3g)"
                  % (i, dual, got, abs(dual - got) / scale, scale, bound))
            assert abs(dual - got) <= bound * scale
    finally:
        cov.close()


def test_refusals_leave_the_outputs_untouched_and_loops_are_unsupported(cclqr, orc):
    capi = cclqr._capi
    L = capi.lib()
    c = dev_case(cclqr, orc)
    dev = cclqr.lqr._device_mech(c["mech"])
    n, N, nb, mu = c["n"], c["N"], c["t"].nb, len(c["cj"])
    mx = 12 * nb
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = lambda a: None if a is None else a.ctypes.data_as(dp)
    cj = np.ascontiguousarray(c["cj"], dtype=np.int32)
    zd, Fd = np.ascontiguousarray(c["zd"]), np.ascontiguousarray(c["Fd"])
    Q, R = np.ascontiguousarray(c["tpv"].Q), np.ascontiguousarray(c["tpv"].R)
    W3 = np.ones((3, mu, mu))
    SENTINEL = 0x5A5A
    ph = c["plants"].handle(dev)
    one_row = capi.CtrlHandle(dev, c["cj"], K=np.zeros((1, mu, mx)), N=0, zd=c["zd"][0][0])
    no_gains = capi.CtrlHandle(dev, c["cj"], K=None, N=0, zd=c["zd"][0][0])      # setpoints only
    loop_dev = cclqr.lqr._device_mech(cclqr.examples.fourbar()["mech"])
    f = L.cclqr_value_create_policy_tracking

    def call(mech=dev, plants=ph, first=0, n_=n, N_=N, mu_=mu, ctrl=c["ctl"]._handle, n_weights=1, Q_=Q, R_=R, n_noise=1, Wu_=W3, knot=0, wb=0, zd_=zd, price_=True,
             total_=True):
        price, tot = np.full((n, N), 7.5), np.full(n, 7.5)
        out = C.c_void_p(SENTINEL)
        rc = f(mech.ptr, None if plants is None else plants.ptr, C.c_int64(first), C.c_int32(n_), C.c_int32(N_), d(zd_), d(Fd), C.c_int32(0), C.c_int32(mu_),
               cj.ctypes.data_as(ip), ctrl.ptr, C.c_int32(n_weights), d(Q_), d(R_), C.c_int32(n_noise), d(Wu_), C.c_int32(knot), C.c_int64(wb),
               d(price) if price_ else None, d(tot) if total_ else None, None, C.byref(out))
        untouched = bool((price == 7.5).all() and (tot == 7.5).all() and out.value == SENTINEL)
        if rc == capi.OK:
            capi.check(L.cclqr_value_destroy(out))
        return rc, untouched

    try:
        rc, untouched = call()
        assert rc == capi.OK and not untouched
        assert call(ctrl=one_row)[0] == capi.OK and call(Wu_=None, price_=False, total_=False)[0] == capi.OK and call(knot=N - 1)[0] == capi.OK
        refused = dict(without_Q=call(Q_=None), without_R=call(R_=None), n_noise_3=call(n_noise=3), price_without_Wu=call(Wu_=None, total_=False),
                       total_without_Wu=call(Wu_=None, price_=False), n_weights_3=call(n_weights=3), rows_not_N_minus_1=call(N_=N - 2), tables_not_n=call(n_=n - 1),
                       no_models=call(n_=0), N_0=call(N_=0), other_joints=call(mu_=0), no_gains=call(ctrl=no_gains), plants_out_of_range=call(first=2),
                       small_workspace=call(wb=1000), zd_null=call(zd_=None), knot_N=call(knot=N), knot_negative=call(knot=-1))
        for what, (rc, untouched) in refused.items():
            assert rc == capi.EINVAL and untouched, (what, rc, untouched, L.cclqr_last_error().decode())
        rc, untouched = call(mech=loop_dev, plants=None)
        assert rc == capi.EUNSUPPORTED and untouched
    finally:
        one_row.close()
        no_gains.close()
