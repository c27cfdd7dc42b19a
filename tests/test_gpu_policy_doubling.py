"""cclqr_policy_value_doubling on the device: every case of tests/policy_doubling_common.py on every path its shape has, against the extended-precision STEPPING
references and the acceptance rule stated there (the CPU twin tests/test_policy_doubling_reference.py shows that the cases cannot pass vacuously).
  * fixed horizon: P within the bound, levels exact, norm(M(n)) reported; and P within TWICE the bound of the device's own cclqr_policy_value (nK = 1, tol = 0, same
    N): both lie within the bound of the one reference.
  * to convergence: levels and reason exact, P, dnorm and gnorm within the rule; the unstable closed loop stops with reason 2 and a finite P; max_levels = 3 stops
    with reason 1 at the cost-to-go of 8 steps.
  * bitwise: shared against replicated gains and weights, a problem alone against inside a batch, path 1 against path 0 where 0 chooses the resident kernel.
  * every CCLQR_EINVAL leaves the outputs untouched; a singular G Bλ is CCLQR_ESINGULAR."""
import numpy as np
import pytest

import dlqr_reference as ref
import policy_doubling_common as pdc

pytestmark = pytest.mark.gpu

RUNS = [(c["name"], path) for c in pdc.CASES for path in c["paths"]]


def _models(pr, sl=slice(None)):
    return pr["A"][sl], pr["Bu"][sl], pr["Bl"][sl], pr["G"][sl]


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_fixed_horizon_against_extended_precision_and_the_stepping_kernels(cclqr, name, path):
    capi = cclqr._capi
    pr = pdc.build_case(name)
    for n in pr["steps"]:
        P, lv, rs, dn, gn = capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], n + 1, path=path)
        Ps, _, _ = capi.policy_value(*_models(pr), pr["K"][None], pr["Q"], pr["R"], n + 1, tol=0.0, path=path)
        for p in range(pr["nprob"]):
            what = "%s path %d problem %d, %d steps" % (name, path, p, n)
            pdc.check_fixed(P[p], lv[p], gn[p], dn[p], pr["fixed"][n][p], what)
            assert rs[p] == 0
            bound, scale = ref.tolerance(pr["fixed"][n][p][3]), float(np.abs(pr["fixed"][n][p][0]).max())
            dev = float(np.abs(P[p] - Ps[p]).max()) / scale
            print("%s: against the stepping kernels %.3g relative, bound 2 x %.3g" % (what, dev, bound))
            assert dev <= 2.0 * bound, what
            if n == 0:
                assert np.array_equal(P[p], pr["Q"]), what      # no step: Q, bitwise


@pytest.mark.parametrize("name,path", RUNS, ids=["%s-path%d" % r for r in RUNS])
def test_every_run_to_convergence_against_extended_precision(cclqr, name, path):
    pr = pdc.build_case(name)
    P, lv, rs, dn, gn = cclqr._capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], 0, tol=pr["tol"], max_levels=pr["max_levels"], path=path)
    for p in range(pr["nprob"]):
        pdc.check_conv(P[p], lv[p], rs[p], dn[p], gn[p], pr["conv"][p], "%s path %d problem %d" % (name, path, p))
    if name == "pd_unstable":
        assert rs[2] == 2 and np.isfinite(P[2]).all() and gn[2, 0] > pdc.GROWTH > gn[2, 1] and rs[0] == 0


@pytest.mark.parametrize("name,path", [("pd_12", 1), ("pd_12", 2), ("pd_30", 2)])
def test_max_levels_stops_with_reason_one(cclqr, name, path):
    """tol = 0 never converges: three levels are 8 steps, and P is the fixed horizon's of N = 9"""
    pr = pdc.build_case(name)
    P, lv, rs, dn, gn = cclqr._capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], 0, tol=0.0, max_levels=3, path=path)
    assert (lv == 3).all() and (rs == 1).all() and np.isfinite(dn).all() and np.isfinite(gn).all()
    for p in range(pr["nprob"]):
        pdc.check_fixed(P[p], 3, None, None, pr["fixed"][8][p], "%s path %d problem %d, max_levels 3" % (name, path, p))


@pytest.mark.parametrize("name,path,N", [("pd_24", 1, 38), ("pd_24", 1, 0), ("pd_30", 2, 38), ("pd_30", 2, 0), ("pd_84", 1, 10), ("pd_97", 2, 0)])
def test_shared_replicated_alone_and_batched_give_the_same_bits(cclqr, name, path, N):
    capi = cclqr._capi
    pr = pdc.build_case(name)
    n = pr["nprob"]
    kw = dict(tol=pr["tol"], max_levels=pr["max_levels"], path=path)
    same = lambda a, b: all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    base = capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], N, **kw)
    assert same(base, capi.policy_value_doubling(*_models(pr), np.stack([pr["K"]] * n), pr["Q"], pr["R"], N, **kw))
    assert same(base, capi.policy_value_doubling(*_models(pr), pr["K"], np.stack([pr["Q"]] * n), np.stack([pr["R"]] * n), N, **kw))
    for p in range(n):
        alone = capi.policy_value_doubling(*_models(pr, slice(p, p + 1)), pr["K"], pr["Q"], pr["R"], N, **kw)
        assert same([x[p:p + 1] for x in base], alone), p
    # and per-problem arguments are read per problem: a gain of zeros for problem 1 alone changes problem 1 alone
    if pr["mu"]:
        Kz = np.stack([pr["K"]] * n)
        Kz[1] = 0.0
        Pz = capi.policy_value_doubling(*_models(pr), Kz, pr["Q"], pr["R"], N, **kw)[0]
        assert np.array_equal(Pz[0], base[0][0]) and not np.array_equal(Pz[1], base[0][1])


@pytest.mark.parametrize("name", ["pd_12", "pd_24", "pd_36", "pd_nonsym"])
@pytest.mark.parametrize("N", [0, 38])
def test_path_zero_is_the_resident_kernel_where_it_chooses_it(cclqr, name, N):
    capi = cclqr._capi
    pr = pdc.build_case(name)
    assert pr["mx"] < 64 and pr["mx"] % 4 == 0      # small problems run resident whatever their number
    kw = dict(tol=pr["tol"], max_levels=pr["max_levels"])
    a = capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], N, path=0, **kw)
    b = capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], N, path=1, **kw)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_a_nonsymmetric_problem_keeps_a_nonsymmetric_cost_to_go_and_null_diagnostics_change_nothing(cclqr):
    pr = pdc.build_case("pd_nonsym")
    for path in (1, 2):
        P = cclqr._capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], 38, path=path)[0]
        assert all(np.abs(P[p] - P[p].T).max() > 1e-3 * np.abs(P[p]).max() for p in range(pr["nprob"]))
        P0, lv, rs, dn, gn = cclqr._capi.policy_value_doubling(*_models(pr), pr["K"], pr["Q"], pr["R"], 38, path=path, want_diag=False)
        assert lv is None and rs is None and dn is None and gn is None and np.array_equal(P0, P)


def test_every_refusal_code_and_untouched_outputs(cclqr):
    capi = cclqr._capi
    pr = pdc.build_case("pd_36")
    Bl = np.ascontiguousarray(pr["Bl"])
    call = pdc.refusal_call(capi, pr)
    assert call()[0] == capi.OK and call(N=0)[0] == capi.OK and call(N=0, max_levels=1)[0] == capi.OK and call(N=0, max_levels=60, tol=1e300)[0] == capi.OK
    assert call(max_levels=0)[0] == capi.OK      # (max_levels is not read for a fixed horizon)
    refused = {what: call(**kw) for what, kw in pdc.refusal_cases().items()}
    for what, (rc, untouched, msg) in refused.items():
        assert rc == capi.EINVAL and untouched, (what, rc, untouched, msg)
    assert call(Bl_=np.zeros_like(Bl))[0] == capi.ESINGULAR and call(N=0, Bl_=np.zeros_like(Bl))[0] == capi.ESINGULAR
    assert call(N=1, Bl_=np.zeros_like(Bl))[0] == capi.OK      # no step reaches the model, as in the stepping recursion
