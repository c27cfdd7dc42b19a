"""The closed-loop covariance by doubling without a GPU: the schedule the device runs, restated in numpy float64 on (Abar', W / w, Σ0 / w), meets the acceptance rule
of tests/covariance_common.py against the longdouble STEPPING references on every case, variant and horizon -- so the GPU test cannot pass vacuously and the bound is
not a property of the code under test --; e64 of the fixed horizons stays where it was measured when the cases were written (at most 4e-15 on five cases, 3e-14 on
pd_mu0, the all-Σ0 propagation), so their bound is max(10 e64, 1e-12) = 1e-12 everywhere (a run to convergence takes its own e64: the unstable problem of pd_unstable
grows to 1e50 before it stops, and its float64 stepping twins are 2e-12 apart); and the duality tr(Qbar C(n)) = tr(S(n) W) with the cost recursion of policy_doubling_common."""
import numpy as np
import pytest

import covariance_common as cc
import dlqr_reference as ref
import policy_doubling_common as pdc

LD = np.longdouble


def _twin(pr, p, wu, s0, w):
    A64 = pdc.closed_loop(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"], pr["K"], np.float64, True)[0]
    W64 = cc.noise(cc.input_map(pr["Bu"][p], pr["Bl"][p], pr["G"][p], np.float64, True), wu, np.float64)
    S064 = np.zeros((pr["mx"], pr["mx"])) if s0 is None else np.asarray(s0, dtype=np.float64)
    return A64.T, W64 / w, S064 / w


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_restated_schedule_meets_the_rule_on_every_case(name):
    pr = cc.build_case(name)
    worst = 0.0
    for vname, v in pr["variants"].items():
        for p in range(pr["nprob"]):
            wu = None if v["Wu"] is None else (v["Wu"][p] if v["Wu"].ndim == 3 else v["Wu"])
            At, Ws, S0s = _twin(pr, p, wu, v["Sigma0"], v["w"][p])
            for n, rows in v["fixed"].items():
                r = rows[p]
                S, levels, _, gM = pdc.doubling_fixed(At, Ws, S0s, n)
                S = S * v["w"][p]
                cost, zvar, uvar, _, _ = cc.moments(S, pr["Q"], pr["R"], pr["K"])
                cc.check_fixed(S, cost, np.sqrt(np.maximum(zvar, 0)), np.sqrt(np.maximum(uvar, 0)), levels, [gM, np.nan], np.full(2, np.nan), r,
                               "%s %s problem %d, %d steps" % (name, vname, p, n))
                worst = max(worst, r["e64"])
            if "conv" in v:
                r = v["conv"][p]
                with np.errstate(over="ignore", invalid="ignore"):
                    S, levels, reason, incs, gs = pdc.doubling_converge(At, Ws, S0s, v["tol"], v["max_levels"])
                S = S * v["w"][p]
                cost, zvar, uvar, _, _ = cc.moments(S, pr["Q"], pr["R"], pr["K"])
                cc.check_conv(S, cost, np.sqrt(np.maximum(zvar, 0)), np.sqrt(np.maximum(uvar, 0)), levels, reason, pdc.last_two(incs) * v["w"][p], pdc.last_two(gs), r,
                              "%s %s problem %d to convergence" % (name, vname, p))
                print("%s %s problem %d to convergence: e64 %.3g" % (name, vname, p, r["e64"]))
    print("%s: largest e64 of the fixed horizons %.3g" % (name, worst))
    assert ref.tolerance(worst) == 1e-12, "%s: e64 = %.3g needs a wider bound than 1e-12: a finding about the case" % (name, worst)


def test_the_unstable_case_stops_on_growth():
    v = cc.build_case("pd_unstable")["variants"]["nostart"]
    assert [r["reason"] for r in v["conv"]].count(2) >= 1 and all(np.isfinite(r["S"]).all() for r in v["conv"])


@pytest.mark.parametrize("name", ["pd_12", "pd_30", "pd_ml0"])
def test_duality_with_the_cost_recursion(name):
    """tr(Qbar C(n)) = tr(S(n) W): the expected stage cost at C(n) is the n-step cost-to-go weighed by the noise, term by term the same sum"""
    pr = cc.build_case(name)
    for p in range(pr["nprob"]):
        Abar, Qbar = pdc.closed_loop(pr["A"][p], pr["Bu"][p], pr["Bl"][p], pr["G"][p], pr["Q"], pr["R"], pr["K"])
        W = cc.noise(cc.input_map(pr["Bu"][p], pr["Bl"][p], pr["G"][p]), pr["Wu"])
        Z = np.zeros_like(W)
        for n in (1, 2, 9, 37):
            Cn = cc.step_covariance(Abar, W, Z, (n,))[n][0]
            Sn, M = Z, np.eye(pr["mx"], dtype=LD)
            for _ in range(n):
                Sn, M = Sn + M.T @ Qbar @ M, Abar @ M
            a, b = np.sum(Qbar * Cn.T), np.sum(Sn * W.T)
            scale = np.sum(np.abs(Qbar) * np.abs(Cn))
            print("%s problem %d, %d steps: tr(Qbar C) = %.18Lg, tr(S W) = %.18Lg" % (name, p, n, a, b))
            assert abs(a - b) <= 1e-16 * scale
            cost, _, _, _, _ = cc.moments(Cn, pr["Q"], pr["R"], pr["K"])
            assert abs(cost[0] + cost[1] - a) <= 1e-16 * scale      # tr(Q Σ) + tr(R K Σ K') = tr(Qbar Σ)
