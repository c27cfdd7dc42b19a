"""The references of the Riccati doubling, without a GPU: on every case of riccati_doubling_common the doubling schedule in numpy float64 stays inside the bound the
GPU tests hold the kernels to, against a longdouble reference that steps lqr.jl:151-170 and shares no schedule with it; the operation counts are those of
square-and-multiply; tol of a run to convergence is placed away from every longdouble increment (asserted by the builder)."""
import numpy as np
import pytest

import dlqr_reference as ref
import riccati_doubling_common as rdc


@pytest.mark.parametrize("name", [c["name"] for c in rdc.CASES])
def test_numpy_schedule_stays_inside_the_bound(name):
    c = rdc.build_case(name)
    for n, rows in c["fixed"].items():
        for p, (Kref, Pref, levels, e64K, e64P, eK, eP) in enumerate(rows):
            print("%s N-1=%d problem %d: levels %d, schedule eK %.3g eP %.3g, e64K %.3g e64P %.3g" % (name, n, p, levels, eK, eP, e64K, e64P))
            assert levels == n.bit_length() - 1
            assert eK <= ref.tolerance(e64K) and eP <= ref.tolerance(e64P)
    for p, (Kref, Pref, levels, reason, dn, an, e64K, e64P, eK, eP) in enumerate(c["conv"]):
        print("%s to convergence (tol %.3g) problem %d: levels %d reason %d dnorm %s anorm %s, schedule eK %.3g eP %.3g, e64K %.3g e64P %.3g"
              % (name, c["tol"], p, levels, reason, dn, an, eK, eP, e64K, e64P))
        assert eK <= ref.tolerance(e64K) and eP <= ref.tolerance(e64P)
    assert c["conv"][0][2] >= c["level"] and c["conv"][0][3] == 0


def test_schedule_counts():
    for n in (1, 2, 7, 8, 9, 37, 1000):
        ops = rdc.schedule(n)
        assert ops[0] in "CD" and ops.count("C") == 1 and ops[-1] in "CA"
        assert ops.count("A") + ops.count("D") == bin(n).count("1") - 1 + n.bit_length() - 1
        assert ops.count("D") == n.bit_length() - 1


def test_unstable_problem_stops_for_growth():
    A, Bu, Bl, G, Q, R, levels, reason = rdc.unstable_problem()
    assert reason == 2 and 8 <= levels <= 14
