"""The Python binding's argument marshalling, without a GPU: what _capi.py and the classes of lqr.py hand the library is what the commit before their helpers were
shared handed it (tests/golden/capi_calls_parent.json, written by tests/capi_recorder.py from that commit), call by call and argument by argument; and each shared
piece exists once."""
import json
import os
import re

import pytest

import capi_recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "constrainedcontrol.jl_amd")

# The one difference from the parent's record: an EMPTY panel (Bu, R with mu = 0; Bl, G with ml = 0) now reaches these entry points as NULL, as it already reached the
# later ones.  All four run cclqr_riccati_value's host sequence (csrc/capi.hip: cclqr_riccati_ex -> cclqr_riccati_weights -> cclqr_riccati_value <- cclqr_riccati_tv),
# which reads no panel whose extent is zero -- the lines below, which the test finds in the source:
NULL_FOR_EMPTY = ("cclqr_riccati_ex", "cclqr_riccati_weights", "cclqr_riccati_value", "cclqr_riccati_tv")
HOST_SEQUENCE_GUARDS = (
    ("capi.hip", "if (!A || !Q || (mu > 0 && (!Bu || !R)) || (ml > 0 && (!Bl || !G)) || !K) return fail(CCLQR_EINVAL, \"null argument\");"),      # cclqr_riccati_value, :1152
    ("capi.hip", "if (mu > 0) HIPTRY(what, hipMemcpy(d.Bu, Bu, count * mx * mu * sizeof(double), hipMemcpyHostToDevice));"),                      # upload_models, :1131
    ("capi.hip", "if (ml > 0) HIPTRY(what, hipMemcpy(d.Bl, Bl, count * mx * ml * sizeof(double), hipMemcpyHostToDevice));"),                      # :1132
    ("capi.hip", "if (ml > 0) HIPTRY(what, hipMemcpy(d.G, G, count * ml * mx * sizeof(double), hipMemcpyHostToDevice));"),                        # :1133
    ("capi.hip", "if (mu > 0) HIPTRY(\"riccati\", hipMemcpy(dR, R, nw * mu * mu * sizeof(double), hipMemcpyHostToDevice));"),                     # run_riccati, :1104
    ("cclqr_internal.h", "return (ric_symmetric(Q, mx) && (mu == 0 || ric_symmetric(R, mu))) ? 0 : 1; }"),                                        # ric_p_rows, :198
    ("cclqr_internal.h", "if (ric_p_rows(Q + p * mx * mx, mx, mu == 0 ? R : R + p * mu * mu, mu)) return 1;"),                                    # ric_p_rows_batch, :203
)


@pytest.fixture(scope="module")
def records(cclqr):
    with pytest.MonkeyPatch.context() as mp:
        got = capi_recorder.record(cclqr, mp.setattr)
    with open(os.path.join(ROOT, "tests", "golden", "capi_calls_parent.json")) as f:
        return got, json.load(f)


def _empty_panel(tag):
    return isinstance(tag, str) and re.match(r"float64\[(\d+, )*0(, \d+)*\] #", tag) is not None


def test_the_recorder_drives_what_it_says(records):
    got, _ = records
    symbols = {c[0] for case in got.values() for c in case["calls"]}
    for name in ("riccati_ex", "riccati_weights", "riccati_value", "policy_value", "policy_value_doubling", "covariance_doubling", "covariance_tracking",
                 "policy_value_tracking", "riccati_doubling", "riccati_tv", "riccati_tracking_ex", "ctrl_create_lqr_batch", "ctrl_create_lqr_batch_plants",
                 "ctrl_create_lqr_batch_weights", "ctrl_create_lqr_batch_value", "ctrl_create_lqr_batch_doubling", "ctrl_create_tracking_batch_plants",
                 "value_create_policy", "value_create_policy_doubling", "value_create_covariance_doubling", "value_create_covariance_tracking",
                 "value_create_policy_tracking", "mech_create", "mech_destroy", "ctrl_create", "ctrl_destroy", "plants_create", "value_create", "value_get",
                 "value_destroy", "score_create", "ctrl_get_gains"):
        assert "cclqr_" + name in symbols, name
    for case in ("PlantLQR", "LQRSweep", "StationaryLQR", "PolicyValue", "StationaryPolicyValue", "StationaryCovariance_noise_scale", "TrackingCovariance",
                 "TrackingPolicyValue"):
        assert got[case]["returns"] == case.split("_")[0] and got[case]["calls"] and got[case]["attributes"], case
    assert len(got) > 300 and sum("raises" in c for c in got.values()) > 100


def test_calls_are_the_parents(records):
    """every case: the same calls with the same arguments, the same structure of the result, the same attributes, the same refusal with the same words"""
    got, want = records
    assert sorted(got) == sorted(want)
    nulled = 0
    for name in sorted(want):
        g, w = got[name], want[name]
        assert {k: v for k, v in g.items() if k != "calls"} == {k: v for k, v in w.items() if k != "calls"}, name
        assert [c[0] for c in g["calls"]] == [c[0] for c in w["calls"]], name
        for (symbol, gargs), (_, wargs) in zip(g["calls"], w["calls"]):
            assert len(gargs) == len(wargs), (name, symbol)
            for k, (ga, wa) in enumerate(zip(gargs, wargs)):
                if ga is None and _empty_panel(wa) and symbol in NULL_FOR_EMPTY:
                    nulled += 1
                    continue
                assert ga == wa, (name, symbol, k)
    assert nulled > 0


def test_the_entries_that_now_get_null_read_no_empty_panel():
    csrc = os.path.join(PKG, "csrc")
    for fname, line in HOST_SEQUENCE_GUARDS:
        assert open(os.path.join(csrc, fname)).read().count(line) == 1, line
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "return cclqr_riccati_weights(nprob, mx, mu, ml, A, Bu, Bl, G, 1, Q, R, N, tol, K, kbreak, opts);" in capi
    assert "return cclqr_riccati_value(nprob, mx, mu, ml, A, Bu, Bl, G, n_weights, Q, R, N, tol, 0, K, nullptr, kbreak, opts);" in capi
    assert "return cclqr_riccati_value(1, mx, mu, ml, A, Bu, Bl, G, 1, Q, R, N, tol, 1, K, nullptr, kbreak, nullptr);" in capi


def test_one_copy_each():
    capi = open(os.path.join(PKG, "_capi.py")).read()
    lqr = open(os.path.join(PKG, "lqr.py")).read()
    # the model reshape (flat and [nprob][nlin] form), the gain-table check and the weight pair
    assert len(re.findall(r"\.shape\[-1\] if \w+\.ndim > 1 else -1", capi)) <= 2 and len(re.findall(r"A\.reshape\(-1, mx, mx\)", capi)) <= 2
    assert len(re.findall(r"mx, -1\)+ if \w+\.size else", capi)) <= 2
    assert len(re.findall(r"K\.shape\[-2:\] != \(mu, mx\)", capi)) <= 2
    assert len(re.findall(r"Q\)?\.reshape\(-1", capi)) <= 2 and len(re.findall(r"R\)?\.reshape\(nw, mu, mu\)", capi)) <= 2
    assert capi.count("def __del__") == 1
    assert len(re.findall(r"^def _d\(|^def _i\(", capi, re.M)) == 2 and capi.count(".ctypes.data_as(") == 2, "_d and _i: the only places where an array becomes a pointer"
    assert lqr.count("def _value_handle") <= 3
    assert lqr.count("is not a Controller: it holds costs-to-go") == 1
    assert lqr.count("noise_scale and Wu are both given") == 1
    assert lqr.count("that is rolled out starts at plant 0") == 1
