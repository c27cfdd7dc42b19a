"""What the six raw analysis entry points of csrc/capi.hip refuse as CCLQR_EINVAL, pinned without a device: cclqr_policy_value, cclqr_policy_value_doubling,
cclqr_covariance_doubling, cclqr_covariance_tracking, cclqr_policy_value_tracking and cclqr_riccati_doubling.  Every refusal of theirs comes before the first HIP call,
so the library answers them on a machine without a GPU.  The cases are the lists the GPU tests run (refusal_call / refusal_cases of the *_common.py modules); here each
is held to its return code, to the FULL sentence of cclqr_last_error() and to sentinel-filled outputs left untouched, and pairs of faults present at once are held to
the sentence that wins.  A rewrite of the host code that changes a wording or the order of two refusals fails here.

No call in this file is valid: a valid call reaches HIP.  The arrays are zeros of the smallest sizes at which every case of the lists IS a refusal: nprob = 3 (the
lists pass counts of 2 and 0 as the bad ones), mu = 2 (a 1 x 1 R cannot fail to be symmetric), ml = 1 (a null Bl is refused only when ml > 0), mx = 4, N = 11.

TEXTS was recorded from the library before the host sequences of these entry points were merged into shared functions."""
import os

import numpy as np
import pytest

import covariance_common as cc
import policy_doubling_common as pdc
import policy_value_common as pvc
import riccati_doubling_common as rdc
import tracking_covariance_common as tc
import tracking_policy_common as tp

NPROB, MX, MU, ML, N = 3, 4, 2, 1, 11

_N_GAINS_TABLE = "n_gains = %d: the gains are one table shared by all (1) or one table per problem (3)"
_N_GAINS_ONE = "n_gains = %d: one gain shared by all (1) or one per problem (3)"
_N_WEIGHTS = "n_weights = %d: the weights are one pair shared by all (1) or one pair per problem (3)"
_N_NOISE_BOTH = "n_noise = %d: Wu / Sigma0 are one shared by all (1) or one per problem (3)"
_NK_STEP = "nK = %d: a gain table holds one row (a stationary gain) or N - 1 = 10 rows, one per backward step"
_NK_KNOT = "nK = %d: a gain table holds one row (a stationary gain) or N - 1 = 10 rows, one per knot 0 .. N-2"
_NLIN = "nlin = %d: one time-invariant model (1) or one per knot 0 .. N-2 (10)"
_LEVELS = "max_levels = %d: 1 .. 60 (2^max_levels steps)"
_TOL = "tol is negative or not a number"
_TOO_MANY = "nprob = 65536: at most 65535 problems per call (they are the y extent of the launch grids)"
_WU_MU0 = "Wu is given with mu = 0: there is no input for the noise to enter through"
_NO_SOURCE = "Wu and Sigma0 are both null: there is no covariance to propagate"
_N_DBL = "N = -1: a horizon of N >= 1 knots, or 0 = to convergence"
_POL_PATH, _POL_BF16 = "policy evaluation options: path in 0..2", "policy evaluation runs in fp64 only (bf16_terms = 0)"

TEXTS = {
    "policy_value": dict(
        n_gains_2=_N_GAINS_TABLE % 2, n_gains_0=_N_GAINS_TABLE % 0, nK_2=_NK_STEP % 2, nK_0=_NK_STEP % 0, nK_N=_NK_STEP % 11, n_weights_2=_N_WEIGHTS % 2,
        n_weights_0=_N_WEIGHTS % 0, N_0="bad sizes", path_3=_POL_PATH, path_neg=_POL_PATH, bf16=_POL_BF16, nprob_0="bad sizes", A_null="null argument",
        P_null="null argument", K_null="null argument"),
    "policy_doubling": dict(
        N_neg=_N_DBL, levels_0=_LEVELS % 0, levels_61=_LEVELS % 61, tol_neg=_TOL, tol_nan=_TOL, tol_nan_conv=_TOL, n_gains_2=_N_GAINS_ONE % 2, n_gains_0=_N_GAINS_ONE % 0,
        n_weights_2=_N_WEIGHTS % 2, n_weights_0=_N_WEIGHTS % 0, path_3=_POL_PATH, path_neg=_POL_PATH, bf16=_POL_BF16, nprob_0="bad sizes", A_null="null argument",
        P_null="null argument", K_null="null argument"),
    "covariance": dict(
        N_neg=_N_DBL, levels_0=_LEVELS % 0, levels_61=_LEVELS % 61, tol_neg=_TOL, tol_nan=_TOL, n_gains_2=_N_GAINS_ONE % 2, n_weights_2=_N_WEIGHTS % 2,
        n_weights_0=_N_WEIGHTS % 0, path_3=_POL_PATH, bf16=_POL_BF16, nprob_0="bad sizes", A_null="null argument", S_null="null argument", K_null="null argument",
        n_noise_2=_N_NOISE_BOTH % 2, n_noise_0=_N_NOISE_BOTH % 0, no_source=_NO_SOURCE, cost_without_Q="cost is asked for without Q / R",
        cost_without_R="cost is asked for without Q / R", Wu_with_mu_0=_WU_MU0,
        start_with_N_0="N = 0 with Sigma0: a steady state does not depend on the start (pass Sigma0 = NULL)"),
    "tracking_covariance": dict(
        nprob_0="bad sizes", mx_0="bad sizes", N_0="bad sizes", nlin_2=_NLIN % 2, nlin_0=_NLIN % 0, n_gains_2=_N_GAINS_TABLE % 2, nK_2=_NK_KNOT % 2,
        n_weights_2=_N_WEIGHTS % 2, n_weights_0=_N_WEIGHTS % 0, n_noise_2=_N_NOISE_BOTH % 2, n_noise_0=_N_NOISE_BOTH % 0, no_source=_NO_SOURCE, Wu_with_mu_0=_WU_MU0,
        cost_without_Q="cost / total are asked for without Q / R", total_without_R="cost / total are asked for without Q / R", A_null="null argument",
        K_null="null argument", Bl_null="null argument", path_3="tracking covariance options: path in 0..2", path_neg="tracking covariance options: path in 0..2",
        bf16="the tracking covariance runs in fp64 only (bf16_terms = 0)", too_many=_TOO_MANY),
    "tracking_policy": dict(
        nprob_0="bad sizes", mx_0="bad sizes", N_0="bad sizes", nlin_2=_NLIN % 2, nlin_0=_NLIN % 0, n_gains_2=_N_GAINS_TABLE % 2, nK_2=_NK_KNOT % 2,
        n_weights_2=_N_WEIGHTS % 2, n_weights_0=_N_WEIGHTS % 0, n_noise_2="n_noise = 2: Wu is one shared by all (1) or one per problem (3)",
        n_noise_0="n_noise = 0: Wu is one shared by all (1) or one per problem (3)",
        price_without_Wu="price / noise_total are asked for without Wu: there is no noise to price",
        total_without_Wu="price / noise_total are asked for without Wu: there is no noise to price", Wu_with_mu_0=_WU_MU0, without_Q="the cost-to-go needs Q / R",
        without_R="the cost-to-go needs Q / R", A_null="null argument", K_null="null argument", Bl_null="null argument",
        path_3="tracking policy value options: path in 0..2", path_neg="tracking policy value options: path in 0..2",
        bf16="the tracking policy value runs in fp64 only (bf16_terms = 0)", too_many=_TOO_MANY),
    "riccati_doubling": dict(
        N_1="N = 1: a horizon of N >= 2 knots, or 0 = to convergence", N_neg="N = -1: a horizon of N >= 2 knots, or 0 = to convergence", levels_0=_LEVELS % 0,
        levels_61=_LEVELS % 61, tol_neg=_TOL, tol_nan=_TOL, tol_nan_conv=_TOL, n_weights_2=_N_WEIGHTS % 4, n_weights_0=_N_WEIGHTS % 0,
        bf16="the Riccati doubling runs in fp64 only (bf16_terms = 0)", nprob_0="bad sizes", mx_0="bad sizes",
        mx_huge="bad sizes: mx = 20000, mu = 2 exceed the LDS panels of the doubling kernels", A_null="null argument", K_null="null argument",
        Q_nonsym="Q or R of weight pair 0 is not symmetric: the composition of Riccati maps holds for exactly symmetric weights only",
        R_nonsym="Q or R of weight pair 0 is not symmetric: the composition of Riccati maps holds for exactly symmetric weights only"),
}

# Two faults at once: (the two cases whose arguments are passed together, the one whose sentence is returned).  The pairs straddle the functions the entry points'
# checks are split into -- the entry's own tests of nulls and sizes, the n_gains test, policy_check / doubling_check / covariance_check / the tracking checks with
# check_n_weights inside them, the path / bf16 pair -- so that merging or reordering those functions shows here.
PRECEDENCE = {
    "policy_value": [("A_null", "nprob_0", "A_null"), ("nprob_0", "n_gains_0", "nprob_0"), ("n_gains_0", "nK_2", "n_gains_0"), ("nK_2", "n_weights_0", "nK_2"),
                     ("n_weights_0", "path_3", "n_weights_0"), ("path_3", "bf16", "path_3")],
    "policy_doubling": [("A_null", "nprob_0", "A_null"), ("nprob_0", "n_gains_0", "nprob_0"), ("n_gains_0", "N_neg", "n_gains_0"), ("N_neg", "tol_neg", "N_neg"),
                        ("levels_0", "tol_nan_conv", "levels_0"), ("tol_neg", "path_3", "tol_neg"), ("path_3", "bf16", "path_3"), ("bf16", "n_weights_0", "bf16"),
                        ("path_neg", "n_weights_2", "path_neg")],
    "covariance": [("A_null", "nprob_0", "A_null"), ("nprob_0", "n_gains_2", "nprob_0"), ("n_gains_2", "N_neg", "n_gains_2"), ("tol_neg", "path_3", "tol_neg"),
                   ("path_3", "n_weights_0", "path_3"), ("n_weights_0", "n_noise_0", "n_weights_0"), ("bf16", "n_noise_2", "bf16"), ("n_noise_0", "no_source", "n_noise_0"),
                   ("no_source", "cost_without_Q", "no_source"), ("Wu_with_mu_0", "cost_without_Q", "Wu_with_mu_0"), ("cost_without_Q", "start_with_N_0", "cost_without_Q")],
    "tracking_covariance": [("nprob_0", "A_null", "nprob_0"), ("A_null", "nlin_2", "A_null"), ("nlin_0", "n_gains_2", "nlin_0"), ("n_gains_2", "nK_2", "n_gains_2"),
                            ("nK_2", "n_weights_0", "nK_2"), ("n_weights_0", "n_noise_0", "n_weights_0"), ("n_noise_0", "path_3", "n_noise_0"),
                            ("n_noise_2", "no_source", "n_noise_2"), ("no_source", "cost_without_Q", "no_source"), ("cost_without_Q", "too_many", "cost_without_Q"),
                            ("too_many", "path_3", "too_many"), ("too_many", "bf16", "too_many"), ("path_3", "bf16", "path_3")],
    "tracking_policy": [("nprob_0", "A_null", "nprob_0"), ("A_null", "nlin_2", "A_null"), ("nlin_0", "n_gains_2", "nlin_0"), ("n_gains_2", "nK_2", "n_gains_2"),
                        ("nK_2", "n_weights_0", "nK_2"), ("n_weights_0", "n_noise_0", "n_weights_0"), ("n_noise_0", "path_3", "n_noise_0"),
                        ("n_noise_2", "price_without_Wu", "n_noise_2"), ("price_without_Wu", "without_Q", "price_without_Wu"), ("without_Q", "too_many", "without_Q"),
                        ("too_many", "path_3", "too_many"), ("too_many", "bf16", "too_many"), ("path_3", "bf16", "path_3")],
    "riccati_doubling": [("A_null", "nprob_0", "A_null"), ("nprob_0", "n_weights_0", "nprob_0"), ("n_weights_0", "N_1", "n_weights_0"), ("N_1", "tol_nan", "N_1"),
                         ("levels_0", "tol_nan_conv", "levels_0"), ("tol_neg", "bf16", "tol_neg"), ("bf16", "mx_huge", "bf16"), ("mx_huge", "Q_nonsym", "mx_huge")],
}


def _problem():
    z = np.zeros
    return dict(nprob=NPROB, mx=MX, mu=MU, ml=ML, N=N, tol=1e-8, A=z((NPROB, MX, MX)), Bu=z((NPROB, MX, MU)), Bl=z((NPROB, MX, ML)), G=z((NPROB, ML, MX)),
                K=z((N - 1, MU, MX)), Q=z((MX, MX)), R=z((MU, MU)), Wu=z((MU, MU)), Sigma0=z((MX, MX)))


def _tracked():
    z = np.zeros
    return dict(_problem(), A=z((NPROB, N - 1, MX, MX)), Bu=z((NPROB, N - 1, MX, MU)), Bl=z((NPROB, N - 1, MX, ML)), G=z((NPROB, N - 1, ML, MX)),
                K=z((NPROB, N - 1, MU, MX)))


def _entries(capi):
    """entry -> (call, cases)"""
    pr, tr = _problem(), _tracked()
    stationary = dict(pr, K=np.zeros((MU, MX)))
    return {"policy_value": (pvc.refusal_call(capi, pr), pvc.refusal_cases(pr)),
            "policy_doubling": (pdc.refusal_call(capi, stationary), pdc.refusal_cases()),
            "covariance": (cc.refusal_call(capi, stationary), cc.refusal_cases()),
            "tracking_covariance": (tc.refusal_call(capi, tr, N), tc.refusal_cases()),
            "tracking_policy": (tp.refusal_call(capi, tr, N), tp.refusal_cases()),
            "riccati_doubling": (rdc.refusal_call(capi, pr), rdc.refusal_cases(pr))}


@pytest.fixture(scope="module")
def entries(cclqr):
    import __graft_entry__ as graft
    if not os.path.exists(cclqr._capi.LIB_PATH):
        graft.build()
    return _entries(cclqr._capi)


@pytest.mark.parametrize("entry", sorted(TEXTS))
def test_every_refusal_code_sentence_and_untouched_outputs(cclqr, entries, entry):
    call, cases = entries[entry]
    assert sorted(cases) == sorted(TEXTS[entry]), "the list of the GPU test and the table of sentences name different cases"
    for what, kw in cases.items():
        rc, untouched, msg = call(**kw)
        print("%s %s: %d %r" % (entry, what, rc, msg))
        assert rc == cclqr._capi.EINVAL and untouched and msg == TEXTS[entry][what], (entry, what, rc, untouched, msg)


@pytest.mark.parametrize("entry", sorted(PRECEDENCE))
def test_which_of_two_refusals_wins(cclqr, entries, entry):
    call, cases = entries[entry]
    assert len(PRECEDENCE[entry]) >= 3
    for a, b, winner in PRECEDENCE[entry]:
        assert winner in (a, b) and TEXTS[entry][a] != TEXTS[entry][b]
        rc, untouched, msg = call(**dict(cases[a], **cases[b]))
        print("%s %s + %s: %d %r" % (entry, a, b, rc, msg))
        assert rc == cclqr._capi.EINVAL and untouched and msg == TEXTS[entry][winner], (entry, a, b, rc, untouched, msg)
