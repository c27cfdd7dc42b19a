"""cclqr_riccati_weights on the device: one (Q, R) per problem through every Riccati kernel that reads the weights (tests/riccati_weights_common.py; the CPU twin
tests/test_riccati_weights_reference.py shows that the cases cannot pass vacuously).  Each case runs on every path its shape has and must give
  * per problem, against the extended-precision reference under THAT problem's weights: kbreak equal, max|K - Kref| <= tolerance(e64) max|Kref|, the back-filled
    rows bitwise K[kbreak - 1];
  * bitwise (all-symmetric cases): problem p of the per-problem call = problem p of cclqr_riccati_ex on the same nprob models with (Q_p, R_p) shared, same path --
    the kernels, the batch and the arithmetic are the same, only the address of the weights differs;
  * n_weights = 1 bitwise cclqr_riccati_ex; with keep_last bitwise row 0 of the full table."""
import numpy as np
import pytest

from riccati_weights_common import CASES, build_case, check_gains

pytestmark = pytest.mark.gpu


def _models(pr):
    return pr["A"], pr["Bu"], pr["Bl"], pr["G"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_per_problem_weights_against_extended_precision_and_the_shared_call(cclqr, c):
    capi = cclqr._capi
    pr = build_case(c["name"])
    N, tol, nprob = pr["N"], pr["tol"], pr["nprob"]
    for path in c["paths"]:
        K, kb = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path)
        for p in range(nprob):
            check_gains(K[p], int(kb[p]), pr["ref"][p], "%s path %d problem %d" % (c["name"], path, p))
        Kl, kbl = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], N, tol=tol, path=path, keep_last=True)
        assert np.array_equal(kbl, kb) and np.array_equal(Kl[:, 0], K[:, 0]), "%s path %d: keep_last differs from row 0 of the full table" % (c["name"], path)
        if not pr["symmetric"]:
            continue
        for p in range(nprob):
            Ks, kbs = capi.riccati(*_models(pr), pr["Q"][p], pr["R"][p], N, tol=tol, path=path)
            assert kbs[p] == kb[p] and np.array_equal(Ks[p], K[p]), "%s path %d problem %d: not bitwise the shared-weights call with its pair" % (c["name"], path, p)
            if p == 0:      # n_weights = 1 is cclqr_riccati_ex
                K1, kb1 = capi.riccati_weights(*_models(pr), pr["Q"][:1], pr["R"][:1], N, tol=tol, path=path)
                assert np.array_equal(kb1, kbs) and np.array_equal(K1, Ks), "%s path %d: n_weights = 1 differs from cclqr_riccati_ex" % (c["name"], path)


@pytest.mark.parametrize("path", [1, 2])
def test_bf16_mode_reads_each_problems_weights(cclqr, path):
    """the measured-error mode (bf16_terms = 2: Q fetched behind the tile on the resident kernel) compared only with itself: problem p of the per-problem call is
    bitwise problem p of the shared-weights call with (Q_p, R_p)"""
    capi = cclqr._capi
    pr = build_case("w_frag_1_6")
    K, kb = capi.riccati_weights(*_models(pr), pr["Q"], pr["R"], pr["N"], tol=pr["tol"], path=path, bf16_terms=2)
    assert np.isfinite(K).all()
    for p in range(pr["nprob"]):
        Ks, kbs = capi.riccati(*_models(pr), pr["Q"][p], pr["R"][p], pr["N"], tol=pr["tol"], path=path, bf16_terms=2)
        assert kbs[p] == kb[p] and np.array_equal(Ks[p], K[p]), (path, p)
    assert not np.array_equal(K[0], K[1])


def test_a_weight_count_that_is_neither_one_nor_the_problem_count_is_refused(cclqr):
    """n_weights = 2 with nprob = 3: CCLQR_EINVAL naming both numbers, K untouched"""
    capi = cclqr._capi
    pr = build_case("w_frag_1_3")
    K = np.full((3, pr["N"] - 1, pr["mu"], pr["mx"]), 7.25)
    with pytest.raises(capi.CclqrError) as e:
        capi.riccati_weights(*_models(pr), pr["Q"][:2], pr["R"][:2], pr["N"], tol=pr["tol"], K=K)
    assert e.value.code == capi.EINVAL and "n_weights = 2" in str(e.value) and "(3)" in str(e.value)
    assert (K == 7.25).all()
