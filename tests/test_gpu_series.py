"""GPU tests of cclqr_series_ensemble / cclqr_series_quantiles (csrc/joints.hip in front of ens_finish_kernel / ens_select_kernel): the statistics of any
per-instance series [n_inst][steps][nc] across its instances against the numpy definitions (joints_common.series_moments, quantile_common.quantiles_of) within
ensemble_common's bounds, on series with ties, signed zeros, Inf and NaN; extremes bit for bit; bits independent of the workspace, a second call and the
instance order; one instance; the refusals."""
import numpy as np
import pytest

import ensemble_common as ec
import joints_common as jc
import quantile_common as qc

pytestmark = pytest.mark.gpu

PROBS = qc.PROBS


def _series(n, steps, nc, seed):
    """random values of mixed scale; a tied column, a column of signed zeros, a column with |mean| >> spread; Inf and NaN planted (n > 2)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, steps, nc)) * 10.0 ** rng.integers(-2, 3, size=(1, 1, nc))
    x[:, :, 0] = rng.integers(-2, 3, size=(n, steps))
    if nc > 3:
        x[:, :, 1] = rng.choice(np.array([0.0, -0.0]), size=(n, steps))
        x[:, :, 2] = 1.0 + 1e-6 * rng.normal(size=(n, steps))
    if n > 2:
        x[n // 2, 0, nc - 1], x[1, steps - 1, nc // 2], x[n - 1, steps - 1, nc // 2] = np.nan, np.inf, -np.inf
    return np.ascontiguousarray(x)


def _moments(cclqr, x, calls=1):
    import torch
    capi = cclqr._capi
    n, steps, nc = x.shape
    d = torch.from_numpy(x).cuda()
    wb = capi.series_ensemble_ws_bytes(n, steps, nc)
    assert wb > 0 and wb % 8 == 0
    for _ in range(calls):
        mean = torch.full((steps, nc), float("nan"), dtype=torch.float64, device="cuda")
        m2 = torch.full((steps, nc), float("nan"), dtype=torch.float64, device="cuda")
        ws = torch.full((wb // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        capi.series_ensemble(n, steps, nc, d.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return mean.cpu().numpy(), m2.cpu().numpy()


def _quantiles(cclqr, x, probs=PROBS, ws_bytes=None, calls=1, with_finite=True):
    import torch
    capi = cclqr._capi
    n, steps, nc = x.shape
    d = torch.from_numpy(x).cuda()
    lo, full = capi.series_quantiles_ws_bytes(n, steps, nc)
    assert 0 < lo <= full and full == lo * steps and lo % 8 == 0
    wb = full if ws_bytes is None else (lo if ws_bytes == "min" else int(ws_bytes))
    for _ in range(calls):
        quant = torch.full((steps, len(probs), nc), float("nan"), dtype=torch.float64, device="cuda")
        fin = torch.full((steps, nc), -1, dtype=torch.int32, device="cuda")
        ws = torch.full((wb // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        capi.series_quantiles(n, steps, nc, d.data_ptr(), probs, quant.data_ptr(), fin.data_ptr() if with_finite else 0, ws.data_ptr(), wb,
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return quant.cpu().numpy(), fin.cpu().numpy()


@pytest.mark.parametrize("nc,n", [(1, 1), (1, 257), (34, 64), (34, 65), (34, 1025), (128, 65), (128, 257), (130, 3)])
def test_series_statistics_meet_the_definitions(cclqr, nc, n):
    steps = 3
    x = _series(n, steps, nc, seed=nc + n)
    mean, M2 = _moments(cclqr, x)
    rm, rq, Am, Aq = jc.series_moments(x)
    ec.assert_close(mean, rm, Am, "mean nc %d n %d" % (nc, n))
    ec.assert_close(M2, rq, Aq, "M2 nc %d n %d" % (nc, n))
    assert not np.isinf(mean).any() and not np.isinf(M2).any()
    if n > 2:
        assert np.isnan(mean[0, nc - 1]) and np.isnan(mean[steps - 1, nc // 2]) and np.isnan(mean).sum() == 2
    quant, fin = _quantiles(cclqr, x)
    jc.assert_series_quantiles(quant, fin, x, PROBS, "quantiles nc %d n %d" % (nc, n))
    s = np.where(np.isfinite(x), x, np.nan)
    with np.errstate(all="ignore"):
        lo, hi = np.nanmin(s, axis=0), np.nanmax(s, axis=0)
    assert np.array_equal(quant[:, 0], lo) and np.array_equal(quant[:, 1], hi)      # p = 0, 1: the extremes themselves
    if n == 1:
        assert qc.same_bits(mean, x[0]) and (M2 == 0).all() and all(qc.same_bits(quant[:, j], x[0]) for j in range(len(PROBS)))


def test_bits_do_not_depend_on_the_workspace_a_second_call_or_the_instance_order(cclqr):
    n, steps, nc = 257, 5, 34
    x = _series(n, steps, nc, seed=7)
    mean, M2 = _moments(cclqr, x)
    again = _moments(cclqr, x, calls=2)
    assert qc.same_bits(mean, again[0]) and qc.same_bits(M2, again[1])
    quant, fin = _quantiles(cclqr, x)
    lo, full = cclqr._capi.series_quantiles_ws_bytes(n, steps, nc)
    for wb in ("min", 2 * lo + 8, full + 4096):
        q2, f2 = _quantiles(cclqr, x, ws_bytes=wb)
        assert qc.same_bits(quant, q2) and np.array_equal(fin, f2), wb
    q2, f2 = _quantiles(cclqr, x, calls=2)
    assert qc.same_bits(quant, q2) and np.array_equal(fin, f2)
    perm = np.random.default_rng(1).permutation(n)
    q3, f3 = _quantiles(cclqr, np.ascontiguousarray(x[perm]), with_finite=False)
    assert qc.same_bits(quant, q3) and (f3 == -1).all()


def test_refusals(cclqr):
    import torch
    capi = cclqr._capi
    n, steps, nc = 9, 2, 5
    x = torch.zeros((n, steps, nc), dtype=torch.float64, device="cuda")
    out = torch.full((steps, 16, nc), float("nan"), dtype=torch.float64, device="cuda")
    out2 = torch.full((steps, nc), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
    for a, cause in (((0, steps, nc), "n_inst"), ((n, 0, nc), "steps"), ((n, steps, 0), "nc"), ((n, steps, 1025), "CCLQR_SERIES_MAX_COORDS")):
        with pytest.raises(capi.CclqrError, match=cause):
            capi.series_ensemble_ws_bytes(*a)
        with pytest.raises(capi.CclqrError, match=cause):
            capi.series_quantiles_ws_bytes(*a)
        with pytest.raises(capi.CclqrError, match=cause):
            capi.series_ensemble(*a, x.data_ptr(), out.data_ptr(), out2.data_ptr(), ws.data_ptr(), 8 * 4096)
    with pytest.raises(capi.CclqrError, match="16384") as e:
        capi.series_quantiles_ws_bytes(16385, steps, nc)
    assert e.value.code == capi.EUNSUPPORTED
    assert capi.series_ensemble_ws_bytes(16385, steps, nc) > 0      # the moments take any batch
    ens = lambda **k: capi.series_ensemble(n, steps, nc, k.get("x", x.data_ptr()), k.get("mean", out.data_ptr()), k.get("m2", out2.data_ptr()), k.get("ws", ws.data_ptr()),
                                           k.get("wb", 8 * 4096))
    qnt = lambda **k: capi.series_quantiles(n, steps, nc, k.get("x", x.data_ptr()), k.get("probs", (0.5,)), k.get("quant", out.data_ptr()), 0, k.get("ws", ws.data_ptr()),
                                            k.get("wb", 8 * 4096))
    for f, k, cause in ((ens, dict(x=0), "null"), (ens, dict(mean=0), "null"), (ens, dict(m2=0), "null"), (ens, dict(ws=0), "null workspace"), (ens, dict(wb=8), "too small"),
                        (ens, dict(ws=ws.data_ptr() + 4), "aligned"), (qnt, dict(x=0), "null"), (qnt, dict(quant=0), "null"), (qnt, dict(ws=0), "null workspace"),
                        (qnt, dict(wb=8), "too small"), (qnt, dict(ws=ws.data_ptr() + 4), "aligned"), (qnt, dict(probs=()), "n_prob|null"),
                        (qnt, dict(probs=tuple(np.linspace(0, 1, 17))), "n_prob"), (qnt, dict(probs=(0.5, 1.5)), r"\[0, 1\]"), (qnt, dict(probs=(float("nan"),)), r"\[0, 1\]")):
        with pytest.raises(capi.CclqrError, match=cause) as e:
            f(**k)
        assert e.value.code == capi.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(out2).all() and torch.isnan(ws).all()
