"""Shared by tests/test_quantiles_host.py and tests/test_gpu_quantiles.py: the definition of cclqr_rollout_quantiles restated in numpy float64 on
ensemble_common.rows_of's x, the host emulation of the select kernel's per-lane functions (tests/emu/emu_quantiles.cpp) and the device call on a synthetic case.

The definition (include/cclqr.h).  Per step and coordinate s_0 <= ... <= s_{cnt-1} are the FINITE values over the instances, sorted as numbers with -0.0 before +0.0;
    h = p (cnt - 1),  lo = floor(h),  g = h - lo,  hi = min(lo + 1, cnt - 1),  q = s_lo + g (s_hi - s_lo)
in float64 as written (numpy does not fuse a multiply into an add, so the formula is reproducible); g = 0 gives s_lo itself, bit for bit; cnt = 0 gives NaN."""
import ctypes as C

import numpy as np

import ensemble_common as ec
from build_common import host_library

PROBS = (0.0, 1.0, 0.5, 0.05, 0.95, 1.0 / 3.0)
MAX_INST, MAX_PROBS = 16384, 16


def sorted_finite(v):
    """the finite entries of the 1-d array v in numeric order, -0.0 before +0.0"""
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return v[np.lexsort((~np.signbit(v), v))]      # (np.sort leaves the order of -0.0 and +0.0 open: the sign bit breaks the tie)


def quantile_of_sorted(s, p):
    cnt = len(s)
    if cnt == 0:
        return np.nan
    h = np.float64(p) * np.float64(cnt - 1)
    lo = int(np.floor(h))
    g = h - np.float64(lo)
    hi = min(lo + 1, cnt - 1)
    if g == 0.0:
        return s[lo]
    with np.errstate(over="ignore", invalid="ignore"):
        d = s[hi] - s[lo]
        gd = g * d
        return s[lo] + gd


def quantiles_of(x, probs):
    """x [steps][n][nx] -> (quant [steps][n_prob][nx], finite [steps][nx] int32)"""
    steps, _, nx = x.shape
    q, cnt = np.full((steps, len(probs), nx), np.nan), np.zeros((steps, nx), dtype=np.int32)
    for r in range(steps):
        for c in range(nx):
            s = sorted_finite(x[r, :, c])
            cnt[r, c] = len(s)
            for j, p in enumerate(probs):
                q[r, j, c] = quantile_of_sorted(s, p)
    return q, cnt


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_quantiles(got, finite, case, probs, k0=1, first_instance=0, what=""):
    """an order statistic is 1-Lipschitz in the sup norm of its data, and so is an interpolation between two of them: |got - ref| <= RTOL max_i xm_i per (row,
    coordinate), RTOL and xm those of ensemble_common; every value counted"""
    x, xm = ec.rows_of(case["traj"], case["zd"], case["K"], case["N"], k0=k0, first_instance=first_instance)
    ref, cnt = quantiles_of(x, probs)
    bound = ec.RTOL * xm.max(axis=1)[:, None, :]
    err = np.abs(got - ref)
    assert np.isfinite(got).all() and (err <= bound).all(), "%s: |got - ref| max %.3g, worst ratio to the bound %.3g" % (what, err.max(), (err / np.maximum(bound, 1e-300)).max())
    if finite is not None:
        assert np.array_equal(finite, cnt) and (cnt == x.shape[1]).all(), what
    return x, xm


def emu_quantiles():
    """tests/emu/emu_quantiles.cpp, compiled for the host"""
    return host_library("libemu_quantiles.so", ["emu/emu_quantiles.cpp"])


def emu_quantiles_run(lib, v, probs):
    """the select kernel's per-lane functions on one coordinate's values: (quant [n_prob], finite)"""
    dp = C.POINTER(C.c_double)
    v, p = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(probs, dtype=np.float64)
    q, cnt = np.full(len(p), 7.0), C.c_int(-1)
    lib.emu_quantiles.restype = C.c_int
    rc = lib.emu_quantiles(C.c_longlong(len(v)), v.ctypes.data_as(dp), C.c_int(len(p)), p.ctypes.data_as(dp), q.ctypes.data_as(dp), C.byref(cnt))
    assert rc == 0
    return q, cnt.value


def gpu_quantiles(cclqr, mech, case, cj, probs, k0=1, first_instance=0, slab=None, ws_bytes=None, calls=1, with_finite=True):
    """the controller of `case` on the device and `calls` identical cclqr_rollout_quantiles launches over `slab` (default: the case's whole slab) into buffers full of
    NaN / -1, with a workspace of ws_bytes (default: full_bytes; "min" = min_bytes); returns (quant [steps][n_prob][12 nb + mu], finite [steps][12 nb + mu])"""
    import torch
    capi = cclqr._capi
    nb = mech.tables.nb
    n_ctrl = case["zd"].shape[0]
    K = case["K"]
    mu = len(cj)
    ctrl = capi.CtrlHandle(mech, cj, K=None if K is None else K.reshape(-1, mu, 12 * nb), N=case["N"], zd=case["zd"].reshape(-1, nb, 13), n_ctrl=n_ctrl if n_ctrl > 1 else 0)
    try:
        traj = torch.from_numpy(np.ascontiguousarray(case["traj"] if slab is None else slab)).cuda()
        n, steps = traj.shape[:2]
        nx = 12 * nb + mu
        lo, full = capi.rollout_quantiles_ws_bytes(mech, mu, n, steps)
        assert 0 < lo <= full and full == lo * steps and lo % 8 == 0
        wb = full if ws_bytes is None else (lo if ws_bytes == "min" else int(ws_bytes))
        for _ in range(calls):
            quant = torch.full((steps, len(probs), nx), float("nan"), dtype=torch.float64, device="cuda")
            fin = torch.full((steps, nx), -1, dtype=torch.int32, device="cuda")
            ws = torch.full((wb // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
            capi.rollout_quantiles(mech, ctrl, n, steps, k0, traj.data_ptr(), probs, quant.data_ptr(), fin.data_ptr() if with_finite else 0, ws.data_ptr(), wb,
                                   stream=torch.cuda.current_stream().cuda_stream, first_instance=first_instance)
            torch.cuda.synchronize()
        return quant.cpu().numpy(), fin.cpu().numpy()
    finally:
        ctrl.close()
