"""What the Python binding hands the library, recorded without one: record(pkg, setattr) replaces _capi.lib by a stub whose every cclqr_* symbol notes its name and
arguments and returns OK, and _capi._d / _capi._i by versions whose pointers carry a tag (dtype, shape, a hash of the bytes), then drives the array-level functions,
the handles and the public classes of lqr.py on small seeded inputs.  Per case: the calls, the structure of what came back, and for objects the public attributes.
tests/test_capi_marshalling.py compares the tree's record with tests/golden/capi_calls_parent.json, which

    python tests/capi_recorder.py <directory of the package at the parent commit> tests/golden/capi_calls_parent.json

wrote from the commit before the binding's helpers were shared."""
import ctypes as C
import hashlib
import importlib.util
import json
import math
import os
import sys

import numpy as np

_BASE = {"d": C.POINTER(C.c_double), "i": C.POINTER(C.c_int32)}


class _TagD(_BASE["d"]):
    _type_ = C.c_double


class _TagI(_BASE["i"]):
    _type_ = C.c_int32


def _tag(a):
    return "%s%s%s #%s" % (a.dtype, list(a.shape), "" if a.flags.c_contiguous else " strided", hashlib.sha1(a.tobytes()).hexdigest()[:10])


class Recorder:
    def __init__(self, pkg, setattr_):
        self.pkg, self.capi = pkg, pkg._capi
        self.calls, self.handles, self.by_address, self.last_pointers = [], set(), {}, []
        setattr_(self.capi, "lib", lambda: self)
        setattr_(self.capi, "_d", lambda a: self._pointer(a, "d", _TagD, np.float64))
        setattr_(self.capi, "_i", lambda a: self._pointer(a, "i", _TagI, np.int32))

    # the stub library
    def __getattr__(self, name):
        if not name.startswith("cclqr_"):
            raise AttributeError(name)
        if name == "cclqr_last_error":
            return lambda: b""
        if name == "cclqr_version":
            return lambda: self.capi.ABI_VERSION

        def call(*args):
            frame = sys._getframe(1)
            while frame is not None:      # a finaliser's destroy falls into whichever case is running when the object dies: not part of any case
                if frame.f_code.co_name == "__del__":
                    return self.capi.OK
                frame = frame.f_back
            self.last_pointers = [a for a in args if isinstance(a, (_TagD, _TagI))]
            self.calls.append([name, [self._norm(a) for a in args]])
            return self.capi.OK
        return call

    def _pointer(self, a, kind, cls, dtype):
        if a is None:
            return None
        assert isinstance(a, np.ndarray) and a.dtype == dtype, (type(a), getattr(a, "dtype", None))
        p = C.cast(a.ctypes.data_as(_BASE[kind]), cls)
        p.tag, p.arr = _tag(a), a
        self.by_address[a.ctypes.data] = p.tag
        return p

    def _struct(self, s):
        out = {}
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ in (_BASE["d"], _BASE["i"]):
                addr = C.cast(v, C.c_void_p).value
                out[name] = None if not addr else self.by_address.get(addr, "untagged")
            else:
                out[name] = v
        return out

    def _norm(self, a):
        if a is None:
            return None
        if isinstance(a, (_TagD, _TagI)):
            return a.tag
        if type(a).__name__ == "CArgObject":      # byref(x)
            x = a._obj
            if isinstance(x, C.c_void_p):         # a handle the library hands out
                x.value = 0x1000 + 16 * len(self.handles)
                self.handles.add(x.value)
                return "byref(handle)"
            if isinstance(x, C.Structure):
                return {"byref": type(x).__name__, "fields": self._struct(x)}
            return "byref(%s %r)" % (type(x).__name__, x.value)
        if isinstance(a, C.c_void_p):
            return "handle" if a.value in self.handles else "c_void_p %r" % a.value
        if isinstance(a, C._SimpleCData):
            return "%s %r" % (type(a).__name__, a.value)
        raise TypeError("the library was handed a %s" % type(a).__name__)

    # what came back
    def shape_of(self, x):
        if x is None or isinstance(x, (bool, str)):
            return x
        if isinstance(x, np.ndarray):
            return "%s%s" % (x.dtype, list(x.shape))
        if isinstance(x, (tuple, list)):
            return [self.shape_of(v) for v in x] if len(x) <= 12 else "%s of %d" % (type(x).__name__, len(x))
        if isinstance(x, (int, float, np.integer, np.floating)):
            return "%s %r" % (type(x).__name__, x.item() if hasattr(x, "item") else x)
        if hasattr(x, "ptr") and isinstance(getattr(x, "ptr"), C.c_void_p):
            return {"handle": type(x).__name__, "open": bool(x.ptr), "n_tables": getattr(x, "n_tables", None)}
        return type(x).__name__

    def attributes(self, obj):
        return {k: self.shape_of(v) for k, v in sorted(vars(obj).items()) if not k.startswith("_") and k not in ("ptr", "desc")}

    def kept_alive(self, handle):
        """per pointer of the last call: does the handle hold the array it points into?"""
        held = list(getattr(handle, "_arrs", [])) + list(vars(handle).values())
        return [any(p.arr is h for h in held) for p in self.last_pointers]

    def case(self, out, name, fn):
        """run fn(); note its calls and the structure of its result (or the refusal); returns the result"""
        self.calls = []
        entry = {}
        try:
            got = fn()
            entry["returns"] = self.shape_of(got)
            if hasattr(got, "__dict__") and not isinstance(got, np.ndarray):
                entry["attributes"] = self.attributes(got)
                if hasattr(got, "_arrs"):
                    entry["kept_alive"] = self.kept_alive(got)
        except (ValueError, TypeError, AssertionError) as e:
            got = None
            entry["raises"] = [type(e).__name__, str(e)]
        entry["calls"], self.calls = self.calls, []      # (what runs between two cases belongs to neither)
        assert name not in out, name
        out[name] = entry
        return got


def _models(rng, nprob, mx, mu, ml, nlin=None):
    lead = (nprob,) if nlin is None else (nprob, nlin)
    return (rng.normal(size=lead + (mx, mx)), rng.normal(size=lead + (mx, mu)), rng.normal(size=lead + (mx, ml)), rng.normal(size=lead + (ml, mx)))


def _spd(rng, n, size):
    M = rng.normal(size=(n, size, size))
    return M @ M.transpose(0, 2, 1) + np.eye(size)


def array_level(r, out):
    """every array-level function of _capi.py from riccati to riccati_tv"""
    capi, mx = r.capi, 4
    rng = np.random.default_rng(1)
    shapes = {"": (2, 1, 2), "_mu0": (2, 0, 2), "_ml0": (1, 2, 0)}
    for tag, (nprob, mu, ml) in shapes.items():
        N = 4
        refusal = r.case if not tag else (lambda *a: None)      # (the refusals do not depend on an empty panel: once)
        A, Bu, Bl, G = _models(rng, nprob, mx, mu, ml)
        Q, R = _spd(rng, nprob, mx), _spd(rng, nprob, mu)
        r.case(out, "riccati" + tag, lambda: capi.riccati(A, Bu, Bl, G, Q[0], R[0], N, tol=1e-6, path=2, bf16_terms=1))
        r.case(out, "riccati_2d_keep_last" + tag, lambda: capi.riccati(A[0], Bu[0], Bl[0], G[0], Q[0], R[0], N, keep_last=True))
        r.case(out, "riccati_flat_panels_N1" + tag, lambda: capi.riccati(A, Bu.reshape(-1), Bl.reshape(-1), G.reshape(-1), Q[0], R[0], 1))
        r.case(out, "riccati_weights_one" + tag, lambda: capi.riccati_weights(A, Bu, Bl, G, Q[0], R[0], N, path=1))
        r.case(out, "riccati_weights_each_K_given" + tag, lambda: capi.riccati_weights(A, Bu, Bl, G, Q, R, N, keep_last=True, K=np.ones((nprob, 1, mu, mx))))
        refusal(out, "riccati_weights_bad_K" + tag, lambda: capi.riccati_weights(A, Bu, Bl, G, Q, R, N, K=np.ones((nprob, 2, mu, mx))))
        r.case(out, "riccati_value" + tag, lambda: capi.riccati_value(A, Bu, Bl, G, Q, R, N, tol=1e-7, bf16_terms=2))
        r.case(out, "riccati_value_no_P_2d" + tag, lambda: capi.riccati_value(A[0], Bu[0], Bl[0], G[0], Q[0], R[0], N, want_P=False, keep_last=True))
        At, But, Blt, Gt = _models(rng, nprob * (N - 1), mx, mu, ml)
        r.case(out, "riccati_value_time_varying" + tag, lambda: capi.riccati_value(At, But, Blt, Gt, Q[0], R[0], N, time_varying=True))
        r.case(out, "riccati_value_time_varying_4d" + tag, lambda: capi.riccati_value(At.reshape(nprob, N - 1, mx, mx), But, Blt, Gt, Q, R, N, time_varying=True))
        refusal(out, "riccati_value_time_varying_bad_count" + tag, lambda: capi.riccati_value(At[:-1], But[:-1], Blt[:-1], Gt[:-1], Q[0], R[0], N, time_varying=True))
        for nK in (1, N - 1):
            K4 = rng.normal(size=(nprob, nK, mu, mx))
            r.case(out, "policy_value_K4_nK%d%s" % (nK, tag), lambda: capi.policy_value(A, Bu, Bl, G, K4, Q, R, N, tol=1e-6, path=1))
            r.case(out, "policy_value_K3_nK%d_2d_no_diag%s" % (nK, tag), lambda: capi.policy_value(A[0], Bu[0], Bl[0], G[0], K4[0], Q[0], R[0], N, want_diag=False))
        refusal(out, "policy_value_bad_K" + tag, lambda: capi.policy_value(A, Bu, Bl, G, np.zeros((mu + 1, mx)), Q, R, N))
        K3 = rng.normal(size=(nprob, mu, mx))
        r.case(out, "policy_value_doubling_K3" + tag, lambda: capi.policy_value_doubling(A, Bu, Bl, G, K3, Q, R, 0, tol=1e-6, max_levels=30, path=2))
        r.case(out, "policy_value_doubling_K2_2d_no_diag" + tag, lambda: capi.policy_value_doubling(A[0], Bu[0], Bl[0], G[0], K3[0], Q[0], R[0], N, want_diag=False))
        refusal(out, "policy_value_doubling_bad_K" + tag, lambda: capi.policy_value_doubling(A, Bu, Bl, G, np.zeros((1, 1, mu, mx + 1)), Q, R, N))
        Wu, S0 = (_spd(rng, nprob, mu) if mu else [None] * nprob), _spd(rng, nprob, mx)
        Wus = Wu if mu else None
        r.case(out, "covariance_doubling_K3" + tag, lambda: capi.covariance_doubling(A, Bu, Bl, G, K3, Q, R, Wus, S0, N, tol=1e-9, max_levels=20, bf16_terms=1))
        r.case(out, "covariance_doubling_K2_no_Q_steady" + tag,
               lambda: capi.covariance_doubling(A[0], Bu[0], Bl[0], G[0], K3[0], None, None, Wu[0], None, 0, want_cost=False, want_std=False, want_diag=False))
        r.case(out, "covariance_doubling_one_Wu_many_Sigma0" + tag, lambda: capi.covariance_doubling(A, Bu, Bl, G, K3, Q[0], R[0], Wu[0], S0, N))
        refusal(out, "covariance_doubling_bad_K" + tag, lambda: capi.covariance_doubling(A, Bu, Bl, G, np.zeros(mx), Q, R, Wus, S0, N))
        refusal(out, "covariance_doubling_bad_Wu" + tag, lambda: capi.covariance_doubling(A, Bu, Bl, G, K3, Q, R, np.zeros((mu + 1, mu + 1)), S0, N))
        r.case(out, "riccati_doubling" + tag, lambda: capi.riccati_doubling(A, Bu, Bl, G, Q, R, 0, tol=1e-6, max_levels=25, bf16_terms=1))
        r.case(out, "riccati_doubling_2d_no_P_no_diag" + tag, lambda: capi.riccati_doubling(A[0], Bu[0], Bl[0], G[0], Q[0], R[0], N, want_P=False, want_diag=False))
        r.case(out, "riccati_doubling_K_P_given" + tag,
               lambda: capi.riccati_doubling(A, Bu, Bl, G, Q[0], R[0], N, K=np.ones((nprob, mu, mx)), P=np.ones((nprob, mx, mx)), want_P=False))
        refusal(out, "riccati_doubling_bad_K" + tag, lambda: capi.riccati_doubling(A, Bu, Bl, G, Q, R, N, K=np.ones((nprob, mu + 1, mx))))
        refusal(out, "riccati_doubling_bad_P" + tag, lambda: capi.riccati_doubling(A, Bu, Bl, G, Q, R, N, P=np.ones((nprob, mx))))
        r.case(out, "riccati_tv" + tag, lambda: capi.riccati_tv(At[:N - 1], But[:N - 1], Blt[:N - 1], Gt[:N - 1], Q[0], R[0], N, tol=1e-6))
        for nlin in (1, N - 1):
            A4, Bu4, Bl4, G4 = _models(rng, nprob, mx, mu, ml, nlin)
            for nK in (1, N - 1) if not tag else (N - nlin,):      # (with an empty panel: the two mixed pairs)
                K4 = rng.normal(size=(nprob, nK, mu, mx))
                name = "_nlin%d_nK%d%s" % (nlin, nK, tag)
                r.case(out, "covariance_tracking_K4" + name,
                       lambda: capi.covariance_tracking(A4, Bu4, Bl4, G4, K4, Q, R, Wus, S0, N, path=1, bf16_terms=1, want_all=True))
                r.case(out, "covariance_tracking_K3_no_Q" + name,
                       lambda: capi.covariance_tracking(A4, Bu4, Bl4, G4, K4[0], None, None, Wu[0], None, N, want_cost=False, want_std=False, want_total=False))
                r.case(out, "policy_value_tracking_K4" + name, lambda: capi.policy_value_tracking(A4, Bu4, Bl4, G4, K4, Q, R, Wus, N, path=2, want_all=True))
                r.case(out, "policy_value_tracking_K3_no_Wu" + name, lambda: capi.policy_value_tracking(A4, Bu4, Bl4, G4, K4[0], Q[0], R[0], None, N, want_P=False))
            r.case(out, "covariance_tracking_K2_nlin%d%s" % (nlin, tag), lambda: capi.covariance_tracking(A4, Bu4, Bl4, G4, K3[0], Q[0], R[0], None, S0[0], N))
            r.case(out, "policy_value_tracking_K2_nlin%d%s" % (nlin, tag),
                   lambda: capi.policy_value_tracking(A4, Bu4, Bl4, G4, K3[0], Q, R, Wu[0], N, want_price=False, want_total=False))
        refusal(out, "covariance_tracking_bad_K" + tag, lambda: capi.covariance_tracking(A4, Bu4, Bl4, G4, np.zeros((mu, mx + 1)), Q, R, Wus, S0, N))
        refusal(out, "policy_value_tracking_bad_K" + tag, lambda: capi.policy_value_tracking(A4, Bu4, Bl4, G4, np.zeros((1, 1, 1, mu, mx)), Q, R, Wus, N))
        refusal(out, "covariance_tracking_bad_A" + tag, lambda: capi.covariance_tracking(A, Bu, Bl, G, K3, Q, R, Wus, S0, N))
        refusal(out, "policy_value_tracking_bad_A" + tag, lambda: capi.policy_value_tracking(A4[..., :-1], Bu4, Bl4, G4, K3, Q, R, Wus, N))


def _cartpole(pkg):
    ex = pkg.examples.cartpole_n(1)
    mech = ex["mech"]
    ids, eids = [pkg.getid(b) for b in ex["bodies"]], [pkg.getid(j) for j in ex["ctrl"]]
    return ex, mech, ids, eids


def mechanism_level(r, out):
    """the handles, the five value_create_* functions (host and on_device) and riccati_tracking, on a two-body cartpole"""
    pkg, capi = r.pkg, r.capi
    ex, mech, ids, eids = _cartpole(pkg)
    rng = np.random.default_rng(2)
    dev = r.case(out, "MechHandle", lambda: capi.MechHandle(mech.tables()))
    nb, mx, mu, n, N = 2, 24, 1, 3, 5
    cj = [mech.joint_index(e) for e in eids]
    zd = pkg.examples.cartpole_states(1, rng.uniform(-0.2, 0.2, n), rng.uniform(-0.1, 0.1, (n, 1)))
    Fd = rng.normal(size=(n, mu))
    Q, R = _spd(rng, n, mx), _spd(rng, n, mu)
    plants = r.case(out, "PlantsHandle", lambda: pkg.PlantBatch.scaled(mech, n + 1, mass=(0.8, 1.2), seed=3).handle(dev))
    r.case(out, "PlantsHandle_on_device", lambda: capi.PlantsHandle(dev, mass=0x5000, p1=0x6000, n_plant=4, first_index=2, on_device=True, stream=7))
    for name, kw in (("plain", {}), ("plants", dict(plants=plants, first_plant=1)), ("weights", dict(n_weights=n, Fd=Fd)),
                     ("weights_plants", dict(n_weights=n, plants=plants)), ("value", dict(keep_value=True, infinite_horizon=True)),
                     ("value_weights_plants", dict(keep_value=True, n_weights=n, plants=plants, first_plant=1, Fd=Fd, tol=1e-7))):
        one = "weights" not in name
        h = r.case(out, "BatchLqrHandle_" + name, lambda: capi.BatchLqrHandle(dev, zd, cj, Q[0] if one else Q, R[0] if one else R, N, **kw))
        r.case(out, "BatchLqrHandle_%s_value" % name, lambda: h.value)
        r.case(out, "BatchLqrHandle_%s_gains" % name, lambda: capi.ctrl_gains(dev, h, 1))
        r.case(out, "BatchLqrHandle_%s_close" % name, lambda: (h.close(), h.close(), h.__del__(), h)[3])
    for name, kw in (("plain", {}), ("plants", dict(plants=plants, first_plant=1, N=N, max_levels=12)), ("value", dict(keep_value=True, Fd=Fd, tol=1e-7)),
                     ("value_plants", dict(keep_value=True, plants=plants))):
        h = r.case(out, "BatchLqrDoublingHandle_" + name, lambda: capi.ctrl_create_lqr_batch_doubling(dev, zd, cj, Q if "plants" in name else Q[0], R if "plants" in name else R[0], **kw))
        r.case(out, "BatchLqrDoublingHandle_%s_value" % name, lambda: h.value)
        r.case(out, "BatchLqrDoublingHandle_%s_gains" % name, lambda: capi.ctrl_gains(dev, h, 2))
        r.case(out, "BatchLqrDoublingHandle_%s_close" % name, lambda: (h.close(), h.close(), h)[2])
    ztraj = np.stack([pkg.examples.cartpole_states(1, rng.uniform(-0.2, 0.2, N), rng.uniform(-0.1, 0.1, (N, 1))) for _ in range(n)])
    Ftraj = rng.normal(size=(n, N, mu))
    r.case(out, "BatchTrackingHandle_host", lambda: capi.BatchTrackingHandle(dev, ztraj, cj, Q[0], R[0], Fd=Ftraj, plants=plants, first_plant=1, tol=1e-6))
    r.case(out, "BatchTrackingHandle_host_law", lambda: capi.BatchTrackingHandle(dev, ztraj, cj, Q[0], R[0], fric=[0.1, 0.2], noise_scale=0.5, noise_seed=9, workspace_bytes=1 << 20))
    r.case(out, "BatchTrackingHandle_on_device", lambda: capi.BatchTrackingHandle(dev, 0x7000, cj, Q[0], R[0], Fd=0x8000, n_ctrl=n, N=N, on_device=True, stream=5))
    r.case(out, "BatchTrackingHandle_on_device_no_shape", lambda: capi.BatchTrackingHandle(dev, 0x7000, cj, Q[0], R[0], on_device=True))
    r.case(out, "BatchTrackingHandle_bad_zd", lambda: capi.BatchTrackingHandle(dev, ztraj[0], cj, Q[0], R[0]))
    trk = r.case(out, "BatchTrackingHandle_for_values", lambda: capi.BatchTrackingHandle(dev, ztraj, cj, Q[0], R[0]))
    ctrl = r.case(out, "CtrlHandle", lambda: capi.CtrlHandle(dev, cj, K=rng.normal(size=(1, mu, mx)), N=0, zd=zd[0], Fd=Fd[0], fric=[0.1, 0.2], noise_scale=0.3, noise_seed=4))
    r.case(out, "CtrlHandle_setpoints", lambda: capi.CtrlHandle(dev, cj, K=None, N=0, zd=zd, n_ctrl=n))
    r.case(out, "ValueHandle", lambda: capi.ValueHandle(dev, _spd(rng, 2, mx)))
    r.case(out, "ValueHandle_bad_P", lambda: capi.ValueHandle(dev, np.zeros((mx, mx + 1))))
    r.case(out, "ScoreHandle", lambda: capi.ScoreHandle(dev, rng.normal(size=(nb, 12, 12)), R[0], settle_tol=0.5))
    Wu, S0 = _spd(rng, n, mu), _spd(rng, n, mx)
    for name, kw in (("one_pair", dict(Q=Q[0], R=R[0])), ("each_plants", dict(Q=Q, R=R, Fd=Fd, plants=plants, first_plant=1))):
        r.case(out, "value_create_policy_" + name, lambda: capi.value_create_policy(dev, ctrl, zd, cj, N=N, tol=1e-6, **kw))
        r.case(out, "value_create_policy_doubling_" + name, lambda: capi.value_create_policy_doubling(dev, ctrl, zd, cj, N=0, max_levels=22, **kw))
        r.case(out, "value_create_covariance_doubling_" + name, lambda: capi.value_create_covariance_doubling(dev, ctrl, zd, cj, Wu=Wu, Sigma0=S0[0], N=N, tol=1e-9, **kw))
        r.case(out, "value_create_covariance_doubling_steady_" + name, lambda: capi.value_create_covariance_doubling(dev, ctrl, zd, cj, Wu=Wu[0], Sigma0=None, N=0, **kw))
    for name, kw in (("host", dict(Fd=Ftraj, plants=plants, first_plant=1, workspace_bytes=1 << 22)), ("host_no_Fd", {}),
                     ("on_device", dict(Fd=0x8000, on_device=True, stream=5)), ("on_device_no_Fd", dict(on_device=True, plants=plants))):
        z = 0x7000 if "on_device" in name else ztraj
        r.case(out, "value_create_covariance_tracking_" + name, lambda: capi.value_create_covariance_tracking(dev, trk, z, n, N, cj, Q, R, Wu, S0, **kw))
        r.case(out, "value_create_covariance_tracking_no_noise_" + name, lambda: capi.value_create_covariance_tracking(dev, trk, z, n, N, cj, Q[0], R[0], None, S0[0], **kw))
        r.case(out, "value_create_policy_tracking_" + name, lambda: capi.value_create_policy_tracking(dev, trk, z, n, N, cj, Q, R, Wu, knot=2, **kw))
        r.case(out, "value_create_policy_tracking_no_Wu_" + name, lambda: capi.value_create_policy_tracking(dev, trk, z, n, N, cj, Q[0], R[0], None, **kw))
    r.case(out, "riccati_tracking", lambda: capi.riccati_tracking(dev, cj, ztraj[0], Ftraj[0], Q[0], R[0], N, tol=1e-6, path=1, bf16_terms=1))
    # every handle class: close() destroys once with its own symbol, a second close() and the finaliser find nothing left, and the finaliser alone closes too
    for name, make in (("MechHandle", lambda: capi.MechHandle(mech.tables())), ("PlantsHandle", lambda: capi.PlantsHandle(dev, mass=np.ones((2, nb)))),
                       ("CtrlHandle", lambda: capi.CtrlHandle(dev, cj)), ("ValueHandle", lambda: capi.ValueHandle(dev, np.eye(mx))),
                       ("ScoreHandle", lambda: capi.ScoreHandle(dev, np.ones((nb, 12, 12)), np.eye(mu))),
                       ("BatchTrackingHandle", lambda: capi.BatchTrackingHandle(dev, ztraj, cj, Q[0], R[0]))):
        h, left = make(), make()
        r.case(out, name + "_close_twice", lambda: (h.close(), h.close(), h.__del__(), h)[3])
        r.case(out, name + "_finaliser", lambda: (left.__del__(), left)[1])


def _refusals(r, out, name, obj, dev, value):
    """the private methods simulate and predicted_cost reach a controller or a value table through, and what they refuse"""
    other = r.capi.MechHandle(obj.mechanism.tables())
    if value:
        r.case(out, name + "_P", lambda: obj.P(0))
        r.case(out, name + "_value_handle", lambda: obj._value_handle(dev))
        r.case(out, name + "_value_handle_other_device", lambda: obj._value_handle(other))
        r.case(out, name + "_ctrl_handle", lambda: (obj._ctrl_handle(dev), obj._ctrl_handle(dev))[1])
        r.case(out, name + "_ctrl_handle_law", lambda: obj._ctrl_handle(dev, noise_scale=1.0))
        r.case(out, name + "_ctrl_handle_other_device", lambda: obj._ctrl_handle(other))
    else:
        r.case(out, name + "_gains", lambda: obj.gains(1))
        r.case(out, name + "_P", lambda: obj.P(1))
        r.case(out, name + "_value_handle", lambda: obj._value_handle(dev))
        r.case(out, name + "_value_handle_other_device", lambda: obj._value_handle(other))
        r.case(out, name + "_ctrl_handle", lambda: obj._ctrl_handle(dev))
        r.case(out, name + "_ctrl_handle_fric", lambda: obj._ctrl_handle(dev, fric=np.zeros(2)))
        r.case(out, name + "_ctrl_handle_noise", lambda: obj._ctrl_handle(dev, noise_seed=0))
        r.case(out, name + "_ctrl_handle_other_device", lambda: obj._ctrl_handle(other))
    r.case(out, name + "_close", lambda: (obj.close(), obj.close(), obj)[2])
    if not value:
        r.case(out, name + "_ctrl_handle_closed", lambda: obj._ctrl_handle(dev))


def classes(r, out):
    """the public classes of lqr.py that reach the library through the shared helpers, on a two-body cartpole with the bodies named in reverse"""
    pkg = r.pkg
    lqr = pkg.lqr
    ex, mech, ids, eids = _cartpole(pkg)
    ids = ids[::-1]
    rng = np.random.default_rng(3)
    nb, mx, mu, n, N = 2, 24, 1, 3, 5
    Qs = [[np.diag(rng.uniform(1, 2, 12)) for _ in range(nb)] for _ in range(n)]
    Rs = [[np.array([[rng.uniform(1, 2)]])] for _ in range(n)]
    zd = pkg.examples.cartpole_states(1, rng.uniform(-0.2, 0.2, n), rng.uniform(-0.1, 0.1, (n, 1)))
    Fd = rng.normal(size=(n, mu))
    plants = pkg.PlantBatch.scaled(mech, n + 1, mass=(0.8, 1.2), seed=3)
    shifted = pkg.PlantBatch.scaled(mech, n, mass=(0.8, 1.2), seed=3, first_index=2)
    dev = lqr._device_mech(mech)

    made = {}
    for name, fn, value in (
            ("PlantLQR", lambda: pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], 0.05, zd, Fτd=Fd, keep_value=True), False),
            ("PlantLQR_inf_no_value", lambda: pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], math.inf, zd, tol=1e-7), False),
            ("PlantLQR_shifted", lambda: pkg.PlantLQR(mech, shifted, ids, eids, Qs[0], Rs[0], 0.05, zd), False),
            ("LQRSweep", lambda: pkg.LQRSweep(mech, ids, eids, Qs, Rs, 0.05, zd[0], keep_value=True), False),
            ("LQRSweep_plants_inf", lambda: pkg.LQRSweep(mech, ids, eids, Qs, Rs[:1], math.inf, zd, Fτd=Fd, plants=shifted), False),
            ("StationaryLQR", lambda: pkg.StationaryLQR(mech, ids, eids, Qs[0], Rs[0], zd, keep_value=True, max_levels=30), False),
            ("StationaryLQR_horizon_pairs_plants", lambda: pkg.StationaryLQR(mech, ids, eids, Qs, Rs, zd, horizon=0.05, Fτd=Fd, plants=shifted, tol=1e-7), False)):
        made[name] = r.case(out, name, fn)
        _refusals(r, out, name, made[name], dev, value)
    for name, fn in (("PlantLQR_controlfunction", lambda: pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], 0.05, zd, controlfunction=print)),
                     ("PlantLQR_bad_zd", lambda: pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], 0.05, zd[0])),
                     ("PlantLQR_bad_Fd", lambda: pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], 0.05, zd, Fτd=Fd[:2])),
                     ("LQRSweep_bad_counts", lambda: pkg.LQRSweep(mech, ids, eids, Qs, Rs[:2], 0.05, zd)),
                     ("StationaryLQR_bad_levels", lambda: pkg.StationaryLQR(mech, ids, eids, Qs[0], Rs[0], zd, max_levels=61)),
                     ("StationaryLQR_bad_zd", lambda: pkg.StationaryLQR(mech, ids, eids, Qs[0], Rs[0], zd[:0])),
                     ("StationaryLQR_one_knot", lambda: pkg.StationaryLQR(mech, ids, eids, Qs[0], Rs[0], zd, horizon=mech.Δt))):
        r.case(out, name, fn)

    def nominal(N_):      # an LQR as the host tests assemble one: the fields its _ctrl_handle reads
        c = pkg.LQR.__new__(pkg.LQR)
        c.mechanism, c.N, c.ctrl_joints = mech, N_, [mech.joint_index(e) for e in eids]
        c.K, c.zd, c.Fd = rng.normal(size=(max(N_ - 1, 1), mu, mx)), zd[:1], np.zeros((1, mu))
        return c
    table, gain = nominal(N), nominal(0)
    per_plant = pkg.PlantLQR(mech, plants, ids, eids, Qs[0], Rs[0], math.inf, zd)
    for name, fn in (
            ("PolicyValue", lambda: pkg.PolicyValue(mech, table, ids, eids, Qs[0], Rs[0], 0.05, zd, tol=1e-6)),
            ("PolicyValue_pairs_plants", lambda: pkg.PolicyValue(mech, per_plant, ids, eids, Qs, Rs, math.inf, zd, plants=shifted, Fτd=Fd)),
            ("StationaryPolicyValue", lambda: pkg.StationaryPolicyValue(mech, gain, ids, eids, Qs[0], Rs[0], None, zd, max_levels=30)),
            ("StationaryPolicyValue_pairs_plants", lambda: pkg.StationaryPolicyValue(mech, per_plant, ids, eids, Qs, Rs, 0.05, zd, plants=plants, first_plant=1, Fτd=Fd))):
        _refusals(r, out, name, r.case(out, name, fn), dev, True)
    S0 = _spd(rng, n, mx)
    for name, fn in (
            ("StationaryCovariance_noise_scale", lambda: pkg.StationaryCovariance(mech, gain, ids, eids, Qs[0], Rs[0], None, zd, noise_scale=0.5, max_levels=30)),
            ("StationaryCovariance_Wu_Sigma0", lambda: pkg.StationaryCovariance(mech, per_plant, ids, eids, Qs, Rs, 0.05, zd, Wu=_spd(rng, n, mu), Sigma0=S0, plants=shifted,
                                                                                 Fτd=Fd, tol=1e-9)),
            ("StationaryCovariance_Sigma0_only", lambda: pkg.StationaryCovariance(mech, gain, ids, eids, Qs[0], Rs[0], math.inf, zd, Sigma0=S0[0]))):
        cov = r.case(out, name, fn)
        r.case(out, name + "_Sigma", lambda: cov.Sigma(0))
        r.case(out, name + "_close", lambda: (cov.close(), cov)[1])
    bad = dict(PolicyValue=lambda **kw: pkg.PolicyValue(mech, kw.pop("controller", table), ids, eids, Qs[0], Rs[0], 0.05, kw.pop("zd", zd), **kw),
               StationaryPolicyValue=lambda **kw: pkg.StationaryPolicyValue(mech, kw.pop("controller", gain), ids, eids, Qs[0], Rs[0], kw.pop("horizon", None),
                                                                            kw.pop("zd", zd), **kw),
               StationaryCovariance=lambda **kw: pkg.StationaryCovariance(mech, kw.pop("controller", gain), ids, eids, Qs[0], Rs[0], kw.pop("horizon", None),
                                                                          kw.pop("zd", zd), **kw))
    other_mech = _cartpole(pkg)[1]
    for cls, make in bad.items():
        for why, kw in (("controller", dict(controller=object())), ("zd", dict(zd=zd[0])), ("plants", dict(plants=pkg.PlantBatch.scaled(other_mech, n))),
                        ("Fd", dict(Fτd=Fd[:2])), ("rows", dict(plants=shifted, first_plant=0))):
            r.case(out, "%s_bad_%s" % (cls, why), lambda: make(**kw))
    for cls in ("StationaryPolicyValue", "StationaryCovariance"):
        noise = dict(noise_scale=1.0) if cls == "StationaryCovariance" else {}
        r.case(out, cls + "_bad_levels", lambda: bad[cls](max_levels=0, **noise))
        r.case(out, cls + "_bad_tol", lambda: bad[cls](tol=-1.0, **noise))
        r.case(out, cls + "_bad_table", lambda: bad[cls](controller=table, **noise))
    for why, kw in (("nothing", {}), ("both", dict(noise_scale=1.0, Wu=np.ones((1, 1)))), ("Sigma0_steady", dict(Sigma0=S0[0])), ("Wu", dict(Wu=np.ones((2, 2)))),
                    ("Sigma0", dict(Sigma0=S0[:2], horizon=0.05))):
        r.case(out, "StationaryCovariance_bad_" + why, lambda: bad["StationaryCovariance"](**kw))

    ztraj = np.stack([pkg.examples.cartpole_states(1, rng.uniform(-0.2, 0.2, N), rng.uniform(-0.1, 0.1, (N, 1))) for _ in range(n)])
    Ftraj = rng.normal(size=(n, N, mu))
    trk = pkg.TrackingLQR.__new__(pkg.TrackingLQR)      # as the host tests assemble one
    trk.mechanism, trk.N, trk.eqcids, trk.controlfunction, trk.ctrl_joints = mech, N, [int(e) for e in eids], None, [mech.joint_index(e) for e in eids]
    trk.zd, trk.Fd, trk.K = ztraj[0], Ftraj[0], rng.normal(size=(N - 1, mu, mx))
    batched = r.case(out, "PlantTrackingLQR", lambda: pkg.PlantTrackingLQR(mech, plants, ztraj, Ftraj, eids, Qs[0], Rs[0], fric=[0.1, 0.2], noise_scale=0.2))
    for name, fn in (
            ("TrackingCovariance", lambda: pkg.TrackingCovariance(mech, trk, ids, eids, Qs[0], Rs[0], noise_scale=0.5)),
            ("TrackingCovariance_storage_pairs", lambda: pkg.TrackingCovariance(mech, trk, ids, eids, Qs, Rs, Wu=_spd(rng, n, mu), Sigma0=S0, plants=shifted, storage=ztraj,
                                                                                  Fτ=Ftraj, workspace_bytes=1 << 22)),
            ("TrackingCovariance_batched", lambda: pkg.TrackingCovariance(mech, batched, ids, eids, Qs[0], Rs[0], Sigma0=S0[0]))):
        cov = r.case(out, name, fn)
        r.case(out, name + "_Sigma", lambda: cov.Sigma(0))
        r.case(out, name + "_close", lambda: (cov.close(), cov)[1])
    for name, fn in (
            ("TrackingPolicyValue", lambda: pkg.TrackingPolicyValue(mech, trk, ids, eids, Qs[0], Rs[0])),
            ("TrackingPolicyValue_storage_pairs", lambda: pkg.TrackingPolicyValue(mech, trk, ids, eids, Qs, Rs, Wu=_spd(rng, n, mu), plants=shifted, storage=ztraj, Fτ=Ftraj,
                                                                                   knot=2)),
            ("TrackingPolicyValue_batched", lambda: pkg.TrackingPolicyValue(mech, batched, ids, eids, Qs[0], Rs[0], noise_scale=0.5, knot=N - 1))):
        _refusals(r, out, name, r.case(out, name, fn), dev, True)
    for cls in (pkg.TrackingCovariance, pkg.TrackingPolicyValue):
        for why, kw in (("both", dict(noise_scale=1.0, Wu=np.ones((1, 1)))), ("Wu", dict(Wu=np.ones((2, 2)))), ("storage", dict(storage=ztraj[:, :-1], noise_scale=1.0))):
            r.case(out, "%s_bad_%s" % (cls.__name__, why), lambda: cls(mech, trk, ids, eids, Qs[0], Rs[0], **kw))
    r.case(out, "TrackingCovariance_bad_nothing", lambda: pkg.TrackingCovariance(mech, trk, ids, eids, Qs[0], Rs[0]))
    r.case(out, "TrackingCovariance_bad_Sigma0", lambda: pkg.TrackingCovariance(mech, trk, ids, eids, Qs[0], Rs[0], Sigma0=S0[:2]))


def record(pkg, setattr_):
    """{case: {"calls": [[symbol, [arguments]]], "returns" | "raises": ..., "attributes": ...}} of the package `pkg` with its library stubbed through setattr_"""
    r = Recorder(pkg, setattr_)
    out = {}
    array_level(r, out)
    mechanism_level(r, out)
    classes(r, out)
    return json.loads(json.dumps(out))      # (tuples as lists, numpy scalars as numbers: what the fixture holds)


def load(directory, name):
    """the package directory `directory` imported under `name` (the directory's own name carries a dot)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(directory, "__init__.py"), submodule_search_locations=[directory])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    got = record(load(os.path.abspath(sys.argv[1]), "cclqr_recorded"), setattr)
    with open(sys.argv[2], "w") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d cases, %d calls" % (len(got), sum(len(c["calls"]) for c in got.values())))
