"""ctypes binding of libcclqr.so (include/cclqr.h).  There is no fallback: if the HIP library is missing or a
call fails, this raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcclqr.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

OK, EINVAL, ESINGULAR, ENOCONV, EHIP, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
_ERRNAME = {EINVAL: "CCLQR_EINVAL", ESINGULAR: "CCLQR_ESINGULAR", ENOCONV: "CCLQR_ENOCONV", EHIP: "CCLQR_EHIP", EUNSUPPORTED: "CCLQR_EUNSUPPORTED"}

EXPORTS = ["cclqr_last_error", "cclqr_version", "cclqr_device_count", "cclqr_set_device", "cclqr_mech_create", "cclqr_mech_destroy",
           "cclqr_ctrl_create", "cclqr_ctrl_create_lqr_batch", "cclqr_ctrl_destroy", "cclqr_linearize", "cclqr_linearize_projected", "cclqr_riccati", "cclqr_riccati_tv", "cclqr_riccati_tracking", "cclqr_rollout",
           "cclqr_rollout_dev", "cclqr_rollout_ex", "cclqr_rollout_host_ex", "cclqr_ctrl_reserve_noise", "cclqr_riccati_ex", "cclqr_riccati_tracking_ex",
           "cclqr_release_workspaces", "cclqr_rollout_geometry", "cclqr_rollout_layout_links", "cclqr_ctrl_set_feedforward", "cclqr_abi_layout", "cclqr_rollout_lanes_per_link", "cclqr_rollout_instances_per_wavefront",
           "cclqr_plants_create", "cclqr_plants_destroy", "cclqr_rollout_plants", "cclqr_linearize_plants", "cclqr_ctrl_create_lqr_batch_plants",
           "cclqr_ctrl_create_tracking_batch_plants", "cclqr_ctrl_get_gains", "cclqr_score_create", "cclqr_score_destroy", "cclqr_rollout_score",
           "cclqr_riccati_weights", "cclqr_ctrl_create_lqr_batch_weights",
           "cclqr_riccati_value", "cclqr_ctrl_create_lqr_batch_value", "cclqr_value_create", "cclqr_value_get", "cclqr_value_destroy", "cclqr_value_eval",
           "cclqr_policy_value", "cclqr_value_create_policy", "cclqr_policy_value_doubling", "cclqr_value_create_policy_doubling",
           "cclqr_riccati_doubling", "cclqr_ctrl_create_lqr_batch_doubling", "cclqr_covariance_doubling", "cclqr_value_create_covariance_doubling",
           "cclqr_covariance_tracking", "cclqr_value_create_covariance_tracking", "cclqr_policy_value_tracking", "cclqr_value_create_policy_tracking",
           "cclqr_rollout_ensemble_ws_bytes", "cclqr_rollout_ensemble", "cclqr_rollout_quantiles_ws_bytes", "cclqr_rollout_quantiles",
           "cclqr_rollout_joints", "cclqr_series_ensemble_ws_bytes", "cclqr_series_ensemble", "cclqr_series_quantiles_ws_bytes", "cclqr_series_quantiles",
           "cclqr_rollout_invariants"]
ABI_VERSION = 202     # include/cclqr.h CCLQR_ABI_VERSION: the structs below mirror that header (verified field by field against cclqr_abi_layout at load time)
ROLLOUT_NO_ALLOC = 1  # cclqr_rollout_opts.flags: the call may neither allocate nor synchronise (a hipGraph capture is open on the device)
ROLLOUT_CARRY_STATUS = 4  # ... `status` is read and written: an instance lost in an earlier launch stays frozen, the others merge this launch's result into it
ROLLOUT_RUNTIME_PLAN = 16  # ... a single 16- / 17-link chain runs on the general chain kernel (plan of the solve read at run time) instead of its fixed-plan kernel: same bits
ROLLOUT_PACK_WAVEFRONTS = 2  # ... every wavefront of a chain launch full, whatever the batch size (many launches sharing the device at once)
PHILOX_INKERNEL_STEPS = 8
SCORE_LEN = 4           # CCLQR_SCORE_LEN: Jx, Ju, peak, last_out per instance (cclqr_rollout_score)
NEWTON_MAXIT = 100      # newtonIter of ConstrainedDynamics' newton!: |status| of an instance that hit the cap


class CclqrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (_ERRNAME.get(code, "?"), code, msg))
        self.code = code


class MechDesc(C.Structure):
    _fields_ = [("nb", C.c_int32), ("ne", C.c_int32), ("dt", C.c_double), ("g", C.c_double),
                ("mass", _dp), ("inertia", _dp), ("parent", _ip), ("child", _ip), ("type", _ip),
                ("p1", _dp), ("p2", _dp), ("axis", _dp), ("qoff", _dp)]


class CtrlDesc(C.Structure):
    _fields_ = [("mu", C.c_int32), ("ctrl_joint", _ip), ("nK", C.c_int32), ("N", C.c_int32), ("K", _dp),
                ("nsp", C.c_int32), ("zd", _dp), ("Fd", _dp), ("fric", _dp), ("noise_scale", C.c_double),
                ("npid", C.c_int32), ("pid_joint", _ip), ("pid_P", _dp), ("pid_I", _dp), ("pid_D", _dp), ("pid_goal", _dp),
                ("noise_philox", C.c_int32), ("noise_seed", C.c_uint64), ("n_ctrl", C.c_int32)]


class RiccatiOpts(C.Structure):
    _fields_ = [("path", C.c_int32), ("bf16_terms", C.c_int32), ("keep_last", C.c_int32), ("reserved", C.c_int32)]


class RolloutOpts(C.Structure):
    _fields_ = [("first_instance", C.c_int64), ("pid_state_dev", C.c_void_p), ("pid_state_len", C.c_int64),
                ("noise_ws_dev", C.c_void_p), ("noise_ws_len", C.c_int64), ("newton_mode", C.c_int32), ("flags", C.c_int32),
                ("newton_eps_alone", C.c_double)]


_lib = None


def mirrored_layout():
    """sizeof / offsetof of the four ctypes mirrors in the order cclqr_abi_layout reports the library's own (include/cclqr.h)"""
    out = []
    for S in (MechDesc, CtrlDesc, RiccatiOpts, RolloutOpts):
        out.append(C.sizeof(S))
        out += [getattr(S, name).offset for name, _ in S._fields_]
    return out


def _preload_shared_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and links it by the name
    `libamdhip64.so`; libcclqr.so needs `libamdhip64.so.7`.  If libcclqr.so is loaded first the system copy comes in, torch later
    adds its bundled copy, and the second runtime reports `no ROCm-capable device`.  Loading torch's copy first (when torch is
    installed; torch itself is NOT imported) makes both resolve to the same runtime whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """load libcclqr.so; raises if it has not been built (`python -c 'import __graft_entry__ as g; g.build()'`)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libcclqr.so is missing at %s: the HIP extension must be built (no CPU fallback exists)" % LIB_PATH)
        _preload_shared_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.cclqr_last_error.restype = C.c_char_p
        L.cclqr_version.restype = C.c_int
        if L.cclqr_version() != ABI_VERSION:      # before any other symbol is touched: an older library lacks the newer exports
            raise ImportError("libcclqr.so has ABI version %d, this binding was written for %d: rebuild the library" % (L.cclqr_version(), ABI_VERSION))
        for name in EXPORTS[1:]:
            try:
                getattr(L, name).restype = C.c_int
            except AttributeError:
                raise ImportError("libcclqr.so (ABI version %d) does not export %s, which include/cclqr.h declares: rebuild the library" % (L.cclqr_version(), name))
        want = mirrored_layout()
        got = (C.c_int32 * len(want))()
        n = L.cclqr_abi_layout(got, C.c_int32(len(want)))
        if n != len(want) or list(got) != want:
            raise ImportError("struct layout mismatch between libcclqr.so and this binding (cclqr_abi_layout: %s, ctypes mirrors: %s)" % (list(got), want))
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise CclqrError(rc, lib().cclqr_last_error().decode())


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


# The argument marshalling every entry point below shares, each piece stated once.  _d and _i above stay the only places where an array becomes a pointer.

def _panel(a):
    """the pointer of a panel that may be empty (Bu, R, K with mu = 0; Bl, G with ml = 0) or absent: NULL then -- the library reads no panel whose extent is zero"""
    return _d(a) if a is not None and a.size else None


def _models(A, Bu, Bl, G, per=1, tracked=False):
    """the projected-model arguments as contiguous float64 arrays -> ((A, Bu, Bl, G), (nprob, mx, mu, ml)).  Flat form: A [nmod][mx][mx] (or [mx][mx]) with `per`
    models per problem (N - 1 of a time-varying problem); tracked: A [nprob][nlin][mx][mx].  mu and ml are read off Bu and Bl"""
    A = f64(A)
    if tracked:
        if A.ndim != 4 or A.shape[-1] != A.shape[-2]:
            raise ValueError("A must be [nprob][nlin][mx][mx] (got %s)" % (A.shape,))
        lead, mx = A.shape[:2], A.shape[-1]
        panel = lambda B: B.reshape(lead + (mx, -1)) if B.size else B.reshape(lead + (mx, 0))
    else:
        mx = A.shape[-1]
        A = A.reshape(-1, mx, mx)
        if A.shape[0] % per:
            raise ValueError("time_varying: A must hold N - 1 = %d models per problem (got %d models)" % (per, A.shape[0]))
        lead = A.shape[:1]
        panel = lambda B: B.reshape(lead + (mx, B.shape[-1] if B.ndim > 1 else -1))      # (the trailing size stated: mu = 0 / ml = 0 leave nothing to infer -1 from)
    Bu, Bl = panel(f64(Bu)), panel(f64(Bl))
    mu, ml = Bu.shape[-1], Bl.shape[-1]
    return (A, Bu, Bl, f64(G).reshape(lead + (ml, mx))), (lead[0] // per, mx, mu, ml)


def _model_args(dims, models):
    """the head of an array-level call: nprob, mx, mu, ml, A, Bu, Bl, G -- nlin before A in the tracked form, an empty panel as NULL"""
    return tuple(C.c_int32(v) for v in dims + models[0].shape[1:-2]) + (_d(models[0]),) + tuple(_panel(M) for M in models[1:])


def _gains(K, mu, mx, full, lowest):
    """a gain table of any accepted rank lowest .. full as the full-rank array: full = 3, [n_gains][mu][mx] (a stationary gain), or 4, [n_gains][nK][mu][mx]"""
    K = f64(K)
    if not lowest <= K.ndim <= full or K.shape[-2:] != (mu, mx):
        lead = ["[n_gains]", "[nK]"][:full - 2]
        names = ["".join(lead[full - rank:]) + "[mu][mx]" for rank in range(lowest, full + 1)]
        raise ValueError("K must be %s or %s with mu = %d, mx = %d (got %s)" % (", ".join(names[:-1]), names[-1], mu, mx, K.shape))
    return K.reshape((1,) * (full - K.ndim) + K.shape)


def _weights(Q, R, mx, mu, nw=None, optional=False):
    """Q [n_weights][mx][mx], R [n_weights][mu][mu] -> (Q, R, n_weights): the count read off Q, or `nw` as the caller states it.  optional: Q = None (a call that
    takes no cost) gives (None, None, 1)"""
    if optional and Q is None:
        return None, None, 1
    Q = f64(Q).reshape(-1 if nw is None else nw, mx, mx)
    nw = Q.shape[0]
    return Q, f64(R).reshape(nw, mu, mu), nw


def _on_plants(mech, plants, first_plant):
    """the head of a mechanism-side call: the mechanism, the PlantsHandle (None: the mechanism's own plant) and the global index of its first plant"""
    return mech.ptr, None if plants is None else plants.ptr, C.c_int64(int(first_plant))


def _mech_side(mech, zd, ctrl_joint, Fd, Q, R, nw=None, traj=None, on_device=False):
    """the mechanism-side arguments -> ((zd, ctrl_joint, Fd, Q, R) as arrays, n_weights, (zd, Fd) as the library takes them).  zd [n][nb][13], Fd [n][mu] or None; traj =
    (n, N): trajectories zd [n][N][nb][13], Fd [n][N][mu], with on_device raw device addresses, passed as they are.  Q [n_weights][12 nb][12 nb], R [n_weights][mu][mu]"""
    nb = mech.tables.nb
    cj = i32(ctrl_joint).reshape(-1)
    mu = len(cj)
    if on_device:
        zd, Fd, ptrs = None, None, (C.c_void_p(int(zd)), None if Fd is None else C.c_void_p(int(Fd)))
    else:
        zd = f64(zd).reshape(((-1,) if traj is None else traj) + (nb, 13))
        Fd = None if Fd is None else f64(Fd).reshape(zd.shape[:-2] + (mu,))
        ptrs = (_d(zd), _d(Fd))
    Q, R, nw = _weights(Q, R, 12 * nb, mu, nw)
    return (zd, cj, Fd, Q, R), nw, ptrs


def _setpoint_args(mech, ctrl, zd, ctrl_joint, Fd, Q, R, plants, first_plant):
    """the head the value_create_* entries on setpoints share -- mechanism, plants, first_plant, n, zd, mu, ctrl_joint, Fd, the controller, n_weights, Q, R -> (n, head)"""
    (zd, cj, _, Q, R), nw, (zp, fp) = _mech_side(mech, zd, ctrl_joint, Fd, Q, R)
    n = zd.shape[0]
    return n, _on_plants(mech, plants, first_plant) + (C.c_int32(n), zp, C.c_int32(len(cj)), _i(cj), fp, ctrl.ptr, C.c_int32(nw), _d(Q), _d(R))


def _trajectory_args(mech, ctrl, zd, n, N, ctrl_joint, Fd, Q, R, plants, first_plant, on_device):
    """the head the value_create_* entries on trajectories share -- mechanism, plants, first_plant, n, N, zd, Fd, on_device, mu, ctrl_joint, the controller, n_weights, Q, R"""
    (_, cj, _, Q, R), nw, (zp, fp) = _mech_side(mech, zd, ctrl_joint, Fd, Q, R, traj=(n, N), on_device=on_device)
    return _on_plants(mech, plants, first_plant) + (C.c_int32(n), C.c_int32(N), zp, fp, C.c_int32(1 if on_device else 0), C.c_int32(len(cj)), _i(cj), ctrl.ptr,
                                                    C.c_int32(nw), _d(Q), _d(R))


def _diagnostics(n, want=True, fill=0.0):
    """the four diagnostics of a doubling call -- levels, reason [n], dnorm and the second norm [n][2] --, or four None (the library then takes NULL)"""
    if not want:
        return None, None, None, None
    return np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.full((n, 2), fill), np.full((n, 2), fill)


class _Handle:
    """an object of the library behind `ptr`: destroyed once, by close() or when collected.  A subclass names the destroy symbol and keeps in _arrs the host arrays
    its descriptor points into"""
    _destroy = None

    def close(self):
        if self.ptr:
            getattr(lib(), self._destroy)(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = C.c_int32(0)
    check(lib().cclqr_device_count(C.byref(n)))
    return n.value


def set_device(dev):
    check(lib().cclqr_set_device(C.c_int32(dev)))


class MechHandle(_Handle):
    """cclqr_mech*: device-resident mechanism tables"""
    _destroy = "cclqr_mech_destroy"

    def __init__(self, tables):
        t = tables
        self.tables = t
        self._arrs = [f64(t.mass), f64(t.inertia), i32(t.parent), i32(t.child), i32(t.type), f64(t.p1), f64(t.p2), f64(t.axis), f64(t.qoff)]
        a = self._arrs
        self.desc = MechDesc(t.nb, t.ne, t.dt, t.g, _d(a[0]), _d(a[1]), _i(a[2]), _i(a[3]), _i(a[4]), _d(a[5]), _d(a[6]), _d(a[7]), _d(a[8]))
        self.ptr = C.c_void_p()
        check(lib().cclqr_mech_create(C.byref(self.desc), C.byref(self.ptr)))

    def geometry(self):
        lanes, ldsb = C.c_int32(0), C.c_int32(0)
        check(lib().cclqr_rollout_geometry(self.ptr, C.byref(lanes), C.byref(ldsb)))
        return lanes.value, ldsb.value

    def layout_links(self):
        """links the rollout kernel's LDS image is laid out for (names the instantiation of the chain / tree kernel); 0 for closed-loop mechanisms"""
        n = C.c_int32(0)
        check(lib().cclqr_rollout_layout_links(self.ptr, C.byref(n)))
        return n.value

    def lanes_per_link(self):
        """(lanes that work for one link, links per sub-lane group) of the chain kernel's instantiation; (1, lanes per instance) elsewhere"""
        kl, nl = C.c_int32(0), C.c_int32(0)
        check(lib().cclqr_rollout_lanes_per_link(self.ptr, C.byref(kl), C.byref(nl)))
        return kl.value, nl.value

    def instances_per_wavefront(self, n_inst, steps, flags=0):
        """instances one wavefront of such a launch holds (chains: a small batch is spread over more wavefronts unless ROLLOUT_PACK_WAVEFRONTS)"""
        v = C.c_int32(0)
        check(lib().cclqr_rollout_instances_per_wavefront(self.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(flags)), C.byref(v)))
        return v.value


class CtrlHandle(_Handle):
    """cclqr_ctrl*: device-resident controller tables"""
    _destroy = "cclqr_ctrl_destroy"

    def __init__(self, mech, ctrl_joint, K=None, N=0, zd=None, Fd=None, fric=None, noise_scale=0.0, pid=None, noise_seed=None, n_ctrl=0):
        """n_ctrl > 1: one controller table per instance -- K [n_ctrl][nK][mu][12 nb], zd [n_ctrl][nsp][nb][13], Fd [n_ctrl][nsp][mu]"""
        nb = mech.tables.nb
        cj = i32(ctrl_joint).reshape(-1)
        mu = len(cj)
        nc = n_ctrl if n_ctrl > 1 else 1
        if zd is None:
            zd = np.zeros((nc, nb, 13))
            zd[:, :, 3] = 1.0
        zd = f64(zd).reshape(-1, nb, 13)
        nsp = zd.shape[0] // nc
        Fd = f64(np.zeros((nc * nsp, mu)) if Fd is None else Fd).reshape(nc * nsp, mu)
        K = None if K is None else f64(K).reshape(-1, mu, 12 * nb)
        fric = None if fric is None else f64(fric).reshape(mech.tables.ne)          # one entry per joint (ne == nb on a tree)
        pj = pP = pI = pD = pg = None
        if pid is not None:
            pj, pP, pI, pD, pg = i32(pid["joint"]).reshape(-1), f64(pid["P"]).reshape(-1), f64(pid["I"]).reshape(-1), f64(pid["D"]).reshape(-1), f64(pid["goal"]).reshape(-1)
        self._arrs = [cj, K, zd, Fd, fric, pj, pP, pI, pD, pg]
        self.mu, self.N, self.nsp = mu, int(N), nsp
        self.desc = CtrlDesc(mu, _i(cj), 0 if K is None else K.shape[0] // nc, int(N), _d(K), nsp, _d(zd), _d(Fd), _d(fric), float(noise_scale),
                             0 if pj is None else len(pj), _i(pj), _d(pP), _d(pI), _d(pD), _d(pg),
                             0 if noise_seed is None else 1, 0 if noise_seed is None else int(noise_seed), int(n_ctrl))
        self.ptr = C.c_void_p()
        check(lib().cclqr_ctrl_create(mech.ptr, C.byref(self.desc), C.byref(self.ptr)))

    def reserve_noise(self, n_inst, steps):
        """size the handle's Philox workspace (needed before a noise_philox launch is captured into a hipGraph)"""
        check(lib().cclqr_ctrl_reserve_noise(self.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps))))

    def set_feedforward(self, Fd=None, dev_ptr=None, length=None, stream=0):
        """the controlfunction hook (lqr.jl:14, :56): replace the feed-forward table [n_ctrl][nsp][mu] -- host array Fd, or device address dev_ptr
        (+ length in doubles) copied on `stream`"""
        if dev_ptr is not None:
            check(lib().cclqr_ctrl_set_feedforward(self.ptr, C.c_void_p(int(dev_ptr)), C.c_int64(int(length)), C.c_int32(1), C.c_void_p(int(stream)) if stream else None))
            return
        Fd = f64(Fd).reshape(-1)
        check(lib().cclqr_ctrl_set_feedforward(self.ptr, _d(Fd), C.c_int64(Fd.size), C.c_int32(0), None))


class BatchLqrHandle(_Handle):
    """cclqr_ctrl* built by cclqr_ctrl_create_lqr_batch: one LQR per setpoint (linearsystem + dlqr + controller tables), gains device-resident"""
    _destroy = "cclqr_ctrl_destroy"

    def __init__(self, mech, zd, ctrl_joint, Q, R, N, Fd=None, tol=1e-5, infinite_horizon=False, plants=None, first_plant=0, n_weights=None, keep_value=False):
        """infinite_horizon: LQR{T,Inf} -- N = Ntemp = ceil(10/Δt) (lqr.jl:26), only Ku[1] per setpoint is kept.
        keep_value: every table's cost-to-go stays on the device as self.value, a ValueHandle (cclqr_ctrl_create_lqr_batch_value); False: self.value is None and
        nothing is allocated.
        plants: a PlantsHandle (cclqr_ctrl_create_lqr_batch_plants) -- table k is designed on the plant with global index first_plant + k.
        n_weights: Q [n_weights][12 nb][12 nb], R [n_weights][mu][mu], one pair per table (cclqr_ctrl_create_lqr_batch_weights; the library refuses any count but
        1 and the number of setpoints); None: one pair, through the entry points that take one"""
        head, nw, weights = self._arguments(mech, zd, ctrl_joint, Fd, Q, R, 1 if n_weights is None else int(n_weights), 0 if infinite_horizon else int(N), plants,
                                            first_plant)
        self.kbreak = np.zeros(self.n_ctrl, dtype=np.int32)
        last = weights + (C.c_int32(int(N)), C.c_int32(1 if infinite_horizon else 0), C.c_double(float(tol)), _i(self.kbreak), C.byref(self.ptr))
        on = _on_plants(mech, plants, first_plant)
        if keep_value:
            vptr = C.c_void_p()
            check(lib().cclqr_ctrl_create_lqr_batch_value(*on, *head, C.c_int32(nw), *last, C.byref(vptr)))
            self.value = ValueHandle(mech, ptr=vptr, n_tables=self.n_ctrl)
        elif n_weights is not None:
            check(lib().cclqr_ctrl_create_lqr_batch_weights(*on, *head, C.c_int32(nw), *last))
        elif plants is None:
            check(lib().cclqr_ctrl_create_lqr_batch(mech.ptr, *head, *last))
        else:
            check(lib().cclqr_ctrl_create_lqr_batch_plants(*on, *head, *last))

    def _arguments(self, mech, zd, ctrl_joint, Fd, Q, R, nw, N, plants, first_plant):
        """the fields both batched constructors keep -> (the call's arguments from the setpoint count to Fd, n_weights, the pointers of Q and R)"""
        arrs, nw, (zp, fp) = _mech_side(mech, zd, ctrl_joint, Fd, Q, R, nw)
        self._arrs = list(arrs)
        n, mu = arrs[0].shape[0], len(arrs[1])
        self.mu, self.N, self.nsp, self.n_ctrl = mu, N, 1, n
        self.mech = mech
        self.plants, self.first_plant = plants, int(first_plant)      # (the plants it was designed on: kept for error messages only)
        self.ptr, self.value = C.c_void_p(), None
        return (C.c_int32(n), zp, C.c_int32(mu), _i(arrs[1]), fp), nw, (_d(arrs[3]), _d(arrs[4]))

    def close(self):
        super().close()
        if getattr(self, "value", None) is not None:
            self.value.close()


class BatchLqrDoublingHandle(BatchLqrHandle):
    """cclqr_ctrl* built by cclqr_ctrl_create_lqr_batch_doubling: one stationary gain per setpoint by doubling the Riccati map (lqr.jl:25-27, 39-43, 141-184), gains
    device-resident, one row per table.  N >= 2: the horizon's first gain; N = 0: to convergence.  levels, reason [n], dnorm, anorm [n][2] as the library reports them;
    keep_value: every table's P stays on the device as self.value"""

    def __init__(self, mech, zd, ctrl_joint, Q, R, N=0, Fd=None, tol=1e-5, max_levels=40, plants=None, first_plant=0, keep_value=False):
        head, nw, weights = self._arguments(mech, zd, ctrl_joint, Fd, Q, R, None, 0, plants, first_plant)
        self.kbreak = None
        self.levels, self.reason, self.dnorm, self.anorm = _diagnostics(self.n_ctrl, fill=np.nan)
        vptr = C.c_void_p()
        check(lib().cclqr_ctrl_create_lqr_batch_doubling(*_on_plants(mech, plants, first_plant), *head, C.c_int32(nw), *weights, C.c_int32(int(N)), C.c_double(float(tol)),
                                                         C.c_int32(int(max_levels)), _i(self.levels), _i(self.reason), _d(self.dnorm), _d(self.anorm),
                                                         C.byref(self.ptr), C.byref(vptr) if keep_value else None))
        if keep_value:
            self.value = ValueHandle(mech, ptr=vptr, n_tables=self.n_ctrl)


def ctrl_create_lqr_batch_doubling(mech, zd, ctrl_joint, Q, R, N=0, Fd=None, tol=1e-5, max_levels=40, plants=None, first_plant=0, keep_value=False):
    """cclqr_ctrl_create_lqr_batch_doubling -> BatchLqrDoublingHandle"""
    return BatchLqrDoublingHandle(mech, zd, ctrl_joint, Q, R, N, Fd, tol, max_levels, plants, first_plant, keep_value)


class ValueHandle(_Handle):
    """cclqr_value*: device-resident cost-to-go tables P [n_tables][12 nb][12 nb] in the mechanism's body order, one shared by every instance or one per controller
    table.  P: a host array (cclqr_value_create); ptr / n_tables: a handle the library has already filled (cclqr_ctrl_create_lqr_batch_value)"""
    _destroy = "cclqr_value_destroy"

    def __init__(self, mech, P=None, ptr=None, n_tables=None):
        mx = 12 * mech.tables.nb
        self.mech, self.mx = mech, mx      # (the handle must not outlive the mechanism's)
        if ptr is not None:
            self.ptr, self.n_tables = ptr, int(n_tables)
            return
        P = f64(P)
        if P.ndim < 2 or P.shape[-2:] != (mx, mx):
            raise ValueError("P must be [n_tables][12 nb][12 nb] = [..][%d][%d] (got %s)" % (mx, mx, P.shape))
        P = np.ascontiguousarray(P.reshape(-1, mx, mx))
        self.n_tables = P.shape[0]
        self.ptr = C.c_void_p()
        check(lib().cclqr_value_create(mech.ptr, C.c_int64(self.n_tables), _d(P), C.byref(self.ptr)))

    def get(self, table=0):
        """one table read back: P [12 nb][12 nb] (cclqr_value_get)"""
        P = np.zeros((self.mx, self.mx))
        check(lib().cclqr_value_get(self.ptr, C.c_int64(int(table)), _d(P)))
        return P


def value_eval(mech, ctrl, value, n_inst, z_ptr, out_ptr, stream=0, first_instance=0, z_stride=None):
    """cclqr_value_eval on device addresses (asynchronous on `stream`): out[i] = dz_i' P_t dz_i for the states at z_ptr + 8 i z_stride (z_stride in doubles; default: packed,
    13 nb) about setpoint row 0 of controller table first_instance + i"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    zs = 13 * mech.tables.nb if z_stride is None else int(z_stride)
    check(lib().cclqr_value_eval(mech.ptr, ctrl.ptr, value.ptr, C.c_int64(int(n_inst)), C.c_int64(int(first_instance)), vp(z_ptr), C.c_int64(zs), vp(out_ptr), vp(stream)))


class BatchTrackingHandle(_Handle):
    """cclqr_ctrl* built by cclqr_ctrl_create_tracking_batch_plants: one TrackingLQR per plant and / or reference trajectory (linearsystem at every knot, the
    time-varying recursion, the controller's tables), gains device-resident.
    zd [n][N][nb][13], Fd [n][N][mu] or None: host arrays, or (on_device=True) raw device addresses read on `stream` -- n_ctrl and N must then be given.
    plants: a PlantsHandle or None (the mechanism's own plant for every trajectory); table k is designed on the plant with global index first_plant + k.
    fric [ne], noise_scale, noise_seed: the friction / noise law, fixed at construction.  workspace_bytes <= 0: the library's default budget."""
    _destroy = "cclqr_ctrl_destroy"

    def __init__(self, mech, zd, ctrl_joint, Q, R, Fd=None, plants=None, first_plant=0, n_ctrl=None, N=None, on_device=False, stream=0, tol=1e-5, fric=None,
                 noise_scale=0.0, noise_seed=None, workspace_bytes=0):
        nb = mech.tables.nb
        cj = i32(ctrl_joint).reshape(-1)
        mu = len(cj)
        if on_device:
            if n_ctrl is None or N is None:
                raise ValueError("device addresses carry no shape: n_ctrl and N must be given")
            zarg, farg = C.c_void_p(int(zd)), (C.c_void_p(int(Fd)) if Fd else None)
            self._arrs = []
        else:
            zd = f64(zd)
            if zd.ndim != 4 or zd.shape[2:] != (nb, 13):
                raise ValueError("zd must be [n][N][nb][13] = [n][N][%d][13] (got %s)" % (nb, zd.shape))
            if n_ctrl is None:
                n_ctrl = zd.shape[0]
            if N is None:
                N = zd.shape[1]
            if zd.shape[:2] != (n_ctrl, N):
                raise ValueError("zd does not hold n_ctrl x N = %d x %d setpoints (got %s)" % (n_ctrl, N, zd.shape))
            Fd = None if Fd is None else f64(Fd)
            if Fd is not None and Fd.shape != (n_ctrl, N, mu):
                raise ValueError("Fd must be [n][N][mu] = [%d][%d][%d] (got %s)" % (n_ctrl, N, mu, Fd.shape))
            zarg, farg = _d(zd), _d(Fd)
            self._arrs = [zd, Fd]
        Q, R = f64(Q).reshape(12 * nb, 12 * nb), f64(R).reshape(mu, mu)
        fric = None if fric is None else f64(fric).reshape(mech.tables.ne)
        self._arrs += [cj, Q, R, fric]
        law = None
        if fric is not None or noise_scale or noise_seed is not None:
            law = CtrlDesc()
            law.fric, law.noise_scale = _d(fric), float(noise_scale)
            law.noise_philox, law.noise_seed = (0 if noise_seed is None else 1), (0 if noise_seed is None else int(noise_seed))
        self.kbreak = np.zeros(int(n_ctrl), dtype=np.int32)
        self.mu, self.N, self.nsp, self.nK, self.n_ctrl = mu, int(N), int(N), int(N) - 1, int(n_ctrl)
        self.mech, self.plants, self.first_plant = mech, plants, int(first_plant)
        self.ptr = C.c_void_p()
        check(lib().cclqr_ctrl_create_tracking_batch_plants(mech.ptr, None if plants is None else plants.ptr, C.c_int64(int(first_plant)), C.c_int32(int(n_ctrl)),
                                                            C.c_int32(int(N)), zarg, farg, C.c_int32(1 if on_device else 0), C.c_int32(mu), _i(cj), _d(Q), _d(R),
                                                            C.c_double(float(tol)), None if law is None else C.byref(law), C.c_int64(int(workspace_bytes)),
                                                            _i(self.kbreak), C.c_void_p(int(stream)) if stream else None, C.byref(self.ptr)))


def ctrl_gains(mech, handle, table=0, nK=None, mu=None):
    """cclqr_ctrl_get_gains: one table's gains [nK][mu][12 nb] of a controller handle, in the mechanism's body order.  nK, mu: the handle's own by default
    (BatchLqrHandle keeps N: nK = N - 1, or 1 for the infinite horizon)"""
    mu = handle.mu if mu is None else int(mu)
    if nK is None:
        nK = getattr(handle, "nK", None)
        if nK is None and hasattr(handle, "desc"):
            nK = handle.desc.nK or 1
        if nK is None:
            nK = handle.N - 1 if handle.N > 0 else 1
    K = np.zeros((int(nK), mu, 12 * mech.tables.nb))
    check(lib().cclqr_ctrl_get_gains(mech.ptr, handle.ptr, C.c_int64(int(table)), _d(K)))
    return K


class PlantsHandle(_Handle):
    """cclqr_plants*: device-resident per-instance plants of a tree mechanism.  mass [n][nb], inertia [n][nb][9], p1 / p2 [n][ne][3] in the mechanism's
    body / joint order, None = the mechanism's own value; host arrays, or (on_device=True) raw device addresses read on `stream`; n_plant must be given
    with device addresses.  first_index: global instance index of row 0."""
    _destroy = "cclqr_plants_destroy"

    def __init__(self, mech, mass=None, inertia=None, p1=None, p2=None, first_index=0, n_plant=None, on_device=False, stream=0):
        nb, ne = mech.tables.nb, mech.tables.ne
        self.mech = mech      # (the handle must not outlive the mechanism's)
        if on_device:
            args = [C.c_void_p(int(a)) if a else None for a in (mass, inertia, p1, p2)]
        else:
            arrs = [None if a is None else f64(a).reshape((-1,) + sh) for a, sh in ((mass, (nb,)), (inertia, (nb, 9)), (p1, (ne, 3)), (p2, (ne, 3)))]
            sizes = {a.shape[0] for a in arrs if a is not None}
            if len(sizes) > 1:
                raise ValueError("the plant arrays have different leading sizes: %s" % sorted(sizes))
            if n_plant is None:
                n_plant = sizes.pop() if sizes else 0
            elif sizes and sizes.pop() != n_plant:
                raise ValueError("the plant arrays do not have n_plant rows")
            self._arrs = arrs
            args = [_d(a) for a in arrs]
        self.n_plant, self.first_index = int(n_plant or 0), int(first_index)
        self.ptr = C.c_void_p()
        check(lib().cclqr_plants_create(mech.ptr, C.c_int64(self.n_plant), C.c_int64(self.first_index), args[0], args[1], args[2], args[3],
                                        C.c_int32(1 if on_device else 0), C.c_void_p(int(stream)) if stream else None, C.byref(self.ptr)))


def _rollout_plants(mech, ctrl, plants, z0, steps, k0, noise, record, first_instance, newton_mode, newton_eps_alone, flags):
    """rollout(..., plants=): cclqr_rollout_plants takes device pointers, so the batch is staged in torch tensors on the current device"""
    import torch
    n, nb = z0.shape[0], mech.tables.nb
    td = torch.device("cuda", torch.cuda.current_device())
    dz0 = torch.from_numpy(z0).to(td)
    dzT = torch.empty_like(dz0)
    dst = torch.zeros(n, dtype=torch.int32, device=td)
    dtraj = torch.empty((n, steps, nb, 13), dtype=torch.float64, device=td) if record else None
    dnoise = None if noise is None else torch.from_numpy(noise).to(td)
    stream = torch.cuda.current_stream().cuda_stream
    # noise is indexed by the absolute step k-1: the base is shifted so that k0 maps to column 0 of the caller's array
    rollout_dev(mech, ctrl, n, steps, k0, dz0.data_ptr(), 0, 0 if dnoise is None else dnoise.data_ptr() - 8 * (k0 - 1), steps, 0 if dtraj is None else dtraj.data_ptr(),
                dzT.data_ptr(), dst.data_ptr(), stream, first_instance=first_instance, newton_mode=newton_mode, newton_eps_alone=newton_eps_alone, flags=flags,
                plants=plants)
    torch.cuda.current_stream().synchronize()
    return dzT.cpu().numpy(), (dtraj.cpu().numpy() if record else None), dst.cpu().numpy()


def rollout(mech, ctrl, z0, steps, k0=1, noise=None, record=False, first_instance=0, newton_mode=0, newton_eps_alone=0.0, flags=0, plants=None):
    """host-pointer rollout: returns (zT, traj or None, status).  plants: a PlantsHandle -- instance i runs plant first_instance + i - plants.first_index"""
    nb = mech.tables.nb
    z0 = f64(z0).reshape(-1, nb, 13)
    n = z0.shape[0]
    if plants is not None:
        return _rollout_plants(mech, ctrl, plants, z0, steps, k0, None if noise is None else f64(noise).reshape(n, steps), record, first_instance,
                               newton_mode, newton_eps_alone, flags)
    traj = np.zeros((n, steps, nb, 13)) if record else None
    zT = np.zeros_like(z0)
    status = np.zeros(n, dtype=np.int32)
    noise = None if noise is None else f64(noise).reshape(n, steps)
    o = RolloutOpts(int(first_instance), None, 0, None, 0, int(newton_mode), int(flags), float(newton_eps_alone))
    check(lib().cclqr_rollout_host_ex(mech.ptr, ctrl.ptr, C.c_int64(n), C.c_int32(steps), C.c_int32(k0), _d(z0), _d(noise), _d(traj), _d(zT),
                                      _i(status), C.byref(o)))
    return zT, traj, status


def rollout_dev(mech, ctrl, n_inst, steps, k0, z0_ptr, lam_ptr, noise_ptr, noise_stride, traj_ptr, zT_ptr, status_ptr, stream=0,
                first_instance=None, pid_state=None, noise_ws=None, noise_ws_len=0, newton_mode=0, newton_eps_alone=0.0, flags=0, plants=None):
    """device-pointer rollout (integers are raw device addresses, e.g. torch.Tensor.data_ptr()); asynchronous.
    Options (cclqr_rollout_opts): first_instance, pid_state = device address of [n_inst][joints][2] doubles, noise_ws / noise_ws_len = caller's
    Philox workspace, newton_mode, flags (ROLLOUT_NO_ALLOC: what a caller with a hipGraph capture open passes; ROLLOUT_PACK_WAVEFRONTS); none given: cclqr_rollout_dev
    (= NULL options).  plants: a PlantsHandle (cclqr_rollout_plants) -- instance i runs plant first_instance + i - plants.first_index"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    if plants is None and first_instance is None and pid_state is None and noise_ws is None and not newton_mode and not flags:
        check(lib().cclqr_rollout_dev(mech.ptr, ctrl.ptr, C.c_int64(n_inst), C.c_int32(steps), C.c_int32(k0), vp(z0_ptr), vp(lam_ptr),
                                      vp(noise_ptr), C.c_int64(noise_stride), vp(traj_ptr), vp(zT_ptr), vp(status_ptr), vp(stream)))
        return
    o = RolloutOpts(int(first_instance or 0), int(pid_state) if pid_state else None, n_inst * mech.tables.ne * 2 if pid_state else 0,       # one pair per joint (a tree has nb joints, a loop mechanism more)
                    int(noise_ws) if noise_ws else None, int(noise_ws_len) if noise_ws else 0, int(newton_mode), int(flags), float(newton_eps_alone))
    if plants is not None:
        check(lib().cclqr_rollout_plants(mech.ptr, plants.ptr, ctrl.ptr, C.c_int64(n_inst), C.c_int32(steps), C.c_int32(k0), vp(z0_ptr), vp(lam_ptr),
                                         vp(noise_ptr), C.c_int64(noise_stride), vp(traj_ptr), vp(zT_ptr), vp(status_ptr), C.byref(o), vp(stream)))
        return
    check(lib().cclqr_rollout_ex(mech.ptr, ctrl.ptr, C.c_int64(n_inst), C.c_int32(steps), C.c_int32(k0), vp(z0_ptr), vp(lam_ptr),
                                 vp(noise_ptr), C.c_int64(noise_stride), vp(traj_ptr), vp(zT_ptr), vp(status_ptr), C.byref(o), vp(stream)))


class ScoreHandle(_Handle):
    """cclqr_score*: the device-resident weights a rollout is scored with.  Qb [nb][12][12] per-body blocks in the mechanism's body order, R [mu][mu], both already
    Δt-scaled (lqr.jl:18-19); settle_tol: the stage cost above which an instance counts as not settled (last_out)"""
    _destroy = "cclqr_score_destroy"

    def __init__(self, mech, Qb, R, settle_tol=0.0):
        nb = mech.tables.nb
        Qb = f64(Qb).reshape(nb, 12, 12)
        R = f64(R)
        mu = int(round(np.sqrt(R.size)))
        if mu * mu != R.size:
            raise ValueError("R must be [mu][mu] (got %d entries)" % R.size)
        R = R.reshape(mu, mu)
        self.mech, self.mu, self.settle_tol = mech, mu, float(settle_tol)      # (the handle must not outlive the mechanism's)
        self._arrs = [Qb, R]
        self.ptr = C.c_void_p()
        check(lib().cclqr_score_create(mech.ptr, _d(Qb), C.c_int32(mu), _d(R) if mu else None, C.c_double(self.settle_tol), C.byref(self.ptr)))


def rollout_score(mech, ctrl, score, n_inst, steps, k0, traj_ptr, score_ptr, stream=0, first_instance=0):
    """cclqr_rollout_score on device addresses (asynchronous on `stream`): scores the slab traj [n_inst][steps][nb][13] a rollout launch has just written into
    score [n_inst][SCORE_LEN] (read when k0 > 1, always written)"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    check(lib().cclqr_rollout_score(mech.ptr, ctrl.ptr, score.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(k0)), C.c_int64(int(first_instance)),
                                    vp(traj_ptr), vp(score_ptr), vp(stream)))


def chunk_plan(steps, chunk_steps):
    """the launches of a chunked horizon: [(k0, steps of the launch), ...] covering the steps 1 .. steps exactly once, in order"""
    steps, chunk_steps = int(steps), int(chunk_steps)
    if steps < 1 or chunk_steps < 1:
        raise ValueError("need steps >= 1 and chunk_steps >= 1 (got %d, %d)" % (steps, chunk_steps))
    return [(k0, min(chunk_steps, steps - k0 + 1)) for k0 in range(1, steps + 1, chunk_steps)]


def default_chunk_steps(n_inst, nb, steps, slab_bytes=1 << 30):
    """the largest chunk whose slab [n_inst][chunk][nb][13] of doubles stays under slab_bytes (at least one step)"""
    return max(1, min(int(steps), int(slab_bytes) // max(1, int(n_inst) * int(nb) * 13 * 8)))


ENSEMBLE_MAX_COV = 64   # listed steps of one cclqr_rollout_ensemble call


def rollout_ensemble_ws_bytes(mech, mu, n_inst, steps, n_cov):
    """cclqr_rollout_ensemble_ws_bytes: bytes of device workspace one cclqr_rollout_ensemble call of these sizes needs"""
    out = C.c_size_t(0)
    check(lib().cclqr_rollout_ensemble_ws_bytes(mech.ptr, C.c_int32(int(mu)), C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(n_cov)), C.byref(out)))
    return int(out.value)


def rollout_ensemble(mech, ctrl, n_inst, steps, k0, traj_ptr, mean_ptr, m2_ptr, ws_ptr, ws_bytes, cov_steps=(), cov_ptr=0, stream=0, first_instance=0):
    """cclqr_rollout_ensemble on device addresses (asynchronous on `stream`): per row of the slab traj [n_inst][steps][nb][13] the mean and the centred sum of squares
    of (Δz, Δu) across the instances into mean / m2 [steps][12 nb + mu], and for the absolute steps cov_steps (host integers within k0 .. k0 + steps - 1) the centred
    co-moment matrices of Δz into cov [len(cov_steps)][12 nb][12 nb]"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    cs = i32(list(cov_steps)).reshape(-1)
    check(lib().cclqr_rollout_ensemble(mech.ptr, ctrl.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(k0)), C.c_int64(int(first_instance)),
                                       vp(traj_ptr), vp(mean_ptr), vp(m2_ptr), C.c_int32(len(cs)), _i(cs) if len(cs) else None, vp(cov_ptr),
                                       vp(ws_ptr), C.c_size_t(int(ws_bytes)), vp(stream)))


QUANTILE_MAX_INST = 16384    # CCLQR_QUANTILE_MAX_INST: instances of one cclqr_rollout_quantiles call
QUANTILE_MAX_PROBS = 16      # CCLQR_QUANTILE_MAX_PROBS


def quantile_probs(probs):
    """the probabilities of a quantile request as a float64 vector: 0 .. QUANTILE_MAX_PROBS of them (none: no request), each in [0, 1]"""
    p = f64(list(probs)).reshape(-1)
    if len(p) > QUANTILE_MAX_PROBS:
        raise ValueError("at most %d quantile probabilities per run (got %d)" % (QUANTILE_MAX_PROBS, len(p)))
    if not ((p >= 0.0) & (p <= 1.0)).all():
        raise ValueError("quantile probabilities must lie in [0, 1] (got %s)" % p.tolist())
    return p


def rollout_quantiles_ws_bytes(mech, mu, n_inst, steps):
    """cclqr_rollout_quantiles_ws_bytes: (min_bytes, full_bytes) of device workspace -- one slab row, all `steps` rows"""
    lo, full = C.c_size_t(0), C.c_size_t(0)
    check(lib().cclqr_rollout_quantiles_ws_bytes(mech.ptr, C.c_int32(int(mu)), C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.byref(lo), C.byref(full)))
    return int(lo.value), int(full.value)


def rollout_quantiles(mech, ctrl, n_inst, steps, k0, traj_ptr, probs, quant_ptr, finite_ptr, ws_ptr, ws_bytes, stream=0, first_instance=0):
    """cclqr_rollout_quantiles on device addresses (asynchronous on `stream`): per row of the slab traj [n_inst][steps][nb][13] and per coordinate of (Δz, Δu) the
    quantiles of its finite values across the instances at the probabilities `probs` (host numbers) into quant [steps][len(probs)][12 nb + mu], and their number into
    finite [steps][12 nb + mu] (int32; 0: not wanted)"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    pr = f64(list(probs)).reshape(-1)
    check(lib().cclqr_rollout_quantiles(mech.ptr, ctrl.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(k0)), C.c_int64(int(first_instance)),
                                        vp(traj_ptr), C.c_int32(len(pr)), _d(pr) if len(pr) else None, vp(quant_ptr), vp(finite_ptr),
                                        vp(ws_ptr), C.c_size_t(int(ws_bytes)), vp(stream)))


JOINTS_RAW, JOINTS_CONTINUOUS = 0, 1      # CCLQR_JOINTS_RAW / CCLQR_JOINTS_CONTINUOUS: the mode of cclqr_rollout_joints
SERIES_MAX_COORDS = 1024                  # CCLQR_SERIES_MAX_COORDS


def rollout_joints(mech, n_inst, steps, k0, traj_ptr, mode, out_steps, theta_ptr, rate_ptr=0, carry_ptr=0, stream=0, first_instance=0, plants=None):
    """cclqr_rollout_joints on device addresses (asynchronous on `stream`): the joint coordinate (and, with rate_ptr, the relative joint velocity) of every joint at
    every row of the slab traj [n_inst][steps][nb][13] into the rows k0 - 1 .. k0 + steps - 2 of theta / rate [n_inst][out_steps][ne]; mode JOINTS_CONTINUOUS
    carries (w_prev, turns) in carry [n_inst][ne][2] from launch to launch.  plants: a PlantsHandle -- instance i reads the vertices of plant first_instance + i"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    check(lib().cclqr_rollout_joints(mech.ptr, None if plants is None else plants.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(k0)),
                                     C.c_int64(int(first_instance)), vp(traj_ptr), C.c_int32(int(mode)), C.c_int64(int(out_steps)), vp(theta_ptr), vp(rate_ptr),
                                     vp(carry_ptr), vp(stream)))


def series_ensemble_ws_bytes(n_inst, steps, nc):
    """cclqr_series_ensemble_ws_bytes: bytes of device workspace one cclqr_series_ensemble call of these sizes needs"""
    out = C.c_size_t(0)
    check(lib().cclqr_series_ensemble_ws_bytes(C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(nc)), C.byref(out)))
    return int(out.value)


def series_ensemble(n_inst, steps, nc, x_ptr, mean_ptr, m2_ptr, ws_ptr, ws_bytes, stream=0):
    """cclqr_series_ensemble on device addresses (asynchronous on `stream`): per step the mean and the centred sum of squares of every coordinate of the series
    x [n_inst][steps][nc] across the instances into mean / m2 [steps][nc]"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    check(lib().cclqr_series_ensemble(C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(nc)), vp(x_ptr), vp(mean_ptr), vp(m2_ptr), vp(ws_ptr),
                                      C.c_size_t(int(ws_bytes)), vp(stream)))


def series_quantiles_ws_bytes(n_inst, steps, nc):
    """cclqr_series_quantiles_ws_bytes: (min_bytes, full_bytes) of device workspace -- one row of the series, all `steps` rows"""
    lo, full = C.c_size_t(0), C.c_size_t(0)
    check(lib().cclqr_series_quantiles_ws_bytes(C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(nc)), C.byref(lo), C.byref(full)))
    return int(lo.value), int(full.value)


def series_quantiles(n_inst, steps, nc, x_ptr, probs, quant_ptr, finite_ptr, ws_ptr, ws_bytes, stream=0):
    """cclqr_series_quantiles on device addresses (asynchronous on `stream`): per step and coordinate of the series x [n_inst][steps][nc] the quantiles of its finite
    values across the instances at the probabilities `probs` (host numbers) into quant [steps][len(probs)][nc], and their number into finite [steps][nc] (int32; 0:
    not wanted)"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    pr = f64(list(probs)).reshape(-1)
    check(lib().cclqr_series_quantiles(C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(nc)), vp(x_ptr), C.c_int32(len(pr)), _d(pr) if len(pr) else None,
                                       vp(quant_ptr), vp(finite_ptr), vp(ws_ptr), C.c_size_t(int(ws_bytes)), vp(stream)))


def _joint_series_results(td, stream, n, steps, ne, continuous, rates, keep, probs, jth, jrt):
    """the statistics of the finished joint series across the instances: one cclqr_series_ensemble and, with probs, one cclqr_series_quantiles over
    [n][steps][ne] (rates: [n][steps][2 ne] = theta, then the rate).  Returns the dict JointSeries is built from"""
    import torch
    nc = 2 * ne if rates else ne
    x = torch.cat((jth, jrt), dim=2).contiguous() if rates else jth
    mean = torch.empty((steps, nc), dtype=torch.float64, device=td)
    m2 = torch.empty((steps, nc), dtype=torch.float64, device=td)
    wb = series_ensemble_ws_bytes(n, steps, nc)
    ws = torch.empty(wb // 8 + 1, dtype=torch.float64, device=td)
    series_ensemble(n, steps, nc, x.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), wb, stream)
    out = dict(count=n, continuous=bool(continuous), mean=None, M2=None, rate_mean=None, rate_M2=None, probs=None, quantiles=None, finite_count=None, theta=None, rate=None)
    if len(probs):
        quant = torch.empty((steps, len(probs), nc), dtype=torch.float64, device=td)
        fin = torch.empty((steps, nc), dtype=torch.int32, device=td)
        qb = series_quantiles_ws_bytes(n, steps, nc)[1]
        qws = torch.empty(qb // 8 + 1, dtype=torch.float64, device=td)
        series_quantiles(n, steps, nc, x.data_ptr(), probs, quant.data_ptr(), fin.data_ptr(), qws.data_ptr(), qb, stream)
    torch.cuda.current_stream().synchronize()
    mean, m2 = mean.cpu().numpy(), m2.cpu().numpy()
    out["mean"], out["M2"] = mean[:, :ne], m2[:, :ne]
    if rates:
        out["rate_mean"], out["rate_M2"] = mean[:, ne:], m2[:, ne:]
    if len(probs):
        out["probs"], out["quantiles"], out["finite_count"] = tuple(float(p) for p in probs), quant.cpu().numpy(), fin.cpu().numpy()
    if keep:
        out["theta"] = jth.cpu().numpy()
        out["rate"] = jrt.cpu().numpy() if rates else None
    return out


INVARIANTS_LEN = 6            # CCLQR_INVARIANTS_LEN: T, V, E, gap, twist, quat per instance and step (cclqr_rollout_invariants)
INVARIANTS_SUMMARY_LEN = 8    # CCLQR_INVARIANTS_SUMMARY_LEN: E_first, E_min, E_max, gap_max, gap_step, twist_max, quat_max, bad_rows per instance


def rollout_invariants(mech, n_inst, steps, k0, traj_ptr, out_steps, inv_ptr=0, rows_ptr=0, summary_ptr=0, stream=0, first_instance=0, plants=None):
    """cclqr_rollout_invariants on device addresses (asynchronous on `stream`): T, V, E, gap, twist, quat of every row of the slab traj [n_inst][steps][nb][13] into
    the rows k0 - 1 .. k0 + steps - 2 of inv [n_inst][out_steps][6], the constraint rows themselves into rows [n_inst][out_steps][ne][5], and the per-instance
    summary [n_inst][8], which is read when k0 > 1 and travels from launch to launch; any of the three may be 0.  plants: a PlantsHandle -- instance i reads the
    masses, inertias and vertices of plant first_instance + i"""
    vp = lambda p: C.c_void_p(int(p)) if p else None
    check(lib().cclqr_rollout_invariants(mech.ptr, None if plants is None else plants.ptr, C.c_int64(int(n_inst)), C.c_int32(int(steps)), C.c_int32(int(k0)),
                                         C.c_int64(int(first_instance)), vp(traj_ptr), C.c_int64(int(out_steps)), vp(inv_ptr), vp(rows_ptr), vp(summary_ptr), vp(stream)))


def _invariant_series_results(td, stream, n, steps, ne, keep, rows, probs, inv, grows, summ):
    """the finished invariants: the summary, the kept series, and the statistics of the series [n][steps][6] across the instances by one cclqr_series_ensemble and,
    with probs, one cclqr_series_quantiles.  Returns the dict InvariantSeries is built from"""
    import torch
    nc = INVARIANTS_LEN
    mean = torch.empty((steps, nc), dtype=torch.float64, device=td)
    m2 = torch.empty((steps, nc), dtype=torch.float64, device=td)
    wb = series_ensemble_ws_bytes(n, steps, nc)
    ws = torch.empty(wb // 8 + 1, dtype=torch.float64, device=td)
    series_ensemble(n, steps, nc, inv.data_ptr(), mean.data_ptr(), m2.data_ptr(), ws.data_ptr(), wb, stream)
    out = dict(count=n, mean=None, M2=None, probs=None, quantiles=None, finite_count=None, series=None, g=None, summary=None)
    if len(probs):
        quant = torch.empty((steps, len(probs), nc), dtype=torch.float64, device=td)
        fin = torch.empty((steps, nc), dtype=torch.int32, device=td)
        qb = series_quantiles_ws_bytes(n, steps, nc)[1]
        qws = torch.empty(qb // 8 + 1, dtype=torch.float64, device=td)
        series_quantiles(n, steps, nc, inv.data_ptr(), probs, quant.data_ptr(), fin.data_ptr(), qws.data_ptr(), qb, stream)
    torch.cuda.current_stream().synchronize()
    out["mean"], out["M2"], out["summary"] = mean.cpu().numpy(), m2.cpu().numpy(), summ.cpu().numpy()
    if len(probs):
        out["probs"], out["quantiles"], out["finite_count"] = tuple(float(p) for p in probs), quant.cpu().numpy(), fin.cpu().numpy()
    if keep:
        out["series"] = inv.cpu().numpy()
    if rows:
        out["g"] = grows.cpu().numpy()
    return out


def rollout_scored(mech, ctrl, score, z0, steps, chunk_steps, noise=None, first_instance=0, plants=None, newton_mode=0, newton_eps_alone=0.0, flags=0, traj_out=None,
                   ensemble=None, joints=None, invariants=None):
    """A horizon rolled out AND scored on the device without its trajectory ever existing: ceil(steps / chunk_steps) launches of cclqr_rollout_ex (plants:
    cclqr_rollout_plants) into ONE slab of chunk_steps rows, each followed on the same stream by cclqr_rollout_score.  The state, the multipliers, the status
    (ROLLOUT_CARRY_STATUS), the PID state and the noise column travel from launch to launch, so the result is bitwise that of one launch.
    noise [n_inst][steps] injected samples or None.  traj_out: a numpy array [n_inst][steps][nb][13] that receives the slabs (the recorded run), or None.
    score: a ScoreHandle, or None = no score pass.  ensemble: None, or (mu, cov_rows) -- cclqr_rollout_ensemble runs behind every launch on the same slab, and the
    0-based rows of the horizon in cov_rows (row j = step j + 1) get their co-moment matrix, each from the chunk that holds it --, or (mu, cov_rows, probs):
    cclqr_rollout_quantiles runs behind the ensemble call on the same slab, with a workspace of as many rows as the chunk has.
    joints: None (nothing changes, nothing is allocated), or (continuous, rates, keep, probs) -- behind every launch cclqr_rollout_joints runs on the same slab and
    stream into whole-horizon device arrays [n_inst][steps][ne], the carry buffer travelling from chunk to chunk; after the last chunk one cclqr_series_ensemble and,
    with probs, one cclqr_series_quantiles reduce them across the instances.
    invariants: None (nothing changes, nothing is allocated), or (keep, rows, probs) -- behind every launch cclqr_rollout_invariants runs on the same slab and stream
    into a whole-horizon device array [n_inst][steps][6] (rows: and [n_inst][steps][ne][5]), the summary [n_inst][8] travelling from chunk to chunk; after the last
    chunk the series is reduced across the instances as the joint series is.
    Returns (zT, status, score [n_inst][SCORE_LEN] or None), with ensemble a fourth element (mean [steps][12 nb + mu], M2 the same, {row: C [12 nb][12 nb]}), which
    the three-element form extends by (quant [steps][len(probs)][12 nb + mu], finite [steps][12 nb + mu]); with joints a further element, the dict of
    _joint_series_results, and with invariants a last one, the dict of _invariant_series_results."""
    import torch
    nb, ne = mech.tables.nb, mech.tables.ne
    z0 = f64(z0).reshape(-1, nb, 13)
    n = z0.shape[0]
    plan = chunk_plan(steps, chunk_steps)
    rows = plan[0][1]
    if ensemble is not None:      # (before anything touches the device)
        mu, cov_rows = int(ensemble[0]), sorted({int(j) for j in ensemble[1]})
        if cov_rows and (cov_rows[0] < 0 or cov_rows[-1] >= steps):
            raise ValueError("cov_knots must lie in 0 .. steps - 1 = %d (got %s)" % (steps - 1, cov_rows))
        cov_of = [[j + 1 for j in cov_rows if k0 <= j + 1 < k0 + s] for k0, s in plan]
        if max(len(c) for c in cov_of) > ENSEMBLE_MAX_COV:
            raise ValueError("more than %d cov_knots fall into one chunk: lower chunk_steps" % ENSEMBLE_MAX_COV)
        probs = quantile_probs(ensemble[2]) if len(ensemble) > 2 else ()
        if len(probs) and n > QUANTILE_MAX_INST:
            raise ValueError("quantiles are taken over at most %d instances per call (got %d)" % (QUANTILE_MAX_INST, n))
    if joints is not None:        # (before anything touches the device)
        jcont, jrates, jkeep = bool(joints[0]), bool(joints[1]), bool(joints[2])
        jprobs = quantile_probs(joints[3])
        if len(jprobs) and n > QUANTILE_MAX_INST:
            raise ValueError("quantiles are taken over at most %d instances per call (got %d)" % (QUANTILE_MAX_INST, n))
        if (2 * ne if jrates else ne) > SERIES_MAX_COORDS:
            raise ValueError("a series has at most %d coordinates" % SERIES_MAX_COORDS)
    if invariants is not None:    # (before anything touches the device)
        ikeep, irows = bool(invariants[0]), bool(invariants[1])
        iprobs = quantile_probs(invariants[2])
        if len(iprobs) and n > QUANTILE_MAX_INST:
            raise ValueError("quantiles are taken over at most %d instances per call (got %d)" % (QUANTILE_MAX_INST, n))
    td = torch.device("cuda", torch.cuda.current_device())
    z = torch.from_numpy(z0).to(td)
    zn = torch.empty_like(z)
    lam = torch.zeros((n, 5 * ne), dtype=torch.float64, device=td)
    st = torch.zeros(n, dtype=torch.int32, device=td)
    pid = torch.zeros((n, ne, 2), dtype=torch.float64, device=td)
    sc = None if score is None else torch.zeros((n, SCORE_LEN), dtype=torch.float64, device=td)
    slab = torch.empty((n, rows, nb, 13), dtype=torch.float64, device=td)
    dnoise = None if noise is None else torch.from_numpy(f64(noise).reshape(n, steps)).to(td)
    stream = torch.cuda.current_stream().cuda_stream
    if ensemble is not None:
        nx, mx, most = 12 * nb + mu, 12 * nb, max(1, max(len(c) for c in cov_of))
        emean = torch.empty((steps, nx), dtype=torch.float64, device=td)
        em2 = torch.empty((steps, nx), dtype=torch.float64, device=td)
        ecov = torch.empty((max(1, len(cov_rows)), mx, mx), dtype=torch.float64, device=td)
        ws_bytes = rollout_ensemble_ws_bytes(mech, mu, n, rows, most if cov_rows else 0)
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=td)
        cov_done = 0
        if len(probs):
            equant = torch.empty((steps, len(probs), nx), dtype=torch.float64, device=td)
            efin = torch.empty((steps, nx), dtype=torch.int32, device=td)
            qws_bytes = rollout_quantiles_ws_bytes(mech, mu, n, rows)[1]
            qws = torch.empty(qws_bytes // 8 + 1, dtype=torch.float64, device=td)
    if joints is not None:
        jth = torch.empty((n, steps, ne), dtype=torch.float64, device=td)
        jrt = torch.empty((n, steps, ne), dtype=torch.float64, device=td) if jrates else None
        jcarry = torch.zeros((n, ne, 2), dtype=torch.float64, device=td) if jcont else None
    if invariants is not None:
        iser = torch.empty((n, steps, INVARIANTS_LEN), dtype=torch.float64, device=td)
        igr = torch.empty((n, steps, ne, 5), dtype=torch.float64, device=td) if irows else None
        isum = torch.zeros((n, INVARIANTS_SUMMARY_LEN), dtype=torch.float64, device=td)
    for ci, (k0, s) in enumerate(plan):
        # the noise array is indexed by the absolute step k - 1: its base stays where it is whatever k0 is
        rollout_dev(mech, ctrl, n, s, k0, z.data_ptr(), lam.data_ptr(), 0 if dnoise is None else dnoise.data_ptr(), steps, slab.data_ptr(), zn.data_ptr(),
                    st.data_ptr(), stream, first_instance=first_instance, pid_state=pid.data_ptr(), newton_mode=newton_mode, newton_eps_alone=newton_eps_alone,
                    flags=flags | ROLLOUT_CARRY_STATUS, plants=plants)
        if score is not None:
            rollout_score(mech, ctrl, score, n, s, k0, slab.data_ptr(), sc.data_ptr(), stream, first_instance=first_instance)
        if ensemble is not None:      # (a chunk's statistics are complete: every instance of its steps is in the slab)
            rollout_ensemble(mech, ctrl, n, s, k0, slab.data_ptr(), emean[k0 - 1:].data_ptr(), em2[k0 - 1:].data_ptr(), ws.data_ptr(), ws_bytes,
                             cov_steps=cov_of[ci], cov_ptr=ecov[cov_done:].data_ptr() if cov_of[ci] else 0, stream=stream, first_instance=first_instance)
            cov_done += len(cov_of[ci])
            if len(probs):
                rollout_quantiles(mech, ctrl, n, s, k0, slab.data_ptr(), probs, equant[k0 - 1:].data_ptr(), efin[k0 - 1:].data_ptr(), qws.data_ptr(), qws_bytes,
                                  stream=stream, first_instance=first_instance)
        if joints is not None:
            rollout_joints(mech, n, s, k0, slab.data_ptr(), JOINTS_CONTINUOUS if jcont else JOINTS_RAW, steps, jth.data_ptr(), 0 if jrt is None else jrt.data_ptr(),
                           0 if jcarry is None else jcarry.data_ptr(), stream, first_instance=first_instance, plants=plants)
        if invariants is not None:
            rollout_invariants(mech, n, s, k0, slab.data_ptr(), steps, iser.data_ptr(), 0 if igr is None else igr.data_ptr(), isum.data_ptr(), stream,
                               first_instance=first_instance, plants=plants)
        if traj_out is not None:      # (a launch of s < rows steps fills the slab as [n][s][nb][13] from its base)
            traj_out[:, k0 - 1:k0 - 1 + s] = slab.reshape(-1)[:n * s * nb * 13].reshape(n, s, nb, 13).cpu().numpy()
        z, zn = zn, z
    jres = () if joints is None else (_joint_series_results(td, stream, n, steps, ne, jcont, jrates, jkeep, jprobs, jth, jrt),)
    if invariants is not None:
        jres += (_invariant_series_results(td, stream, n, steps, ne, ikeep, irows, iprobs, iser, igr, isum),)
    torch.cuda.current_stream().synchronize()
    out = (z.cpu().numpy(), st.cpu().numpy(), None if sc is None else sc.cpu().numpy())
    if ensemble is None:
        return out + jres
    covs = ecov.cpu().numpy()
    stats = (emean.cpu().numpy(), em2.cpu().numpy(), {j: covs[q] for q, j in enumerate(cov_rows)})
    if len(probs):
        stats += (equant.cpu().numpy(), efin.cpu().numpy())
    return out + (stats,) + jres


def linearize(mech, zd, ctrl_joint, Fd=None, plants=None, first_plant=0):
    """batched linearsystem: zd [nk][nb][13] -> A [nk][mx][mx], Bu, Bl, G.  plants: a PlantsHandle (cclqr_linearize_plants) -- knot k is linearised on the
    plant with global index first_plant + k"""
    t = mech.tables
    zd = f64(zd).reshape(-1, t.nb, 13)
    nk = zd.shape[0]
    cj = i32(ctrl_joint).reshape(-1)
    mu, mx, ml = len(cj), 12 * t.nb, 5 * t.ne
    Fd = f64(np.zeros((nk, mu)) if Fd is None else Fd).reshape(nk, mu)
    A, Bu, Bl, G = np.zeros((nk, mx, mx)), np.zeros((nk, mx, mu)), np.zeros((nk, mx, ml)), np.zeros((nk, ml, mx))
    tail = (C.c_int32(nk), _d(zd), C.c_int32(mu), _i(cj), _d(Fd), _d(A), _d(Bu), _d(Bl), _d(G))
    if plants is None:
        check(lib().cclqr_linearize(mech.ptr, *tail))
    else:
        check(lib().cclqr_linearize_plants(mech.ptr, plants.ptr, C.c_int64(int(first_plant)), *tail))
    return A, Bu, Bl, G


def linearize_projected(mech, zd, ctrl_joint, Fd=None, h=0.0):
    """projected linear model (A', D) of the constrained step map: zd [nk][nb][13] -> A' [nk][mx][mx], D [nk][mx][mu] (cclqr_linearize_projected;
    any topology, the only linearisation of closed-loop mechanisms).  h <= 0: analytic on the device; h > 0: central differences of the device's step"""
    t = mech.tables
    zd = f64(zd).reshape(-1, t.nb, 13)
    nk = zd.shape[0]
    cj = i32(ctrl_joint).reshape(-1)
    mu, mx = len(cj), 12 * t.nb
    Fd = f64(np.zeros((nk, mu)) if Fd is None else Fd).reshape(nk, mu)
    Ap, D = np.zeros((nk, mx, mx)), np.zeros((nk, mx, mu))
    check(lib().cclqr_linearize_projected(mech.ptr, C.c_int32(nk), _d(zd), C.c_int32(mu), _i(cj), _d(Fd), C.c_double(float(h)), _d(Ap), _d(D)))
    return Ap, D


def riccati(A, Bu, Bl, G, Q, R, N, tol=1e-5, path=0, bf16_terms=0, keep_last=False):
    """batched dlqr: A [nprob][mx][mx] (or [mx][mx]) -> K [nprob][N-1][mu][mx], kbreak [nprob].
    path: 0 auto / 1 resident / 2 tiled; bf16_terms: 0 = fp64 MFMA (parity), 1..3 = split-bf16 measured-error mode (cclqr_riccati_opts);
    keep_last: K [nprob][1][mu][mx] = Ku[1] only (LQR{T,Inf})"""
    single = np.ndim(A) == 2
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    Q, R = f64(Q).reshape(mx, mx), f64(R).reshape(mu, mu)
    K = np.zeros((nprob, (1 if keep_last else N - 1) if N > 1 else 0, mu, mx))
    kb = np.zeros(nprob, dtype=np.int32)
    o = RiccatiOpts(int(path), int(bf16_terms), 1 if keep_last else 0, 0)
    check(lib().cclqr_riccati_ex(*_model_args(dims, models), _d(Q), _panel(R), C.c_int32(N), C.c_double(tol), _d(K), _i(kb), C.byref(o)))
    return (K[0], int(kb[0])) if single else (K, kb)


def riccati_weights(A, Bu, Bl, G, Q, R, N, tol=1e-5, path=0, bf16_terms=0, keep_last=False, K=None):
    """batched dlqr with one pair of weights per problem (cclqr_riccati_weights): A [nprob][mx][mx], Q [n_weights][mx][mx], R [n_weights][mu][mu] with n_weights = 1
    or nprob (the library refuses anything else) -> K [nprob][N-1][mu][mx], kbreak [nprob].  path, bf16_terms, keep_last as riccati.  K: the array to fill
    (default: a new one)"""
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    Q, R, nw = _weights(Q, R, mx, mu)
    shape = (nprob, (1 if keep_last else N - 1) if N > 1 else 0, mu, mx)
    if K is None:
        K = np.zeros(shape)
    if K.shape != shape or K.dtype != np.float64 or not K.flags.c_contiguous:
        raise ValueError("K must be a contiguous float64 array of shape %s" % (shape,))
    kb = np.zeros(nprob, dtype=np.int32)
    o = RiccatiOpts(int(path), int(bf16_terms), 1 if keep_last else 0, 0)
    check(lib().cclqr_riccati_weights(*_model_args(dims, models), C.c_int32(nw), _d(Q), _panel(R), C.c_int32(N), C.c_double(tol), _d(K), _i(kb), C.byref(o)))
    return K, kb


def riccati_value(A, Bu, Bl, G, Q, R, N, tol=1e-5, path=0, bf16_terms=0, keep_last=False, time_varying=False, want_P=True):
    """batched dlqr that also returns the cost-to-go (cclqr_riccati_value): A [nprob][mx][mx] -- with time_varying [nprob][N-1][mx][mx], the model of backward step k at
    index k - 1 -- Q [n_weights][mx][mx], R [n_weights][mu][mu] with n_weights = 1 or nprob -> K [nprob][N-1][mu][mx], P [nprob][mx][mx], kbreak [nprob].  P[p] is the
    Pkp1 (lqr.jl:170) of the last backward step problem p executed, Q_p when N = 1.  want_P=False passes P = NULL (P is returned as None)"""
    models, dims = _models(A, Bu, Bl, G, per=(N - 1) if time_varying else 1)
    nprob, mx, mu, ml = dims
    Q, R, nw = _weights(Q, R, mx, mu)
    K = np.zeros((nprob, (1 if keep_last else N - 1) if N > 1 else 0, mu, mx))
    P = np.zeros((nprob, mx, mx)) if want_P else None
    kb = np.zeros(nprob, dtype=np.int32)
    o = RiccatiOpts(int(path), int(bf16_terms), 1 if keep_last else 0, 0)
    check(lib().cclqr_riccati_value(*_model_args(dims, models), C.c_int32(nw), _d(Q), _panel(R), C.c_int32(int(N)), C.c_double(float(tol)),
                                    C.c_int32(1 if time_varying else 0), _d(K), _d(P), _i(kb), C.byref(o)))
    return K, P, kb


def policy_value(A, Bu, Bl, G, K, Q, R, N, tol=1e-5, path=0, bf16_terms=0, want_diag=True):
    """batched policy evaluation (cclqr_policy_value): dlqr's cost recursion (lqr.jl:147-177) with the gains given.  A [nprob][mx][mx] (or [mx][mx]), Bu, Bl, G per
    problem; K [nK][mu][mx] (one table shared by all) or [n_gains][nK][mu][mx] with n_gains = nprob, nK = 1 (a stationary gain) or N - 1; Q [n_weights][mx][mx],
    R [n_weights][mu][mu] with n_weights = 1 or nprob (the library refuses any other count) -> P [nprob][mx][mx], kbreak [nprob], dnorm [nprob][2] (the norm(Pk - Pkp1)
    of the last executed step and of the step before it; NaN where no such step ran).  path: 0 auto / 1 resident / 2 tiled.  want_diag=False passes kbreak = dnorm =
    NULL (both are returned as None)"""
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    K = _gains(K, mu, mx, full=4, lowest=3)
    Q, R, nw = _weights(Q, R, mx, mu)
    P = np.zeros((nprob, mx, mx))
    kb = np.zeros(nprob, dtype=np.int32) if want_diag else None
    dn = np.zeros((nprob, 2)) if want_diag else None
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_policy_value(*_model_args(dims, models), C.c_int32(K.shape[0]), C.c_int32(K.shape[1]), _panel(K), C.c_int32(nw), _d(Q), _panel(R),
                                   C.c_int32(int(N)), C.c_double(float(tol)), _d(P), _i(kb), _d(dn), C.byref(o)))
    return P, kb, dn


def value_create_policy(mech, ctrl, zd, ctrl_joint, Q, R, N, tol=1e-5, Fd=None, plants=None, first_plant=0):
    """cclqr_value_create_policy: the policy evaluation of controller handle `ctrl` (its device-resident gains: one table, or one per model) on the models linearised at
    zd [n_models][nb][13], setpoint k on plant first_plant + k of the PlantsHandle `plants` (None: the mechanism's own plant).  Q [n_weights][12 nb][12 nb],
    R [n_weights][mu][mu], n_weights = 1 or n_models -> (ValueHandle of n_models tables, kbreak [n_models], dnorm [n_models][2])"""
    n, head = _setpoint_args(mech, ctrl, zd, ctrl_joint, Fd, Q, R, plants, first_plant)
    kb = np.zeros(n, dtype=np.int32)
    dn = np.zeros((n, 2))
    vptr = C.c_void_p()
    check(lib().cclqr_value_create_policy(*head, C.c_int32(int(N)), C.c_double(float(tol)), _i(kb), _d(dn), C.byref(vptr)))
    return ValueHandle(mech, ptr=vptr, n_tables=n), kb, dn


def policy_value_doubling(A, Bu, Bl, G, K, Q, R, N, tol=1e-5, max_levels=40, path=0, bf16_terms=0, want_diag=True):
    """a stationary gain's cost-to-go by doubling (cclqr_policy_value_doubling; lqr.jl:169-170 with the one gain of lqr.jl:40-43).  Models and weights as for
    policy_value; K [mu][mx] (one gain shared by all) or [n_gains][mu][mx] with n_gains = nprob.  N >= 1: N - 1 steps exactly; N = 0: level by level to convergence
    (increment < tol, at most max_levels levels) -> P [nprob][mx][mx], levels [nprob], reason [nprob] (0 converged, 1 max_levels, 2 norm(M) > 1e50), dnorm [nprob][2],
    gnorm [nprob][2] (the increment norms and norm(M) of the last level and of the one before; NaN where no such level ran).  want_diag=False passes NULL for the
    four diagnostics (returned as None)"""
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    K = _gains(K, mu, mx, full=3, lowest=2)
    Q, R, nw = _weights(Q, R, mx, mu)
    P = np.zeros((nprob, mx, mx))
    lv, rs, dn, gn = _diagnostics(nprob, want_diag)
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_policy_value_doubling(*_model_args(dims, models), C.c_int32(K.shape[0]), _panel(K), C.c_int32(nw), _d(Q), _panel(R), C.c_int32(int(N)),
                                            C.c_double(float(tol)), C.c_int32(int(max_levels)), _d(P), _i(lv), _i(rs), _d(dn), _d(gn), C.byref(o)))
    return P, lv, rs, dn, gn


def value_create_policy_doubling(mech, ctrl, zd, ctrl_joint, Q, R, N, tol=1e-5, max_levels=40, Fd=None, plants=None, first_plant=0):
    """cclqr_value_create_policy_doubling: the doubling evaluation of controller handle `ctrl`'s stationary gain (one table, or one per model; one row each) on the models
    linearised as for value_create_policy.  N >= 1 knots, or 0 = to convergence -> (ValueHandle of n_models tables, levels, reason, dnorm [n][2], gnorm [n][2])"""
    n, head = _setpoint_args(mech, ctrl, zd, ctrl_joint, Fd, Q, R, plants, first_plant)
    lv, rs, dn, gn = _diagnostics(n)
    vptr = C.c_void_p()
    check(lib().cclqr_value_create_policy_doubling(*head, C.c_int32(int(N)), C.c_double(float(tol)), C.c_int32(int(max_levels)), _i(lv), _i(rs), _d(dn), _d(gn),
                                                   C.byref(vptr)))
    return ValueHandle(mech, ptr=vptr, n_tables=n), lv, rs, dn, gn


def _noise_arrays(Wu, Sigma0, mu, mx):
    """Wu [mu][mu] or [n][mu][mu], Sigma0 [mx][mx] or [n][mx][mx], either None -> (Wu [n_noise][mu][mu] or None, Sigma0 [n_noise][mx][mx] or None, n_noise); both
    given: the same count"""
    if Wu is not None:
        Wu = f64(Wu)
        if Wu.ndim not in (2, 3) or Wu.shape[-2:] != (mu, mu):
            raise ValueError("Wu must be [mu][mu] or [n_noise][mu][mu] with mu = %d (got %s)" % (mu, Wu.shape))
        Wu = np.ascontiguousarray(Wu.reshape(-1, mu, mu))
    if Sigma0 is not None:
        Sigma0 = f64(Sigma0)
        if Sigma0.ndim not in (2, 3) or Sigma0.shape[-2:] != (mx, mx):
            raise ValueError("Sigma0 must be [mx][mx] or [n_noise][mx][mx] with mx = %d (got %s)" % (mx, Sigma0.shape))
        Sigma0 = np.ascontiguousarray(Sigma0.reshape(-1, mx, mx))
    if Wu is not None and Sigma0 is not None and Wu.shape[0] != Sigma0.shape[0]:
        if Wu.shape[0] == 1:
            Wu = np.ascontiguousarray(np.repeat(Wu, Sigma0.shape[0], axis=0))
        elif Sigma0.shape[0] == 1:
            Sigma0 = np.ascontiguousarray(np.repeat(Sigma0, Wu.shape[0], axis=0))
        else:
            raise ValueError("Wu and Sigma0 hold %d and %d matrices: one shared by all, or one per problem" % (Wu.shape[0], Sigma0.shape[0]))
    n_noise = Wu.shape[0] if Wu is not None else (Sigma0.shape[0] if Sigma0 is not None else 1)
    return Wu, Sigma0, n_noise


def covariance_doubling(A, Bu, Bl, G, K, Q, R, Wu, Sigma0, N, tol=1e-8, max_levels=40, path=0, bf16_terms=0, want_cost=True, want_std=True, want_diag=True):
    """the closed-loop state covariance of a stationary gain under input noise, by doubling (cclqr_covariance_doubling; lqr.jl:169 with the one gain of lqr.jl:40-43 and
    the noise of trackingLQR_triple_cartpole.jl:98).  Models, K, Q, R as for policy_value_doubling (Q = R = None with want_cost=False); Wu [mu][mu] or [n][mu][mu],
    Sigma0 [mx][mx] or [n][mx][mx], either None (= 0).  N >= 1: N - 1 steps exactly from Sigma0; N = 0: the steady state (Sigma0 must be None), level by level until
    the increment relative to w = 2^floor(log2 tr(D Wu D')) falls below tol -> Sigma [nprob][mx][mx], cost [nprob][2] (tr(Q Sigma), tr(R K Sigma K')), zstd [nprob][mx],
    ustd [nprob][mu], levels, reason, dnorm, gnorm as there (dnorm in Sigma's units).  want_cost / want_std / want_diag = False pass NULL (returned as None)"""
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    K = _gains(K, mu, mx, full=3, lowest=2)
    Q, R, nw = _weights(Q, R, mx, mu, optional=True)
    Wu, Sigma0, n_noise = _noise_arrays(Wu, Sigma0, mu, mx)
    S = np.zeros((nprob, mx, mx))
    cost = np.zeros((nprob, 2)) if want_cost else None
    zstd = np.zeros((nprob, mx)) if want_std else None
    ustd = np.zeros((nprob, mu)) if want_std else None
    lv, rs, dn, gn = _diagnostics(nprob, want_diag)
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_covariance_doubling(*_model_args(dims, models), C.c_int32(K.shape[0]), _panel(K), C.c_int32(nw), _d(Q), _panel(R), C.c_int32(n_noise), _d(Wu),
                                          _d(Sigma0), C.c_int32(int(N)), C.c_double(float(tol)), C.c_int32(int(max_levels)), _d(S), _d(cost), _d(zstd), _panel(ustd),
                                          _i(lv), _i(rs), _d(dn), _d(gn), C.byref(o)))
    return S, cost, zstd, ustd, lv, rs, dn, gn


def value_create_covariance_doubling(mech, ctrl, zd, ctrl_joint, Q, R, Wu, Sigma0, N, tol=1e-8, max_levels=40, Fd=None, plants=None, first_plant=0):
    """cclqr_value_create_covariance_doubling: the covariance above for controller handle `ctrl`'s stationary gain on the models linearised as for
    value_create_policy_doubling; Q, Sigma0 in the mechanism's body order.  N >= 1 knots, or 0 = the steady state -> (ValueHandle of n_models tables holding Sigma,
    cost [n][2], zstd [n][12 nb], ustd [n][mu], levels, reason, dnorm [n][2], gnorm [n][2])"""
    n, head = _setpoint_args(mech, ctrl, zd, ctrl_joint, Fd, Q, R, plants, first_plant)
    mu, mx = np.size(ctrl_joint), 12 * mech.tables.nb
    Wu, Sigma0, n_noise = _noise_arrays(Wu, Sigma0, mu, mx)
    cost, zstd, ustd = np.zeros((n, 2)), np.zeros((n, mx)), np.zeros((n, mu))
    lv, rs, dn, gn = _diagnostics(n)
    vptr = C.c_void_p()
    check(lib().cclqr_value_create_covariance_doubling(*head, C.c_int32(n_noise), _d(Wu), _d(Sigma0), C.c_int32(int(N)), C.c_double(float(tol)),
                                                       C.c_int32(int(max_levels)), _d(cost), _d(zstd), _d(ustd), _i(lv), _i(rs), _d(dn), _d(gn), C.byref(vptr)))
    return ValueHandle(mech, ptr=vptr, n_tables=n), cost, zstd, ustd, lv, rs, dn, gn


def covariance_tracking(A, Bu, Bl, G, K, Q, R, Wu, Sigma0, N, path=0, bf16_terms=0, want_all=False, want_cost=True, want_std=True, want_total=True):
    """the state covariance of a tracked run at every knot (cclqr_covariance_tracking; lqr_tracking.jl:63, 88, 107 under the noise of trackingLQR_triple_cartpole.jl:98):
    Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j', j = 0 .. N-2.  A [nprob][nlin][mx][mx], Bu [nprob][nlin][mx][mu], Bl [nprob][nlin][mx][ml], G [nprob][nlin][ml][mx] with
    nlin = 1 or N - 1; K [mu][mx], [nK][mu][mx] or [n_gains][nK][mu][mx] with nK = 1 or N - 1; Q, R one pair or one per problem (None with want_cost = want_total = False);
    Wu [mu][mu] or [n][mu][mu], Sigma0 [mx][mx] or [n][mx][mx], either None (= 0) -> Sigma [nprob][mx][mx] = Σ_{N-1}, Sigma_all [nprob][N][mx][mx], cost [nprob][N][2],
    zstd [nprob][N][mx], ustd [nprob][N][mu], total [nprob][2]; want_* = False pass NULL (returned as None)"""
    models, dims = _models(A, Bu, Bl, G, tracked=True)
    nprob, mx, mu, ml = dims
    K = _gains(K, mu, mx, full=4, lowest=2)
    Q, R, nw = _weights(Q, R, mx, mu, optional=True)
    Wu, Sigma0, n_noise = _noise_arrays(Wu, Sigma0, mu, mx)
    N = int(N)
    S = np.zeros((nprob, mx, mx))
    Sall = np.zeros((nprob, N, mx, mx)) if want_all else None
    cost = np.zeros((nprob, N, 2)) if want_cost else None
    zstd = np.zeros((nprob, N, mx)) if want_std else None
    ustd = np.zeros((nprob, N, mu)) if want_std else None
    total = np.zeros((nprob, 2)) if want_total else None
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_covariance_tracking(*_model_args(dims, models), C.c_int32(K.shape[0]), C.c_int32(K.shape[1]), _panel(K), C.c_int32(nw),
                                          _d(Q), _panel(R), C.c_int32(n_noise), _d(Wu), _d(Sigma0), C.c_int32(N), _d(S), _d(Sall), _d(cost), _d(zstd), _panel(ustd),
                                          _d(total), C.byref(o)))
    return S, Sall, cost, zstd, ustd, total


def value_create_covariance_tracking(mech, ctrl, zd, n, N, ctrl_joint, Q, R, Wu, Sigma0, Fd=None, plants=None, first_plant=0, workspace_bytes=0, on_device=False,
                                     stream=None):
    """cclqr_value_create_covariance_tracking: the covariance above for controller handle `ctrl`'s gain rows along n trajectories zd [n][N][nb][13] (Fd [n][N][mu]),
    linearised at the knots 0 .. N-2 on plant first_plant + k; numpy arrays, or with on_device=True device addresses read in place on `stream`.  Q, Sigma0 in the
    mechanism's body order -> (ValueHandle of n tables holding Σ_{N-1}, cost [n][N][2], zstd [n][N][12 nb], ustd [n][N][mu], total [n][2])"""
    n, N, mu, mx = int(n), int(N), np.size(ctrl_joint), 12 * mech.tables.nb
    head = _trajectory_args(mech, ctrl, zd, n, N, ctrl_joint, Fd, Q, R, plants, first_plant, on_device)
    Wu, Sigma0, n_noise = _noise_arrays(Wu, Sigma0, mu, mx)
    cost, zstd, ustd, total = np.zeros((n, N, 2)), np.zeros((n, N, mx)), np.zeros((n, N, mu)), np.zeros((n, 2))
    vptr = C.c_void_p()
    check(lib().cclqr_value_create_covariance_tracking(*head, C.c_int32(n_noise), _d(Wu), _d(Sigma0), C.c_int64(int(workspace_bytes)), _d(cost), _d(zstd), _d(ustd),
                                                       _d(total), None if stream is None else C.c_void_p(int(stream)), C.byref(vptr)))
    return ValueHandle(mech, ptr=vptr, n_tables=n), cost, zstd, ustd, total


def policy_value_tracking(A, Bu, Bl, G, K, Q, R, Wu, N, path=0, bf16_terms=0, want_P=True, want_all=False, want_price=True, want_total=True):
    """the cost-to-go of a tracked run at every knot and the price of its noise (cclqr_policy_value_tracking; lqr_tracking.jl:63, 88, 107, 108 under the noise of
    trackingLQR_triple_cartpole.jl:98): P_{N-1} = Q, P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j, price_j = tr(Wu D_j' P_{j+1} D_j).  Models, K, Q, R as
    covariance_tracking takes them (Q, R required); Wu [mu][mu] or [n][mu][mu], or None: no price -> P [nprob][mx][mx] = P_0, P_all [nprob][N][mx][mx],
    price [nprob][N], noise_total [nprob]; want_* = False pass NULL (returned as None), as does Wu = None for the last two"""
    models, dims = _models(A, Bu, Bl, G, tracked=True)
    nprob, mx, mu, ml = dims
    K = _gains(K, mu, mx, full=4, lowest=2)
    Q, R, nw = _weights(Q, R, mx, mu)
    Wu, _, n_noise = _noise_arrays(Wu, None, mu, mx)
    N = int(N)
    P = np.zeros((nprob, mx, mx)) if want_P else None
    Pall = np.zeros((nprob, N, mx, mx)) if want_all else None
    price = np.zeros((nprob, N)) if (want_price and Wu is not None) else None
    total = np.zeros(nprob) if (want_total and Wu is not None) else None
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_policy_value_tracking(*_model_args(dims, models), C.c_int32(K.shape[0]), C.c_int32(K.shape[1]), _panel(K), C.c_int32(nw), _d(Q), _panel(R),
                                            C.c_int32(n_noise), _d(Wu), C.c_int32(N), _d(P), _d(Pall), _d(price), _d(total), C.byref(o)))
    return P, Pall, price, total


def value_create_policy_tracking(mech, ctrl, zd, n, N, ctrl_joint, Q, R, Wu, knot=0, Fd=None, plants=None, first_plant=0, workspace_bytes=0, on_device=False, stream=None):
    """cclqr_value_create_policy_tracking: the cost-to-go above for controller handle `ctrl`'s gain rows along n trajectories zd [n][N][nb][13] (Fd [n][N][mu]),
    linearised at the knots 0 .. N-2 on plant first_plant + k; numpy arrays, or with on_device=True device addresses read in place on `stream`.  Q in the mechanism's
    body order; the recursion runs down to `knot` -> (ValueHandle of n tables holding P_knot, price [n][N], noise_total [n]); Wu = None: the last two are None"""
    n, N = int(n), int(N)
    head = _trajectory_args(mech, ctrl, zd, n, N, ctrl_joint, Fd, Q, R, plants, first_plant, on_device)
    Wu, _, n_noise = _noise_arrays(Wu, None, np.size(ctrl_joint), 12 * mech.tables.nb)
    price, total = (np.zeros((n, N)), np.zeros(n)) if Wu is not None else (None, None)
    vptr = C.c_void_p()
    check(lib().cclqr_value_create_policy_tracking(*head, C.c_int32(n_noise), _d(Wu), C.c_int32(int(knot)), C.c_int64(int(workspace_bytes)), _d(price), _d(total),
                                                   None if stream is None else C.c_void_p(int(stream)), C.byref(vptr)))
    return ValueHandle(mech, ptr=vptr, n_tables=n), price, total


def riccati_doubling(A, Bu, Bl, G, Q, R, N, tol=1e-5, max_levels=40, bf16_terms=0, want_P=True, want_diag=True, K=None, P=None):
    """the stationary LQR gain by doubling the Riccati map (cclqr_riccati_doubling; lqr.jl:25-27, 39-43, 141-184).  Models and weights as for riccati_value (Q, R exactly
    symmetric).  N >= 2: N - 1 steps exactly, what riccati_value(N, tol=0, keep_last=True) returns to rounding; N = 0: level by level to convergence (increment < tol,
    at most max_levels levels) -> K [nprob][mu][mx], P [nprob][mx][mx], levels [nprob], reason [nprob] (0 converged, 1 max_levels, 2 norm(A) > 1e50 or not finite,
    3 pivot), dnorm [nprob][2], anorm [nprob][2].  want_P=False passes P = NULL, want_diag=False NULL for the four diagnostics (returned as None); K, P: arrays to
    write into instead of fresh ones"""
    models, dims = _models(A, Bu, Bl, G)
    nprob, mx, mu, ml = dims
    Q, R, nw = _weights(Q, R, mx, mu)
    if K is None:
        K = np.zeros((nprob, mu, mx))
    if K.shape != (nprob, mu, mx) or K.dtype != np.float64 or not K.flags.c_contiguous:
        raise ValueError("K must be a contiguous float64 [nprob][mu][mx] = %s (got %s)" % ((nprob, mu, mx), K.shape))
    if want_P and P is None:
        P = np.zeros((nprob, mx, mx))
    if P is not None and (P.shape != (nprob, mx, mx) or P.dtype != np.float64 or not P.flags.c_contiguous):
        raise ValueError("P must be a contiguous float64 [nprob][mx][mx] = %s (got %s)" % ((nprob, mx, mx), P.shape))
    lv, rs, dn, an = _diagnostics(nprob, want_diag)
    o = RiccatiOpts(0, int(bf16_terms), 1, 0)
    check(lib().cclqr_riccati_doubling(*_model_args(dims, models), C.c_int32(nw), _d(Q), _panel(R), C.c_int32(int(N)), C.c_double(float(tol)), C.c_int32(int(max_levels)),
                                       _panel(K), _d(P), _i(lv), _i(rs), _d(dn), _d(an), C.byref(o)))
    return K, P, lv, rs, dn, an


def riccati_tv(A, Bu, Bl, G, Q, R, N, tol=1e-5):
    """time-varying dlqr on caller-supplied per-knot models: A [N-1][mx][mx], Bu [N-1][mx][mu], Bl [N-1][mx][ml], G [N-1][ml][mx] -> K [N-1][mu][mx], kbreak"""
    models, dims = _models(A, Bu, Bl, G)
    nk, mx, mu, ml = dims
    assert nk == N - 1
    K = np.zeros((nk, mu, mx))
    kb = np.zeros(1, dtype=np.int32)
    check(lib().cclqr_riccati_tv(*_model_args(dims, models)[1:], _d(f64(Q)), _panel(f64(R)), C.c_int32(int(N)), C.c_double(float(tol)), _d(K), _i(kb)))
    return K, int(kb[0])


def riccati_tracking(mech, ctrl_joint, zd, Fd, Q, R, N, tol=1e-5, path=0, bf16_terms=0):
    t = mech.tables
    cj = i32(ctrl_joint).reshape(-1)
    mu, mx = len(cj), 12 * t.nb
    zd = f64(zd).reshape(N, t.nb, 13)
    Fd = f64(Fd).reshape(N, mu)
    K = np.zeros((N - 1, mu, mx))
    kb = C.c_int32(0)
    o = RiccatiOpts(int(path), int(bf16_terms), 0, 0)
    check(lib().cclqr_riccati_tracking_ex(mech.ptr, C.c_int32(mu), _i(cj), _d(zd), _d(Fd), _d(f64(Q).reshape(mx, mx)), _d(f64(R).reshape(mu, mu)),
                                          C.c_int32(N), C.c_double(tol), _d(K), C.byref(kb), C.byref(o)))
    return K, kb.value


def rate_or_refusal(n_units, seconds, status):
    """throughput string of a run, or a refusal when any instance came back with status <= 0 (a rate of failed rollouts means nothing)"""
    import numpy as np
    bad = int((np.asarray(status) <= 0).sum())
    if bad:
        return "NO RATE: %d of %d instances failed (status <= 0)" % (bad, np.asarray(status).size)
    return "%.3g inst-steps/s" % (n_units / seconds)
