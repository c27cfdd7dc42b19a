"""Host-side mirror of the reference's controllers.  Same constructor arguments, same assertions, same field
meaning; the arithmetic (linearsystem, dlqr, simulate!) runs in HIP through the C-ABI (include/cclqr.h).

    LQR(mechanism, bodyids, eqcids, Q, R, horizon; xd, vd, qd, ωd, Fτd)            src/control/lqr.jl:49-66
    LQR(A, Bu, Bλ, G, Q, R, horizon, eqcids, xd, vd, qd, ωd, Fτd, Δt)              src/control/lqr.jl:17-47
    PlantLQR(mechanism, plants, bodyids, eqcids, Q, R, horizon, zd; Fτd)           the first of these once per plant of a PlantBatch, in one call
    PlantTrackingLQR(mechanism, plants, storage, Fτ, eqcids, Q, R; fric, noise_*)   TrackingLQR (below) once per plant / trajectory, in one call
    LQRSweep(mechanism, bodyids, eqcids, Qs, Rs, horizon, zd; Fτd, plants)          the first of these once per weight candidate (Q_k, R_k), in one call
    TrackingLQR(mechanism, storage, Fτ, eqcids, Q, R)                                src/control/lqr_tracking.jl:17-43
    simulate!(mechanism, tend | storage, controller; record)                         e.g. examples/lqr_cartpole.jl:44
    Storage{T}(steps, Nb)                                                            examples/trackingLQR_triple_cartpole.jl:50-51

What is new relative to the reference (which has no batch API): simulate(..., z0=batch) rolls out n_inst
independent instances at once.  A custom `controlfunction(batch, controller, k)` (lqr.jl:14, :56) is a host closure: simulate then steps the
device one launch per step, shows the closure the batch's states (BatchState) and applies the joint inputs it sets with setForce
(cclqr_ctrl_set_feedforward) -- the built-in laws (LQR / TrackingLQR / friction + noise / PID) stay fused in one persistent launch.
"""
import math

import numpy as np

from . import _capi
from .mechanism import Mechanism, minimal_to_maximal, one_quaternion


def _blockdiag(blocks):
    n = sum(b.shape[0] for b in blocks)
    M = np.zeros((n, n))
    o = 0
    for b in blocks:
        k = b.shape[0]
        M[o:o + k, o:o + k] = b
        o += k
    return M


def _pack_setpoint(nb, xd, vd, qd, ωd):
    z = np.zeros((nb, 13))
    for i in range(nb):
        z[i, 0:3] = np.asarray(xd[i], dtype=np.float64).reshape(3)
        z[i, 3:7] = np.asarray(qd[i], dtype=np.float64).reshape(4)
        z[i, 7:10] = np.asarray(vd[i], dtype=np.float64).reshape(3)
        z[i, 10:13] = np.asarray(ωd[i], dtype=np.float64).reshape(3)
    return z


def _device_mech(mechanism):
    h = getattr(mechanism, "_cclqr_handle", None)
    if h is None or not h.ptr:
        h = _capi.MechHandle(mechanism.tables())
        mechanism._cclqr_handle = h
    return h


def _body_order(bodyids, nb):
    """state blocks follow the order of `bodyids`, the device works in mechanism body order: position in `bodyids` of every body of the mechanism"""
    order = [int(b) - 1 for b in bodyids]
    if sorted(order) != list(range(nb)):
        raise ValueError("bodyids must name every body exactly once")
    return np.argsort(order)


def _weights_and_horizon(Q, R, horizon, Δt):
    """the head of LQR(A, Bu, Bλ, G, Q, R, horizon, ...) (lqr.jl:18-27): Δt-scaled block-diagonal weights, the gated horizon N in steps (math.inf: LQR{T,Inf})
    and the number of knots Ntemp the recursion runs over"""
    Qm = _blockdiag(Q) * Δt                                 # lqr.jl:18
    Rm = _blockdiag(R) * Δt                                 # lqr.jl:19
    N = horizon / Δt                                        # lqr.jl:21
    if N < math.inf:
        N = int(math.ceil(horizon / Δt))                    # lqr.jl:23
        Ntemp = N
    else:
        Ntemp = int(math.ceil(10 / Δt))                     # lqr.jl:26: 10 s as maximal horizon for Inf
    return Qm, Rm, N, Ntemp


def _pair_lists(Q, R, n, of):
    """Q, R as PolicyValue, StationaryPolicyValue and StationaryLQR take them -- a single pair (Q: nb blocks of 12 x 12) or lists of one pair per `of` -- as two lists
    of 1 or n candidates"""
    single = len(Q) > 0 and np.ndim(Q[0]) == 2
    Qs, Rs = ([Q], [R]) if single else (list(Q), list(R))
    if len(Qs) not in (1, n) or len(Rs) not in (1, n):
        raise ValueError("Q and R must be a single pair or lists of one pair per %s, %d (got %d and %d)" % (of, n, len(Qs), len(Rs)))
    return Qs, Rs


def _scaled_pairs(Qs, Rs, bodyids, nb, mu, horizon, Δt, symmetric=False):
    """the head of the inner constructor (lqr.jl:18-27) per pair of _pair_lists: the blocks permuted to the mechanism's body order and scaled by Δt ->
    (Q [n_weights][12 nb][12 nb], R [n_weights][mu][mu], the knots Ntemp of `horizon`).  symmetric: a Q block that is not exactly symmetric is refused"""
    assert len(bodyids) == nb, "Missmatched length for bodies"                                                            # lqr.jl:59
    for q in Qs:
        assert len(q) == nb, "Missmatched length for bodies"                                                              # lqr.jl:59
    for r in Rs:
        assert len(r) == mu, "Missmatched length for constraints"                                                         # lqr.jl:60
    inv = _body_order(bodyids, nb)
    Qm, Rm, Ntemp = [], [], None
    for k in range(max(len(Qs), len(Rs))):
        q, r = Qs[k if len(Qs) > 1 else 0], Rs[k if len(Rs) > 1 else 0]
        Qb = [np.asarray(q[i], dtype=np.float64) for i in inv]
        Rb = [np.asarray(x, dtype=np.float64).reshape(1, 1) for x in r]
        if any(b.shape != (12, 12) for b in Qb):
            raise ValueError("every Q block must be 12 x 12 (pair %d)" % k)
        if symmetric and any(not np.array_equal(b, b.T) for b in Qb):
            raise ValueError("Q of pair %d is not symmetric: the composition of Riccati maps holds for exactly symmetric weights only" % k)
        qm, rm, _, Ntemp = _weights_and_horizon(Qb, Rb, horizon, Δt)
        Qm.append(qm)
        Rm.append(rm)
    return np.stack(Qm), np.stack(Rm), Ntemp


def _model_set(mechanism, controller, plants, zd, Q, R, zd_is="[n_models][nb][13]", of="model"):
    """the head of the constructors that take a set of models (PolicyValue, the Stationary* classes): whose mechanism the controller and the plants are, zd as
    [n][nb][13] (`zd_is`: how the refusal names it), Q and R as lists of 1 or n candidates (one per `of`) -> (zd, n, Qs, Rs)"""
    if controller is not None and controller.mechanism is not mechanism:
        raise ValueError("the controller was made for another mechanism")
    if plants is not None and plants.mechanism is not mechanism:
        raise ValueError("the PlantBatch was made for another mechanism")
    nb = len(mechanism.bodies)
    zd = np.ascontiguousarray(zd, dtype=np.float64)
    if zd.ndim != 3 or zd.shape[1:] != (nb, 13) or zd.shape[0] < 1:
        raise ValueError("zd must be %s = [n][%d][13], one setpoint per %s (got %s)" % (zd_is, nb, of, zd.shape))
    n = zd.shape[0]
    return (zd, n) + _pair_lists(Q, R, n, of)


def _model_set_fields(self, mechanism, bodyids, eqcids, Qs, Rs, horizon, zd, plants, first_plant, Fτd, Fd_refusal="Fτd must be [n_models][mu] = [%d][%d]", hold=False,
                      symmetric=False):
    """... and their tail: Fτd as [n][mu] (hold: zeros when None), the Δt-scaled weights in the mechanism's body order, every model's
    plant found; sets mechanism, plants, first_plant, eqcids, ctrl_joints, Q, R, zd, Fd on `self` -> the knots Ntemp of `horizon`"""
    nb, mu, n = len(mechanism.bodies), len(eqcids), zd.shape[0]
    Fd = (np.zeros((n, mu)) if hold else None) if Fτd is None else np.ascontiguousarray(Fτd, dtype=np.float64).reshape(-1, mu)
    if Fd is not None and Fd.shape[0] != n:
        raise ValueError(Fd_refusal % (n, mu))
    Qm, Rm, Ntemp = _scaled_pairs(Qs, Rs, bodyids, nb, mu, horizon, mechanism.Δt, symmetric=symmetric)
    self.first_plant = (0 if plants is None else plants.first_index) if first_plant is None else int(first_plant)
    if plants is not None:
        plants.rows_for(self.first_plant, n)      # every model must find its plant
    self.mechanism, self.plants = mechanism, plants
    self.eqcids = [int(e) for e in eqcids]
    self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
    self.Q, self.R = Qm, Rm      # [n_weights][12 nb][12 nb], [n_weights][mu][mu]: scaled, mechanism body order
    self.zd, self.Fd = zd, Fd
    return Ntemp


def _doubling_limits(horizon, max_levels, tol):
    """what a doubling constructor refuses of max_levels and tol -> (max_levels, the horizon the knots are counted over: math.inf for horizon=None, a run to convergence)"""
    max_levels = int(max_levels)
    if horizon is None and not 1 <= max_levels <= 60:
        raise ValueError("max_levels = %d: a run to convergence makes 1 .. 60 levels (2^max_levels steps)" % max_levels)
    if not float(tol) >= 0.0:
        raise ValueError("tol = %r is negative or not a number" % (tol,))
    return max_levels, math.inf if horizon is None else horizon


def _doubling_result(self, Ntemp, gnorm=None):
    """what a doubling constructor reports next to levels and reason [n]: steps = 2^levels of a run to convergence (Ntemp = 0), else the horizon's N - 1; converged =
    reason == 0 of such a run; with the norms gnorm [n][2] of the last two levels also diverged = reason == 2 and the spectral-radius estimate"""
    to_convergence = Ntemp == 0
    self.steps = 2 ** self.levels.astype(np.int64) if to_convergence else np.full(len(self.levels), Ntemp - 1, dtype=np.int64)
    self.converged = (self.reason == 0) & to_convergence
    if gnorm is not None:
        self.diverged = (self.reason == 2) & to_convergence
        with np.errstate(invalid="ignore", divide="ignore"):
            self.spectral_radius = (gnorm[:, 0] / gnorm[:, 1]) ** (1.0 / 2.0 ** (self.levels - 1))


def _noise_arguments(self, bodyids, nb, mu, n, noise_scale, Wu, Sigma0):
    """the noise of the covariance and tracking classes: noise_scale or Wu ([mu][mu] or one per model), and a start covariance Sigma0 in the order of bodyids ([12 nb][12 nb]
    or one per model) -> (Wu, Sigma0 in the mechanism's body order), either None; sets _to_bodyids on `self`"""
    if noise_scale is not None and Wu is not None:
        raise ValueError("noise_scale and Wu are both given: noise_scale IS Wu = noise_scale^2 ones((mu, mu))")
    if noise_scale is not None:
        Wu = float(noise_scale) ** 2 * np.ones((mu, mu))
    if Wu is not None:
        Wu = np.ascontiguousarray(Wu, dtype=np.float64)
        if Wu.shape not in ((mu, mu), (n, mu, mu)):
            raise ValueError("Wu must be [mu][mu] = [%d][%d] or a list of one per model, %d (got %s)" % (mu, mu, n, Wu.shape))
    inv = _body_order(bodyids, nb)
    self._to_bodyids = np.concatenate([12 * inv[m] + np.arange(12) for m in range(nb)])      # mechanism-order coordinate -> its place in the order of bodyids
    if Sigma0 is not None:
        Sigma0 = np.ascontiguousarray(Sigma0, dtype=np.float64)
        if Sigma0.shape not in ((12 * nb, 12 * nb), (n, 12 * nb, 12 * nb)):
            raise ValueError("Sigma0 must be [12 nb][12 nb] = [%d][%d] or a list of one per model, %d (got %s)" % (12 * nb, 12 * nb, n, Sigma0.shape))
        Sigma0 = np.ascontiguousarray(Sigma0[..., self._to_bodyids, :][..., :, self._to_bodyids])
    return Wu, Sigma0


class Controller:
    """abstract type owned by ConstrainedDynamics (lqr.jl:3 `<: Controller`)"""


class LQR(Controller):
    """LQR{T,N,NK}: K[k][i] (1 x NK rows), xd, vd, qd, ωd, eqcids, Fτd   (lqr.jl:3-15)"""

    def __init__(self, mechanism, bodyids, eqcids, Q, R, horizon, xd=None, vd=None, qd=None, ωd=None, Fτd=None, controlfunction=None, keep_value=False, **kw):
        """keep_value: also keep the cost-to-go .P [12 nb][12 nb] of the recursion (the Pkp1 of lqr.jl:170 at its last executed step, mechanism body order) for
        predicted_cost; False: .P is None and nothing more is computed or allocated"""
        self.keep_value = bool(keep_value)
        if "wd" in kw:
            ωd = kw.pop("wd")
        if "Ftd" in kw:
            Fτd = kw.pop("Ftd")
        if "xθd" in kw:          # minimal-coordinate constructor keywords (lqr.jl:70-72)
            xd = kw.pop("xθd")
        if "vωd" in kw:
            vd = kw.pop("vωd")
        if kw:
            raise TypeError("unexpected keyword(s): %s" % list(kw))
        self.controlfunction = controlfunction          # lqr.jl:14: a host closure (batch, lqr, k); None = control_lqr! on the device
        if not isinstance(mechanism, Mechanism):
            raise TypeError("LQR(mechanism, bodyids, eqcids, Q, R, horizon; ...)")
        nb = len(mechanism.bodies)
        if len(Q) and np.ndim(Q[0]) == 0:
            # LQR(mechanism, controlledids, controlids, Q::Vector{T}, R::Vector{T}, horizon; xθd, vωd, Fτd)      lqr.jl:68-86
            controlledids, controlids = bodyids, eqcids
            xθd = np.zeros(len(controlledids)) if xd is None else np.asarray(xd, dtype=np.float64)
            vωd = np.zeros(len(controlledids)) if vd is None else np.asarray(vd, dtype=np.float64)
            Fτ = np.zeros(len(controlids)) if Fτd is None else np.asarray(Fτd, dtype=np.float64).reshape(-1)
            assert len(controlledids) == len(Q) == len(xθd) == len(vωd) == nb, "Missmatched length for bodies"          # lqr.jl:76
            assert len(controlids) == len(R) == len(Fτ), "Missmatched length for constraints"                          # lqr.jl:77
            xd, vd, qd, ωd = minimal_to_maximal(mechanism, controlledids, xθd, vωd)                                    # lqr.jl:80
            Q = [np.eye(12) * float(q) for q in Q]                                                                     # lqr.jl:82
            R = [np.eye(1) * float(r) for r in R]                                                                      # lqr.jl:83
            Fτd = [[f] for f in Fτ]                                                                                    # lqr.jl:85
            bodyids = [b.id for b in mechanism.bodies]
        z3 = [np.zeros(3) for _ in range(nb)]
        xd = z3 if xd is None else xd                       # lqr.jl:51-55 defaults
        vd = z3 if vd is None else vd
        qd = [one_quaternion() for _ in range(nb)] if qd is None else qd
        ωd = z3 if ωd is None else ωd
        Fτd = [np.zeros(1) for _ in range(len(eqcids))] if Fτd is None else Fτd
        # lqr.jl:59-60
        assert len(bodyids) == len(Q) == len(xd) == len(vd) == len(qd) == len(ωd) == nb, "Missmatched length for bodies"
        assert len(eqcids) == len(R) == len(Fτd), "Missmatched length for constraints"
        inv = _body_order(bodyids, nb)
        Q = [np.asarray(Q[i], dtype=np.float64) for i in inv]
        xd, vd, qd, ωd = ([a[i] for i in inv] for a in (xd, vd, qd, ωd))
        self.mechanism = mechanism
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        self.xd, self.vd, self.qd, self.ωd = xd, vd, qd, ωd
        self.Fτd = [np.asarray(f, dtype=np.float64).reshape(1) for f in Fτd]
        self.zd = _pack_setpoint(nb, xd, vd, qd, ωd)[None]
        self.Fd = np.array([f[0] for f in self.Fτd]).reshape(1, -1)
        dev = _device_mech(mechanism)
        self.projected = bool(getattr(mechanism, "has_loops", False))
        if self.projected:
            # closed loops (examples/lqr_deltabot.jl:47-53): G Bλ of lqr.jl:151 is singular (redundant constraint rows), but the pair the
            # recursion works with -- A' = A - Bλ (G Bλ)^-1 G A, D = Bu - Bλ (G Bλ)^-1 G Bu -- is unique: it is the Jacobian of the
            # constrained one-step map, formed analytically on the device (cclqr_linearize_projected), and the recursion runs on it with no multipliers
            mx = 12 * nb
            Ap, D = _capi.linearize_projected(dev, self.zd, self.ctrl_joints, self.Fd)
            self.A, self.Bu, self.Bλ, self.G = Ap[0], D[0], np.zeros((mx, 0)), np.zeros((0, mx))
        else:
            # linearize (lqr.jl:63)
            A, Bu, Bl, G = _capi.linearize(dev, self.zd, self.ctrl_joints, self.Fd)
            self.A, self.Bu, self.Bλ, self.G = A[0], Bu[0], Bl[0], G[0]
        self._finish(self.A, self.Bu, self.Bλ, self.G, Q, [np.asarray(r, dtype=np.float64) for r in R], horizon, mechanism.Δt)

    def _finish(self, A, Bu, Bl, G, Q, R, horizon, Δt):
        """LQR(A, Bu, Bλ, G, Q, R, horizon, eqcids, xd, ..., Δt)   lqr.jl:17-47"""
        self.Q, self.R, N, Ntemp = _weights_and_horizon(Q, R, horizon, Δt)
        if G.shape[0] == 0 and N == math.inf and not getattr(self, "projected", False):
            # lqr.jl:33 calls dlqr(A,Bu,Q,R,N) which binds N=Inf to the Δt method of util.jl:50 — a defect, not reproduced
            raise ValueError("unconstrained infinite-horizon LQR is not reachable in the reference (lqr.jl:33)")
        self.P = None
        if getattr(self, "keep_value", False):      # the same recursion, its cost-to-go returned with the gains (cclqr_riccati_value)
            K, P, kb = _capi.riccati_value(A, Bu, Bl, G, self.Q, self.R, Ntemp)
            K, self.P, kbreak = K[0], P[0], int(kb[0])
        else:
            K, kbreak = _capi.riccati(A, Bu, Bl, G, self.Q, self.R, Ntemp)   # lqr.jl:36 / :39
        self.kbreak = kbreak
        self.converged = True
        if N == math.inf:
            self.converged = bool(Ntemp < 3 or np.array_equal(K[0], K[1]))
            if not self.converged:
                print("[ Info: Riccati recursion did not converge.")      # lqr.jl:41
            K = K[:1]                                                     # lqr.jl:42
        self.K = K
        self.N = 0 if N == math.inf else N                  # device convention: N <= 0 means LQR{T,Inf}
        self.horizon_steps = N
        self.NK = K.shape[2]

    @classmethod
    def from_matrices(cls, A, Bu, Bλ, G, Q, R, horizon, eqcids, xd, vd, qd, ωd, Fτd, Δt, mechanism=None):
        """the inner constructor lqr.jl:17-47 for callers that bring their own linear model"""
        self = cls.__new__(cls)
        nb = len(xd)
        self.controlfunction = None
        self.mechanism = mechanism
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids] if mechanism is not None else list(range(len(eqcids)))
        self.xd, self.vd, self.qd, self.ωd = xd, vd, qd, ωd
        self.Fτd = [np.asarray(f, dtype=np.float64).reshape(1) for f in Fτd]
        self.zd = _pack_setpoint(nb, xd, vd, qd, ωd)[None]
        self.Fd = np.array([f[0] for f in self.Fτd]).reshape(1, -1)
        self.A, self.Bu, self.Bλ, self.G = (np.asarray(M, dtype=np.float64) for M in (A, Bu, Bλ, G))
        self._finish(self.A, self.Bu, self.Bλ, self.G, [np.asarray(q, dtype=np.float64) for q in Q], [np.asarray(r, dtype=np.float64) for r in R],
                     horizon, Δt)
        return self

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _capi.CtrlHandle(dev, self.ctrl_joints, K=self.K, N=self.N, zd=self.zd, Fd=self.Fd, fric=fric, noise_scale=noise_scale, noise_seed=noise_seed)

    def _value_handle(self, dev):
        """(ValueHandle of .P on dev, whether the caller closes it)"""
        if self.P is None:
            raise ValueError("the LQR was built without keep_value=True: it has no cost-to-go")
        return _capi.ValueHandle(dev, self.P), True


def _kept_value(controller, dev):
    """the device-resident cost-to-go of a batched constructor (PlantLQR, LQRSweep), which stays with its owner"""
    v = controller._handle.value
    if v is None:
        raise ValueError("the %s was built without keep_value=True: it has no cost-to-go" % type(controller).__name__)
    if v.mech is not dev or not v.ptr:
        raise ValueError("the %s was designed on another device handle of the mechanism" % type(controller).__name__)
    return v, False


class _BorrowedCtrl:
    """what a controller that owns its device tables hands simulate: the same cclqr_ctrl*, and a close() that leaves the tables with their owner"""

    def __init__(self, handle):
        self.ptr, self.owner = handle.ptr, handle

    def close(self):
        pass


def _borrow_tables(controller, dev, fric, noise_scale, noise_seed, law_refusal=None):
    """the _ctrl_handle of a controller whose tables stay on the device (PlantLQR, LQRSweep, StationaryLQR, PlantTrackingLQR): its own cclqr_ctrl*, borrowed -- no other
    law than the one it was built with, table i for instance i, on the device handle it was designed on"""
    name = type(controller).__name__
    if fric is not None or noise_scale or noise_seed is not None:
        raise ValueError(law_refusal or "%s carries neither joint friction nor noise: the batched constructor builds the plain LQR law" % name)
    if controller.first_plant != 0:
        raise ValueError("a rollout reads controller table and plant by the global instance index: %s %s that is rolled out starts at plant 0 "
                         "(this one at plant %d)" % ("an" if name.startswith("LQR") else "a", name, controller.first_plant))
    if controller._handle.mech is not dev or not controller._handle.ptr:
        raise ValueError("the %s was designed on another device handle of the mechanism" % name)
    return _BorrowedCtrl(controller._handle)


class _BatchedLQR(Controller):
    """what PlantLQR, LQRSweep and StationaryLQR share: one gain table per plant / candidate / setpoint behind self._handle, which never leaves the device"""

    def _riccati_result(self, N, Ntemp):
        """kbreak and converged [n] of the batched recursion, as LQR's"""
        self.kbreak = self._handle.kbreak
        # LQR{T,Inf} (lqr.jl:40-42): converged when Ku[1] == Ku[2], i.e. when the recursion met its tolerance and back-filled the rest (kbreak > 1)
        self.converged = np.ones(len(self.kbreak), dtype=bool) if N < math.inf else ((self.kbreak > 1) | (Ntemp < 3))
        if not self.converged.all():
            print("[ Info: Riccati recursion did not converge.")      # lqr.jl:41

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _borrow_tables(self, dev, fric, noise_scale, noise_seed)

    def gains(self, i):
        """K[k][j] of table i, [nK][mu][12 nb] in the mechanism's body order, read back from the device (cclqr_ctrl_get_gains)"""
        return _capi.ctrl_gains(_device_mech(self.mechanism), self._handle, i)

    def P(self, i):
        """table i's cost-to-go [12 nb][12 nb] (lqr.jl:170 at the recursion's last executed step), mechanism body order, read back from the device (keep_value=True)"""
        return _kept_value(self, _device_mech(self.mechanism))[0].get(i)

    def _value_handle(self, dev):
        return _kept_value(self, dev)

    def close(self):
        self._handle.close()


class PlantLQR(_BatchedLQR):
    """One LQR per plant of a PlantBatch, designed in one call: for every plant k, LQR(mechanism_k, bodyids, eqcids, Q, R, horizon; xd, vd, qd, ωd, Fτd)
    (lqr.jl:49-66) where mechanism_k is the mechanism rebuilt with plant k's masses, inertias and joint vertices -- one batched linearsystem (lqr.jl:63) and one
    batched dlqr (lqr.jl:141-184) on the device, the gains never leaving it (cclqr_ctrl_create_lqr_batch_plants).

    Q, R, horizon: as for LQR (per-body 12 x 12 and per-constraint 1 x 1 blocks in the order of bodyids / eqcids, scaled by Δt; math.inf = LQR{T,Inf}).
    zd [n][nb][13]: the setpoint of every plant in the mechanism's body order, on that plant's own constraint manifold (joint_position_states(mech, θ,
    plants=plants)); Fτd [n][mu]: the caller's holding inputs (default 0).  first_plant: global index of the plant zd[0] belongs to (default
    plants.first_index).  kbreak [n], converged [n]: per plant, as LQR's.
    simulate(mech, steps, PlantLQR, z0=, plants=, first_instance=): instance i reads table first_instance + i and runs on plant first_instance + i."""

    def __init__(self, mechanism, plants, bodyids, eqcids, Q, R, horizon, zd, Fτd=None, first_plant=None, controlfunction=None, tol=1e-5, keep_value=False):
        """keep_value: every plant's cost-to-go stays on the device next to its gains (cclqr_ctrl_create_lqr_batch_value; 8 (12 nb)^2 bytes per plant) for
        predicted_cost and P(i); False: nothing is kept or allocated"""
        if controlfunction is not None:
            raise ValueError("PlantLQR carries no controlfunction: its gains stay on the device (one LQR per plant with a closure: build an LQR per plant)")
        if not isinstance(mechanism, Mechanism):
            raise TypeError("PlantLQR(mechanism, plants, bodyids, eqcids, Q, R, horizon, zd; ...)")
        if plants.mechanism is not mechanism:
            raise ValueError("the PlantBatch was made for another mechanism")
        nb = len(mechanism.bodies)
        zd = np.ascontiguousarray(zd, dtype=np.float64)
        if zd.ndim != 3 or zd.shape[1:] != (nb, 13):
            raise ValueError("zd must be [n][nb][13] = [n][%d][13], one setpoint per plant (got %s)" % (nb, zd.shape))
        self.first_plant = plants.first_index if first_plant is None else int(first_plant)
        n = zd.shape[0]
        if n < 1:
            raise ValueError("zd must hold at least one setpoint")
        plants.rows_for(self.first_plant, n)      # every setpoint must find its plant
        assert len(bodyids) == len(Q) == nb, "Missmatched length for bodies"                                              # lqr.jl:59
        assert len(eqcids) == len(R), "Missmatched length for constraints"                                                # lqr.jl:60
        mu = len(eqcids)
        Fd = np.zeros((n, mu)) if Fτd is None else np.ascontiguousarray(Fτd, dtype=np.float64).reshape(-1, mu)
        if Fd.shape[0] != n:
            raise ValueError("Fτd must be [n][mu] = [%d][%d], one holding input per plant and controlled constraint" % (n, mu))
        inv = _body_order(bodyids, nb)
        self.mechanism, self.plants, self.n_plant = mechanism, plants, n
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        self.controlfunction = None
        self.zd, self.Fd = zd, Fd
        self.Q, self.R, N, Ntemp = _weights_and_horizon([np.asarray(Q[i], dtype=np.float64) for i in inv], [np.asarray(r, dtype=np.float64) for r in R], horizon,
                                                        mechanism.Δt)
        self.N = 0 if N == math.inf else N
        self.horizon_steps, self.NK = N, 12 * nb
        dev = _device_mech(mechanism)
        self._handle = _capi.BatchLqrHandle(dev, zd, self.ctrl_joints, self.Q, self.R, Ntemp, Fd=Fd, tol=tol, infinite_horizon=N == math.inf,
                                            plants=plants.handle(dev), first_plant=self.first_plant, keep_value=keep_value)
        self._riccati_result(N, Ntemp)


class LQRSweep(_BatchedLQR):
    """One LQR per weight candidate, designed in one call: for every k, LQR(mechanism, bodyids, eqcids, Qs[k], Rs[k], horizon; xd, vd, qd, ωd, Fτd) (lqr.jl:49-66) --
    one batched linearsystem (lqr.jl:63) and one batched dlqr (lqr.jl:141-184) in which problem k reads its own weights, the gains never leaving the device
    (cclqr_ctrl_create_lqr_batch_weights).  The tuning study: simulate(mech, steps, sweep, z0=start replicated, record=False, score=Score(one Q, R)) ranks the
    candidates under a common yardstick in one rollout launch and one score pass.

    Qs: a sequence of candidates, each what LQR takes as Q (nb 12 x 12 blocks in the order of bodyids); Rs: a sequence of candidates, each mu 1 x 1 blocks in the
    order of eqcids.  Either may hold ONE candidate, which is then shared; n = the longer length.  horizon as for LQR (math.inf = LQR{T,Inf}); every candidate
    is scaled by Δt (lqr.jl:18-19).
    zd [nb][13] (one setpoint for every candidate) or [n][nb][13], mechanism body order; Fτd [mu] or [n][mu] (default 0).
    plants: a PlantBatch -- candidate k is designed on plant first_plant + k (default plants.first_index), as PlantLQR designs table k.
    n, kbreak [n], converged [n], gains(i), close().
    simulate(mech, steps, sweep, z0=, first_instance=): instance i runs under table first_instance + i."""

    def __init__(self, mechanism, bodyids, eqcids, Qs, Rs, horizon, zd, Fτd=None, plants=None, first_plant=None, tol=1e-5, controlfunction=None, keep_value=False):
        """keep_value: every candidate's cost-to-go stays on the device next to its gains (cclqr_ctrl_create_lqr_batch_value; 8 (12 nb)^2 bytes per candidate) for
        predicted_cost and P(i); False: nothing is kept or allocated"""
        if controlfunction is not None:
            raise ValueError("LQRSweep carries no controlfunction: its gains stay on the device (one LQR per candidate with a closure: build an LQR per candidate)")
        if not isinstance(mechanism, Mechanism):
            raise TypeError("LQRSweep(mechanism, bodyids, eqcids, Qs, Rs, horizon, zd; ...)")
        if plants is not None and plants.mechanism is not mechanism:
            raise ValueError("the PlantBatch was made for another mechanism")
        nb, mu = len(mechanism.bodies), len(eqcids)
        Qs, Rs = list(Qs), list(Rs)
        n = max(len(Qs), len(Rs))
        if n < 1 or len(Qs) not in (1, n) or len(Rs) not in (1, n):
            raise ValueError("Qs and Rs must hold one candidate (shared) or the same number of candidates each (got %d and %d)" % (len(Qs), len(Rs)))
        assert len(bodyids) == nb, "Missmatched length for bodies"                                                        # lqr.jl:59
        for Q in Qs:
            assert len(Q) == nb, "Missmatched length for bodies"                                                          # lqr.jl:59
        for R in Rs:
            assert len(R) == mu, "Missmatched length for constraints"                                                     # lqr.jl:60
        inv = _body_order(bodyids, nb)
        zd = np.ascontiguousarray(zd, dtype=np.float64)
        if zd.shape == (nb, 13):
            zd = np.ascontiguousarray(np.broadcast_to(zd, (n, nb, 13)))
        if zd.shape != (n, nb, 13):
            raise ValueError("zd must be [nb][13] = [%d][13] (one setpoint for every candidate) or [n][nb][13] = [%d][%d][13] (got %s)" % (nb, n, nb, zd.shape))
        Fd = np.zeros((n, mu)) if Fτd is None else np.ascontiguousarray(Fτd, dtype=np.float64)
        if Fd.shape == (mu,):
            Fd = np.ascontiguousarray(np.broadcast_to(Fd, (n, mu)))
        if Fd.shape != (n, mu):
            raise ValueError("Fτd must be [mu] = [%d] or [n][mu] = [%d][%d] (got %s)" % (mu, n, mu, Fd.shape))
        self.first_plant = (0 if plants is None else plants.first_index) if first_plant is None else int(first_plant)
        if plants is not None:
            plants.rows_for(self.first_plant, n)      # every candidate must find its plant
        # the head of the inner constructor (lqr.jl:18-27) per candidate: Δt scaling, the blocks permuted to the mechanism's body order, math.inf -> LQR{T,Inf}
        Qm, Rm, N, Ntemp = [], [], None, None
        for k in range(n):
            Q, R = Qs[k if len(Qs) > 1 else 0], Rs[k if len(Rs) > 1 else 0]
            Qb = [np.asarray(Q[i], dtype=np.float64) for i in inv]
            Rb = [np.asarray(r, dtype=np.float64).reshape(1, 1) for r in R]
            if any(q.shape != (12, 12) for q in Qb):
                raise ValueError("every Q block must be 12 x 12 (candidate %d)" % k)
            q, r, N, Ntemp = _weights_and_horizon(Qb, Rb, horizon, mechanism.Δt)
            Qm.append(q)
            Rm.append(r)
        self.Q, self.R = np.stack(Qm), np.stack(Rm)      # [n][12 nb][12 nb], [n][mu][mu]: scaled, mechanism body order
        self.mechanism, self.plants, self.n = mechanism, plants, n
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        self.controlfunction = None
        self.zd, self.Fd = zd, Fd
        self.N = 0 if N == math.inf else N
        self.horizon_steps, self.NK = N, 12 * nb
        dev = _device_mech(mechanism)
        self._handle = _capi.BatchLqrHandle(dev, zd, self.ctrl_joints, self.Q, self.R, Ntemp, Fd=Fd, tol=tol, infinite_horizon=N == math.inf,
                                            plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant, n_weights=n,
                                            keep_value=keep_value)
        self._riccati_result(N, Ntemp)


class StationaryLQR(PlantLQR):
    """LQR{T,Inf}'s one gain (lqr.jl:25-27, 39-43) CONVERGED, by doubling the Riccati map instead of stepping it: n backward steps of dlqr (lqr.jl:141-184) in projected
    form are the triple (A_n, G_n, H_n) of the map X -> H_n + A_n' X (I + G_n X)^-1 A_n, and two triples compose in one pivoted solve and five products, so 2^j steps
    cost j compositions on the device (cclqr_ctrl_create_lqr_batch_doubling); gains and P never leave it.  The reference's 10 s / Δt steps leave anything longer than a
    cartpole unconverged; a 17-body chain needs about 3500.

    One gain row per table, one table per setpoint zd[i] ([n][nb][13], mechanism body order) on plant first_plant + i of `plants` (None: the mechanism's own plant).
    Q, R: as for LQR (per-body 12 x 12 and per-constraint 1 x 1 blocks in the order of bodyids / eqcids, scaled by Δt), a single pair or -- as PolicyValue takes them --
    lists of one pair per table; they must be exactly symmetric.  horizon: None = level by level to convergence: level j doubles to 2^j steps and stops when the
    increment norm(H(2^j) - H(2^(j-1))) < tol (reason 0), when norm(A(2^j)) > 1e50 or a norm is not finite (reason 2: not stabilisable), on a zero pivot (reason 3), or
    at j == max_levels (reason 1; 1 .. 60); a number = LQR{T,N}'s first gain Ku[1] (N = ceil(horizon / Δt) knots, math.inf = ceil(10 / Δt)) used as a stationary one.

    gains(i) [1][mu][12 nb], P(i) (keep_value=True), levels [n], steps [n] = 2^levels or N - 1, reason [n], converged = reason == 0 of a run to convergence, dnorm and
    anorm [n][2]: the increment norms and norm(A) of the last level and of the one before (NaN: no such level).  A table that did not converge is still written:
    reason is the answer.  A Controller: simulate(mech, steps, ctl, z0=, plants=, score=) runs it as a PlantLQR / LQRSweep of the same tables, predicted_cost takes it
    with keep_value=True, PolicyValue / StationaryPolicyValue evaluate its gains."""

    def __init__(self, mechanism, bodyids, eqcids, Q, R, zd, horizon=None, Fτd=None, plants=None, first_plant=None, tol=1e-5, max_levels=40, keep_value=False,
                 controlfunction=None):
        if controlfunction is not None:
            raise ValueError("StationaryLQR carries no controlfunction: its gains stay on the device (an LQR with a closure: build an LQR)")
        if not isinstance(mechanism, Mechanism):
            raise TypeError("StationaryLQR(mechanism, bodyids, eqcids, Q, R, zd; horizon, ...)")
        mechanism.tables()      # (sets has_loops)
        if mechanism.has_loops:
            raise ValueError("StationaryLQR is for tree mechanisms: the batched constructor does not take closed loops")
        zd, n, Qs, Rs = _model_set(mechanism, None, plants, zd, Q, R, zd_is="[n][nb][13]", of="table")
        max_levels, span = _doubling_limits(horizon, max_levels, tol)
        Ntemp = _model_set_fields(self, mechanism, bodyids, eqcids, Qs, Rs, span, zd, plants, first_plant, Fτd,
                                  Fd_refusal="Fτd must be [n][mu] = [%d][%d], one holding input per table and controlled constraint", hold=True, symmetric=True)
        if horizon is None:
            Ntemp = 0
        if Ntemp == 1:
            raise ValueError("horizon = %r is one knot: a gain needs at least one backward step (N >= 2)" % (horizon,))
        self.n_plant, self.n, self.controlfunction = n, n, None
        self.N, self.horizon_steps, self.NK = 0, math.inf, 12 * len(mechanism.bodies)      # the device convention: one gain row, never gated
        self.tol, self.max_levels = float(tol), max_levels
        dev = _device_mech(mechanism)
        self._handle = _capi.ctrl_create_lqr_batch_doubling(dev, zd, self.ctrl_joints, self.Q, self.R, Ntemp, Fd=self.Fd, tol=tol, max_levels=max_levels,
                                                            plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant,
                                                            keep_value=keep_value)
        h = self._handle
        self.levels, self.reason, self.dnorm, self.anorm, self.kbreak = h.levels, h.reason, h.dnorm, h.anorm, None
        _doubling_result(self, Ntemp)
        if Ntemp == 0 and not self.converged.all():
            print("[ Info: Riccati recursion did not converge.")      # lqr.jl:41


class _ValueTables:
    """what PolicyValue, StationaryPolicyValue and TrackingPolicyValue share: the device-resident costs-to-go self._value of n_models models, evaluated on the device
    handle self._dev about the setpoints self.zd [n_models][nb][13] -- what predicted_cost reads them through"""

    def P(self, i):
        """model i's cost-to-go [12 nb][12 nb], mechanism body order, read back from the device (cclqr_value_get)"""
        return self._value.get(i)

    def _value_handle(self, dev):
        if self._value.mech is not dev or not self._value.ptr:
            raise ValueError("the %s was evaluated on another device handle of the mechanism" % type(self).__name__)
        return self._value, False

    def _ctrl_handle(self, dev, **law):
        """a setpoint-only controller of n_models tables built from zd: what predicted_cost measures model i's error about"""
        if law:
            raise TypeError("a %s is not a Controller: it holds costs-to-go, not a control law" % type(self).__name__)
        if dev is not self._dev:
            raise ValueError("the %s was evaluated on another device handle of the mechanism" % type(self).__name__)
        if self._setpoints is None:
            self._setpoints = _capi.CtrlHandle(dev, self.ctrl_joints, K=None, N=0, zd=self.zd, n_ctrl=self.n_models if self.n_models > 1 else 0)
        return _BorrowedCtrl(self._setpoints)

    def close(self):
        if self._setpoints is not None:
            self._setpoints.close()
            self._setpoints = None
        self._value.close()


class PolicyValue(_ValueTables):
    """Policy evaluation: what the gains of `controller` cost on OTHER models than the one they were designed on, and whether that closed loop is stable there -- the
    question a robustness study starts with (the nominal controller on plant n), answered on the linear model instead of by a nonlinear rollout per plant.  For every
    model i -- linearsystem (lqr.jl:63) at zd[i] on plant first_plant + i -- dlqr's cost recursion (lqr.jl:147-177) runs with the gain GIVEN (in place of lqr.jl:160):
    Abar = A - Bu K[k] - Bλ Kλ (lqr.jl:169), Pkp1 = Q + K[k]' R K[k] + Abar' Pk Abar (lqr.jl:170), break on norm(Pk - Pkp1) < tol (lqr.jl:172), all on the device
    (cclqr_value_create_policy); the gains never leave it.

    controller: an LQR, PlantLQR or LQRSweep of this mechanism -- one gain table shared by all models (LQR), or table i for model i.  Q, R, horizon: as for LQR
    (per-body 12 x 12 and per-constraint 1 x 1 blocks in the order of bodyids / eqcids, scaled by Δt), a single pair or -- as LQRSweep takes them -- lists of
    candidates, one per model (a list of one is shared).  A controller with a finite horizon is evaluated over that horizon (its table has one row per backward step);
    one with horizon math.inf holds one stationary gain and is evaluated over `horizon` (math.inf: ceil(10 / Δt) steps, lqr.jl:26).
    zd [n_models][nb][13]: every model's setpoint in the mechanism's body order, on its own plant's constraint manifold; Fτd [n_models][mu] (default 0).
    plants: a PlantBatch or None (the mechanism's own plant for every model); first_plant: global index of the plant zd[0] belongs to (default plants.first_index).

    P(i): model i's cost-to-go, read back; kbreak [n]; dnorm [n][2]: norm(Pk - Pkp1) of the last executed step and of the step before it (NaN: no such step);
    converged = dnorm[:, 0] < tol -- a recursion that does not converge is an answer, not an error --; contraction = sqrt(dnorm[:, 0] / dnorm[:, 1]), an estimate of
    the closed loop's spectral radius on the model (> 1: unstable there).  predicted_cost(mechanism, pv, z0) returns V_i = Δz_i' P_i Δz_i about zd[i].
    Not a Controller: simulate(..., pv) raises TypeError."""

    def __init__(self, mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, plants=None, first_plant=None, Fτd=None, tol=1e-5):
        if not isinstance(mechanism, Mechanism):
            raise TypeError("PolicyValue(mechanism, controller, bodyids, eqcids, Q, R, horizon, zd; ...)")
        if not isinstance(controller, (LQR, PlantLQR, LQRSweep)):
            raise TypeError("PolicyValue evaluates the gains of an LQR, PlantLQR or LQRSweep (got %s)" % type(controller).__name__)
        zd, n, Qs, Rs = _model_set(mechanism, controller, plants, zd, Q, R)
        Ntemp = _model_set_fields(self, mechanism, bodyids, eqcids, Qs, Rs, horizon, zd, plants, first_plant, Fτd)
        self.controller, self.n_models, self.N, self.tol = controller, n, Ntemp, float(tol)
        dev = _device_mech(mechanism)
        self._dev, self._setpoints = dev, None
        ctrl = controller._ctrl_handle(dev)
        try:
            self._value, self.kbreak, self.dnorm = _capi.value_create_policy(dev, ctrl, zd, self.ctrl_joints, self.Q, self.R, Ntemp, tol=tol, Fd=self.Fd,
                                                                             plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant)
        finally:
            ctrl.close()
        self.converged = self.dnorm[:, 0] < self.tol
        with np.errstate(invalid="ignore", divide="ignore"):
            self.contraction = np.sqrt(self.dnorm[:, 0] / self.dnorm[:, 1])


def _stationary_arguments(self, name, verb, mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, plants, first_plant, Fτd, tol, max_levels):
    """what StationaryPolicyValue and StationaryCovariance share before the device is asked: the refusals, the Δt-scaled weights in the mechanism's body order and
    the fields both keep (mechanism, controller, plants, n_models, first_plant, eqcids, ctrl_joints, Q, R, zd, Fd, N, tol, max_levels) -> (Fd, N: knots, 0 = to
    convergence)"""
    if not isinstance(mechanism, Mechanism):
        raise TypeError("%s(mechanism, controller, bodyids, eqcids, Q, R, horizon, zd; ...)" % name)
    if not isinstance(controller, (LQR, PlantLQR, LQRSweep)):
        raise ValueError("%s %s the stationary gain of an LQR, PlantLQR or LQRSweep (got %s)" % (name, verb, type(controller).__name__))
    zd, n, Qs, Rs = _model_set(mechanism, controller, plants, zd, Q, R)
    max_levels, span = _doubling_limits(horizon, max_levels, tol)
    ctrl_N = int(getattr(controller, "N", 0))      # the device convention of the three controllers: 0 = LQR{T,Inf}, one gain; N > 0 = a table of N - 1 rows
    if ctrl_N > 0 and ctrl_N - 1 != 1:
        raise ValueError("the controller holds a table of %d gain rows: doubling evaluates ONE stationary gain (horizon math.inf); PolicyValue steps through a table" % (ctrl_N - 1))
    Ntemp = _model_set_fields(self, mechanism, bodyids, eqcids, Qs, Rs, span, zd, plants, first_plant, Fτd)
    if horizon is None:
        Ntemp = 0
    self.controller, self.n_models, self.N, self.tol, self.max_levels = controller, n, Ntemp, float(tol), max_levels
    return self.Fd, Ntemp


class StationaryPolicyValue(_ValueTables):
    """Policy evaluation of a STATIONARY gain by doubling: what PolicyValue answers for the reference's default controller LQR{T,Inf} -- one gain (lqr.jl:40-43) -- in
    about 2 log2 N matrix combinations instead of N - 1 backward steps.  With that gain Abar (lqr.jl:169) and Qbar = Q + K' R K (lqr.jl:170) are constant, and with
    S(n) = sum_{i<n} (Abar^i)' Qbar Abar^i, M(n) = Abar^n the identity S(a+b) = S(a) + M(a)' S(b) M(a) gives P = S(n) + M(n)' Q M(n) for any n by square-and-multiply,
    on the device (cclqr_value_create_policy_doubling); the gains never leave it.

    controller: an LQR, PlantLQR or LQRSweep of this mechanism holding ONE gain row per table (horizon math.inf); anything else raises ValueError (a finite-horizon
    table is what PolicyValue steps through).  Q, R, zd, plants, first_plant, Fτd: as for PolicyValue.
    horizon: as for PolicyValue -- N - 1 steps exactly, math.inf meaning ceil(10 / Δt) knots (lqr.jl:26) --, so P(i) is PolicyValue(..., tol=0).P(i) to rounding;
    or None: level by level to convergence, the infinite-horizon cost.  Level j doubles to 2^j steps and stops when its increment norm(S(2^j) - S(2^(j-1))) < tol
    (reason 0), when norm(M(2^j)) > 1e50 (reason 2: the closed loop is unstable on the model) or at j == max_levels (reason 1; 1 .. 60).

    P(i): model i's cost-to-go, read back; levels [n]; steps [n] = N - 1, or 2^levels; reason [n]; dnorm, gnorm [n][2]: the increment norms and norm(M) of the last
    level and of the one before (NaN: no such level; a fixed horizon has gnorm[:, 0] = norm(M(N - 1)) only); converged = reason == 0 and diverged = reason == 2 (both
    False for a fixed horizon, which makes no test); spectral_radius = (gnorm0 / gnorm1)^(1 / 2^(levels - 1)), an estimate, reported and not promised.
    predicted_cost(mechanism, spv, z0) returns V_i = Δz_i' P_i Δz_i about zd[i].  Not a Controller: simulate(..., spv) raises TypeError."""

    def __init__(self, mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, plants=None, first_plant=None, Fτd=None, tol=1e-5, max_levels=40):
        Fd, Ntemp = _stationary_arguments(self, "StationaryPolicyValue", "evaluates", mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, plants, first_plant, Fτd,
                                          tol, max_levels)
        zd, max_levels = self.zd, self.max_levels
        dev = _device_mech(mechanism)
        self._dev, self._setpoints = dev, None
        ctrl = controller._ctrl_handle(dev)
        try:
            self._value, self.levels, self.reason, self.dnorm, self.gnorm = _capi.value_create_policy_doubling(
                dev, ctrl, zd, self.ctrl_joints, self.Q, self.R, Ntemp, tol=tol, max_levels=max_levels, Fd=Fd,
                plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant)
        finally:
            ctrl.close()
        _doubling_result(self, Ntemp, self.gnorm)


class StationaryCovariance:
    """The closed-loop state covariance of a STATIONARY gain under input noise, on the linear model of every plant: what spread of states and of actuator effort a
    noisy rollout should show.  With the one gain of LQR{T,Inf} (lqr.jl:40-43) the closed loop is Δz⁺ = Abar Δz + D w, Abar = A' - D K (lqr.jl:169; [A' | D] the
    projected model), w ~ (0, Wu) in input space, and after n steps from a start of covariance Σ0
        Σ_n = C(n) + M(n) Σ0 M(n)',   C(n) = sum_{i<n} Abar^i W (Abar^i)',   W = D Wu D',   M(n) = Abar^n
    -- the dual of StationaryPolicyValue, by the same doubling C(a+b) = C(a) + M(a) C(b) M(a)' on the device (cclqr_value_create_covariance_doubling).

    controller, Q, R, zd, plants, first_plant, Fτd: as for StationaryPolicyValue.  horizon: exactly the steps a rollout of that horizon makes after its start (N - 1
    of N knots), from Σ0; or None: the steady state, level by level until the increment relative to 2^floor(log2 tr W) falls below tol (reason 0), norm(M(2^j)) > 1e50
    (reason 2) or j == max_levels (reason 1).
    noise_scale=σ is shorthand for the law as the rollout applies it (simulate(..., noise_scale=σ): feedback_inputs in cclqr_rollout_step.h adds the SAME sample to
    every controlled input, trackingLQR_triple_cartpole.jl:98): Wu = σ² ones((mu, mu)).  Wu: [mu][mu], or a list of n_models of them; not together with noise_scale.
    Sigma0: [12 nb][12 nb] in the order of bodyids (permuted as Q is), or a list of n_models; not with horizon=None (a steady state does not depend on the start).  At
    least one of noise_scale, Wu, Sigma0 must be given.

    Sigma(i): model i's covariance, mechanism body order, read back; stage_cost [n][2] = tr(Q Σ), tr(R K Σ K'): the expected stage costs Score's Jx, Ju grow by per
    step; state_std [n][12 nb] in the order of bodyids and input_std [n][mu]: the RMS of every state coordinate and of every controlled input; levels, steps, reason,
    dnorm (in Σ's units), gnorm, converged, diverged, spectral_radius: as on StationaryPolicyValue.  Not a Controller and not a cost-to-go: simulate(..., cov) and
    predicted_cost(..., cov, ...) raise TypeError."""

    def __init__(self, mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, noise_scale=None, Wu=None, Sigma0=None, plants=None, first_plant=None, Fτd=None,
                 tol=1e-8, max_levels=40):
        Fd, Ntemp = _stationary_arguments(self, "StationaryCovariance", "propagates noise through", mechanism, controller, bodyids, eqcids, Q, R, horizon, zd, plants,
                                          first_plant, Fτd, tol, max_levels)
        n, nb, mu = self.n_models, len(mechanism.bodies), len(self.eqcids)
        if noise_scale is None and Wu is None and Sigma0 is None:
            raise ValueError("none of noise_scale, Wu and Sigma0 is given: there is no covariance to propagate")
        if Sigma0 is not None and horizon is None:
            raise ValueError("Sigma0 with horizon=None: a steady state does not depend on the start")
        self.Wu, self.Sigma0 = Wu, Sigma0 = _noise_arguments(self, bodyids, nb, mu, n, noise_scale, Wu, Sigma0)
        dev = _device_mech(mechanism)
        self._dev = dev
        ctrl = controller._ctrl_handle(dev)
        try:
            self._sigma, self.stage_cost, zstd, self.input_std, self.levels, self.reason, self.dnorm, self.gnorm = _capi.value_create_covariance_doubling(
                dev, ctrl, self.zd, self.ctrl_joints, self.Q, self.R, Wu, Sigma0, Ntemp, tol=tol, max_levels=self.max_levels, Fd=Fd,
                plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant)
        finally:
            ctrl.close()
        self.state_std = np.empty_like(zstd)
        self.state_std[:, self._to_bodyids] = zstd
        _doubling_result(self, Ntemp, self.gnorm)

    def Sigma(self, i):
        """model i's covariance [12 nb][12 nb], mechanism body order, read back from the device (cclqr_value_get)"""
        return self._sigma.get(i)

    def close(self):
        self._sigma.close()


def _is_device_tensor(a):
    return hasattr(a, "data_ptr") and bool(getattr(a, "is_cuda", False))


class PlantTrackingLQR(Controller):
    """One TrackingLQR per plant of a PlantBatch (and per reference trajectory), designed in one call: for every plant k,
    TrackingLQR(mechanism_k, storage_k, Fτ_k, eqcids, Q, R) (lqr_tracking.jl:17-43) where mechanism_k is the mechanism rebuilt with plant k's masses, inertias and
    joint vertices -- linearsystem at the knots 1 .. N-1 of every trajectory (lqr_tracking.jl:88) and the recursion of lqr_tracking.jl:73-122 per plant on the
    device, the gains never leaving it (cclqr_ctrl_create_tracking_batch_plants).

    storage: a batched Storage with one instance per plant, or its raw [n][N][nb][13] array (what simulate(mech, Storage(N, nb), OpenLoop(...), z0=, plants=)
    returns), each trajectory on its own plant's constraint manifold; a torch tensor on the device is read in place.  Fτ: [N][mu] shared, or [n][N][mu].
    plants: a PlantBatch, or None = n trajectories on the mechanism's own plant.  Q, R: per-body 12 x 12 and per-constraint 1 x 1 blocks, scaled by Δt.
    first_plant: global index of the plant storage[0] belongs to (default plants.first_index).  fric [ne], noise_scale, noise_seed: the friction / noise law of
    examples/trackingLQR_triple_cartpole.jl:93-111, fixed at construction.  workspace_bytes: device workspace of the call (0: the library's default).
    kbreak [n] per plant, gains(i) reads plant i's table back.
    simulate(mech, steps, ctl, z0=, plants=, first_instance=): instance i reads table first_instance + i and runs on plant first_instance + i."""

    controlfunction = None

    def __init__(self, mechanism, plants, storage, Fτ, eqcids, Q, R, first_plant=None, fric=None, noise_scale=0.0, noise_seed=None, tol=1e-5, workspace_bytes=0,
                 controlfunction=None):
        if controlfunction is not None:
            raise ValueError("PlantTrackingLQR carries no controlfunction: its gains stay on the device (one TrackingLQR per plant with a closure: build a TrackingLQR per plant)")
        if not isinstance(mechanism, Mechanism):
            raise TypeError("PlantTrackingLQR(mechanism, plants, storage, Fτ, eqcids, Q, R; ...)")
        if plants is not None and plants.mechanism is not mechanism:
            raise ValueError("the PlantBatch was made for another mechanism")
        nb, mu = len(mechanism.bodies), len(eqcids)
        z = storage.z if isinstance(storage, Storage) else storage
        on_dev = _is_device_tensor(z)
        if not on_dev:
            z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim != 4 or tuple(z.shape[2:]) != (nb, 13):
            raise ValueError("storage must be [n][N][nb][13] = [n][N][%d][13], one trajectory per plant (got %s)" % (nb, tuple(z.shape)))
        n, N = int(z.shape[0]), int(z.shape[1])
        if n < 1 or N < 2:
            raise ValueError("storage must hold at least one trajectory of at least two steps (got %s)" % (tuple(z.shape),))
        self.first_plant = (0 if plants is None else plants.first_index) if first_plant is None else int(first_plant)
        if plants is not None:
            plants.rows_for(self.first_plant, n)      # every trajectory must find its plant
        assert len(eqcids) == len(R), "Missmatched length for constraints"
        assert len(Q) == nb, "Missmatched length for bodies"
        F = Fτ
        f_dev = _is_device_tensor(F)
        if F is not None and not f_dev:
            F = np.ascontiguousarray(F, dtype=np.float64)
            if F.shape == (N, mu) or (mu == 1 and F.shape == (N,)):
                F = np.ascontiguousarray(np.broadcast_to(F.reshape(1, N, mu), (n, N, mu)))
        if F is not None and tuple(F.shape) != (n, N, mu):
            raise ValueError("Fτ must be [N][mu] = [%d][%d] (shared) or [n][N][mu] = [%d][%d][%d] (got %s)" % (N, mu, n, N, mu, tuple(F.shape)))
        if F is not None and f_dev != on_dev:
            raise ValueError("storage and Fτ must both be host arrays or both device tensors")
        self.mechanism, self.plants, self.n_plant = mechanism, plants, n
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        self.Q = _blockdiag([np.asarray(q, dtype=np.float64) for q in Q]) * mechanism.Δt     # lqr_tracking.jl:22
        self.R = _blockdiag([np.asarray(r, dtype=np.float64) for r in R]) * mechanism.Δt     # lqr_tracking.jl:23
        self.zd, self.Fd, self.N, self.NK = z, F, N, 12 * nb
        self.fric, self.noise_scale, self.noise_seed = fric, float(noise_scale), noise_seed
        dev = _device_mech(mechanism)
        ph = None if plants is None else plants.handle(dev)
        kw = dict(Fd=F, plants=ph, first_plant=self.first_plant, tol=tol, fric=fric, noise_scale=noise_scale, noise_seed=noise_seed, workspace_bytes=workspace_bytes)
        if on_dev:
            import torch
            if z.dtype != torch.float64 or not z.is_contiguous() or (F is not None and (F.dtype != torch.float64 or not F.is_contiguous())):
                raise ValueError("device tensors must be contiguous float64")
            kw.update(Fd=None if F is None else F.data_ptr(), n_ctrl=n, N=N, on_device=True, stream=torch.cuda.current_stream().cuda_stream)
            self._handle = _capi.BatchTrackingHandle(dev, z.data_ptr(), self.ctrl_joints, self.Q, self.R, **kw)
        else:
            self._handle = _capi.BatchTrackingHandle(dev, z, self.ctrl_joints, self.Q, self.R, **kw)
        self.kbreak = self._handle.kbreak

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _borrow_tables(self, dev, fric, noise_scale, noise_seed,
                              "the friction / noise law of a PlantTrackingLQR is fixed at construction (PlantTrackingLQR(..., fric=, noise_scale=, noise_seed=))")

    def gains(self, i):
        """K[k][j] of plant i's table, [N-1][mu][12 nb] in the mechanism's body order, read back from the device (cclqr_ctrl_get_gains)"""
        return _capi.ctrl_gains(_device_mech(self.mechanism), self._handle, i)

    def close(self):
        self._handle.close()


class Storage:
    """Storage{T}(steps, Nb): x[i][k], q[i][k], v[i][k], ω[i][k]  (lqr_tracking.jl:32-35).  Batched: leading instance axis.
    `z` is the raw [n_inst][steps][nb][13] array; x/q/v/ω index as storage.x[i][k] for instance 0 (or .instance(n))."""

    def __init__(self, steps, nb, n_inst=1, z=None, status=None, zT=None):
        self.steps, self.nb, self.n_inst = int(steps), int(nb), int(n_inst)
        self.z = np.zeros((n_inst, steps, nb, 13)) if z is None else z
        if z is None:
            self.z[..., 3] = 1.0
        self.status = status
        self.zT = zT
        self.score = None          # [n_inst][4] = Jx, Ju, peak, last_out of simulate(..., score=)
        self.ensemble = None       # EnsembleStats of simulate(..., ensemble=): the batch across its instances, per step
        self.joints = None         # JointSeries of simulate(..., joints=): the run in joint coordinates, and its statistics across the instances
        self.invariants = None     # InvariantSeries of simulate(..., invariants=): energy, constraint gaps, quaternion norms, and a verdict per instance

    def instance(self, n):
        one = Storage(self.steps, self.nb, 1, self.z[n:n + 1], None if self.status is None else self.status[n:n + 1],
                      None if self.zT is None else self.zT[n:n + 1])
        one.score = None if self.score is None else self.score[n:n + 1]
        return one

    def _field(self, lo, hi):
        return [self.z[0, :, i, lo:hi] for i in range(self.nb)]

    x = property(lambda self: self._field(0, 3))
    q = property(lambda self: self._field(3, 7))
    v = property(lambda self: self._field(7, 10))
    ω = property(lambda self: self._field(10, 13))
    w = ω


class TrackingLQR(Controller):
    """TrackingLQR{T,N,NK}: per-step setpoints copied out of `storage` and per-step feed-forward Fτ  (lqr_tracking.jl:3-43)"""

    def __init__(self, mechanism, storage, Fτ, eqcids, Q, R, controlfunction=None):
        self.controlfunction = controlfunction          # lqr_tracking.jl:19: a host closure (batch, lqr, k); None = control_trackinglqr! on the device
        nb = len(mechanism.bodies)
        N = storage.steps
        self.mechanism = mechanism
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        self.Q = _blockdiag([np.asarray(q, dtype=np.float64) for q in Q]) * mechanism.Δt     # lqr_tracking.jl:22
        self.R = _blockdiag([np.asarray(r, dtype=np.float64) for r in R]) * mechanism.Δt     # lqr_tracking.jl:23
        self.zd = np.ascontiguousarray(storage.z[0])                                          # lqr_tracking.jl:30-37
        mu = len(self.eqcids)
        self.Fd = np.array([[np.asarray(Fτ[k][i], dtype=np.float64).reshape(-1)[0] for i in range(mu)] for k in range(N)]).reshape(N, mu)
        dev = _device_mech(mechanism)
        self.projected = bool(getattr(mechanism, "has_loops", False))
        if self.projected:
            # closed loops: the projected pair (A'_k, D_k) of every knot from the device's constrained step map (see LQR), recursion with
            # no multipliers left
            mx = 12 * nb
            Ap, D = _capi.linearize_projected(dev, self.zd[:N - 1], self.ctrl_joints, self.Fd[:N - 1])
            self.K, self.kbreak = _capi.riccati_tv(Ap, D, np.zeros((N - 1, mx, 0)), np.zeros((N - 1, 0, mx)), self.Q, self.R, N)
        else:
            self.K, self.kbreak = _capi.riccati_tracking(dev, self.ctrl_joints, self.zd, self.Fd, self.Q, self.R, N)   # lqr_tracking.jl:40
        self.N = N
        self.NK = 12 * nb

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _capi.CtrlHandle(dev, self.ctrl_joints, K=self.K, N=self.N, zd=self.zd, Fd=self.Fd, fric=fric, noise_scale=noise_scale, noise_seed=noise_seed)


class TrackingCovariance:
    """The state covariance of a TRACKED run under input noise, at every knot: what spread of every body and of the actuator effort a noisy tracked swing-up should
    show, and the Jx, Ju that Score should report on average -- without Monte-Carlo rollouts.  Knots are j = 0 .. N-1, knot j being the state the law sees at step
    j + 1 (the indexing of a recorded rollout and of Score).  With [A'_j | D_j] the projected model linearised at knot j (lqr_tracking.jl:88) and K_j the gain row of
    knot j (lqr_tracking.jl:63-65), Abar_j = A'_j - D_j K_j (lqr_tracking.jl:107) and w ~ (0, Wu) in input space (trackingLQR_triple_cartpole.jl:98):
        Σ_0 = Sigma0 (or 0),   Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j',   j = 0 .. N-2
    one sequential recursion on the device (cclqr_value_create_covariance_tracking); models and gains never leave it.  Σ is a second moment: Sigma0 = δδ' with no
    noise is the deterministic perturbed start.

    controller: a TrackingLQR or a PlantTrackingLQR of this mechanism, without a controlfunction.  Its own zd / Fd are the trajectories, device tensors included.
    storage= ([n][N][nb][13], or a batched Storage) and Fτ= ([n][N][mu] or [N][mu]) replace them: that evaluates the NOMINAL TrackingLQR along each perturbed plant's own
    trajectory.  plants / first_plant: trajectory k is linearised on plant first_plant + k (default: the PlantTrackingLQR's own; None = the mechanism's plant).
    Q, R: per-body and per-constraint blocks in the order of bodyids / eqcids, Δt-scaled (lqr_tracking.jl:22-23), or lists of one pair per model -- exactly as
    StationaryCovariance takes them.  noise_scale=σ is Wu = σ² ones((mu, mu)): the rollout adds the SAME sample to every controlled input (see StationaryCovariance).
    Wu: [mu][mu] or one per model; Sigma0: [12 nb][12 nb] in the order of bodyids, or one per model.  At least one of noise_scale, Wu, Sigma0 must be given.
    Friction is not in the linear model: a controller's fric is ignored here.  workspace_bytes: device workspace of the call (0: the library's default); the result
    does not depend on it.

    state_std [n][N][12 nb] in the order of bodyids and input_std [n][N][mu] (zeros at the last knot: no input acts there): the RMS deviation of every state
    coordinate and controlled input at every knot; stage_cost [n][N][2] = tr(Q Σ_j), tr(R K_j Σ_j K_j'); expected_score [n][2] = their sums in knot order = E[Jx], E[Ju]
    of simulate(..., steps=N, score=Score(...)); Sigma(i): Σ_{N-1} of model i, mechanism body order, read back; N, n_models.  Not a Controller and not a cost-to-go:
    simulate(..., tc) and predicted_cost(..., tc, ...) raise TypeError."""

    def __init__(self, mechanism, controller, bodyids, eqcids, Q, R, noise_scale=None, Wu=None, Sigma0=None, plants=None, first_plant=None, storage=None, Fτ=None,
                 workspace_bytes=0):
        call = _tracking_arguments(self, name="TrackingCovariance", verb="propagates noise through", noun="covariance", mechanism=mechanism, controller=controller,
                                   bodyids=bodyids, eqcids=eqcids, Q=Q, R=R, noise_scale=noise_scale, Wu=Wu, Sigma0=Sigma0,
                                   nothing_given="none of noise_scale, Wu and Sigma0 is given: there is no covariance to propagate", plants=plants,
                                   first_plant=first_plant, storage=storage, Fτ=Fτ, workspace_bytes=workspace_bytes)
        try:
            self._sigma, self.stage_cost, zstd, self.input_std, self.expected_score = call(_capi.value_create_covariance_tracking, self.Wu, self.Sigma0)
        finally:
            call.close()
        self.state_std = np.empty_like(zstd)
        self.state_std[..., self._to_bodyids] = zstd

    def Sigma(self, i):
        """Σ_{N-1} of model i [12 nb][12 nb], mechanism body order, read back from the device (cclqr_value_get)"""
        return self._sigma.get(i)

    def close(self):
        self._sigma.close()


class _TrackingCall:
    """what _tracking_arguments hands back: call(entry, *noise, **more) runs a controller entry of _capi on the checked arguments -- entry(dev, ctrl, z, n, N,
    ctrl_joints, Q, R, *noise, Fd=, plants=, first_plant=, workspace_bytes=[, on_device=, stream=], **more); close() releases the controller handle made for it"""

    def __init__(self, dev, ctrl, args, kw, z):
        self.dev, self.ctrl, self.args, self.kw, self.z = dev, ctrl, args, kw, z      # z: the trajectories [n][N][nb][13] as checked, array or device tensor

    def __call__(self, entry, *noise, **more):
        return entry(self.dev, self.ctrl, *self.args, *noise, **self.kw, **more)

    def close(self):
        self.ctrl.close()


def _tracking_arguments(self, *, name, verb, noun, mechanism, controller, bodyids, eqcids, Q, R, noise_scale, Wu, Sigma0, nothing_given, plants, first_plant, storage,
                        Fτ, workspace_bytes, knot=None):
    """The argument handling TrackingCovariance and TrackingPolicyValue share, stated once: the controller (a TrackingLQR or PlantTrackingLQR of this mechanism without
    a controlfunction), the trajectories (its own, or storage= / Fτ=; host arrays or device tensors read in place), one table or one per model, the plants, the noise
    (noise_scale or Wu, one or one per model), a start covariance Sigma0 in the order of bodyids, the weight lists.  nothing_given: the refusal when none of
    noise_scale, Wu, Sigma0 is given (None: that is allowed).  Sets mechanism, controller, plants, first_plant, n_models, N, eqcids, ctrl_joints, Q, R (scaled,
    mechanism body order), Wu, Sigma0 (mechanism body order), _to_bodyids and _dev on `self`, and returns the _TrackingCall of the device entry."""
    if not isinstance(mechanism, Mechanism):
        raise TypeError("%s(mechanism, controller, bodyids, eqcids, Q, R; ...)" % name)
    if not isinstance(controller, (TrackingLQR, PlantTrackingLQR)):
        raise ValueError("%s %s the gain rows of a TrackingLQR or PlantTrackingLQR (got %s)" % (name, verb, type(controller).__name__))
    if controller.mechanism is not mechanism:
        raise ValueError("the controller was made for another mechanism")
    if getattr(controller, "controlfunction", None) is not None:
        raise ValueError("the controller carries a controlfunction: the %s is that of the device's own tracking law (lqr_tracking.jl:63-65), not of a host closure" % noun)
    batched = isinstance(controller, PlantTrackingLQR)
    if plants is None and first_plant is None and batched:
        plants, first_plant = controller.plants, controller.first_plant
    if plants is not None and plants.mechanism is not mechanism:
        raise ValueError("the PlantBatch was made for another mechanism")
    nb, mu, N = len(mechanism.bodies), len(eqcids), int(controller.N)
    if [int(e) for e in eqcids] != list(controller.eqcids):
        raise ValueError("eqcids are not the controller's: its gains act on other constraints")
    if knot is not None and (int(knot) != knot or not 0 <= int(knot) <= N - 1):
        raise ValueError("knot must be a knot of the controller's trajectory, 0 .. N-1 = %d (got %s)" % (N - 1, knot))
    z = controller.zd if storage is None else (storage.z if isinstance(storage, Storage) else storage)
    F = controller.Fd if Fτ is None else Fτ
    on_dev = _is_device_tensor(z)
    if not on_dev:
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim == 3:
            z = z[None]
    if z.ndim != 4 or tuple(z.shape[1:]) != (N, nb, 13) or z.shape[0] < 1:
        raise ValueError("storage must be [n][N][nb][13] = [n][%d][%d][13], one trajectory of the controller's N knots per model (got %s)" % (N, nb, tuple(z.shape)))
    n = int(z.shape[0])
    tables = controller.n_plant if batched else 1
    if tables not in (1, n):
        raise ValueError("the controller holds %d gain tables: one shared by all models, or one per model, %d" % (tables, n))
    f_dev = _is_device_tensor(F)
    if F is not None and not f_dev:
        F = np.ascontiguousarray(F, dtype=np.float64)
        if F.shape == (N, mu) or (mu == 1 and F.shape == (N,)):
            F = np.ascontiguousarray(np.broadcast_to(F.reshape(1, N, mu), (n, N, mu)))
    if F is not None and tuple(F.shape) != (n, N, mu):
        raise ValueError("Fτ must be [N][mu] = [%d][%d] (shared) or [n][N][mu] = [%d][%d][%d] (got %s)" % (N, mu, n, N, mu, tuple(F.shape)))
    if F is not None and f_dev != on_dev:
        raise ValueError("storage and Fτ must both be host arrays or both device tensors")
    if nothing_given is not None and noise_scale is None and Wu is None and Sigma0 is None:
        raise ValueError(nothing_given)
    Wu, Sigma0 = _noise_arguments(self, bodyids, nb, mu, n, noise_scale, Wu, Sigma0)
    Qs, Rs = _pair_lists(Q, R, n, "model")
    self.Q, self.R, _ = _scaled_pairs(Qs, Rs, bodyids, nb, mu, math.inf, mechanism.Δt)      # [n_weights][12 nb][12 nb], [n_weights][mu][mu]: scaled, mechanism body order
    self.first_plant = (0 if plants is None else plants.first_index) if first_plant is None else int(first_plant)
    if plants is not None:
        plants.rows_for(self.first_plant, n)      # every model must find its plant
    self.mechanism, self.controller, self.plants, self.n_models, self.N = mechanism, controller, plants, n, N
    self.eqcids = [int(e) for e in eqcids]
    self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
    self.Wu, self.Sigma0 = Wu, Sigma0
    dev = _device_mech(mechanism)
    self._dev = dev
    kw = dict(Fd=F, plants=None if plants is None else plants.handle(dev), first_plant=self.first_plant, workspace_bytes=workspace_bytes)
    zarg = z
    if on_dev:
        import torch
        if z.dtype != torch.float64 or not z.is_contiguous() or (F is not None and (F.dtype != torch.float64 or not F.is_contiguous())):
            raise ValueError("device tensors must be contiguous float64")
        kw.update(Fd=None if F is None else F.data_ptr(), on_device=True, stream=torch.cuda.current_stream().cuda_stream)
        zarg = z.data_ptr()
    if batched:
        if controller._handle.mech is not dev or not controller._handle.ptr:
            raise ValueError("the PlantTrackingLQR was designed on another device handle of the mechanism")
        ctrl = _BorrowedCtrl(controller._handle)
    else:
        ctrl = controller._ctrl_handle(dev)
    return _TrackingCall(dev, ctrl, (zarg, n, N, self.ctrl_joints, self.Q, self.R), kw, z)


class TrackingPolicyValue(_ValueTables):
    """The cost-to-go of a TRACKED run at every knot, and the price of its noise: what a tracked run is expected to cost from a perturbed start, what the nominal
    table costs along plant n's own trajectory, which knot's noise is the expensive one, and the terminal weight of a receding-horizon caller at knot j -- the
    adjoint of TrackingCovariance.  Knots are j = 0 .. N-1 as there.  With [A'_j | D_j] the projected model linearised at knot j (lqr_tracking.jl:88), K_j the gain
    row of knot j (lqr_tracking.jl:63-65) and Abar_j = A'_j - D_j K_j (lqr_tracking.jl:107), the Pkp1 of lqr_tracking.jl:108 with the gain given:
        P_{N-1} = Q,   P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j,   price_j = tr(Wu D_j' P_{j+1} D_j),   j = N-2 .. knot
    one sequential recursion on the device (cclqr_value_create_policy_tracking); models and gains never leave it.  price_j is what the noise sample injected at step
    j + 1 (trackingLQR_triple_cartpole.jl:98) adds to the expected cost of the rest of the run: with TrackingCovariance on the same arguments,
    sum(expected_score) = tr(P_0 Sigma0) + expected_noise_cost.

    controller, storage=, Fτ=, plants, first_plant, Q, R, noise_scale, Wu, workspace_bytes: exactly as TrackingCovariance takes them; without noise_scale and Wu no
    price is taken (noise_price and expected_noise_cost are zeros).  knot in [0, N-1]: the recursion stops there.

    P(i): P_knot of model i [12 nb][12 nb], mechanism body order, read back; noise_price [n][N] (zeros below knot and at N - 1); expected_noise_cost [n]: the prices
    of the knots j >= knot, summed from N - 2 downwards; N, n_models, knot.  predicted_cost(mechanism, tpv, z) returns V_i = Δz_i' P_knot,i Δz_i about row `knot` of
    trajectory i.  Not a Controller: simulate(..., tpv) raises TypeError."""

    def __init__(self, mechanism, controller, bodyids, eqcids, Q, R, noise_scale=None, Wu=None, plants=None, first_plant=None, storage=None, Fτ=None, knot=0,
                 workspace_bytes=0):
        call = _tracking_arguments(self, name="TrackingPolicyValue", verb="evaluates", noun="cost-to-go", mechanism=mechanism, controller=controller, bodyids=bodyids,
                                   eqcids=eqcids, Q=Q, R=R, noise_scale=noise_scale, Wu=Wu, Sigma0=None, nothing_given=None, plants=plants, first_plant=first_plant,
                                   storage=storage, Fτ=Fτ, workspace_bytes=workspace_bytes, knot=knot)
        self.knot, self._setpoints = int(knot), None
        try:
            self._value, price, total = call(_capi.value_create_policy_tracking, self.Wu, knot=self.knot)
        finally:
            call.close()
        self.noise_price = np.zeros((self.n_models, self.N)) if price is None else price
        self.expected_noise_cost = np.zeros(self.n_models) if total is None else total
        row = call.z[:, self.knot]      # the setpoints predicted_cost measures the error about; a device tensor's row is copied to the host
        self.zd = np.ascontiguousarray(row.cpu().numpy() if _is_device_tensor(row) else row, dtype=np.float64)


class Score:
    """What a run is ranked by: the quadratic cost the gains were designed to minimise, sum_k Δz' Q Δz + Δu' R Δu with the error Δz of lqr.jl:92-103 and the
    feedback command Δu = -K[k] Δz, evaluated on the device from the rollout's own states (cclqr_rollout_score).
    Score(mechanism, bodyids, eqcids, Q, R; settle_tol) takes Q and R as LQR(...) does: per-body 12 x 12 and per-constraint 1 x 1 blocks in the order of bodyids /
    eqcids, scaled by Δt (lqr.jl:18-19).  simulate(..., score=Score) returns a Storage with .score [n_inst][4] = Jx, Ju, peak stage cost, last step whose stage
    cost exceeded settle_tol (0: none; the instance is settled from step last_out + 1)."""

    def __init__(self, mechanism, bodyids, eqcids, Q, R, settle_tol=0.0):
        if not isinstance(mechanism, Mechanism):
            raise TypeError("Score(mechanism, bodyids, eqcids, Q, R; settle_tol)")
        nb = len(mechanism.bodies)
        assert len(bodyids) == len(Q) == nb, "Missmatched length for bodies"                    # lqr.jl:59
        assert len(eqcids) == len(R), "Missmatched length for constraints"                      # lqr.jl:60
        if not math.isfinite(float(settle_tol)):
            raise ValueError("settle_tol must be finite")
        inv = _body_order(bodyids, nb)
        Qb = [np.asarray(Q[i], dtype=np.float64) for i in inv]
        Rb = [np.asarray(r, dtype=np.float64).reshape(1, 1) for r in R]
        if any(q.shape != (12, 12) for q in Qb):
            raise ValueError("every Q block must be 12 x 12")
        self.mechanism = mechanism
        self.eqcids = [int(e) for e in eqcids]
        self.Q, self.R, _, _ = _weights_and_horizon(Qb, Rb, math.inf, mechanism.Δt)             # lqr.jl:18-19
        self.Qb = np.stack([self.Q[12 * b:12 * b + 12, 12 * b:12 * b + 12] for b in range(nb)])  # the blocks, mechanism body order
        self.settle_tol = float(settle_tol)
        if not (np.isfinite(self.Qb).all() and np.isfinite(self.R).all()):
            raise ValueError("the weights must be finite")

    def _handle(self, dev):
        return _capi.ScoreHandle(dev, self.Qb, self.R, self.settle_tol)


class Ensemble:
    """What a batch is summarised by ACROSS its instances: per step the mean and the spread of every coordinate of the error Δz of lqr.jl:92-103 and of the feedback
    command Δu = -K[k] Δz, and at the knots named in cov_knots the full covariance of Δz, evaluated on the device from the rollout's own states
    (cclqr_rollout_ensemble) -- the measurement TrackingCovariance / StationaryCovariance predict.  simulate(..., ensemble=Ensemble(mechanism, cov_knots=(j, ...)))
    returns a Storage with .ensemble, an EnsembleStats; row j of it (0-based, the state the law saw at step j + 1) is knot j of TrackingCovariance.
    quantiles=(p, ...): up to 16 probabilities in [0, 1] -- the same run also takes, per step and coordinate, the quantiles of the finite values across the instances
    (cclqr_rollout_quantiles: 0 the minimum, 0.5 the median, 1 the maximum; at most 16384 instances), the fan chart of a run outside the Gaussian regime."""

    def __init__(self, mechanism, cov_knots=(), quantiles=()):
        if not isinstance(mechanism, Mechanism):
            raise TypeError("Ensemble(mechanism, cov_knots=(), quantiles=())")
        knots = [int(j) for j in cov_knots]
        if any(j < 0 for j in knots) or any(int(j) != j for j in cov_knots):
            raise ValueError("cov_knots are 0-based knots of the run: whole numbers >= 0")
        self.mechanism = mechanism
        self.cov_knots = tuple(sorted(set(knots)))
        self.quantiles = tuple(float(p) for p in _capi.quantile_probs(quantiles))


class EnsembleStats:
    """The statistics of `count` instances at every step of a run: mean [steps][12 nb] and the centred sums of squares M2 of Δz (mechanism body order), input_mean /
    input M2 [steps][mu] of Δu, and the centred co-moment matrices C[j] [12 nb][12 nb] of the knots that were asked for.  var / std are about the ensemble mean,
    rms / second_moment about the setpoint: sqrt((M2 + n mean^2) / n) is what diag Σ_j of a covariance prediction with zero-mean error is compared with.
    With Ensemble(quantiles=): quantile(p) [steps][12 nb] and input_quantile(p) [steps][mu] for the probabilities that were asked for (median, min, max for 0.5, 0, 1)
    and finite_count [steps][12 nb + mu], the number of finite values each was taken over."""

    def __init__(self, count, mean, M2, input_mean, input_M2, C=None, *, probs=None, quantiles=None, finite_count=None, merged=False):
        # probs None: no quantiles were asked for (merged: because this is a merge of shards); else quantiles [steps][len(probs)][12 nb + mu]
        self.probs = None if probs is None else tuple(float(p) for p in probs)
        self._quantiles = None if probs is None else np.asarray(quantiles, dtype=np.float64)
        self.finite_count = None if probs is None else np.asarray(finite_count, dtype=np.int32)
        self._merged = bool(merged)
        self.count = int(count)
        self.mean, self.M2 = np.asarray(mean, dtype=np.float64), np.asarray(M2, dtype=np.float64)
        self.input_mean, self.input_M2 = np.asarray(input_mean, dtype=np.float64), np.asarray(input_M2, dtype=np.float64)
        self.C = {} if C is None else {int(j): np.asarray(c, dtype=np.float64) for j, c in C.items()}

    def var(self, ddof=0):
        return self.M2 / (self.count - ddof)

    def input_var(self, ddof=0):
        return self.input_M2 / (self.count - ddof)

    std = property(lambda self: np.sqrt(self.var()))
    input_std = property(lambda self: np.sqrt(self.input_var()))
    rms = property(lambda self: np.sqrt((self.M2 + self.count * self.mean ** 2) / self.count))
    input_rms = property(lambda self: np.sqrt((self.input_M2 + self.count * self.input_mean ** 2) / self.count))

    def _quantile_rows(self, p):
        if self._merged:
            raise KeyError("a merged EnsembleStats holds no quantiles: the order statistics of shards do not combine")
        asked = () if self.probs is None else self.probs
        if float(p) not in asked:
            raise KeyError("quantile %r was not asked for: Ensemble(quantiles=%s)" % (p, list(asked)))
        return self._quantiles[:, asked.index(float(p))]

    def quantile(self, p):
        """the quantile at probability p of every coordinate of Δz across the instances, [steps][12 nb]"""
        return self._quantile_rows(p)[:, :self.mean.shape[1]]

    def input_quantile(self, p):
        """... of Δu, [steps][mu]"""
        return self._quantile_rows(p)[:, self.mean.shape[1]:]

    median = property(lambda self: self.quantile(0.5))
    min = property(lambda self: self.quantile(0.0))
    max = property(lambda self: self.quantile(1.0))

    def _comoment(self, j):
        if int(j) not in self.C:
            raise KeyError("knot %d is not among the cov_knots of this run (%s)" % (int(j), sorted(self.C)))
        return self.C[int(j)]

    def cov(self, j, ddof=0):
        """covariance of Δz at knot j about the ensemble mean, [12 nb][12 nb]"""
        return self._comoment(j) / (self.count - ddof)

    def second_moment(self, j):
        """E[Δz Δz'] at knot j, about the setpoint: what Σ_j predicts"""
        m = self.mean[int(j)]
        return (self._comoment(j) + self.count * np.outer(m, m)) / self.count

    def merge(self, other):
        """the statistics of this ensemble and `other` together (the shards of dist.shard, on the host): the pairwise formula of Chan, Golub and LeVeque on
        (count, mean, M2, C).  An empty side (count 0) leaves the other's bits.  Co-moments are kept for the knots both sides hold.  The result holds NO quantiles:
        the order statistics of shards do not combine."""
        if not isinstance(other, EnsembleStats):
            raise TypeError("EnsembleStats.merge takes an EnsembleStats")
        if other.count == 0:
            return EnsembleStats(self.count, self.mean, self.M2, self.input_mean, self.input_M2, self.C, merged=True)
        if self.count == 0:
            return EnsembleStats(other.count, other.mean, other.M2, other.input_mean, other.input_M2, other.C, merged=True)
        if self.mean.shape != other.mean.shape or self.input_mean.shape != other.input_mean.shape:
            raise ValueError("the two ensembles differ in steps or coordinates")
        na, nb = float(self.count), float(other.count)
        n = na + nb

        def both(ma, qa, mb, qb):
            d = mb - ma
            return ma + d * (nb / n), (qa + qb) + d * d * (na * nb / n)

        mean, M2 = both(self.mean, self.M2, other.mean, other.M2)
        imean, iM2 = both(self.input_mean, self.input_M2, other.input_mean, other.input_M2)
        C = {}
        for j in sorted(set(self.C) & set(other.C)):
            d = other.mean[j] - self.mean[j]
            C[j] = (self.C[j] + other.C[j]) + np.outer(d, d) * (na * nb / n)
        return EnsembleStats(self.count + other.count, mean, M2, imean, iM2, C, merged=True)

    @staticmethod
    def empty(steps, mx, mu, cov_knots=()):
        """the ensemble of no instances: the identity of merge"""
        return EnsembleStats(0, np.zeros((steps, mx)), np.zeros((steps, mx)), np.zeros((steps, mu)), np.zeros((steps, mu)), {int(j): np.zeros((mx, mx)) for j in cov_knots})


class Joints:
    """A run in joint coordinates: per instance, step and joint the minimal coordinate of pid.jl:43-57 (the angle about / the offset along the joint axis, the number
    PID regulates) and the relative joint velocity the friction law of examples/trackingLQR_triple_cartpole.jl:98-101 acts on, formed on the device from the
    rollout's own states (cclqr_rollout_joints), and their statistics across the instances (cclqr_series_ensemble, cclqr_series_quantiles).
    simulate(..., joints=Joints(mechanism)) returns a Storage with .joints, a JointSeries, in the order of mechanism.eqconstraints.
    continuous: a revolute's angle is made continuous in time per instance (whole turns are counted from step 1), so that its mean, spread and median across
    instances mean something after a pendulum has gone over the top; False: the raw angle in [-2π, 2π] that PID sees.  rates=False: no velocities.  keep=False: only
    the statistics come back.  quantiles=(p, ...): up to 16 probabilities in [0, 1] (at most 16384 instances).  A FixedOrientation constraint has no coordinate: 0."""

    def __init__(self, mechanism, continuous=True, rates=True, keep=True, quantiles=()):
        if not isinstance(mechanism, Mechanism):
            raise TypeError("Joints(mechanism, continuous=True, rates=True, keep=True, quantiles=())")
        for name, v in (("continuous", continuous), ("rates", rates), ("keep", keep)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError("Joints(%s=) takes True or False (got %r)" % (name, v))
        self.mechanism = mechanism
        self.continuous, self.rates, self.keep = bool(continuous), bool(rates), bool(keep)
        self.quantiles = tuple(float(p) for p in _capi.quantile_probs(quantiles))


class JointSeries:
    """The joint coordinates of `count` instances at every step of a run, joints in the order of mechanism.eqconstraints: theta, rate [n][steps][ne] (None with
    keep=False; rate None with rates=False), their statistics across the instances mean, M2, rate_mean, rate_M2 [steps][ne] (std about the ensemble mean), and with
    Joints(quantiles=): quantile(p), rate_quantile(p) [steps][ne] for the probabilities that were asked for (median, min, max for 0.5, 0, 1) and finite_count
    [steps][ne or 2 ne], the number of finite values each was taken over."""

    def __init__(self, count, mean, M2, rate_mean=None, rate_M2=None, theta=None, rate=None, *, continuous=True, probs=None, quantiles=None, finite_count=None):
        arr = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
        self.count, self.continuous = int(count), bool(continuous)
        self.mean, self.M2, self.rate_mean, self.rate_M2, self.theta, self.rate = arr(mean), arr(M2), arr(rate_mean), arr(rate_M2), arr(theta), arr(rate)
        self.probs = None if probs is None else tuple(float(p) for p in probs)
        self._quantiles = None if probs is None else np.asarray(quantiles, dtype=np.float64)
        self.finite_count = None if probs is None else np.asarray(finite_count, dtype=np.int32)

    def var(self, ddof=0):
        return self.M2 / (self.count - ddof)

    def rate_var(self, ddof=0):
        if self.rate_M2 is None:
            raise KeyError("no rates were asked for: Joints(rates=False)")
        return self.rate_M2 / (self.count - ddof)

    std = property(lambda self: np.sqrt(self.var()))
    rate_std = property(lambda self: np.sqrt(self.rate_var()))

    def _quantile_rows(self, p):
        asked = () if self.probs is None else self.probs
        if float(p) not in asked:
            raise KeyError("quantile %r was not asked for: Joints(quantiles=%s)" % (p, list(asked)))
        return self._quantiles[:, asked.index(float(p))]

    def quantile(self, p):
        """the quantile at probability p of every joint coordinate across the instances, [steps][ne]"""
        return self._quantile_rows(p)[:, :self.mean.shape[1]]

    def rate_quantile(self, p):
        """... of every joint rate, [steps][ne]"""
        if self.rate_mean is None:
            raise KeyError("no rates were asked for: Joints(rates=False)")
        return self._quantile_rows(p)[:, self.mean.shape[1]:]

    median = property(lambda self: self.quantile(0.5))
    min = property(lambda self: self.quantile(0.0))
    max = property(lambda self: self.quantile(1.0))


class Invariants:
    """Can this run be trusted?  The integrator's own invariants of a rollout, formed on the device from the rollout's states (cclqr_rollout_invariants): per instance
    and step the kinetic and potential energy and their sum, the largest translational and rotational constraint residual over all joints (the rows the Newton solve
    drives to zero) and the largest | q.q - 1 | over the bodies; per instance an eight-number verdict that survives a run with no trajectory; and their statistics
    across the instances (cclqr_series_ensemble, cclqr_series_quantiles).  simulate(..., invariants=Invariants(mechanism)) returns a Storage with .invariants, an
    InvariantSeries.  With plants= every instance is measured on its own masses, inertias and joint vertices.
    keep=False: only the summary and the statistics come back.  rows=True: also every constraint row, .g [n][steps][ne][5] in the order of mechanism.eqconstraints
    (orc.constraints' layout).  quantiles=(p, ...): up to 16 probabilities in [0, 1] (at most 16384 instances)."""

    def __init__(self, mechanism, keep=True, rows=False, quantiles=()):
        if not isinstance(mechanism, Mechanism):
            raise TypeError("Invariants(mechanism, keep=True, rows=False, quantiles=())")
        for name, v in (("keep", keep), ("rows", rows)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError("Invariants(%s=) takes True or False (got %r)" % (name, v))
        self.mechanism = mechanism
        self.keep, self.rows = bool(keep), bool(rows)
        self.quantiles = tuple(float(p) for p in _capi.quantile_probs(quantiles))


class InvariantSeries:
    """The invariants of `count` instances at every step of a run.  Per instance and step (None with keep=False): kinetic, potential, energy, gap, twist, quat
    [n][steps]; with rows=True g [n][steps][ne][5], the constraint rows themselves.  Per instance, always: energy_first, energy_min, energy_max, energy_drift =
    max(energy_max - energy_first, energy_first - energy_min), gap_max, gap_step (the step, from 1, at which gap_max was first reached; 0: no finite row), twist_max,
    quat_max, bad_rows (rows with an output that is not finite), each [n]; over rows that are not finite nothing is taken, and an instance without a finite row has
    NaN.  Across the instances: mean, M2, std [steps][6] in the order NAMES, and with Invariants(quantiles=): quantile(p) [steps][6] for the probabilities that were
    asked for (median, min, max for 0.5, 0, 1) and finite_count [steps][6], the number of finite values each was taken over."""

    NAMES = ("kinetic", "potential", "energy", "gap", "twist", "quat")

    def __init__(self, count, summary, mean, M2, series=None, g=None, *, probs=None, quantiles=None, finite_count=None):
        arr = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
        self.count = int(count)
        self.summary = np.asarray(summary, dtype=np.float64).reshape(self.count, _capi.INVARIANTS_SUMMARY_LEN)
        self.mean, self.M2, self.series, self.g = arr(mean), arr(M2), arr(series), arr(g)
        self.probs = None if probs is None else tuple(float(p) for p in probs)
        self._quantiles = None if probs is None else np.asarray(quantiles, dtype=np.float64)
        self.finite_count = None if probs is None else np.asarray(finite_count, dtype=np.int32)

    def _column(self, i):
        return None if self.series is None else self.series[:, :, i]

    kinetic = property(lambda self: self._column(0))
    potential = property(lambda self: self._column(1))
    energy = property(lambda self: self._column(2))
    gap = property(lambda self: self._column(3))
    twist = property(lambda self: self._column(4))
    quat = property(lambda self: self._column(5))

    energy_first = property(lambda self: self.summary[:, 0])
    energy_min = property(lambda self: self.summary[:, 1])
    energy_max = property(lambda self: self.summary[:, 2])
    gap_max = property(lambda self: self.summary[:, 3])
    gap_step = property(lambda self: self.summary[:, 4].astype(np.int64))
    twist_max = property(lambda self: self.summary[:, 5])
    quat_max = property(lambda self: self.summary[:, 6])
    bad_rows = property(lambda self: self.summary[:, 7].astype(np.int64))

    @property
    def energy_drift(self):
        """max(E_max - E_1, E_1 - E_min) per instance, E_1 the energy at the first finite row"""
        return np.maximum(self.energy_max - self.energy_first, self.energy_first - self.energy_min)

    def var(self, ddof=0):
        return self.M2 / (self.count - ddof)

    std = property(lambda self: np.sqrt(self.var()))

    def quantile(self, p):
        """the quantile at probability p of each of the six invariants across the instances, [steps][6]"""
        asked = () if self.probs is None else self.probs
        if float(p) not in asked:
            raise KeyError("quantile %r was not asked for: Invariants(quantiles=%s)" % (p, list(asked)))
        return self._quantiles[:, asked.index(float(p))]

    median = property(lambda self: self.quantile(0.5))
    min = property(lambda self: self.quantile(0.0))
    max = property(lambda self: self.quantile(1.0))


class OpenLoop(Controller):
    """control!(mechanism, k) = setForce!(mechanism, joint, [U[k]])  — the open-loop closure of
    examples/trackingLQR_triple_cartpole.jl:46-48 as a table: U[k][i] for controlled joints eqcids."""

    def __init__(self, mechanism, eqcids, U):
        self.mechanism = mechanism
        self.eqcids = [int(e) for e in eqcids]
        self.ctrl_joints = [mechanism.joint_index(e) for e in self.eqcids]
        U = np.asarray(U, dtype=np.float64)
        self.Fd = U.reshape(U.shape[0], len(self.eqcids))
        self.N = self.Fd.shape[0] + 1          # every recorded step applies its force
        nb = len(mechanism.bodies)
        zd = np.zeros((self.Fd.shape[0], nb, 13))
        zd[..., 3] = 1.0
        self.zd = zd

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _capi.CtrlHandle(dev, self.ctrl_joints, K=None, N=self.N, zd=self.zd, Fd=self.Fd, fric=fric, noise_scale=noise_scale, noise_seed=noise_seed)


class PID(Controller):
    """PID{T,N}: P, I, D, eqcids, goals (integratederrors / lasterrors live on the device)   src/control/pid.jl:3-40
    PID(mechanism, eqcid::Int, goal; P, I, D)  /  PID(mechanism, eqcids::Vector, goals::Vector; P, I, D)"""

    def __init__(self, mechanism, eqcids, goals, P=None, I=None, D=None, controlfunction=None):
        self.controlfunction = controlfunction          # pid.jl:16, :27: a host closure (batch, pid, k); None = control_pid! on the device
        scalar = np.ndim(eqcids) == 0
        ids = [int(eqcids)] if scalar else [int(e) for e in eqcids]
        n = len(ids)
        vec = lambda v: np.zeros(n) if v is None else np.asarray(v, dtype=np.float64).reshape(n)
        self.mechanism = mechanism
        self.eqcids = ids
        self.goals, self.P, self.I, self.D = vec(goals), vec(P), vec(I), vec(D)
        for e in ids:
            assert len(mechanism.geteqconstraint(e)) == 5, "Only 1 DOF joints are supported"      # pid.jl:20,36
        self.joints = [mechanism.joint_index(e) for e in ids]

    def _ctrl_handle(self, dev, fric=None, noise_scale=0.0, noise_seed=None):
        return _capi.CtrlHandle(dev, [], K=None, N=0, fric=fric, noise_scale=noise_scale, noise_seed=noise_seed,
                                pid=dict(joint=self.joints, P=self.P, I=self.I, D=self.D, goal=self.goals))


class BatchState:
    """What a `controlfunction(batch, controller, k)` sees at step k: the states of every instance, in the mechanism's body order
    (z [n_inst][nb][13] = x, q, v, ω per body; the reference's closure reads body.state.xsol[2] ... of ONE mechanism, lqr.jl:98-103), and the
    joint inputs it sets with setForce (the reference's setForce!(mechanism, eqc, u), lqr.jl:110)."""

    def __init__(self, mechanism, z, k):
        self.mechanism, self.z, self.k = mechanism, z, int(k)
        self.n_inst = z.shape[0]
        self.u = {}
        self.on_device = not isinstance(z, np.ndarray)          # a torch tensor in HBM: the closure was registered with on_device()

    x = property(lambda self: self.z[:, :, 0:3])
    q = property(lambda self: self.z[:, :, 3:7])
    v = property(lambda self: self.z[:, :, 7:10])
    ω = property(lambda self: self.z[:, :, 10:13])
    w = ω


def on_device(controlfunction=None, graph=False):
    """Marks a `controlfunction(batch, controller, k)` as a DEVICE closure: simulate then hands it the batch's states as a torch tensor in HBM
    (batch.z [n_inst][nb][13], batch.x / .q / .v / .ω views of it) and expects its inputs as tensors (setForce), so the whole loop -- the
    closure's torch kernels, the hand-over of its inputs (cclqr_ctrl_set_feedforward, device to device) and the single-step launch -- runs on
    one stream with no host round trip per step.  control_lqr, state_error and setForce work on either kind of batch.
    graph=True (@on_device(graph=True)): the whole horizon is captured into a hipGraph by the first simulate call and REPLAYED by every later call
    with the same batch size and horizon -- the closure then runs once, at capture time: it must be capturable (no host synchronisation, no
    .item() / .cpu(), the same tensor shapes for every k) and a pure function of (batch, controller, k)."""
    def mark(f):
        f.on_device = True
        f.capture = bool(graph)
        return f
    return mark if controlfunction is None else mark(controlfunction)


def setForce(batch, eqc, u):
    """setForce!(mechanism, eqconstraint, u) on a batch: u a scalar, [n_inst] or [n_inst][1]; eqc an EqualityConstraint or its id"""
    j = batch.mechanism.joint_index(getattr(eqc, "id", eqc))
    if batch.on_device:
        import torch
        u = torch.as_tensor(u, dtype=torch.float64, device=batch.z.device).reshape(-1)
        batch.u[j] = u.expand(batch.n_inst) if u.numel() == 1 else u
        return
    batch.u[j] = np.broadcast_to(np.asarray(u, dtype=np.float64).reshape(-1), (batch.n_inst,)).copy()


def _device_tables(controller, device):
    """the controller's gain / setpoint / feed-forward tables as torch tensors on `device` (made once per controller and device)"""
    import torch
    cache = controller.__dict__.setdefault("_torch_tables", {})
    key = str(device)
    if key not in cache:
        cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device) for a in (controller.K, controller.zd, controller.Fd))
    return cache[key]


def _fused_gain_tables(lqr, device):
    """G [nK][mu][13 nb], h [nK][mu] with u_k = h_k - G_k z (z the state as stored, 13 numbers per body): K_k folded with the affine map z -> Δz of
    the step's setpoint (state_error: identity blocks for x, v, ω, the 3 x 4 matrix of qd' (x) . for the quaternion part)"""
    import torch
    cache = lqr.__dict__.setdefault("_torch_fused", {})
    key = str(device)
    if key not in cache:
        K = np.asarray(lqr.K, dtype=np.float64)
        nK, mu = K.shape[0], K.shape[1]
        nb = K.shape[2] // 12
        Kb = K.reshape(nK, mu, nb, 12)
        zd, Fd = np.asarray(lqr.zd, dtype=np.float64), np.asarray(lqr.Fd, dtype=np.float64)
        d = zd[np.minimum(np.arange(nK), zd.shape[0] - 1)] if zd.shape[0] > 1 else np.repeat(zd[:1], nK, 0)        # setpoint of table row i (step i + 1)
        fd = Fd[np.minimum(np.arange(nK), Fd.shape[0] - 1)] if Fd.shape[0] > 1 else np.repeat(Fd[:1], nK, 0)
        G = np.zeros((nK, mu, nb, 13))
        G[..., 0:3] = Kb[..., 0:3]                   # x
        G[..., 7:10] = Kb[..., 3:6]                  # v
        G[..., 10:13] = Kb[..., 9:12]                # ω
        s0, ax, ay, az = d[:, None, :, 3], -d[:, None, :, 4], -d[:, None, :, 5], -d[:, None, :, 6]
        kx, ky, kz = Kb[..., 6], Kb[..., 7], Kb[..., 8]
        # qe = M (s1, bx, by, bz)' with rows (ax, s0, -az, ay), (ay, az, s0, -ax), (az, -ay, ax, s0): the quaternion columns of G are K_q M
        G[..., 3] = kx * ax + ky * ay + kz * az
        G[..., 4] = kx * s0 + ky * az - kz * ay
        G[..., 5] = -kx * az + ky * s0 + kz * ax
        G[..., 6] = kx * ay - ky * ax + kz * s0
        c = np.zeros((nK, nb, 12))
        c[..., 0:3], c[..., 3:6], c[..., 9:12] = d[..., 0:3], d[..., 7:10], d[..., 10:13]
        h = fd + np.einsum("kmbj,kbj->km", Kb, c)
        cache[key] = (torch.from_numpy(G.reshape(nK, mu, 13 * nb)).to(device), torch.from_numpy(np.ascontiguousarray(h)).to(device))
    return cache[key]


def _state_error_device(batch, controller, k):
    """state_error on a device batch: the same expressions in torch"""
    import torch
    _, zd, _ = _device_tables(controller, batch.z.device)
    d = zd[min(k - 1, zd.shape[0] - 1)] if zd.shape[0] > 1 else zd[0]
    z = batch.z
    s0, a = d[None, :, 3:4], -d[None, :, 4:7]                    # qd' = (s0, a): the conjugate of the setpoint's quaternion
    s1, b = z[:, :, 3:4], z[:, :, 4:7]
    qe = s0 * b + s1 * a + torch.cross(a.expand_as(b), b, dim=2)
    dz = torch.cat([z[:, :, 0:3] - d[None, :, 0:3], z[:, :, 7:10] - d[None, :, 7:10], qe, z[:, :, 10:13] - d[None, :, 10:13]], dim=2)
    return dz.reshape(z.shape[0], -1)


def state_error(batch, controller, k):
    """Δz [n_inst][12 nb] of lqr.jl:92-103 / lqr_tracking.jl:49-62 about the controller's setpoint of step k (bodies in mechanism order)"""
    if getattr(batch, "on_device", False):
        return _state_error_device(batch, controller, k)
    zd = controller.zd
    d = zd[min(k - 1, zd.shape[0] - 1)] if zd.shape[0] > 1 else zd[0]
    zt = batch.z.transpose(1, 2, 0)             # [nb][13][n_inst]
    nb, n = zt.shape[0], zt.shape[2]
    # One [n_inst] plane per component: the batch that simulate hands a closure is stored that way (_simulate_hosted), so every operand below is a
    # contiguous run of n_inst numbers (an instance-major array goes through the same code as strided planes, a few times slower)
    dzt = np.empty((nb, 12, n))
    np.subtract(zt[:, 0:3], d[:, 0:3, None], out=dzt[:, 0:3])
    np.subtract(zt[:, 7:10], d[:, 7:10, None], out=dzt[:, 3:6])
    np.subtract(zt[:, 10:13], d[:, 10:13, None], out=dzt[:, 9:12])
    s0, ax, ay, az = d[:, 3, None], -d[:, 4, None], -d[:, 5, None], -d[:, 6, None]           # qd' = (s0, a): the conjugate of the setpoint's quaternion
    s1, bx, by, bz = zt[:, 3], zt[:, 4], zt[:, 5], zt[:, 6]
    dzt[:, 6] = s0 * bx + s1 * ax + (ay * bz - az * by)                                      # vector part of qd \ q = s0 b + s1 a + a x b
    dzt[:, 7] = s0 * by + s1 * ay + (az * bx - ax * bz)
    dzt[:, 8] = s0 * bz + s1 * az + (ax * by - ay * bx)
    return dzt.reshape(12 * nb, n).T


def control_lqr(batch, lqr, k):
    """control_lqr! (lqr.jl:89-139) / control_trackinglqr! (lqr_tracking.jl:46-71) on the host for a batch: u = Fτd - K[k] Δz on the
    controller's joints, gated by k < N; sets the forces and returns u [n_inst][mu] -- the building block of a custom controlfunction"""
    mu = len(lqr.eqcids)
    if getattr(batch, "on_device", False):
        import torch
        if not (lqr.N <= 0 or k < lqr.N):
            return torch.zeros((batch.n_inst, mu), dtype=torch.float64, device=batch.z.device)
        # Δz is affine in z for a fixed setpoint (the vector part of qd \ q is linear in q), so u = Fd - K Δz = h_k - z G_k' with one row G_k = K_k T_k
        # per input and step, folded on the host once per controller: the whole law is ONE product on the device (a closure's step is bound by
        # the number of torch launches, not by their arithmetic)
        G, h = _fused_gain_tables(lqr, batch.z.device)
        i = 0 if lqr.N <= 0 else min(k - 1, G.shape[0] - 1)
        u = h[i][None, :] - batch.z.reshape(batch.n_inst, -1) @ G[i].T
        for j, e in enumerate(lqr.eqcids):
            setForce(batch, e, u[:, j])
        return u
    u = np.zeros((batch.n_inst, mu))
    if lqr.N <= 0 or k < lqr.N:                                  # LQR{T,Inf}: always; finite: k < N (lqr.jl:106)
        dz = state_error(batch, lqr, k)
        K = lqr.K[0] if lqr.N <= 0 else lqr.K[min(k - 1, lqr.K.shape[0] - 1)]
        Fd = lqr.Fd[min(k - 1, lqr.Fd.shape[0] - 1)] if lqr.Fd.shape[0] > 1 else lqr.Fd[0]
        u = Fd[None, :] - (K.reshape(mu, -1) @ dz.T).T     # (this association: [mu][12 nb] x [12 nb][n_inst] is a row-major product whichever way Δz is stored)
        for i, e in enumerate(lqr.eqcids):
            setForce(batch, e, u[:, i])
    return u


def _simulate_hosted(mechanism, steps, controller, record, z0):
    """simulate! with a host-side controlfunction: one single-step launch per step through the k0 continuation of cclqr_rollout_dev (state and
    multipliers stay on the device), the states copied to the host for the closure and its joint inputs handed back (cclqr_ctrl_set_feedforward)"""
    import torch
    t = mechanism.tables()
    nb, n = t.nb, z0.shape[0]
    dev = _device_mech(mechanism)
    joints = [j for j in range(t.ne) if int(t.type[j]) in (0, 1)]             # every 1-DoF joint can be given an input (revolute, prismatic)
    slot = {j: i for i, j in enumerate(joints)}
    ctrl = _capi.CtrlHandle(dev, joints, K=None, N=0, Fd=np.zeros((n, len(joints))), n_ctrl=n)
    td = torch.device("cuda", torch.cuda.current_device())
    z = torch.from_numpy(np.ascontiguousarray(z0)).to(td)
    zn = torch.empty_like(z)
    lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=td)
    st = torch.zeros(n, dtype=torch.int32, device=td)
    traj = np.zeros((n, steps if record else 0, nb, 13))
    # an instance whose step ended on a non-finite residual is LOST: the fused rollout freezes it at its last pose, at rest, for the rest of
    # the horizon (rollout_chain.hip, LinkC::DEAD).  A launch per step keeps that through CCLQR_ROLLOUT_CARRY_STATUS: the status array travels from
    # launch to launch on the device, a lost instance is not stepped again (the closure still sees it, frozen, as it would in the fused run)
    stream = torch.cuda.current_stream().cuda_stream
    # The states reach the closure through one page-locked buffer, transposed on the device to one [n_inst] plane per state component: BatchState.z
    # is a [n_inst][nb][13] VIEW of it (valid during the call: the next step overwrites it), so that a closure's numpy slices z[:, b, i] are contiguous
    # runs of n_inst numbers.  The recorded trajectory is copied instance-major in a second transfer.
    zt_pinned = torch.empty((nb, 13, n), dtype=torch.float64, pin_memory=True)
    zh = zt_pinned.numpy().transpose(2, 0, 1)
    za_pinned = torch.empty(z.shape, dtype=torch.float64, pin_memory=True) if record else None
    U_pinned = torch.zeros((n, len(joints)), dtype=torch.float64, pin_memory=True)
    U, U_dev = U_pinned.numpy(), torch.zeros((n, len(joints)), dtype=torch.float64, device=td)
    try:
        for k in range(1, steps + 1):
            zt_pinned.copy_(z.permute(1, 2, 0))     # (synchronises the stream: the previous launch no longer reads the feed-forward table set_feedforward rewrites below)
            if record:
                za_pinned.copy_(z)
                traj[:, k - 1] = za_pinned.numpy()
            batch = BatchState(mechanism, zh, k)
            controller.controlfunction(batch, controller, k)
            U[:] = 0.0
            for j, u in batch.u.items():
                if j not in slot:
                    raise ValueError("setForce on a constraint without a degree of freedom")
                U[:, slot[j]] = u
            U_dev.copy_(U_pinned, non_blocking=True)      # (page-locked -> device on the launch's stream; the table is replaced device to device behind it;
                                                          #  U_pinned is rewritten only after the next step's blocking copy of the states has drained the stream)
            ctrl.set_feedforward(dev_ptr=U_dev.data_ptr(), length=U_dev.numel(), stream=stream)
            _capi.rollout_dev(dev, ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, 0, zn.data_ptr(), st.data_ptr(), stream, flags=_capi.ROLLOUT_CARRY_STATUS)
            z, zn = zn, z
        zT = z.cpu().numpy()
        status = st.cpu().numpy()
    finally:
        ctrl.close()
    return zT, traj, status


class _DeviceClosureRun:
    """One (controller, batch size, horizon) instance of the device-closure loop: its buffers in HBM, the per-instance feed-forward controller, and --
    for a closure registered with on_device(f, graph=True) -- the whole horizon captured once into a hipGraph and replayed by every later simulate
    call with the same shape (a Monte-Carlo sweep, an MPC loop over the same horizon): the replay costs no host time per step at all."""

    def __init__(self, mechanism, steps, controller, record, n):
        import torch
        self.torch = torch
        t = mechanism.tables()
        self.mechanism, self.controller, self.steps, self.record, self.n, self.nb, self.ne = mechanism, controller, steps, record, n, t.nb, t.ne
        self.dev = _device_mech(mechanism)
        self.joints = [j for j in range(t.ne) if int(t.type[j]) in (0, 1)]
        self.slot = {j: i for i, j in enumerate(self.joints)}
        self.ctrl = _capi.CtrlHandle(self.dev, self.joints, K=None, N=0, Fd=np.zeros((n, len(self.joints))), n_ctrl=n)
        td = self.td = torch.device("cuda", torch.cuda.current_device())
        self.z0 = torch.empty((n, t.nb, 13), dtype=torch.float64, device=td)
        self.lam = torch.zeros((n, 5 * t.ne), dtype=torch.float64, device=td)
        self.st = torch.zeros(n, dtype=torch.int32, device=td)
        self.traj = torch.empty((n, steps, t.nb, 13), dtype=torch.float64, device=td) if record else None
        self.U = torch.zeros((n, len(self.joints)), dtype=torch.float64, device=td)
        self.graph = None
        self.zT = None

    def close(self):
        self.graph = None
        self.ctrl.close()

    def _steps(self, flags):
        """the horizon on the current stream, from self.z0; leaves the final state in self.zT"""
        torch, n = self.torch, self.n
        stream = torch.cuda.current_stream().cuda_stream
        st, lam, U = self.st, self.lam, self.U
        st.zero_(); lam.zero_()            # (CCLQR_ROLLOUT_CARRY_STATUS: the status array carries every instance's status from launch to launch -- a lost one stays frozen)
        z, zn = self.z0.clone(), torch.empty_like(self.z0)
        for k in range(1, self.steps + 1):
            if self.record:
                self.traj[:, k - 1] = z
            batch = BatchState(self.mechanism, z, k)
            self.controller.controlfunction(batch, self.controller, k)
            U.zero_()
            for j, u in batch.u.items():
                if j not in self.slot:
                    raise ValueError("setForce on a constraint without a degree of freedom")
                U[:, self.slot[j]] = u
            self.ctrl.set_feedforward(dev_ptr=U.data_ptr(), length=U.numel(), stream=stream)
            _capi.rollout_dev(self.dev, self.ctrl, n, 1, k, z.data_ptr(), lam.data_ptr(), 0, 0, 0, zn.data_ptr(), st.data_ptr(), stream,
                              flags=flags | _capi.ROLLOUT_CARRY_STATUS)
            z, zn = zn, z
        self.zT = z

    def run(self, z0):
        torch = self.torch
        self.z0.copy_(torch.from_numpy(np.ascontiguousarray(z0)))
        if getattr(self.controller.controlfunction, "capture", False):
            if self.graph is None:
                # one step outside the capture first: what the closure builds lazily (device copies of its tables) must exist before a capture opens
                self.controller.controlfunction(BatchState(self.mechanism, self.z0, 1), self.controller, 1)
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    graph.capture_begin()
                    self._steps(_capi.ROLLOUT_NO_ALLOC)
                    graph.capture_end()
                torch.cuda.current_stream().wait_stream(side)
                self.graph = graph
            self.graph.replay()
        else:
            self._steps(0)
        zT = self.zT.cpu().numpy()
        status = self.st.cpu().numpy()
        trajh = self.traj.cpu().numpy() if self.record else np.zeros((self.n, 0, self.nb, 13))
        return zT, trajh, status


def _simulate_device_closure(mechanism, steps, controller, record, z0):
    """simulate! with a DEVICE closure (on_device): as _simulate_hosted, but nothing leaves HBM between the steps -- the closure reads a torch view of
    the state and returns tensors, its inputs reach the controller's feed-forward table device to device on the launch's stream, and the lost-instance
    bookkeeping (freeze at the last pose, at rest; status) is the library's (CCLQR_ROLLOUT_CARRY_STATUS).  One synchronisation, at the end.  With graph=True the
    run (buffers + captured graph) is kept on the controller and replayed by later calls of the same shape."""
    n = z0.shape[0]
    if not getattr(controller.controlfunction, "capture", False):
        run = _DeviceClosureRun(mechanism, steps, controller, record, n)
        try:
            return run.run(z0)
        finally:
            run.close()
    cache = controller.__dict__.setdefault("_device_closure_runs", {})
    key = (id(mechanism), id(controller.controlfunction), n, steps, bool(record))
    if key not in cache:
        for old in cache.values():          # one captured horizon per controller: a new shape replaces it
            old.close()
        cache.clear()
        cache[key] = _DeviceClosureRun(mechanism, steps, controller, record, n)
    return cache[key].run(z0)


def simulate(mechanism, tend_or_storage, controller, record=True, z0=None, fric=None, noise=None, noise_scale=None, noise_seed=None,
             first_instance=0, plants=None, score=None, chunk_steps=None, ensemble=None, joints=None, invariants=None):
    """simulate!(mechanism, tend::Real | storage::Storage, controller; record)  -> Storage

    z0 [n_inst][nb][13]: batch of initial states (default: the mechanism's current body states, one instance).
    fric [ne], noise [n_inst][steps] (injected samples) or noise_seed (device-side Philox-4x32 stream per instance), noise_scale:
    the friction/noise law of examples/trackingLQR_triple_cartpole.jl:93-111.  first_instance: global index of z0[0] when z0 is one
    rank's shard of a larger batch (the Philox stream of an instance is keyed by its global index).
    plants: a PlantBatch -- instance i runs with the masses, inertias and joint vertices of plant first_instance + i (the controller's gains stay the
    ones it was built with: the Monte-Carlo robustness run).  z0[i] must lie on plant i's constraint manifold (joint_position_states(..., plants=)).  For the
    fused laws (LQR, TrackingLQR with friction / noise, OpenLoop, PID).
    score: a Score -- the horizon runs in launches of chunk_steps steps (default: the largest whose slab [n_inst][chunk][nb][13] stays under 1 GiB) into one slab,
    each scored on the device behind its launch; the returned Storage carries .score [n_inst][4] (Jx, Ju, peak, last_out).  With record=False nothing larger than
    that slab ever exists; with record=True the slabs are also collected and the recorded trajectory is what was scored.  zT and status are bitwise those of the
    run without score=.  For the fused laws.
    ensemble: an Ensemble -- the same chunk loop (with or without score=, on the same slab) with cclqr_rollout_ensemble behind every launch; the returned Storage
    carries .ensemble, an EnsembleStats: per step the mean and the spread of every coordinate of Δz and Δu across the instances, and the covariance of Δz at the
    Ensemble's cov_knots -- and, with Ensemble(quantiles=), the quantiles of every coordinate at every step (at most 16384 instances).  Any chunk_steps, record or
    not, gives the same bits.  For the fused laws.
    joints: a Joints -- the same chunk loop (alone, or with score= / ensemble= on the same slab) with cclqr_rollout_joints behind every launch; the returned Storage
    carries .joints, a JointSeries: every joint's coordinate and rate per instance and step, and their mean, spread and quantiles across the instances.  Any
    chunk_steps, record or not, gives the same bits.  For the fused laws.
    invariants: an Invariants -- the same chunk loop (alone, or with score= / ensemble= / joints= on the same slab) with cclqr_rollout_invariants behind every launch;
    the returned Storage carries .invariants, an InvariantSeries: energy, constraint gaps and quaternion norm errors per instance and step, an eight-number verdict
    per instance that needs no trajectory, and their statistics across the instances.  Any chunk_steps, record or not, gives the same bits.  For the fused laws.
    After the call the mechanism's bodies hold instance 0's final state (simulate! mutates the mechanism)."""
    if isinstance(controller, PolicyValue):
        raise TypeError("a PolicyValue is not a Controller: simulate rolls out the controller it evaluates (PolicyValue.controller)")
    if isinstance(controller, StationaryPolicyValue):
        raise TypeError("a StationaryPolicyValue is not a Controller: simulate rolls out the controller it evaluates (StationaryPolicyValue.controller)")
    if isinstance(controller, StationaryCovariance):
        raise TypeError("a StationaryCovariance is not a Controller: simulate rolls out the controller it propagates noise through (StationaryCovariance.controller)")
    if isinstance(controller, TrackingCovariance):
        raise TypeError("a TrackingCovariance is not a Controller: simulate rolls out the controller it propagates noise through (TrackingCovariance.controller)")
    if isinstance(controller, TrackingPolicyValue):
        raise TypeError("a TrackingPolicyValue is not a Controller: simulate rolls out the controller it evaluates (TrackingPolicyValue.controller)")
    if isinstance(tend_or_storage, Storage):
        steps = tend_or_storage.steps
    else:
        steps = int(math.ceil(tend_or_storage / mechanism.Δt))     # steps = 1:ceil(tend/Δt)
    nb = len(mechanism.bodies)
    z0 = mechanism.state()[None] if z0 is None else np.asarray(z0, dtype=np.float64).reshape(-1, nb, 13)
    if score is None and ensemble is None and joints is None and invariants is None and chunk_steps is not None:
        raise ValueError("chunk_steps is an option of score= and ensemble=")
    if score is not None:
        if not isinstance(score, Score):
            raise TypeError("score= takes a Score(mechanism, bodyids, eqcids, Q, R)")
        if getattr(controller, "controlfunction", None) is not None:
            raise ValueError("score= with a custom controlfunction is not supported: the device scores the feedback command of the fused laws, a closure computes its own inputs")
        if score.mechanism is not mechanism:
            raise ValueError("the Score was made for another mechanism")
        if steps < 1:
            raise ValueError("score= needs at least one step")
    if ensemble is not None:
        if not isinstance(ensemble, Ensemble):
            raise TypeError("ensemble= takes an Ensemble(mechanism, cov_knots=(), quantiles=())")
        if getattr(controller, "controlfunction", None) is not None:
            raise ValueError("ensemble= with a custom controlfunction is not supported: the device forms the feedback command of the fused laws, a closure computes its own inputs")
        if ensemble.mechanism is not mechanism:
            raise ValueError("the Ensemble was made for another mechanism")
        if steps < 1:
            raise ValueError("ensemble= needs at least one step")
        if ensemble.cov_knots and ensemble.cov_knots[-1] >= steps:
            raise ValueError("cov_knots must lie in 0 .. steps - 1 = %d (got %s)" % (steps - 1, list(ensemble.cov_knots)))
        if ensemble.quantiles and z0.shape[0] > _capi.QUANTILE_MAX_INST:
            raise ValueError("quantiles= are taken over at most %d instances per run (got %d): the moments of shards merge, their order statistics do not"
                             % (_capi.QUANTILE_MAX_INST, z0.shape[0]))
    if joints is not None:
        if not isinstance(joints, Joints):
            raise TypeError("joints= takes a Joints(mechanism, continuous=True, rates=True, keep=True, quantiles=())")
        if getattr(controller, "controlfunction", None) is not None:
            raise ValueError("joints= with a custom controlfunction is not supported: the joint pass runs behind the launches of the fused laws")
        if joints.mechanism is not mechanism:
            raise ValueError("the Joints was made for another mechanism")
        if steps < 1:
            raise ValueError("joints= needs at least one step")
        if joints.quantiles and z0.shape[0] > _capi.QUANTILE_MAX_INST:
            raise ValueError("quantiles= are taken over at most %d instances per run (got %d): the moments of shards merge, their order statistics do not"
                             % (_capi.QUANTILE_MAX_INST, z0.shape[0]))
    if invariants is not None:
        if not isinstance(invariants, Invariants):
            raise TypeError("invariants= takes an Invariants(mechanism, keep=True, rows=False, quantiles=())")
        if getattr(controller, "controlfunction", None) is not None:
            raise ValueError("invariants= with a custom controlfunction is not supported: the invariants pass runs behind the launches of the fused laws")
        if invariants.mechanism is not mechanism:
            raise ValueError("the Invariants was made for another mechanism")
        if steps < 1:
            raise ValueError("invariants= needs at least one step")
        if invariants.quantiles and z0.shape[0] > _capi.QUANTILE_MAX_INST:
            raise ValueError("quantiles= are taken over at most %d instances per run (got %d): the moments of shards merge, their order statistics do not"
                             % (_capi.QUANTILE_MAX_INST, z0.shape[0]))
    if score is not None or ensemble is not None or joints is not None or invariants is not None:
        if chunk_steps is None:
            chunk_steps = _capi.default_chunk_steps(z0.shape[0], nb, steps)
        if int(chunk_steps) < 1:
            raise ValueError("chunk_steps must be at least 1")
    if plants is not None:
        if getattr(controller, "controlfunction", None) is not None:
            raise ValueError("plants= with a custom controlfunction is not supported yet: per-instance plants run under the fused laws (LQR, TrackingLQR, OpenLoop, PID)")
        if plants.mechanism is not mechanism:
            raise ValueError("the PlantBatch was made for another mechanism")
        plants.rows_for(first_instance, z0.shape[0])      # every instance must find its plant
    dev = _device_mech(mechanism)
    if (noise is not None or noise_seed is not None) and noise_scale is None:
        noise_scale = 1.0
    ph = None if plants is None else plants.handle(dev)
    scores = stats = series = checks = None
    if score is not None or ensemble is not None or joints is not None or invariants is not None:
        ctrl = controller._ctrl_handle(dev, fric=fric, noise_scale=0.0 if noise_scale is None else noise_scale, noise_seed=noise_seed)
        sh = None
        try:
            sh = None if score is None else score._handle(dev)
            traj = np.zeros((z0.shape[0], steps, nb, 13)) if record else None
            ens = None if ensemble is None else ((ctrl.mu, ensemble.cov_knots) + ((ensemble.quantiles,) if ensemble.quantiles else ()))
            jnt = None if joints is None else (joints.continuous, joints.rates, joints.keep, joints.quantiles)
            got = _capi.rollout_scored(dev, ctrl, sh, z0, steps, int(chunk_steps), noise=noise, first_instance=first_instance, plants=ph, traj_out=traj, ensemble=ens,
                                       **({} if jnt is None else dict(joints=jnt)),
                                       **({} if invariants is None else dict(invariants=(invariants.keep, invariants.rows, invariants.quantiles))))
            zT, status, scores = got[:3]
            if invariants is not None:
                v, got = got[-1], got[:-1]
                checks = InvariantSeries(v["count"], v["summary"], v["mean"], v["M2"], v["series"], v["g"],
                                         **(dict(probs=v["probs"], quantiles=v["quantiles"], finite_count=v["finite_count"]) if invariants.quantiles else {}))
            if joints is not None:
                j = got[-1]
                series = JointSeries(j["count"], j["mean"], j["M2"], j["rate_mean"], j["rate_M2"], j["theta"], j["rate"], continuous=j["continuous"],
                                     **(dict(probs=j["probs"], quantiles=j["quantiles"], finite_count=j["finite_count"]) if joints.quantiles else {}))
            if ensemble is not None:
                emean, eM2, eC = got[3][:3]
                more = dict(probs=ensemble.quantiles, quantiles=got[3][3], finite_count=got[3][4]) if ensemble.quantiles else {}
                stats = EnsembleStats(z0.shape[0], emean[:, :12 * nb], eM2[:, :12 * nb], emean[:, 12 * nb:], eM2[:, 12 * nb:], eC, **more)
        finally:
            if sh is not None:
                sh.close()
            ctrl.close()
    elif getattr(controller, "controlfunction", None) is not None:
        # a custom controlfunction (lqr.jl:14): the closure owns the whole law, as in the reference -- the built-in extras do not apply on top of it
        if fric is not None or noise is not None or noise_seed is not None:
            raise ValueError("fric / noise are options of the built-in laws; a custom controlfunction computes its own inputs")
        hosted = _simulate_device_closure if getattr(controller.controlfunction, "on_device", False) else _simulate_hosted
        zT, traj, status = hosted(mechanism, steps, controller, record, z0)
    else:
        ctrl = controller._ctrl_handle(dev, fric=fric, noise_scale=0.0 if noise_scale is None else noise_scale, noise_seed=noise_seed)
        try:
            zT, traj, status = _capi.rollout(dev, ctrl, z0, steps, k0=1, noise=noise, record=record, first_instance=first_instance, plants=ph)
        finally:
            ctrl.close()
    mechanism.set_state(zT[0])
    if isinstance(tend_or_storage, Storage) and record:
        tend_or_storage.z = traj
        tend_or_storage.n_inst = z0.shape[0]
        tend_or_storage.status, tend_or_storage.zT = status, zT
        tend_or_storage.score = scores
        tend_or_storage.ensemble = stats
        tend_or_storage.joints = series
        tend_or_storage.invariants = checks
        return tend_or_storage
    out = Storage(steps, nb, z0.shape[0], traj if record else np.zeros((z0.shape[0], 0, nb, 13)), status, zT)
    out.score = scores
    out.ensemble = stats
    out.joints = series
    out.invariants = checks
    return out


def predicted_cost(mechanism, controller, z0, first_instance=0, out=None):
    """V_i = Δz_i' P Δz_i: the cost the controller's gains were designed to achieve from the start z0[i] -- P the cost-to-go of its recursion (lqr.jl:170), Δz_i the
    error of lqr.jl:92-103 of z0[i] about the controller's setpoint.  The realised cost of a run, Jx + Ju of simulate(..., score=Score(Q, R)), over this is 1 inside
    the linear regime.  controller: an LQR, PlantLQR or LQRSweep built with keep_value=True; instance i reads table first_instance + i of the batched ones.
    That P is the cost on the model the gains were DESIGNED on.  For a controller that runs on another plant (simulate(mech, steps, LQR, plants=)) pass a
    PolicyValue(mech, controller, ..., zd, plants=): V_i = Δz_i' P_i Δz_i with P_i the given gains' cost-to-go on plant i's model (lqr.jl:169-170 with the gain
    given) and Δz_i the error about plant i's own setpoint zd[i] -- then realised / predicted tells "outside the linear regime" from "model mismatch".  A
    StationaryPolicyValue (the same cost-to-go of a stationary gain, by doubling) is taken the same way.
    A tracking controller keeps no cost-to-go of its own: pass a TrackingPolicyValue(mech, tracking, ..., knot=) -- V_i = Δz_i' P_knot,i Δz_i with P_knot,i the tracked
    run's cost-to-go at that knot on model i (lqr_tracking.jl:107-108 with the gain given) and Δz_i the error about row `knot` of trajectory i.
    z0 [n_inst][nb][13]: a numpy array -> a numpy array [n_inst]; or a float64 device tensor, read in place -> a device tensor [n_inst] (out: the tensor to fill),
    the evaluation left running on the current stream."""
    if not hasattr(controller, "_value_handle"):
        raise TypeError("predicted_cost takes an LQR, PlantLQR or LQRSweep built with keep_value=True, a PolicyValue or StationaryPolicyValue, or -- for a "
                        "TrackingLQR or PlantTrackingLQR -- a TrackingPolicyValue of it")
    if controller.mechanism is not mechanism:
        raise ValueError("the controller was made for another mechanism")
    import torch
    nb = len(mechanism.bodies)
    dev = _device_mech(mechanism)
    on_dev = _is_device_tensor(z0)
    if on_dev:
        if z0.dtype != torch.float64 or not z0.is_contiguous() or z0.numel() % (13 * nb):
            raise ValueError("a device z0 must be a contiguous float64 tensor [n_inst][%d][13]" % nb)
        dz = z0
    else:
        dz = torch.from_numpy(np.ascontiguousarray(z0, dtype=np.float64).reshape(-1, nb, 13)).to(torch.device("cuda", torch.cuda.current_device()))
    n = dz.numel() // (13 * nb)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=dz.device)
    elif not _is_device_tensor(out) or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != n:
        raise ValueError("out must be a contiguous float64 device tensor of %d entries" % n)
    value, own_value = controller._value_handle(dev)
    ctrl = None
    try:
        ctrl = controller._ctrl_handle(dev)
        _capi.value_eval(dev, ctrl, value, n, dz.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream, first_instance=first_instance)
        if not on_dev or own_value or not isinstance(ctrl, _BorrowedCtrl):
            torch.cuda.current_stream().synchronize()      # the handles made for this call are released below
    finally:
        if ctrl is not None:
            ctrl.close()
        if own_value:
            value.close()
    return out if on_dev else out.cpu().numpy()
