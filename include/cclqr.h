/*
 * cclqr.h -- C ABI of libcclqr.so: the MI355X (gfx950) implementation of ConstrainedControl.jl's batched
 * LQR-rollout hot path.  Plain pointers and sizes only; every entry point returns an int status
 * (0 = ok, < 0 = error, see CCLQR_E*); no exceptions cross the boundary.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference repo,
 * janbruedigam/ConstrainedControl.jl v0.3.0).  The reference has no batch API and no FFI of its own:
 * INTEGRATION.md shows the `ccall` stubs a maintainer adds on the Julia side.
 *
 * Layouts (all fp64, all dense arrays row-major unless stated):
 *   body state   z[13]   = x(3) world, q(4) scalar-first unit quaternion body->world, v(3) world, w(3) body frame
 *   batch state  z0[n_inst][nb][13]            (an instance = 13*nb contiguous doubles -> coalesced wave loads)
 *   trajectory   traj[n_inst][steps][nb][13]   = Storage x/q/v/w of every body at every step (lqr_tracking.jl:32-35)
 *   gains        K[nK][mu][12*nb]              = lqr.K[k][i] rows (lqr.jl:4); error order per body x,v,q~,w (lqr.jl:92-95)
 *   linear model A[mx][mx], Bu[mx][mu], Bl[mx][ml], G[ml][mx], mx = 12*nb, ml = 5*ne
 */
#ifndef CCLQR_H
#define CCLQR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCLQR_OK 0
#define CCLQR_EINVAL -1       /* size / topology mismatch  (the reference's @assert, lqr.jl:59-60) */
#define CCLQR_ESINGULAR -2    /* G*Bl or M singular        (LAPACK exception from lqr.jl:151,160) */
#define CCLQR_ENOCONV -3      /* soft: Newton / Riccati did not converge (lqr.jl:41 `@info`) */
#define CCLQR_EHIP -4         /* HIP runtime error; cclqr_last_error() has the text */
#define CCLQR_EUNSUPPORTED -5 /* valid for the reference, outside this build's scope (> 4 child joints on a body, nb > 64, loop mechanisms beyond 8 bodies / 12 joints) */

/* ABI version = cclqr_version().  A shim built against another header must refuse to run: the structs below are passed by pointer and
 * read in full.  200: cclqr_ctrl_desc.n_ctrl, cclqr_rollout_opts {noise_ws_dev, noise_ws_len, newton_mode}, cclqr_riccati_opts.keep_last,
 * the thread-local setters (cclqr_set_instance_offset, cclqr_set_pid_state, cclqr_riccati_path) removed.
 * 201 (additive over 200: same struct sizes and offsets): cclqr_rollout_opts.reserved became `flags` (CCLQR_ROLLOUT_NO_ALLOC), new entry points
 * cclqr_ctrl_set_feedforward and cclqr_abi_layout.  A shim checks cclqr_version() == the version it was written against AND, through
 * cclqr_abi_layout(), the sizeof / offsetof of every struct it mirrors.
 * 202 (additive over 201: no struct changed): per-instance plants -- the opaque cclqr_plants with cclqr_plants_create / cclqr_plants_destroy, and the
 * launch on them, cclqr_rollout_plants.
 * Still 202 (additive, no struct changed; tests/test_plants_host.py pins the number): one controller per plant -- cclqr_linearize_plants and
 * cclqr_ctrl_create_lqr_batch_plants.  A shim that needs them looks the symbols up: a 202 library built before them lacks them.
 * Still 202 (additive, no struct changed): one TrackingLQR per plant or trajectory -- cclqr_ctrl_create_tracking_batch_plants -- and the gain inspector
 * cclqr_ctrl_get_gains; looked up the same way.
 * Still 202 (additive, no struct changed): scoring a rollout on the device -- the opaque cclqr_score with cclqr_score_create / cclqr_score_destroy, and cclqr_rollout_score;
 * looked up the same way.
 * Still 202 (additive, no struct changed): one (Q, R) per problem / controller table -- cclqr_riccati_weights and cclqr_ctrl_create_lqr_batch_weights; looked up the
 * same way.  With n_weights = 1 they ARE cclqr_riccati_ex and cclqr_ctrl_create_lqr_batch_plants (which call them).
 * Still 202 (additive, no struct changed): the cost-to-go of the recursion and the cost it predicts -- cclqr_riccati_value, cclqr_ctrl_create_lqr_batch_value, the
 * opaque cclqr_value with cclqr_value_create / cclqr_value_get / cclqr_value_destroy, and cclqr_value_eval; looked up the same way.  With P = NULL / value = NULL the
 * first two ARE cclqr_riccati_weights, cclqr_riccati_tv and cclqr_ctrl_create_lqr_batch_weights (which call them).
 * Still 202 (additive, no struct changed): policy evaluation, a gain table's cost-to-go on another model -- cclqr_policy_value, cclqr_value_create_policy; looked up the
 * same way.  Their result is a cost-to-go like cclqr_riccati_value's: cclqr_value_get and cclqr_value_eval take it as it stands.
 * Still 202 (additive, no struct changed): a stationary gain's cost-to-go by doubling -- cclqr_policy_value_doubling, cclqr_value_create_policy_doubling; looked up the
 * same way.  cclqr_policy_value and cclqr_value_create_policy are unchanged.
 * Still 202 (additive, no struct changed): the stationary LQR gain by doubling the Riccati map -- cclqr_riccati_doubling, cclqr_ctrl_create_lqr_batch_doubling; looked up
 * the same way.  cclqr_riccati_value and cclqr_ctrl_create_lqr_batch_value are unchanged.
 * Still 202 (additive, no struct changed): the closed-loop state covariance under input noise by doubling -- cclqr_covariance_doubling, cclqr_value_create_covariance_doubling;
 * looked up the same way.  cclqr_policy_value_doubling and cclqr_value_create_policy_doubling are unchanged.
 * Still 202 (additive, no struct changed): the state covariance of a TRACKED run at every knot, a model and a gain row per knot -- cclqr_covariance_tracking, cclqr_value_create_covariance_tracking;
 * looked up the same way.  cclqr_covariance_doubling and cclqr_value_create_covariance_doubling are unchanged, their refusal of gain tables and tracking controllers included.
 * Still 202 (additive, no struct changed): the cost-to-go of a TRACKED run at every knot and the price of its noise, a model and a gain row per knot -- cclqr_policy_value_tracking, cclqr_value_create_policy_tracking;
 * looked up the same way.  cclqr_policy_value, cclqr_value_create_policy and the two tracking-covariance entries are unchanged.
 * Still 202 (additive, no struct changed): the statistics of a slab ACROSS its instances at every step -- cclqr_rollout_ensemble_ws_bytes, cclqr_rollout_ensemble; looked up
 * the same way.  cclqr_rollout_score is unchanged.
 * Still 202 (additive, no struct changed): the quantiles of a slab ACROSS its instances at every step -- cclqr_rollout_quantiles_ws_bytes, cclqr_rollout_quantiles; looked up
 * the same way.  cclqr_rollout_ensemble is unchanged.
 * Still 202 (additive, no struct changed): the joint coordinates of a slab and the statistics of any per-instance series -- cclqr_rollout_joints,
 * cclqr_series_ensemble_ws_bytes, cclqr_series_ensemble, cclqr_series_quantiles_ws_bytes, cclqr_series_quantiles; looked up the same way.
 * Still 202 (additive, no struct changed): the integrator's invariants of a slab -- cclqr_rollout_invariants; looked up the same way. */
#define CCLQR_ABI_VERSION 202

#define CCLQR_REVOLUTE 0      /* EqualityConstraint(Revolute(a, b, axis; p1, p2, qoffset)),  examples/lqr_cartpole.jl:26 */
#define CCLQR_PRISMATIC 1     /* EqualityConstraint(Prismatic(a, b, axis; p1, p2, qoffset)), examples/lqr_cartpole.jl:25 */
#define CCLQR_FIXED_ORIENTATION 2 /* EqualityConstraint(FixedOrientation(a, b; qoffset)), examples/lqr_deltabot.jl:25 (closed-loop mechanisms) */

/* Mechanism(origin, bodies, eqconstraints; g, Δt) -- examples/lqr_cartpole.jl:32.
 * A tree of nb bodies, each hung off its parent (or the origin, -1) by one 1-DoF joint (ne == nb); a body may carry up to 4 child joints.
 * Forests of chains and trees with branching bodies: up to 64 bodies (one lane of a wavefront per link).
 * Closed kinematic loops (examples/lqr_deltabot.jl:25-33: ne > nb, or a body that is the child of two joints, or a FixedOrientation
 * constraint; up to 8 bodies and 12 joints): cclqr_rollout* run them (LQR / TrackingLQR law with joint friction and noise, PID; one instance per wavefront, multipliers lam
 * [n_inst][5*ne]); cclqr_linearize returns their A, Bu, Bλ, G (ml = 5*ne rows, a FixedOrientation contributing two null rows), but G*Bλ
 * is singular for a loop, so LQR / TrackingLQR construction goes through cclqr_linearize_projected + cclqr_riccati / cclqr_riccati_tv with
 * ml = 0 (cclqr_riccati_tracking, which divides by G*Bλ at every knot, returns CCLQR_EUNSUPPORTED for them). */
typedef struct {
    int32_t nb, ne;
    double dt, g;          /* mechanism.Δt (lqr.jl:65), gravity along z */
    const double *mass;    /* [nb] */
    const double *inertia; /* [nb][9] body frame */
    const int32_t *parent; /* [ne] body index or -1 */
    const int32_t *child;  /* [ne] body index */
    const int32_t *type;   /* [ne] CCLQR_REVOLUTE / CCLQR_PRISMATIC */
    const double *p1;      /* [ne][3] vertex in the parent frame */
    const double *p2;      /* [ne][3] vertex in the child frame */
    const double *axis;    /* [ne][3] axis in the parent frame */
    const double *qoff;    /* [ne][4] orientation offset */
} cclqr_mech_desc;

/* LQR{T,N,NK} (lqr.jl:3-15) / TrackingLQR{T,N,NK} (lqr_tracking.jl:3-15) as flat tables. */
typedef struct {
    int32_t mu;                /* length(eqcids) */
    const int32_t *ctrl_joint; /* [mu] joint indices (eqcids, 0-based joint index) */
    int32_t nK;                /* gain matrices: N-1, or 1 for LQR{T,Inf} (lqr.jl:42) */
    int32_t N;                 /* horizon in steps; feedback is gated by k < N (lqr.jl:106); N <= 0: infinite horizon (lqr.jl:116) */
    const double *K;           /* [nK][mu][12*nb] or NULL (open loop) */
    int32_t nsp;               /* 1: xd,vd,qd,ωd of LQR ; N: per-step setpoints of TrackingLQR (lqr_tracking.jl:6-9) */
    const double *zd;          /* [nsp][nb][13] */
    const double *Fd;          /* [nsp][mu]  Fτd (lqr.jl:12, lqr_tracking.jl:12) */
    const double *fric;        /* [ne] viscous joint friction of examples/trackingLQR_triple_cartpole.jl:98-101, or NULL */
    double noise_scale;        /* cart noise amplitude, same file :98 (`randn()*2`); 0 = none */
    /* PID{T,N} (src/control/pid.jl:3-40) on 1-DoF joints in minimal coordinates; control_pid! (pid.jl:69-88) runs every step.
     * The integrated / last errors live for one launch unless cclqr_rollout_opts.pid_state_dev provides a buffer. npid = 0: none. */
    int32_t npid;
    const int32_t *pid_joint;  /* [npid] joint indices (eqcids) */
    const double *pid_P, *pid_I, *pid_D, *pid_goal; /* [npid]  P, I, D, goals (pid.jl:4-9) */
    /* `randn()` of trackingLQR_triple_cartpole.jl:98,125 as a reproducible counter-based stream: when noise_philox != 0
     * and no noise array is passed, sample (instance n, step k) = Box-Muller of Philox-4x32-10(counter = (k-1, 0, 0, 0),
     * key = (noise_seed low 32 bits ^ high 32 bits, n)), times noise_scale. */
    int32_t noise_philox;
    uint64_t noise_seed;
    /* Batched controllers ("Riccati run per instance on distinct setpoints"): n_ctrl > 1 gives every instance its
     * own table -- K [n_ctrl][nK][mu][12*nb], zd [n_ctrl][nsp][nb][13], Fd [n_ctrl][nsp][mu] -- and instance n of a launch reads table
     * first_instance + n (cclqr_rollout_opts), which must be < n_ctrl.  0 or 1: one table for all instances = the reference's one
     * LQR object per simulate! call (lqr.jl:106-111). */
    int32_t n_ctrl;
} cclqr_ctrl_desc;

typedef struct cclqr_mech cclqr_mech; /* opaque: device-resident mechanism tables */
typedef struct cclqr_ctrl cclqr_ctrl; /* opaque: device-resident controller tables */
typedef struct cclqr_plants cclqr_plants; /* opaque: device-resident per-instance plants (masses, inertias, joint vertices) */

const char *cclqr_last_error(void);
int cclqr_version(void);     /* CCLQR_ABI_VERSION of the library that was loaded */
/* sizeof and offsetof of the four structs that cross this boundary, as THIS library was compiled, so that a foreign-language mirror (the
 * Julia structs of julia/CCLQR.jl, the ctypes Structures of _capi.py -- the reference has no FFI of its own: INTEGRATION.md) can verify its layout
 * at load time instead of trusting a version number.  out[0..n) receives, in this order (CCLQR_ABI_LAYOUT_LEN values):
 *   cclqr_mech_desc:    sizeof, offsetof nb, ne, dt, g, mass, inertia, parent, child, type, p1, p2, axis, qoff                       (14)
 *   cclqr_ctrl_desc:    sizeof, offsetof mu, ctrl_joint, nK, N, K, nsp, zd, Fd, fric, noise_scale, npid, pid_joint, pid_P, pid_I, pid_D,
 *                       pid_goal, noise_philox, noise_seed, n_ctrl                                                                   (20)
 *   cclqr_riccati_opts: sizeof, offsetof path, bf16_terms, keep_last, reserved                                                       (5)
 *   cclqr_rollout_opts: sizeof, offsetof first_instance, pid_state_dev, pid_state_len, noise_ws_dev, noise_ws_len, newton_mode, flags,
 *                       newton_eps_alone                                                                                             (9)
 * Returns the number of values the library has (48), writes min(n, 48) of them; out may be NULL with n = 0. */
#define CCLQR_ABI_LAYOUT_LEN 48
int cclqr_abi_layout(int32_t *out, int32_t n);
int cclqr_device_count(int32_t *n);
int cclqr_set_device(int32_t dev);

/* Mechanism(...) constructor (examples/lqr_cartpole.jl:32): validates the topology, orders links chain by chain, uploads the tables. */
int cclqr_mech_create(const cclqr_mech_desc *desc, cclqr_mech **out);
int cclqr_mech_destroy(cclqr_mech *m);

/* LQR(...) (lqr.jl:17-48) / TrackingLQR(...) (lqr_tracking.jl:17-44) result as a device object consumed by cclqr_rollout*. */
int cclqr_ctrl_create(const cclqr_mech *m, const cclqr_ctrl_desc *desc, cclqr_ctrl **out);
int cclqr_ctrl_destroy(cclqr_ctrl *c);

/* LQR(mechanism, bodyids, eqcids, Q, R, horizon; xd, vd, qd, ωd, Fτd) (lqr.jl:50-66) for n_ctrl setpoints at once, entirely on the device
 * (SURVEY 8d configs[3]: "Riccati run per instance on distinct setpoints"): linearsystem at every zd[i] (lqr.jl:63), dlqr (lqr.jl:141-184)
 * and the per-instance controller tables of cclqr_ctrl_create (instance n of a rollout reads table first_instance + n) without the gains
 * -- n_ctrl (N-1) mu 12 nb doubles: 1 GB for 1024 seven-joint arms at N = 200 -- ever visiting the host.  Q [mx][mx], R [mu][mu] already Δt-scaled
 * (lqr.jl:18-19), N = horizon in steps, zd [n_ctrl][nb][13], Fd [n_ctrl][mu] or NULL, kbreak [n_ctrl] or NULL.  Tree mechanisms.
 * infinite_horizon != 0: LQR{T,Inf} (horizon = Inf, lqr.jl:25-27 and 40-43) -- N is Ntemp = ceil(10/Δt), the recursion runs its N-1 steps
 * (or breaks, lqr.jl:172), only Ku[1] is kept (n_ctrl mu 12 nb doubles: 39 MB for 8192 seven-joint arms) and control_lqr! is never gated
 * (lqr.jl:116-139); a problem whose recursion has not converged is reported through kbreak[i] == 1 (lqr.jl:41 `@info`). */
int cclqr_ctrl_create_lqr_batch(const cclqr_mech *m, int32_t n_ctrl, const double *zd, int32_t mu, const int32_t *ctrl_joint, const double *Fd,
                                const double *Q, const double *R, int32_t N, int32_t infinite_horizon, double tol, int32_t *kbreak,
                                cclqr_ctrl **out);

/* linearsystem(mechanism, xd, vd, qd, ωd, Fτd, bodyids, eqcids) -- call sites lqr.jl:63, lqr_tracking.jl:88.
 * Batched over nk knots (nk = 1 for LQR, N-1 for TrackingLQR).  Host pointers.
 * zd [nk][nb][13], Fd [nk][mu]; outputs A [nk][mx][mx], Bu [nk][mx][mu], Bl [nk][mx][ml], G [nk][ml][mx], ml = 5*ne. */
int cclqr_linearize(const cclqr_mech *m, int32_t nk, const double *zd, int32_t mu, const int32_t *ctrl_joint, const double *Fd,
                    double *A, double *Bu, double *Bl, double *G);

/* The same linear model with the multipliers eliminated -- A' = A - Bλ (G Bλ)^-1 G A and D = Bu - Bλ (G Bλ)^-1 G Bu, the projected pair the
 * recursion of lqr.jl:151-170 works with.  Defined for every topology cclqr_mech_create takes, and the only linearisation of closed-loop
 * mechanisms (examples/lqr_deltabot.jl:47-53), where G Bλ is singular (redundant constraint rows) but A', D are still unique; feed them to
 * cclqr_riccati with ml = 0.
 *   h <= 0: ANALYTIC -- the exact Jacobians of the one-step map on the device (linearsystem of lqr.jl:63 with the multipliers exogenous, for
 *           loops in their own bookkeeping), then G Bλ eliminated with complete pivoting up to its numerical rank.  The elimination keeps
 *           [G Bλ | G A | G Bu] of a knot in one compute unit's 160 KB of LDS; a mechanism it does not fit (from about 15 bodies: the 17-body
 *           chain needs 198 KB) is differenced with h = 1e-6 instead, so the call is defined for every mechanism either way;
 *   h > 0:  central differences (step h in every error coordinate x, v, q~, ω of lqr.jl:92-103 and every input) of the DEVICE's own constrained
 *           one-step map, one launch of nk (1 + 24 nb + 2 mu) single-step rollouts: an independent cross-check of the analytic form.
 * Ap [nk][mx][mx], D [nk][mx][mu]. Host pointers. */
int cclqr_linearize_projected(const cclqr_mech *m, int32_t nk, const double *zd, int32_t mu, const int32_t *ctrl_joint, const double *Fd,
                              double h, double *Ap, double *D);

/* dlqr(A, Bu, Bλ, G, Q, R, N) -- lqr.jl:141-184, batched over nprob independent problems (nprob = 1 in the reference).
 * Q [mx][mx] and R [mu][mu] are the already Δt-scaled block-diagonal weights (lqr.jl:18-19).
 * K [nprob][N-1][mu][mx] ([nprob][mu][mx] with cclqr_riccati_opts.keep_last); kbreak [nprob] = value of the loop index k after the loop
 * (lqr.jl:172-181). Host pointers.
 * Q and R are used as written, symmetric or not (lqr.jl:152-170 never symmetrises them); the kernels that assume a symmetric Pk are used only
 * when both are EXACTLY symmetric.  G*Bλ is factored for the backward steps that reach it, as in the reference: CCLQR_ESINGULAR (kbreak = the
 * step that met it) only when a step that runs meets a singular G*Bλ or M; with N = 1 nothing is factored.  Any mu >= 0 is served (mu > 64
 * on the tiled path). */
int cclqr_riccati(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                  const double *Q, const double *R, int32_t N, double tol, double *K, int32_t *kbreak);

/* Options of cclqr_riccati_ex / cclqr_riccati_tracking_ex (NULL or all zero = defaults).
 *   path        launch shape: 0 = choose by problem size and count, 1 = one LDS-resident workgroup per problem whenever the problem fits
 *               (mx up to ~96), 2 = every backward step tiled over the whole device.  Same results either way.
 *   bf16_terms  0 = fp64 MFMA, the PARITY mode (gains equal the reference recursion's to 1e-7).  1..3 = measured-error mode of
 *               BASELINE configs[3] ("dense Riccati on MFMA bf16 -> fp32 accumulate"): the two mx^3 products of a backward step
 *               (lqr.jl:170) run on v_mfma_f32_16x16x16_bf16 with fp32 accumulation, every fp64 operand split into that many bf16
 *               terms (1 = plain bf16, 3 = bf16x3).  Available on the tiled path for every shape and on the LDS-resident batched
 *               kernel for the Sawyer (mx 84, mu 7) and cartpole (mx 24, mu 1) shapes; other shapes take the tiled path.  Its gain
 *               error and speed are reported, not promised: it does NOT reproduce the fp64 gains and the 1e-5 break
 *               test of lqr.jl:172 never fires.
 *   keep_last   != 0: K is [nprob][mu][mx] and receives only the gain of the last executed backward step = Ku[1] after the back-fill of
 *               lqr.jl:179-181 = the single gain LQR{T,Inf} keeps (lqr.jl:40-43); the (N-1)-fold table is never materialised. */
typedef struct {
    int32_t path;
    int32_t bf16_terms;
    int32_t keep_last;
    int32_t reserved;
} cclqr_riccati_opts;

int cclqr_riccati_ex(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                     const double *Q, const double *R, int32_t N, double tol, double *K, int32_t *kbreak, const cclqr_riccati_opts *opts);
int cclqr_riccati_tracking_ex(const cclqr_mech *m, int32_t mu, const int32_t *ctrl_joint, const double *zd, const double *Fd, const double *Q,
                              const double *R, int32_t N, double tol, double *K, int32_t *kbreak, const cclqr_riccati_opts *opts);

/* cclqr_riccati_ex with one pair of weights per problem -- dlqr(A_p, Bu_p, Bλ_p, G_p, Q_p, R_p, N) (src/control/lqr.jl:141-184) for every p in one launch: the tuning
 * study that tries n_weights weightings of one model (A replicated) or of n_weights models.  Q [n_weights][mx][mx], R [n_weights][mu][mu], host pointers, used as
 * written (the Δt scaling of lqr.jl:18-19 is the caller's).  n_weights is 1 (one pair shared by all problems: exactly cclqr_riccati_ex) or nprob; any other value
 * is CCLQR_EINVAL before anything is allocated or launched, K untouched.  The kernels, the launch shape and the arithmetic are those of the shared-weights call --
 * only the address problem p reads its weights from differs, so problem p's gains are bitwise those of cclqr_riccati_ex on the same nprob models with (Q_p, R_p)
 * shared.  The kernels that assume a symmetric Pk run only when EVERY problem's Q and R are exactly symmetric.  K, kbreak, tol, opts (path, bf16_terms,
 * keep_last) and the error codes as cclqr_riccati_ex. */
int cclqr_riccati_weights(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                          int32_t n_weights, const double *Q, const double *R, int32_t N, double tol, double *K, int32_t *kbreak,
                          const cclqr_riccati_opts *opts);

/* cclqr_riccati_weights that also returns the cost-to-go -- the Pkp1 of src/control/lqr.jl:170, which dlqr (lqr.jl:141-184) computes at every backward step and
 * does not return.  P [nprob][mx][mx] (host) receives, per problem, the Pkp1 of the last backward step the problem executed: the step the break test of lqr.jl:172
 * fired on, step 1 when it never fired, Q_p when N = 1 (no step runs).  Row-major as the recursion holds it, in the order of the models and of Q; not symmetrised
 * when a Q or R is not symmetric.  V(dz) = dz' P dz is the cost the gains achieve on the linear model from the error dz -- the Lyapunov function of the closed loop
 * and the terminal weight of a receding-horizon caller.  A problem that ends CCLQR_ESINGULAR leaves its P unspecified.
 * time_varying != 0: the per-knot models of lqr_tracking.jl:73-122 as cclqr_riccati_tv takes them -- A [nprob][N-1][mx][mx], Bu, Bl, G alike, knot k at index
 * k - 1 (N >= 2) -- and P is the Pkp1 of lqr_tracking.jl:108.  P = NULL: nothing is emitted, and K, kbreak are bitwise those of the same call with P; with
 * time_varying = 0 that IS cclqr_riccati_weights, with time_varying != 0, nprob = 1, n_weights = 1 and opts = NULL it IS cclqr_riccati_tv. */
int cclqr_riccati_value(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                        int32_t n_weights, const double *Q, const double *R, int32_t N, double tol, int32_t time_varying, double *K, double *P, int32_t *kbreak,
                        const cclqr_riccati_opts *opts);

/* Device workspaces of the host-pointer entry points (cclqr_linearize, cclqr_riccati*, cclqr_rollout) are cached per calling thread, on
 * the device that thread was on when they were allocated, and reused by the next call; after cclqr_set_device to another GPU the next
 * call releases them there and starts a cache on the new device.  This returns them to the driver (they are re-allocated on demand);
 * a thread that exits without calling it leaves its blocks allocated until the process ends.  Every entry point that takes a
 * cclqr_mech returns CCLQR_EINVAL when the calling thread is not on the device the handle was created on. */
int cclqr_release_workspaces(void);

/* The recursion of lqr_tracking.jl:73-122 on per-knot linear models the caller brings: A [N-1][mx][mx], Bu [N-1][mx][mu], Bl [N-1][mx][ml],
 * G [N-1][ml][mx] (knot k = 1 .. N-1 at index k-1, as cclqr_riccati_tracking linearises them itself); ml = 0 with the projected pairs of
 * cclqr_linearize_projected gives the TrackingLQR of a closed-loop mechanism.  K [N-1][mu][mx], kbreak [1]. Host pointers.
 * A singular G*Bλ at a knot the sweep never reaches (below the break) is no error, as in lqr_tracking.jl:87-116. */
int cclqr_riccati_tv(int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                     const double *Q, const double *R, int32_t N, double tol, double *K, int32_t *kbreak);

/* dlqr(mechanism, xd, vd, qd, ωd, Fτd, eqcids, Q, R, N) -- lqr_tracking.jl:73-122: re-linearises at every knot (:88).
 * zd [N][nb][13], Fd [N][mu], K [N-1][mu][mx]. Host pointers. */
int cclqr_riccati_tracking(const cclqr_mech *m, int32_t mu, const int32_t *ctrl_joint, const double *zd, const double *Fd, const double *Q,
                           const double *R, int32_t N, double tol, double *K, int32_t *kbreak);

/* simulate!(mechanism, steps, controller; record) for n_inst independent instances -- the rollout loop of every
 * example's last line (e.g. examples/lqr_cartpole.jl:44) with control_lqr! (lqr.jl:89-139) / control_trackinglqr!
 * (lqr_tracking.jl:46-71) fused in.  Step indices run k0 .. k0+steps-1 (1-based like the reference).
 * HOST pointers; traj may be NULL (record=false); noise [n_inst][steps] standard-normal samples or NULL;
 * status[n_inst] = max Newton iterations used, negative if a step failed: -CCLQR_NEWTON_MAXIT when a solve hit the iteration cap, a smaller magnitude when a
 * step ended on a non-finite residual (the instance is LOST: frozen at its last pose, at rest, for the rest of the launch). */
int cclqr_rollout(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, const double *z0,
                  const double *noise, double *traj, double *zT, int32_t *status);

/* Same with DEVICE pointers and an explicit hipStream_t (passed as void*): nothing is copied, the launch is
 * asynchronous.  lam [n_inst][5*ne] carries the multipliers (Newton warm start) between calls; it is read when
 * k0 > 1 and always written; pass NULL to start from zero and discard. */
int cclqr_rollout_dev(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, const double *z0_dev,
                      double *lam_dev, const double *noise_dev, int64_t noise_stride, double *traj_dev, double *zT_dev,
                      int32_t *status_dev, void *stream);

/* Per-launch options of cclqr_rollout_ex (NULL or all zero = defaults).
 *   first_instance  global index of instance 0 of this launch: the Philox noise stream (noise_philox) and the per-instance
 *                   controller table (n_ctrl > 1) of an instance are keyed by its GLOBAL index, so rank r of a sharded batch
 *                   passes its shard's first index and reproduces the unsharded batch;
 *   pid_state_dev   DEVICE buffer [n_inst][nb][2] ([n_inst][joints][2] for a closed-loop mechanism, which has more joints than bodies;
 *                   integrated error, last error per joint, opaque order) that carries the PID
 *                   integrators of pid.jl:10-11 between launches: read when k0 > 1, always written; only used by controllers with
 *                   npid > 0.  NULL: they live for one launch;
 *   pid_state_len   doubles in that buffer (checked against n_inst * nb * 2, closed loops: n_inst * joints * 2);
 *   noise_ws_dev    DEVICE workspace of n_inst * steps doubles for the launch's Philox samples (noise_philox controllers without an
 *                   injected noise array).  NULL: the controller handle's own workspace is used -- ONE buffer per handle, so two
 *                   launches that share a controller on different streams or host threads must each bring their own here, and
 *                   the handle's buffer cannot grow while `stream` is being captured into a hipGraph (CCLQR_EINVAL: size it first
 *                   with cclqr_ctrl_reserve_noise).  Launches of at most CCLQR_PHILOX_INKERNEL_STEPS steps (the step-per-launch / hipGraph
 *                   form of BASELINE configs[4]) on forests of chains generate their samples INSIDE the rollout kernel and touch no
 *                   workspace at all;
 *   noise_ws_len    doubles in that workspace (checked against n_inst * steps);
 *   newton_mode     0 = the reference's stopping rule, ||f|| < eps AND ||step taken|| < eps (the PARITY mode).
 *                   1 = measured-error mode: a Newton solve ALSO stops as soon as ||f|| < newton_eps_alone, whatever the step size.
 *                   Saves the iterations the exact rule spends halving steps on round-off noise; the state deviation from mode 0
 *                   is reported, not promised.  Forests of chains and branching trees under the plain LQR / TrackingLQR
 *                   law (CCLQR_EUNSUPPORTED with the friction / noise / PID laws there), closed-loop mechanisms under every law;
 *   flags           CCLQR_ROLLOUT_NO_ALLOC: the call must neither allocate nor synchronise -- what a caller who is capturing ANY stream of the
 *                   device into a hipGraph needs (a hipMalloc / hipDeviceSynchronize during a global-mode capture invalidates it, whichever
 *                   stream it is issued on).  A launch that would have to grow the handle's Philox workspace is then refused with
 *                   CCLQR_EINVAL (the message names cclqr_ctrl_reserve_noise) before anything is touched, whether or not `stream` itself is
 *                   capturing; without the flag the library still refuses on a capturing `stream` (it can see that one) and grows otherwise;
 *                   CCLQR_ROLLOUT_PACK_WAVEFRONTS: forests of chains and branching trees: 64 / lanes-per-instance instances in every wavefront whatever the batch
 *                   size.  Without it a batch too small to give every SIMD a wavefront that way is spread over more wavefronts (the spare lane
 *                   groups take part in their neighbours' line searches: up to 20 % less time per step at a few hundred instances; a persistent
 *                   launch, steps >= 8, spreads over the whole device, a shorter one over a quarter of it) -- bitwise the same results.  Set it
 *                   when MANY launches share the device at once (more than four concurrent step-per-launch chains, several processes on one
 *                   GPU): spread launches then queue behind one another;
 *                   CCLQR_ROLLOUT_CARRY_STATUS: `status` is read as well as written -- it carries an instance's status ACROSS launches, for callers who
 *                   step a batch one launch (or a few steps) at a time (k0 continuation: the `controlfunction` loops, MPC, a hipGraph of step
 *                   launches).  Zero it before the first launch.  An instance that comes in lost (-CCLQR_NEWTON_MAXIT < status < 0: an earlier step ended on
 *                   a non-finite residual) is not stepped: it stays frozen at its last pose, at rest, as it would inside ONE launch over the whole
 *                   horizon, and keeps its status; for the others this launch's result is merged in (largest Newton count so far, negative once any
 *                   step failed).  A lost instance that had ALSO failed to converge earlier reports -(CCLQR_NEWTON_MAXIT - 1), so that "lost" stays
 *                   readable from the number.  Without the flag every launch reports on its own steps only and forgets what came before;
 *                   CCLQR_ROLLOUT_RUNTIME_PLAN: a mechanism that is ONE chain of 16 or 17 links (the N-link cartpole) runs on a kernel with the plan of its
 *                   block-tridiagonal solve compiled in; with this flag it runs on the general kernel of forests of chains instead, which reads the plan
 *                   at run time -- bitwise the same results, a few per cent slower.  For A/B measurements and tests; ignored by every other mechanism;
 *   newton_eps_alone  threshold of mode 1 (<= 0: 1e-10, the rule's own eps: stop on the residual alone). */
#define CCLQR_NEWTON_MAXIT 100        /* newton!'s iteration cap */
#define CCLQR_ROLLOUT_NO_ALLOC 1
#define CCLQR_ROLLOUT_PACK_WAVEFRONTS 2
#define CCLQR_ROLLOUT_CARRY_STATUS 4
#define CCLQR_ROLLOUT_RUNTIME_PLAN 16     /* (bit 8 stays unassigned and refused: tests/test_gpu_rollout.py uses it as its unknown bit) */
#define CCLQR_PHILOX_INKERNEL_STEPS 8
typedef struct {
    int64_t first_instance;
    double *pid_state_dev;
    int64_t pid_state_len;
    double *noise_ws_dev;
    int64_t noise_ws_len;
    int32_t newton_mode;
    int32_t flags;
    double newton_eps_alone;
} cclqr_rollout_opts;

/* cclqr_rollout_dev with explicit options (opts may be NULL = cclqr_rollout_dev). */
int cclqr_rollout_ex(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, const double *z0_dev,
                     double *lam_dev, const double *noise_dev, int64_t noise_stride, double *traj_dev, double *zT_dev,
                     int32_t *status_dev, const cclqr_rollout_opts *opts, void *stream);

/* Per-instance plants: the numbers that `Box(width, depth, length1, length1)` (examples/lqr_cartpole.jl:21-22: mass, inertia), `Prismatic(origin, cart, ey)` /
 * `Revolute(cart, pole, ex; p2=-p2)` (:25-26: the joint vertices p1, p2) and `Mechanism(origin, links, constraints; g, Δt)` (:32) fix for the ONE plant of a reference
 * run, here one set for every instance of a batch -- the Monte-Carlo robustness run "do these gains survive a plant that is 20 % heavier or 5 % longer" as one
 * launch.  The topology stays the mechanism's: joint types, axes, qoffset, Δt, g.
 *   mass [n_plant][nb], inertia [n_plant][nb][9] (body frame), p1, p2 [n_plant][ne][3], in the caller's body / joint order as in cclqr_mech_desc; any of them
 *   may be NULL = the mechanism's own value for every plant.  on_device = 0: HOST pointers; 1: DEVICE pointers, read on `stream` (a hipStream_t).  Either way the
 *   arrays are packed into link-order records and validated on the device, and the call returns when that is done (the arrays may be released then).
 *   first_index = global instance index of row 0: rank r of a sharded batch uploads its slice only (cclqr_rollout_opts.first_instance).
 * CCLQR_EUNSUPPORTED for a closed-loop mechanism; CCLQR_EINVAL naming the first offending (plant = row of the arrays, body) for a non-finite value, a mass <= 0 or
 * an inertia that is not symmetric positive definite.  The handle must not outlive the mechanism it was created for. */
int cclqr_plants_create(const cclqr_mech *m, int64_t n_plant, int64_t first_index, const double *mass, const double *inertia, const double *p1,
                        const double *p2, int32_t on_device, void *stream, cclqr_plants **out);
int cclqr_plants_destroy(cclqr_plants *p);

/* cclqr_rollout_ex on per-instance plants -- simulate!(mechanism_n, steps, controller) (examples/lqr_cartpole.jl:44) where mechanism_n is the `Mechanism(...)` of
 * examples/lqr_cartpole.jl:32 rebuilt with instance n's `Box(...)` / `Revolute(...; p1, p2)` numbers (:21-26).  Instance n of the launch runs plant
 * first_instance + n - first_index; a launch whose instances are not all inside the table is refused with CCLQR_EINVAL before anything is launched.  The plant set
 * is an argument of the launch: nothing of it is kept in the mechanism or controller handle.  plants == NULL: exactly cclqr_rollout_ex.  The states z0 must lie on
 * each instance's OWN plant's constraint manifold (its own joint vertices).  Forests of chains and branching trees, every control law. */
int cclqr_rollout_plants(const cclqr_mech *m, const cclqr_plants *plants, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, const double *z0_dev,
                         double *lam_dev, const double *noise_dev, int64_t noise_stride, double *traj_dev, double *zT_dev, int32_t *status_dev,
                         const cclqr_rollout_opts *opts, void *stream);

/* cclqr_linearize on per-instance plants -- linearsystem(mechanism_k, xd, vd, qd, ωd, Fτd, bodyids, eqcids) (src/control/lqr.jl:63) where mechanism_k is the
 * `Mechanism(...)` of examples/lqr_cartpole.jl:32 rebuilt with plant k's `Box(...)` / `Revolute(...; p1, p2)` numbers (:21-26).  Knot k is linearised on the plant
 * with GLOBAL index first_plant + k, i.e. row first_plant + k - first_index of the handle; the topology, Δt and g are the mechanism's.  zd[k] must lie on plant k's
 * own constraint manifold, Fd[k] is the caller's holding input for plant k.  Everything else as cclqr_linearize: host pointers, the caller's body / joint order.
 * plants == NULL: exactly cclqr_linearize.  CCLQR_EINVAL, before anything is launched, when the plants were created for another mechanism or the plants
 * first_plant .. first_plant + nk - 1 are not all in the table; CCLQR_EUNSUPPORTED for plants on a closed-loop mechanism. */
int cclqr_linearize_plants(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t nk, const double *zd, int32_t mu,
                           const int32_t *ctrl_joint, const double *Fd, double *A, double *Bu, double *Bl, double *G);

/* cclqr_ctrl_create_lqr_batch with one plant per controller table -- for every k, LQR(mechanism_k, bodyids, eqcids, Q, R, horizon; xd, vd, qd, ωd, Fτd)
 * (src/control/lqr.jl:49-66): linearsystem at lqr.jl:63 and dlqr at lqr.jl:141-184, evaluated on the `Mechanism(...)` of examples/lqr_cartpole.jl:32 rebuilt with plant
 * k's `Box(...)` / `Revolute(...; p1, p2)` numbers (:21-26).  Table k is designed on the plant with GLOBAL index first_plant + k (row first_plant + k - first_index of
 * the handle).  A rollout reads the controller table AND (cclqr_rollout_plants) the plant of an instance by its global index, cclqr_rollout_opts.first_instance + i:
 * with first_plant = 0 instance n runs on plant n under the gains designed for plant n.  (first_plant > 0 designs for a slice of a larger table; its tables are
 * still numbered from 0.)  kbreak, infinite_horizon, the per-table zero pad and
 * the error codes are cclqr_ctrl_create_lqr_batch's.  plants == NULL: exactly cclqr_ctrl_create_lqr_batch.  The refusals of cclqr_linearize_plants apply, before
 * anything is launched or allocated on the device. */
int cclqr_ctrl_create_lqr_batch_plants(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_ctrl, const double *zd, int32_t mu,
                                       const int32_t *ctrl_joint, const double *Fd, const double *Q, const double *R, int32_t N, int32_t infinite_horizon,
                                       double tol, int32_t *kbreak, cclqr_ctrl **out);

/* cclqr_ctrl_create_lqr_batch_plants with one pair of weights per controller table -- for every k, LQR(mechanism_k, bodyids, eqcids, Q_k, R_k, horizon; ...)
 * (src/control/lqr.jl:49-66): the last batch dimension of that constructor.  Q [n_weights][12 nb][12 nb], R [n_weights][mu][mu]: host pointers, block-diagonal in
 * the caller's body / constraint order and already Δt-scaled (lqr.jl:18-19), used as written.  n_weights is 1 (exactly cclqr_ctrl_create_lqr_batch_plants) or n_ctrl;
 * any other value is CCLQR_EINVAL before anything is allocated or launched.  Table k's gains are bitwise those of the shared-weights call on the same n_ctrl
 * setpoints (and plants) with (Q_k, R_k).  kbreak, infinite_horizon, the per-table zero pad, plants == NULL, the error codes and the refusals of
 * cclqr_linearize_plants as there.  Closed-loop mechanisms: CCLQR_EUNSUPPORTED.  A rollout reads table first_instance + i for instance i, so n_weights candidates
 * from one start state are one launch with that state replicated; cclqr_rollout_score then ranks them under ONE set of score weights, the common yardstick. */
int cclqr_ctrl_create_lqr_batch_weights(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_ctrl, const double *zd, int32_t mu,
                                        const int32_t *ctrl_joint, const double *Fd, int32_t n_weights, const double *Q, const double *R, int32_t N,
                                        int32_t infinite_horizon, double tol, int32_t *kbreak, cclqr_ctrl **out);

/* The cost-to-go of a controller's tables as a device object, and the cost it predicts (additive, still 202, no struct changed; looked up by name like the entries
 * above).  The reference's LQR(...) (src/control/lqr.jl:49-66) keeps the gains of dlqr (lqr.jl:141-184) and drops the Pkp1 of lqr.jl:170 they were derived from;
 * a cclqr_value holds it: n_tables matrices P [12 nb][12 nb] in the caller's body order, row-major, one shared by every instance (n_tables = 1) or one per
 * controller table. */
typedef struct cclqr_value cclqr_value;   /* opaque: device-resident cost-to-go tables */
/* cclqr_ctrl_create_lqr_batch_weights that also keeps every table's cost-to-go (lqr.jl:170; cclqr_riccati_value says which step's) on the device: *value receives
 * a cclqr_value of n_ctrl tables (8 (12 nb)^2 bytes each: 8192 tables of a 7-body arm are 462 MB).  value = NULL: nothing is kept or allocated -- that IS
 * cclqr_ctrl_create_lqr_batch_weights.  The controller's gains and kbreak are bitwise the same either way.  On an error neither handle is returned. */
int cclqr_ctrl_create_lqr_batch_value(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_ctrl, const double *zd, int32_t mu,
                                      const int32_t *ctrl_joint, const double *Fd, int32_t n_weights, const double *Q, const double *R, int32_t N,
                                      int32_t infinite_horizon, double tol, int32_t *kbreak, cclqr_ctrl **out, cclqr_value **value);
/* a cclqr_value from the caller's own matrices -- the P of cclqr_riccati_value on the models of cclqr_linearize (lqr.jl:63, 141-184), or any other quadratic form:
 * P_host [n_tables][12 nb][12 nb], used as written (symmetric or not).  cclqr_value_get reads table `table` back; CCLQR_EINVAL for n_tables < 1 or a table out of
 * range. */
int cclqr_value_create(const cclqr_mech *m, int64_t n_tables, const double *P_host, cclqr_value **out);
int cclqr_value_get(const cclqr_value *v, int64_t table, double *P_host);
int cclqr_value_destroy(cclqr_value *v);
/* out_dev[i] = dz_i' P_t dz_i, the cost the gains were designed to achieve from state i: dz_i is the error of control_lqr! (lqr.jl:92-103: per body x - xd, v - vd,
 * vec(qd \ q), ω - ωd) of the state at z_dev + i * z_stride ([nb][13], caller's body order; z_stride in doubles, >= 13 nb, so a caller can point into a recorded
 * slab at any step) about setpoint row 0 of controller table first_instance + i (table 0 when the controller has one), and t = first_instance + i when the value
 * holds several tables, 0 otherwise.  DEVICE pointers, asynchronous on `stream`.  An instance's result is the same bits whatever n_inst, first_instance or its place
 * in the batch; a NaN state gives NaN.  realised / predicted -- Jx + Ju of cclqr_rollout_score over this -- measures how far a start lies outside the linear regime.
 * CCLQR_EINVAL, before anything is launched: a value or controller made for another mechanism or device, n_tables neither 1 nor the controller's table count,
 * first_instance + n_inst beyond the tables, a controller without a setpoint table, z_stride < 13 nb.  Every topology cclqr_mech_create takes. */
int cclqr_value_eval(const cclqr_mech *m, const cclqr_ctrl *c, const cclqr_value *v, int64_t n_inst, int64_t first_instance, const double *z_dev,
                     int64_t z_stride, double *out_dev, void *stream);

/* Policy evaluation (additive, Still 202, no struct changed; looked up by name like the entries above): dlqr's cost recursion (src/control/lqr.jl:147-177) with the gains
 * GIVEN instead of solved for -- what a gain table costs on a model it was NOT designed on (the nominal controller on plant n), and whether that closed loop is stable
 * on the linear model.  Per problem p, with its model (A, Bu, Bλ, G)_p, its weights (Q, R)_p and the table K_t[k], k = 1 .. nK:
 *     Pk = Q                                                                          lqr.jl:147
 *     for k = N-1:-1:1                                                                lqr.jl:150
 *         Kuk  = K_t[k] (nK == N-1)  or  K_t[1] (nK == 1: a stationary gain)          in place of lqr.jl:160: the gain is given
 *         Kλk  = (G*Bλ) \ (G*(A - Bu*Kuk))                                            second block row of M*Kk = b, lqr.jl:154-160: independent of Pk
 *         Abar = A - Bu*Kuk - Bλ*Kλk                                                  lqr.jl:169
 *         Pkp1 = Q + Kuk'*R*Kuk + Abar'*Pk*Abar                                       lqr.jl:170
 *         norm(Pk - Pkp1) < tol -> break ; Pk = Pkp1                                  lqr.jl:172-176 (Frobenius)
 * P[p] is the last Pkp1 computed (of the step the test fired on, of step 1 when it never fired, Q when N = 1), kbreak[p] the loop index after the loop (the convention
 * of cclqr_riccati_value), dnorm[p][0..1] the norm(Pk - Pkp1) of the last executed step and of the step before it, NaN where no such step ran.  The evaluation
 * converged if and only if dnorm[p][0] < tol; a closed loop that is unstable on model p shows dnorm growing, and sqrt(dnorm[p][0] / dnorm[p][1]) estimates its
 * contraction (reported, not promised).  A recursion that does not converge is NOT an error: it is the answer.  Q and R are used as written, symmetric or not.  On a
 * table dlqr produced on the SAME model, weights and N with tol = 0 the result is the Riccati cost-to-go to rounding; on any other model it is not.
 * cclqr_policy_value -- HOST pointers, the caller's models (the sibling of cclqr_riccati_value): A [nprob][mx][mx], Bu [nprob][mx][mu], Bl [nprob][mx][ml],
 * G [nprob][ml][mx]; K [n_gains][nK][mu][mx] with n_gains = 1 (one table shared by all) or nprob, nK = 1 or N - 1 (K may be NULL when mu = 0 or N = 1);
 * Q [n_weights][mx][mx], R [n_weights][mu][mu] with n_weights = 1 or nprob; P [nprob][mx][mx]; kbreak [nprob] and dnorm [nprob][2] may be NULL.  opts: only `path`
 * is read (0 auto, 1 resident, 2 tiled, as cclqr_riccati_ex; a shape the resident kernel cannot hold runs tiled whatever it says); bf16_terms != 0 is CCLQR_EINVAL
 * (fp64 only).  Time-invariant models only.  Any other count or size is CCLQR_EINVAL before anything is allocated or launched, with the outputs untouched; a singular
 * G*Bλ is CCLQR_ESINGULAR, as in the Riccati. */
int cclqr_policy_value(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                       int32_t n_gains, int32_t nK, const double *K, int32_t n_weights, const double *Q, const double *R, int32_t N, double tol,
                       double *P, int32_t *kbreak, double *dnorm, const cclqr_riccati_opts *opts);
/* cclqr_value_create_policy -- the same recursion (lqr.jl:147-177 with lqr.jl:160 given) for a CONTROLLER on a mechanism's plants (Still 202): linearsystem (lqr.jl:63)
 * at the n_models setpoints zd [n_models][nb][13] (caller's body order, Fd [n_models][mu] or NULL = 0, HOST pointers), setpoint k on the plant with global index
 * first_plant + k exactly as cclqr_ctrl_create_lqr_batch_plants linearises it (plants == NULL: the mechanism's own plant); the gains of controller c gathered on the
 * device into the caller's body order -- one table shared by all models, or table k for model k; they never visit the host --; the recursion with Q [n_weights][12 nb][12 nb],
 * R [n_weights][mu][mu] (n_weights = 1 or n_models, already Δt-scaled, HOST pointers).  *out: a cclqr_value of n_models tables in the caller's body order, for
 * cclqr_value_eval and cclqr_value_get as it stands.  kbreak [n_models], dnorm [n_models][2]: HOST, or NULL.  The horizon: a controller with ONE gain row
 * (LQR{T,Inf}, lqr.jl:40-43) is stationary and N is the caller's; one with nK > 1 rows requires N == nK + 1.
 * Refused before any launch or allocation: mu / ctrl_joint that are not the controller's, a controller without gains, one made for another mechanism or device, a
 * table count that is neither 1 nor n_models (CCLQR_EINVAL); a controller with more than one setpoint row per table (tracking) and closed-loop mechanisms
 * (CCLQR_EUNSUPPORTED); the refusals of cclqr_linearize_plants.  During the run CCLQR_ENOCONV names the setpoint whose Newton solve failed, CCLQR_ESINGULAR the model. */
int cclqr_value_create_policy(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_models, const double *zd, int32_t mu,
                              const int32_t *ctrl_joint, const double *Fd, const cclqr_ctrl *c, int32_t n_weights, const double *Q, const double *R, int32_t N,
                              double tol, int32_t *kbreak, double *dnorm, cclqr_value **out);

/* Policy evaluation of a STATIONARY gain by doubling (additive, Still 202, no struct changed; looked up by name).  The reference's default controller LQR{T,Inf} keeps
 * one gain (src/control/lqr.jl:40-43); with it the recursion above has a constant Abar = A - Bu*K - Bλ*Kλ (lqr.jl:169) and Qbar = Q + K'*R*K (lqr.jl:170), and with
 *     S(n) = sum_{i<n} (Abar^i)' Qbar Abar^i,  M(n) = Abar^n:     S(a+b) = S(a) + M(a)' S(b) M(a),  M(a+b) = M(a) M(b),     P = S(n) + M(n)' Q M(n)
 * gives the cost-to-go after n backward steps in at most 2 log2(n) combinations instead of n steps.  K [n_gains][mu][mx], Q and R used as written, symmetric or not.
 *   N >= 1  fixed horizon: n = N - 1 steps exactly, square-and-multiply over the bits of n (least significant first).  P is what cclqr_policy_value returns for nK = 1,
 *           tol = 0 and the same N, to rounding; no break test and no growth stop (tol and max_levels are not read).  levels = the doublings made, reason = 0,
 *           dnorm = NaN, gnorm[p][0] = norm(M(n)), gnorm[p][1] = NaN
 *   N == 0  to convergence: level j = 1, 2, .. doubles to 2^j steps; its increment norm(S(2^j) - S(2^(j-1))) comes out of the doubling.  Stop after level j, in this
 *           order: reason 0 the increment < tol; reason 2 norm(M(2^j)) > 1e50 (one more level could overflow: the closed loop is unstable on the model); reason 1
 *           j == max_levels (1 .. 60).  levels = j; dnorm[p][0..1] the increment norms and gnorm[p][0..1] norm(M) of the last level and of the one before, NaN where
 *           no such level ran.  (gnorm0 / gnorm1)^(1 / 2^(levels-1)) estimates the closed loop's spectral radius (reported, not promised).  All norms Frobenius.
 * A run that does not converge is NOT an error: reason is the answer.  Results do not depend on the batch a problem is in, nor on whether gains / weights are shared.
 * cclqr_policy_value_doubling -- HOST pointers, laid out as for cclqr_policy_value; n_gains and n_weights = 1 or nprob; levels, reason [nprob] and dnorm, gnorm
 * [nprob][2] may be NULL.  opts: as in cclqr_policy_value (only `path`; bf16_terms != 0 is CCLQR_EINVAL).  CCLQR_EINVAL before anything is allocated or launched, with
 * the outputs untouched: N < 0, max_levels outside 1..60 when N == 0, tol < 0 or NaN, any other count or size.  A singular G*Bλ is CCLQR_ESINGULAR. */
int cclqr_policy_value_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                                int32_t n_gains, const double *K, int32_t n_weights, const double *Q, const double *R, int32_t N, double tol, int32_t max_levels,
                                double *P, int32_t *levels, int32_t *reason, double *dnorm, double *gnorm, const cclqr_riccati_opts *opts);
/* cclqr_value_create_policy_doubling -- the same evaluation (lqr.jl:169-170 with the one gain of lqr.jl:40-43) for a CONTROLLER on a mechanism's plants (Still 202): the
 * linearisation and the device-side gather of the gains are those of cclqr_value_create_policy (the gains never visit the host); *out is a cclqr_value of n_models
 * tables for cclqr_value_eval / cclqr_value_get as it stands.  levels, reason [n_models], dnorm, gnorm [n_models][2]: HOST, or NULL.  Refused as there, and besides:
 * a controller whose tables hold more than one gain row (a finite-horizon table is what cclqr_value_create_policy steps through) is CCLQR_EINVAL. */
int cclqr_value_create_policy_doubling(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_models, const double *zd, int32_t mu,
                                       const int32_t *ctrl_joint, const double *Fd, const cclqr_ctrl *c, int32_t n_weights, const double *Q, const double *R,
                                       int32_t N, double tol, int32_t max_levels, int32_t *levels, int32_t *reason, double *dnorm, double *gnorm, cclqr_value **out);

/* Closed-loop state covariance under input noise, by doubling (additive, Still 202, no struct changed; looked up by name).  The reference's flagship example drives the
 * cart with randn()*2 (examples/trackingLQR_triple_cartpole.jl:98); the rollout adds one such sample to every controlled input.  With the one gain of LQR{T,Inf}
 * (src/control/lqr.jl:40-43) the closed loop on the linear model is Δz⁺ = Abar Δz + D w, Abar = A - Bu*K - Bλ*Kλ = A' - D K (lqr.jl:169-170; [A' | D] the projected
 * model), w ~ (0, Wu) in input space, and after n steps from a start of covariance Sigma0
 *     Σ_n = C(n) + M(n) Σ0 M(n)',  C(n) = sum_{i<n} Abar^i W (Abar^i)',  W = D Wu D',  M(n) = Abar^n:     C(a+b) = C(a) + M(a) C(b) M(a)',  M(a+b) = M(a) M(b)
 * -- the pair recursion of cclqr_policy_value_doubling on (Abar', W) with Σ0 as the terminal matrix, run by the same kernels.  It runs on W / w and Σ0 / w with
 * w = 2^floor(log2 tr W) per problem (exact; 1 when tr W is 0 or mu = 0): tol is RELATIVE to the noise, and 4 Wu gives exactly 4 Σ.
 *   N >= 1  exactly N - 1 steps; no test.  levels = the doublings made, reason = 0, dnorm = NaN, gnorm[p][0] = norm(M(n)), gnorm[p][1] = NaN.  N = 1: Σ = Sigma0
 *   N == 0  to convergence, the steady state: level j stops, in this order, on reason 0 norm(C(2^j) - C(2^(j-1))) / w < tol; reason 2 norm(M(2^j)) > 1e50; reason 1
 *           j == max_levels (1 .. 60).  Sigma0 must be NULL.  dnorm[p][0..1] are reported in Σ's units (not divided by w), gnorm[p][0..1] as above.
 * Moments, each written only if its pointer is not NULL: cost[p][0] = tr(Q Σ) and cost[p][1] = tr(R K Σ K'), the expected stage costs E[cx], E[cu] per step at Σ;
 * zstd[p][i] = sqrt(max(Σ_ii, 0)); ustd[p][j] = sqrt(max((K Σ K')_jj, 0)).  Wu, Sigma0, Q, R are used as written: a matrix that is not symmetric positive
 * semidefinite is the caller's business.  Results do not depend on the batch a problem is in, nor on whether gains / weights / noise are shared.
 * cclqr_covariance_doubling -- HOST pointers; models, K, n_gains, n_weights, levels .. gnorm, opts as for cclqr_policy_value_doubling; Wu [n_noise][mu][mu] and Sigma0
 * [n_noise][mx][mx] with n_noise = 1 or nprob, either NULL (= 0) but not both; Q, R may be NULL when cost is; Sigma [nprob][mx][mx], cost [nprob][2], zstd [nprob][mx],
 * ustd [nprob][mu].  CCLQR_EINVAL before anything is allocated or launched, with the outputs untouched: what cclqr_policy_value_doubling refuses, n_noise neither 1 nor
 * nprob, Wu and Sigma0 both NULL, cost without Q / R, Wu with mu == 0, Sigma0 with N == 0.  A singular G*Bλ is CCLQR_ESINGULAR (N = 1 reaches no model and cannot be):
 * that problem gets no moments and its Sigma is unspecified, as P is there. */
int cclqr_covariance_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                              int32_t n_gains, const double *K, int32_t n_weights, const double *Q, const double *R, int32_t n_noise, const double *Wu,
                              const double *Sigma0, int32_t N, double tol, int32_t max_levels, double *Sigma, double *cost, double *zstd, double *ustd,
                              int32_t *levels, int32_t *reason, double *dnorm, double *gnorm, const cclqr_riccati_opts *opts);
/* cclqr_value_create_covariance_doubling -- the same covariance (lqr.jl:169-170 with the one gain of lqr.jl:40-43) for a CONTROLLER on a mechanism's plants (Still 202):
 * linearisation, gain gather and refusals are those of cclqr_value_create_policy_doubling (tracking controllers and closed loops: CCLQR_EUNSUPPORTED; more than one gain
 * row: CCLQR_EINVAL), and besides the refusals above.  Q, Sigma0, zstd and the tables of *out are in the order in which cclqr_value_create_policy_doubling takes Q and
 * returns P.  *out is a cclqr_value of n_models tables holding Σ: cclqr_value_get reads a table back (a covariance is not a cost-to-go: cclqr_value_eval of it means
 * nothing). */
int cclqr_value_create_covariance_doubling(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_models, const double *zd, int32_t mu,
                                           const int32_t *ctrl_joint, const double *Fd, const cclqr_ctrl *c, int32_t n_weights, const double *Q, const double *R,
                                           int32_t n_noise, const double *Wu, const double *Sigma0, int32_t N, double tol, int32_t max_levels, double *cost,
                                           double *zstd, double *ustd, int32_t *levels, int32_t *reason, double *dnorm, double *gnorm, cclqr_value **out);

/* The state covariance of a TRACKED run under input noise, knot by knot (additive, Still 202, no struct changed; looked up by name).  The reference's flagship example
 * drives the cart with randn()*2 (examples/trackingLQR_triple_cartpole.jl:98) under a TrackingLQR: the law applies gain row Ku[k] while k < N
 * (src/control/lqr_tracking.jl:63, 65), designed on the model linearised at knot k (lqr_tracking.jl:88-89).  Knots are j = 0 .. N-1, knot j being the state the law sees
 * at step j + 1 -- the indexing of cclqr_rollout_score and of a recorded rollout passed in as zd.  With [A'_j | D_j] the projected pair of knot j (lqr_tracking.jl:88)
 * and K_j its gain row:
 *     Abar_j  = A'_j - D_j K_j                       (lqr_tracking.jl:107)
 *     Σ_0     = Sigma0 (or 0)
 *     Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j'     j = 0 .. N-2
 *     cx_j = tr(Q Σ_j)                j = 0 .. N-1
 *     cu_j = tr(R K_j Σ_j K_j')       j = 0 .. N-2,  cu_{N-1} = 0
 *     zstd_j = sqrt(max(diag Σ_j, 0))
 *     ustd_j = sqrt(max(diag K_j Σ_j K_j', 0)),      ustd_{N-1} = 0
 *     total  = (sum_j cx_j, sum_j cu_j), summed in knot order = E[Jx], E[Ju] of simulate(..., steps = N, score = Score(...))
 * Σ is a second moment: a rank-one Sigma0 = δδ' with Wu = 0 is the deterministic perturbed start.  Wu, Sigma0, Q, R are used as written: nothing assumes symmetry.
 * N = 1: Σ = Sigma0, and no model is read.  One sequential recursion on the device, two mx^3 products per step on the fp64 matrix pipe.
 * cclqr_covariance_tracking -- HOST pointers, caller models: A [nprob][nlin][mx][mx], Bu [nprob][nlin][mx][mu], Bl [nprob][nlin][mx][ml], G [nprob][nlin][ml][mx] with
 * nlin = 1 (one time-invariant model) or N - 1 (model j = knot j); K [n_gains][nK][mu][mx] with n_gains = 1 or nprob and nK = 1 (a stationary gain) or N - 1 (row j = knot
 * j); Q [n_weights][mx][mx], R [n_weights][mu][mu] with n_weights = 1 or nprob, both may be NULL when cost and total are; Wu [n_noise][mu][mu], Sigma0 [n_noise][mx][mx]
 * with n_noise = 1 or nprob, either NULL (= 0) but not both.  Outputs, each written only if not NULL: Sigma [nprob][mx][mx] = Σ_{N-1}; Sigma_all [nprob][N][mx][mx];
 * cost [nprob][N][2] = (cx_j, cu_j); zstd [nprob][N][mx]; ustd [nprob][N][mu]; total [nprob][2].  opts: only `path` is read (0 / 1: one workgroup per problem where the shape
 * fits -- mx a multiple of 4 up to 96 --, 2: every step as device-wide launches, which every other shape takes anyway); bf16_terms != 0 is CCLQR_EINVAL.
 * Results do not depend on the batch a problem is in, nor on whether gains / weights / noise are shared, nor on which outputs are asked for.
 * CCLQR_EINVAL before anything is allocated or launched, with the outputs untouched: sizes below 1 (mu, ml below 0), nlin neither 1 nor N - 1, n_gains / n_weights / n_noise
 * neither 1 nor nprob, nK neither 1 nor N - 1, Wu and Sigma0 both NULL, Wu with mu == 0, cost or total without Q / R, more than 65535 problems, path outside 0 .. 2.
 * A singular G*Bλ at a knot the recursion reaches is CCLQR_ESINGULAR, naming problem and knot; the outputs are filled for the problems before it. */
int cclqr_covariance_tracking(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, int32_t nlin, const double *A, const double *Bu, const double *Bl, const double *G,
                              int32_t n_gains, int32_t nK, const double *K, int32_t n_weights, const double *Q, const double *R, int32_t n_noise, const double *Wu,
                              const double *Sigma0, int32_t N, double *Sigma, double *Sigma_all, double *cost, double *zstd, double *ustd, double *total,
                              const cclqr_riccati_opts *opts);

/* cclqr_value_create_covariance_tracking -- the same recursion (lqr_tracking.jl:63, 88, 107 under the noise of trackingLQR_triple_cartpole.jl:98) for a CONTROLLER on a
 * mechanism's plants (Still 202).  zd [n_models][N][nb][13] and Fd [n_models][N][mu] (or NULL) as cclqr_ctrl_create_tracking_batch_plants takes them: host arrays
 * (on_device = 0), or device arrays read in place on `stream` (on_device = 1) -- a recorded traj_dev passes straight in.  linearsystem runs at the knots 0 .. N-2 of
 * trajectory k on plant first_plant + k (plants NULL: the mechanism's own); the gains of c are gathered on the device into the models' body order and never visit the
 * host.  c holds N - 1 gain rows or one, and one table or n_models.  The problems run in chunks whose models, recursion workspace and per-knot records stay within
 * workspace_bytes (<= 0: the library default of 4 GiB); the result does not depend on the chunking.  The budget covers what grows with the chunk and the weights and noise;
 * NOT counted in it: the device copy of host trajectories (n_models N (13 nb + mu) doubles), the gathered gain rows of the controller's tables and the tables of *out.  Q, Sigma0, zstd and the tables of *out are in the order in which
 * cclqr_value_create_policy takes Q and returns P.  *out is a cclqr_value of n_models tables holding Σ_{N-1}: cclqr_value_get reads a table back (a covariance is not a
 * cost-to-go: cclqr_value_eval of it means nothing).  The per-knot moments go to the HOST arrays cost [n_models][N][2], zstd [n_models][N][12 nb], ustd [n_models][N][mu],
 * total [n_models][2], each written only if not NULL; Q, R may be NULL when cost and total are.
 * Refused before anything is allocated or launched, outputs and *out untouched: what cclqr_linearize_plants refuses; a controller without gains, or for another mechanism,
 * device or set of joints; a table count other than 1 or n_models, a row count other than 1 or N - 1, the counts and the noise as for cclqr_covariance_tracking, a
 * workspace that does not hold one problem (the message names the bytes it needs) -- CCLQR_EINVAL; closed-loop mechanisms -- CCLQR_EUNSUPPORTED.  During the run a
 * setpoint solve that does not converge is CCLQR_ENOCONV and a singular G*Bλ CCLQR_ESINGULAR, both naming table and knot. */
int cclqr_value_create_covariance_tracking(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_models, int32_t N, const double *zd,
                                           const double *Fd, int32_t on_device, int32_t mu, const int32_t *ctrl_joint, const cclqr_ctrl *c, int32_t n_weights,
                                           const double *Q, const double *R, int32_t n_noise, const double *Wu, const double *Sigma0, int64_t workspace_bytes,
                                           double *cost, double *zstd, double *ustd, double *total, void *stream, cclqr_value **out);

/* The cost-to-go of a TRACKED run at every knot, and the price of its noise (additive, Still 202, no struct changed; looked up by name): the adjoint of the tracking
 * covariance above.  With the knots, the gain rows (lqr_tracking.jl:63-65), the models (lqr_tracking.jl:88-89) and Abar_j = A'_j - D_j K_j (lqr_tracking.jl:107) as
 * there, the recursion is the Pkp1 of lqr_tracking.jl:108 with the gain of line 98 GIVEN instead of solved for:
 *     P_{N-1} = Q
 *     P_j     = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j      j = N-2 .. 0
 *     price_j = tr(Wu D_j' P_{j+1} D_j)                      j = 0 .. N-2,  price_{N-1} = 0
 * Δz' P_j Δz is what the rest of the tracked run costs from a deviation Δz at knot j; price_j is what the noise sample w ~ (0, Wu) injected at step j + 1
 * (examples/trackingLQR_triple_cartpole.jl:98) adds to it in expectation.  With Σ_0 and total of cclqr_covariance_tracking on the same arrays:
 *     total[0] + total[1] = tr(P_0 Σ_0) + sum_j price_j.
 * Q, R, Wu are used as written: nothing assumes symmetry.  N = 1: P = Q, and no model is read.  One sequential recursion on the device, two mx^3 products per step on
 * the fp64 matrix pipe.
 * cclqr_policy_value_tracking -- HOST pointers, caller models: A, Bu, Bl, G, nlin, K, n_gains, nK, Q, R, n_weights exactly as cclqr_covariance_tracking takes them (Q and R
 * are required here); Wu [n_noise][mu][mu] with n_noise = 1 or nprob, or NULL: then price and noise_total must be NULL.  Outputs, each written only if not NULL:
 * P [nprob][mx][mx] = P_0; P_all [nprob][N][mx][mx]; price [nprob][N]; noise_total [nprob] = the prices summed in the order the recursion produces them, j = N-2 down to
 * 0.  opts: only `path` is read (0 / 1: one workgroup per problem where the shape fits -- the shapes of cclqr_covariance_tracking --, 2: every step as device-wide
 * launches); bf16_terms != 0 is CCLQR_EINVAL.  Results do not depend on the batch a problem is in, nor on whether gains / weights / noise are shared, nor on which
 * outputs are asked for.
 * CCLQR_EINVAL before anything is allocated or launched, with the outputs untouched: sizes below 1 (mu, ml below 0), nlin neither 1 nor N - 1, n_gains / n_weights / n_noise
 * neither 1 nor nprob, nK neither 1 nor N - 1, Wu with mu == 0, price or noise_total without Wu, Q / R NULL, more than 65535 problems, path outside 0 .. 2.
 * A singular G*Bλ at a knot the recursion reaches is CCLQR_ESINGULAR, naming problem and knot; the outputs are filled for the problems before it. */
int cclqr_policy_value_tracking(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, int32_t nlin, const double *A, const double *Bu, const double *Bl, const double *G,
                                int32_t n_gains, int32_t nK, const double *K, int32_t n_weights, const double *Q, const double *R, int32_t n_noise, const double *Wu,
                                int32_t N, double *P, double *P_all, double *price, double *noise_total, const cclqr_riccati_opts *opts);

/* cclqr_value_create_policy_tracking -- the same recursion (lqr_tracking.jl:63, 88, 107, 108 under the noise of trackingLQR_triple_cartpole.jl:98) for a CONTROLLER on a
 * mechanism's plants (Still 202), by the host sequence of cclqr_value_create_covariance_tracking: the same trajectories zd / Fd (host, or device arrays read in place on
 * `stream`), plants, gain gather, chunking within workspace_bytes (the prices are counted per problem, the weights and Wu once), refusals and error naming.  The
 * recursion runs from knot N - 1 down to `knot` in [0, N-1]: *out is a cclqr_value of n_models tables holding P_knot, in the order in which cclqr_value_create_policy
 * takes Q and returns P, for cclqr_value_get and cclqr_value_eval as they stand -- the terminal weight of a receding-horizon caller at that knot, and with knot = 0 the
 * expected cost of the whole tracked run from a perturbed start.  price [n_models][N] (zeros below `knot` and at N - 1) and noise_total [n_models] (the prices of the
 * knots j >= knot, summed from N - 2 downwards) are HOST arrays, each written only if not NULL; both must be NULL when Wu is.  linearsystem runs at ALL knots 0 .. N-2
 * whatever `knot`; a singular G*Bλ below `knot` is not reached and is no error.
 * Refused as cclqr_value_create_covariance_tracking refuses, and: Q / R NULL, price or noise_total without Wu, knot outside 0 .. N-1 -- CCLQR_EINVAL. */
int cclqr_value_create_policy_tracking(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_models, int32_t N, const double *zd, const double *Fd,
                                       int32_t on_device, int32_t mu, const int32_t *ctrl_joint, const cclqr_ctrl *c, int32_t n_weights, const double *Q, const double *R,
                                       int32_t n_noise, const double *Wu, int32_t knot, int64_t workspace_bytes, double *price, double *noise_total, void *stream,
                                       cclqr_value **out);

/* The stationary LQR gain by doubling the Riccati map (additive, Still 202, no struct changed; looked up by name).  LQR{T,Inf} steps dlqr Ntemp = 10 s / Δt times and
 * keeps Ku[1] (src/control/lqr.jl:25-27, 39-43), converged or not.  In projected form a backward step of dlqr (lqr.jl:141-184, its step lqr.jl:151-170) is
 *     Ku = (R + D'PD)^-1 D'P A',    Pkp1 = Q + A'' P (I + G0 P)^-1 A'    with G0 = D R^-1 D'
 * and n steps are the triple (A_n, G_n, H_n) of the map X -> H_n + A_n' X (I + G_n X)^-1 A_n, H_n = the recursion's Pk after n - 1 steps.  One step is (A', G0, Q), and
 * triple 1 applied after triple 2 is     W = (I + G1 H2)^-1,  A = A2 W A1,  G = G2 + A2 W G1 A2',  H = H1 + A1' H2 W A1
 * (one partially pivoted solve and five products), so n steps cost at most 2 log2(n) compositions.  The final step is taken in the recursion's own form on X = H_n.
 * Q and R must be EXACTLY symmetric: the composition does not hold otherwise.
 *   N >= 2  fixed horizon: n = N - 1 single-step triples, square-and-multiply over the bits of n (least significant first).  K is Ku[1] of dlqr(.., N) with tol = 0 and P
 *           its last Pkp1: what cclqr_riccati_value(N, tol = 0, keep_last) returns, to rounding.  No stop test (tol and max_levels are not read).  levels = the
 *           doublings made, reason = 0, dnorm = NaN, anorm[p][0] = norm(A_n), anorm[p][1] = NaN
 *   N == 0  to convergence: level j = 1, 2, .. doubles to 2^j triples; the increment norm(H(2^j) - H(2^(j-1))) comes out of the composition.  Stop after level j, in this
 *           order: reason 0 the increment < tol; reason 2 norm(A(2^j)) > 1e50 or a norm of the level that is not finite (the model is not stabilisable: one more level
 *           could overflow); reason 3 an exactly zero or non-finite pivot of I + G1 H2 (the triple of the level before is kept); reason 1 j == max_levels (1 .. 60).
 *           The result equals the fixed horizon N = 2^levels + 1.  dnorm[p][0..1] the increment norms and anorm[p][0..1] norm(A) of the last level and of the one
 *           before, NaN where no such level ran.  All norms Frobenius.
 * A problem that ends with reason 1, 2 or 3 is NOT an error of the call: its gain is still written, finite or not, and reason is the answer.  Results do not depend on
 * the batch a problem is in, nor on whether the weights are shared.
 * cclqr_riccati_doubling -- HOST pointers, laid out as for cclqr_riccati_value: K [nprob][mu][mx]; P [nprob][mx][mx] or NULL; n_weights = 1 or nprob; levels, reason
 * [nprob] and dnorm, anorm [nprob][2] may be NULL.  opts: only bf16_terms is looked at, and bf16_terms != 0 is CCLQR_EINVAL.  CCLQR_EINVAL before anything is allocated
 * or launched, with the outputs untouched: N == 1 or N < 0, max_levels outside 1..60 when N == 0, tol < 0 or NaN, n_weights neither 1 nor nprob, a Q or R that is not
 * exactly symmetric, any other bad size (among them an mx or mu whose panels the kernels' LDS does not hold: mx beyond 12 800, mu * mx beyond about 9 600).  A
 * singular G*Bλ is CCLQR_ESINGULAR. */
int cclqr_riccati_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double *A, const double *Bu, const double *Bl, const double *G,
                           int32_t n_weights, const double *Q, const double *R, int32_t N, double tol, int32_t max_levels, double *K, double *P,
                           int32_t *levels, int32_t *reason, double *dnorm, double *anorm, const cclqr_riccati_opts *opts);
/* cclqr_ctrl_create_lqr_batch_doubling -- LQR{T,Inf} (lqr.jl:25-27, 39-43) for n_ctrl setpoints / plants / weight pairs with the gain by the doubling above (Still 202):
 * cclqr_ctrl_create_lqr_batch_value with infinite_horizon = 1 and the doubling in place of the stepped recursion -- the same checks, the same linearisation on the
 * plants, one gain row per table, the same link order and pad; the gains and P never visit the host.  N, tol, max_levels as above; levels, reason [n_ctrl], dnorm, anorm
 * [n_ctrl][2]: HOST, or NULL; value NULL: no P is kept.  Refused as there (closed-loop mechanisms: CCLQR_EUNSUPPORTED) and as above; a setpoint whose Newton solve or
 * G*Bλ fails is CCLQR_ENOCONV / CCLQR_ESINGULAR. */
int cclqr_ctrl_create_lqr_batch_doubling(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_ctrl, const double *zd, int32_t mu,
                                         const int32_t *ctrl_joint, const double *Fd, int32_t n_weights, const double *Q, const double *R, int32_t N, double tol,
                                         int32_t max_levels, int32_t *levels, int32_t *reason, double *dnorm, double *anorm, cclqr_ctrl **out, cclqr_value **value);

/* One TrackingLQR per plant and / or per reference trajectory, in one call -- for every k, TrackingLQR(mechanism_k, storage_k, Fτ_k, eqcids, Q, R)
 * (src/control/lqr_tracking.jl:17-43): linearsystem at the knots 1 .. N-1 of trajectory k (lqr_tracking.jl:88) and the recursion of lqr_tracking.jl:73-122 with its own
 * break and back-fill per problem, evaluated on the `Mechanism(...)` rebuilt with plant k's numbers as for cclqr_linearize_plants -- the question of
 * examples/trackingLQR_triple_cartpole.jl:93-125 ("does the tracking controller still swing the perturbed plant up") asked with the controller DESIGNED for each plant.
 * Table k is designed on the plant with GLOBAL index first_plant + k (row first_plant + k - first_index of the handle); plants == NULL: n_ctrl distinct reference
 * trajectories on the mechanism's own plant.
 *   zd [n_ctrl][N][nb][13] in the caller's body order, each trajectory on its own plant's constraint manifold; Fd [n_ctrl][N][mu] or NULL = 0.  on_device = 0: HOST
 *   pointers; 1: DEVICE pointers read on `stream` (a hipStream_t) -- the traj_dev of a recorded cclqr_rollout_plants with steps = N has exactly zd's layout and can be
 *   passed straight in.  Q [mx][mx], R [mu][mu] already Δt-scaled (lqr_tracking.jl:22-23), host pointers; kbreak [n_ctrl] (host) or NULL.
 *   law: NULL = the plain tracking law; else ONLY fric, noise_scale, noise_philox and noise_seed are read (the friction / noise law of
 *   examples/trackingLQR_triple_cartpole.jl:93-111, as cclqr_ctrl_create takes it).
 *   workspace_bytes: upper bound of the call's device workspace (the per-knot models, [A'|D] and the recursion's scratch: about 64 KB per knot of a triple cartpole);
 *   <= 0: 4 GiB.  The problems run in as many chunks as that takes, and the result does not depend on the chunking; CCLQR_EINVAL, naming the bytes one problem needs,
 *   when not even one fits.
 * The result is a controller of n_ctrl tables for cclqr_rollout* (instance n reads table first_instance + n): K [n_ctrl][N-1][mu][12 nb], zd [n_ctrl][N], Fd [n_ctrl][N],
 * every table with the zero pad of cclqr_ctrl_create_lqr_batch; the gains never visit the host (cclqr_ctrl_get_gains reads a table back).  The call returns when the
 * controller is complete.  The refusals of cclqr_linearize_plants apply before anything is launched or allocated; CCLQR_ENOCONV names the table and the knot whose
 * Newton solve failed, CCLQR_ESINGULAR the table; tree mechanisms (CCLQR_EUNSUPPORTED for closed loops). */
int cclqr_ctrl_create_tracking_batch_plants(const cclqr_mech *m, const cclqr_plants *plants, int64_t first_plant, int32_t n_ctrl, int32_t N, const double *zd,
                                            const double *Fd, int32_t on_device, int32_t mu, const int32_t *ctrl_joint, const double *Q, const double *R, double tol,
                                            const cclqr_ctrl_desc *law, int64_t workspace_bytes, int32_t *kbreak, void *stream, cclqr_ctrl **out);

/* lqr.K[k][i] (src/control/lqr.jl:4, lqr_tracking.jl:4) of one table of a controller, read back from the device: K_host [nK][mu][12 nb] in the caller's body order,
 * table in [0, n_ctrl).  For any controller that has gains, however it was built.  CCLQR_EINVAL for a table out of range or a controller without gains. */
int cclqr_ctrl_get_gains(const cclqr_mech *m, const cclqr_ctrl *c, int64_t table, double *K_host);

/* Scoring a rollout on the device (additive, still 202, no struct changed; looked up by name like the entries above).  The reference ranks a run by the
 * quadratic cost its gains were designed to minimise -- the weights Q, R handed to LQR(...) and scaled by Δt at src/control/lqr.jl:18-19, on the error
 * Δz of control_lqr! (lqr.jl:92-103: per body x - xd, v - vd, vec(qd \ q), ω - ωd) and the feedback command Δu = -K[k] Δz of lqr.jl:106-111 -- but has no
 * function that evaluates it: a user reads it off the recorded Storage (lqr_tracking.jl:32-35).  Here it is a reduction over the slab a rollout launch
 * has just written: score[i] = { Jx = sum_k cx_k, Ju = sum_k cu_k, peak = max_k cx_k, last_out = the largest k with cx_k > settle_tol (0: none) } with
 * cx_k = sum_b Δz_b' Qb[b] Δz_b and cu_k = Δu_k' R Δu_k; friction, noise and PID terms are plant and disturbance, not part of Δu.  A non-finite cx_k makes
 * Jx and peak NaN and sets last_out = k.
 * cclqr_score_create -- the weights of LQR(mechanism, bodyids, eqcids, Q, R, horizon) (lqr.jl:49-66) as a device object: Qb [nb][12][12] per-body blocks in the
 * caller's body order, used as written (symmetric or not), R [mu][mu], both already Δt-scaled (lqr.jl:18-19); HOST pointers.  CCLQR_EINVAL for a
 * non-finite weight or settle_tol. */
typedef struct cclqr_score cclqr_score;   /* opaque: device-resident weights */
#define CCLQR_SCORE_LEN 4
int cclqr_score_create(const cclqr_mech *m, const double *Qb, int32_t mu, const double *R, double settle_tol, cclqr_score **out);
int cclqr_score_destroy(cclqr_score *s);
/* cclqr_rollout_score -- the cost of simulate!(mechanism, steps, controller; record = true) (examples/lqr_cartpole.jl:44) under control_lqr! (lqr.jl:89-139) /
 * control_trackinglqr! (lqr_tracking.jl:46-71): instance i (global index first_instance + i: its controller table when the controller has several), steps
 * k = k0 .. k0 + steps - 1 (1-based), traj_dev [n_inst][steps][nb][13] as cclqr_rollout_* wrote it (the state the law saw at step k), setpoint row
 * min(k, nsp) - 1, gain min(k, nK) - 1 gated by k < N (N <= 0: gain 0, always).  DEVICE pointers, asynchronous on `stream`.  score_dev [n_inst][CCLQR_SCORE_LEN]
 * is read when k0 > 1 and always written, and an instance's steps are accumulated in step order: a horizon scored chunk by chunk (the k0 continuation of
 * cclqr_rollout_ex into one small slab) gives bitwise the score of one call.  A lost instance is scored on its frozen pose: read `status`.
 * CCLQR_EINVAL, before anything is launched: mu differs from the controller's, the controller has no setpoint table, first_instance + n_inst > n_ctrl for a
 * controller with several tables, steps < 1 or k0 < 1, a handle made for another mechanism or device.  Every topology cclqr_mech_create takes. */
int cclqr_rollout_score(const cclqr_mech *m, const cclqr_ctrl *c, const cclqr_score *s, int64_t n_inst, int32_t steps, int32_t k0,
                        int64_t first_instance, const double *traj_dev, double *score_dev, void *stream);

/* Ensemble statistics of a rollout on the device (additive, still 202, no struct changed; looked up by name like the entries above).  cclqr_rollout_score reduces a
 * slab along time, per instance; this reduces it ACROSS the instances, per step: what a Monte-Carlo run of the reference -- simulate! under control_lqr!
 * (src/control/lqr.jl:89-139) / control_trackinglqr! (lqr_tracking.jl:46-71) with the `randn()` of trackingLQR_triple_cartpole.jl:98 -- is compared with the
 * predictions of cclqr_covariance_tracking by, without its trajectory.  The indexing is that of cclqr_rollout_score: slab row r = k - k0 holds the state the law saw
 * at the absolute step k (1-based), instance i has the global index gi = first_instance + i, and
 *     Δz_{i,k} [12 nb] = the error of lqr.jl:92-103 about setpoint row min(k, nsp) - 1 of table gi (a one-table controller: table 0),
 *     Δu_{i,k} [mu]    = -K[kidx] Δz_{i,k} of lqr.jl:106-111, kidx = min(k, nK) - 1 (N <= 0: 0), under the gate N <= 0 || k < N, else 0; 0 without gains,
 *     x_{i,k}          = (Δz_{i,k}, Δu_{i,k}), 12 nb + mu coordinates.
 * Per step the call writes  mean_dev [steps][12 nb + mu] = (1/n) sum_i x_{i,k}  and  m2_dev [steps][12 nb + mu] = sum_i (x_{i,k} - mean)^2, the CENTRED sum of squares
 * per coordinate (variance = M2 / n; the mean square about the setpoint = (M2 + n mean^2) / n), and for each of the n_cov absolute steps listed in cov_steps (HOST
 * array, each within k0 .. k0 + steps - 1, at most 64 per call)  cov_dev [n_cov][12 nb][12 nb] = sum_i (Δz_i - mean)(Δz_i - mean)', exactly symmetric, its diagonal
 * equal to M2 to rounding.  Δz is in the CALLER'S body order in every output (as cclqr_value_get returns Σ), Δu in the controller's input order.  Row j (0-based) of
 * a run from step 1 is knot j of cclqr_covariance_tracking.
 * Nothing is formed as S2 / n - mean^2: tiles of 64 instances are reduced about their own means and merged pairwise (Chan, Golub, LeVeque), in ONE order that depends
 * on n_inst and the mechanism only -- no floating-point atomics --, so a horizon taken chunk by chunk, or twice, gives the same bits.  All instances count: a value
 * that is not finite makes the coordinates it enters NaN at that step, and only those; a lost instance enters with its frozen pose (read `status`).
 * All pointers are DEVICE pointers except cov_steps; asynchronous on `stream`; nothing is allocated.  ws_dev: cclqr_rollout_ensemble_ws_bytes(m, mu, n_inst, steps,
 * n_cov) bytes, 8-byte aligned.  CCLQR_EINVAL, before anything is launched, with the cause in cclqr_last_error: a null or short workspace, a cov_steps entry outside
 * the launch, n_inst < 1, steps < 1 or k0 < 1, n_cov outside 0 .. 64, a controller made for another mechanism or device or without a setpoint table, first_instance +
 * n_inst > n_ctrl for a controller with several tables.  Every topology cclqr_mech_create takes. */
int cclqr_rollout_ensemble_ws_bytes(const cclqr_mech *m, int32_t mu, int64_t n_inst, int32_t steps, int32_t n_cov, size_t *bytes);
int cclqr_rollout_ensemble(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance,
                           const double *traj_dev, double *mean_dev, double *m2_dev,
                           int32_t n_cov, const int32_t *cov_steps /* host; absolute steps, each within k0 .. k0+steps-1 */, double *cov_dev,
                           void *ws_dev, size_t ws_bytes, void *stream);

/* Ensemble quantiles of a rollout on the device (additive, still 202, no struct changed; looked up by name like the entries above).  cclqr_rollout_ensemble gives
 * the second moments of a Monte-Carlo run of the reference -- simulate! (examples/lqr_cartpole.jl:44) under the `randn()` of examples/trackingLQR_triple_cartpole.jl:98
 * --; this gives its fan chart: the median, the tails and the extremes of every coordinate at every step, without the trajectory.  Indexing and x are those of
 * cclqr_rollout_ensemble: slab row r = k - k0, instance i has the global index gi = first_instance + i, x_{i,k} = (Δz_{i,k}, Δu_{i,k}) with 12 nb + mu coordinates,
 * Δz in the CALLER'S body order, Δu in the controller's input order under the same gate (0 without gains); x is bit for bit the x that call reduces.
 * For each step k and coordinate c let s_0 <= ... <= s_{cnt-1} be the FINITE values among x_{i,k,c}, i = 0 .. n_inst - 1, sorted as numbers, -0.0 before +0.0; values
 * that are not finite are left out and counted out.  For each of the n_prob probabilities p in [0, 1] listed in prob (HOST array, at most CCLQR_QUANTILE_MAX_PROBS)
 *     h = p (cnt - 1),  lo = floor(h),  g = h - lo,  hi = min(lo + 1, cnt - 1),  q = s_lo + g (s_hi - s_lo)
 * in fp64 as written, each operation rounded once (no fused multiply-add); whenever g = 0 the result is the order statistic s_lo itself, bit for bit: p = 0 is the
 * minimum, p = 1 the maximum.  cnt = 0 gives NaN.  The call writes  quant_dev [steps][n_prob][12 nb + mu]  and, unless it is NULL,  finite_dev [steps][12 nb + mu]
 * (int32) = cnt.  All instances count: a lost instance enters with its frozen pose (read `status`).
 * The result is a function of the multiset of values only: the same bits for any chunking of the horizon, any workspace size, a second call, and any permutation of
 * the instances under a one-table controller.
 * All pointers are DEVICE pointers except prob; asynchronous on `stream`; nothing is allocated, nothing synchronises.  ws_dev, 8-byte aligned: the values of the rows,
 * transposed.  cclqr_rollout_quantiles_ws_bytes gives min_bytes (one slab row) and full_bytes (all `steps` rows); the call works through the rows in blocks of as many
 * as ws_bytes holds, and the bits do not depend on ws_bytes.  CCLQR_EINVAL, before anything is launched, with the cause in cclqr_last_error and the outputs untouched:
 * a null, short (ws_bytes < min_bytes) or misaligned workspace, n_prob outside 1 .. 16, a prob entry outside [0, 1] or NaN, n_inst < 1, steps < 1 or k0 < 1, and every
 * controller and handle refusal of cclqr_rollout_ensemble.  n_inst > CCLQR_QUANTILE_MAX_INST (a coordinate's keys are sorted in one workgroup's LDS) is
 * CCLQR_EUNSUPPORTED.  Every topology cclqr_mech_create takes. */
#define CCLQR_QUANTILE_MAX_INST  16384
#define CCLQR_QUANTILE_MAX_PROBS 16
int cclqr_rollout_quantiles_ws_bytes(const cclqr_mech *m, int32_t mu, int64_t n_inst, int32_t steps, size_t *min_bytes, size_t *full_bytes);
int cclqr_rollout_quantiles(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance,
                            const double *traj_dev, int32_t n_prob, const double *prob /* host */,
                            double *quant_dev, int32_t *finite_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* Joint coordinates of a rollout on the device (additive, still 202, no struct changed; looked up by name like the entries above).  The slab holds maximal
 * coordinates; the reference's users think in joint coordinates: its minimal-coordinate LQR constructor takes xθd and vωd (src/control/lqr.jl:68-86), its PID runs on
 * minimalCoordinates(mechanism, eqc)[1] (src/control/pid.jl:43-57), and the friction law of examples/trackingLQR_triple_cartpole.jl:98-101 acts on the relative joint
 * velocity.  This call returns both for every joint at every row of a slab.
 * The definition.  For joint j in the CALLER'S joint order (the index ctrl_joint uses), a = its parent body or the origin (x = 0, q = 1, velocities 0), b = its child
 * body, poses from slab row r = k - k0 of instance i:
 *     revolute   e = conj(q_a) q_b conj(qoff),  s = axis . vec(e),  c = e_0,  θ_raw = 2 atan2(s, c)          rate = axis . ω_b - axis . ω_a  (entries 10..12 as stored)
 *     prismatic  θ_raw = axis . (R_a'(x_b + R_b p2 - x_a) - p1)                                              rate = axis . R_a'(v_b - v_a)
 * exactly the coordinate the PID law of the rollout forms (pid.jl:43-57) and the relative velocity its friction law forms (trackingLQR_triple_cartpole.jl:98-101).  A
 * CCLQR_FIXED_ORIENTATION joint has no coordinate: 0.0 for both.
 * mode CCLQR_JOINTS_RAW: θ = θ_raw, the number PID sees.  mode CCLQR_JOINTS_CONTINUOUS, revolutes (prismatic joints as in mode 0): the principal value w in [-π, π] is
 * 2 atan2(s, c) with (s, c) negated when c < 0, so the two quaternions of one rotation give the same w; θ_k = w_k + 2π turns_k with turns an integer, 0 at step 1;
 * with d = w_k - w_prev, turns goes down by 1 if d > π and up by 1 if d < -π.  A w_k that is not finite gives θ_k = NaN and leaves (w_prev, turns) as they were.
 * carry_dev [n_inst][ne][2] holds (w_prev, turns): read when k0 > 1, always written in mode 1, so a horizon taken chunk by chunk gives the bits of one call.  The rate
 * has no state.  A value that is not finite makes the outputs it enters NaN (never Inf) and nothing else.
 * The call writes rows k0 - 1 .. k0 + steps - 2 of each instance's out_steps rows of theta_dev [n_inst][out_steps][ne] and, unless it is NULL, rate_dev of the same
 * shape: the absolute step, as the noise array is indexed, so the chunks of a horizon fill one series.  With a cclqr_plants handle instance i reads p1, p2 of the
 * plant record cclqr_rollout_plants would read for the global index first_instance + i (prismatic joints of chains and trees); plants = NULL reads the mechanism's.
 * Device pointers; asynchronous on `stream`; nothing is allocated.  CCLQR_EINVAL, before anything is launched, with the cause in cclqr_last_error and the outputs
 * untouched: n_inst < 1, steps < 1, k0 < 1, out_steps < k0 + steps - 1, a mode outside 0 / 1, mode 1 without carry_dev, a null traj_dev or theta_dev, plants made for
 * another mechanism or device or not covering first_instance .. first_instance + n_inst - 1.  Every topology cclqr_mech_create takes, loops included. */
#define CCLQR_JOINTS_RAW 0
#define CCLQR_JOINTS_CONTINUOUS 1
int cclqr_rollout_joints(const cclqr_mech *m, const cclqr_plants *plants, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance,
                         const double *traj_dev, int32_t mode, int64_t out_steps,
                         double *theta_dev /* [n_inst][out_steps][ne] */, double *rate_dev /* same shape, or NULL */,
                         double *carry_dev /* [n_inst][ne][2]; mode 1 only, else NULL */, void *stream);

/* The integrator's own invariants of a rollout on the device (additive, still 202, no struct changed; looked up by name like the entries above): can this run be
 * trusted?  A variational integrator in maximal coordinates promises closed joints, unit quaternions and an energy that oscillates without drift (SURVEY.md,
 * "Integrator invariants"); this call measures all three at every row of a slab, and keeps an eight-number verdict per instance for runs whose states are gone.
 * The definition.  For instance i and slab row r (absolute step k = k0 + r, as cclqr_rollout_joints indexes) take the row's 13 entries per body AS STORED: x 0..2,
 * q 3..6, v 7..9, ω 10..12 (body frame).  m_b, J_b, p1, p2 are the mechanism's, or -- with a cclqr_plants handle -- those of the plant record cclqr_rollout_plants
 * would read for the global index first_instance + i.  inv_dev [i][k - 1][0..5]:
 *     0  T      Σ_b ( ½ m_b v_b·v_b + ½ ω_b·(J_b ω_b) )
 *     1  V      -g Σ_b m_b x_b[2]                      g: the mechanism's signed g
 *     2  E      T + V, that one addition of outputs 0 and 1
 *     3  gap    max |g_r| over all TRANSLATIONAL constraint rows of all joints
 *     4  twist  max |g_r| over all ROTATIONAL rows
 *     5  quat   max_b | q_b·q_b - 1 |
 * g_r are the rows the rollout's Newton solve drives to zero: R(q_a)'(x_b + R(q_b) p2 - x_a) - p1 and vec(conj(q_a) q_b conj(qoff)), picked by the mechanism's row
 * selectors (a revolute has 3 translational and 2 rotational rows, a prismatic joint 2 and 3); the origin is x = 0, q = 1.  A CCLQR_FIXED_ORIENTATION constraint of a
 * loop mechanism contributes its rotational rows and no translational ones; rows a joint does not have count as 0.
 * rows_dev [i][k - 1][j][0..4], optional: g of joint j in the CALLER'S joint order, five rows per joint, rows the joint does not have 0.
 * Summation order of T and V: one term per link in the library's link order (parents first, chain by chain; loop mechanisms: the caller's body order), padded with
 * zeros to the next of 8, 16, 32, 64 terms, added by the xor butterfly v_t += v_{t xor o}, o = 1, 2, 4, ...  Adding a zero is exact: the bits depend on the link
 * order alone.
 * Values that are not finite: anything not finite that enters an output makes THAT output NaN -- never Inf -- and nothing else.  The max PROPAGATES a NaN: one
 * constraint row or quaternion that is not finite makes gap / twist / quat of that step NaN.  In rows_dev such a row is NaN.
 * summary_dev [i][0..7], accumulated across launches: initialised when k0 == 1, read and merged when k0 > 1, always written:
 *     0     E at the first row where it is finite (NaN until one is seen)
 *     1, 2  min and max of E over the rows where it is finite (NaN until one is seen)
 *     3     max of gap over the rows where it is finite (NaN until one is seen)
 *     4     the absolute step k at which 3 was first reached (0 if there is no such row)
 *     5, 6  max of twist, of quat over their finite rows (NaN until one is seen)
 *     7     the number of rows with any of the six outputs not finite
 * Min, max and "first" do not depend on how the horizon is cut: any chunk plan gives the bits of one call.  energy_drift = max(E_max - E_1, E_1 - E_min) is the host's.
 * The call writes rows k0 - 1 .. k0 + steps - 2 of inv_dev / rows_dev only.  Device pointers; asynchronous on `stream`; nothing is allocated.  Every topology
 * cclqr_mech_create takes, loops included; plants on chains and trees.  CCLQR_EINVAL, before anything is launched, with the cause in cclqr_last_error and the outputs
 * untouched: n_inst < 1, steps < 1, k0 < 1, out_steps < k0 + steps - 1 when inv_dev or rows_dev is given, a null traj_dev, all three outputs NULL, plants made for
 * another mechanism or device or not covering first_instance .. first_instance + n_inst - 1. */
#define CCLQR_INVARIANTS_LEN 6
#define CCLQR_INVARIANTS_SUMMARY_LEN 8
int cclqr_rollout_invariants(const cclqr_mech *m, const cclqr_plants *plants, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance,
                             const double *traj_dev, int64_t out_steps,
                             double *inv_dev /* [n_inst][out_steps][6], or NULL */, double *rows_dev /* [n_inst][out_steps][ne][5], or NULL */,
                             double *summary_dev /* [n_inst][8], or NULL; read when k0 > 1 */, void *stream);

/* The statistics of any per-instance series x_dev [n_inst][steps][nc] ACROSS its instances, per step (additive, still 202; looked up by name): what
 * cclqr_rollout_ensemble / cclqr_rollout_quantiles compute, with x GIVEN instead of formed -- the joint series above (the fan chart of a swing-up in joint angles, the
 * quantity pid.jl:43-57 regulates), or any other.  They know nothing of mechanisms.
 * cclqr_series_ensemble: mean_dev, m2_dev [steps][nc] = the mean and the CENTRED sum of squares of every coordinate; a value that is not finite makes its coordinate
 * NaN at that step.  Summation order: a tile is 64 consecutive instances, reduced about its own mean in two passes; the tiles are merged in tile order (Chan, Golub,
 * LeVeque).  No atomics: a second call gives the same bits.  ws_dev: cclqr_series_ensemble_ws_bytes bytes, 8-byte aligned.
 * cclqr_series_quantiles: quant_dev [steps][n_prob][nc] = the quantiles of the FINITE values by the formula of cclqr_rollout_quantiles above, finite_dev [steps][nc]
 * (int32, or NULL) their number; n_inst <= CCLQR_QUANTILE_MAX_INST (else CCLQR_EUNSUPPORTED), n_prob <= CCLQR_QUANTILE_MAX_PROBS, prob a HOST array.  The workspace
 * block rule is that call's: min_bytes holds one row, full_bytes all, and the bits do not depend on ws_bytes.
 * Device pointers except prob; asynchronous on `stream`; nothing is allocated.  CCLQR_EINVAL, before anything is launched, with the cause in cclqr_last_error and the
 * outputs untouched: n_inst < 1, steps < 1, nc outside 1 .. CCLQR_SERIES_MAX_COORDS, a null argument, a null, short or misaligned workspace, n_prob outside 1 .. 16, a
 * prob entry outside [0, 1] or NaN. */
#define CCLQR_SERIES_MAX_COORDS 1024
int cclqr_series_ensemble_ws_bytes(int64_t n_inst, int32_t steps, int32_t nc, size_t *bytes);
int cclqr_series_ensemble(int64_t n_inst, int32_t steps, int32_t nc, const double *x_dev, double *mean_dev, double *m2_dev,
                          void *ws_dev, size_t ws_bytes, void *stream);
int cclqr_series_quantiles_ws_bytes(int64_t n_inst, int32_t steps, int32_t nc, size_t *min_bytes, size_t *full_bytes);
int cclqr_series_quantiles(int64_t n_inst, int32_t steps, int32_t nc, const double *x_dev, int32_t n_prob, const double *prob /* host */,
                           double *quant_dev, int32_t *finite_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* cclqr_rollout (HOST pointers) with options: first_instance and newton_mode apply, the device-buffer fields must be NULL. */
int cclqr_rollout_host_ex(const cclqr_mech *m, const cclqr_ctrl *c, int64_t n_inst, int32_t steps, int32_t k0, const double *z0,
                          const double *noise, double *traj, double *zT, int32_t *status, const cclqr_rollout_opts *opts);

/* Sizes the controller handle's Philox noise workspace for launches of up to n_inst * steps samples (the `randn()` stream of
 * examples/trackingLQR_triple_cartpole.jl:98,125 as generated by noise_philox).  Synchronises the device when it has to re-allocate.
 * Call it before capturing step-per-launch rollouts of a noise_philox controller into a hipGraph (BASELINE configs[4]), from a thread that is on
 * the controller's device (CCLQR_EINVAL otherwise), and never while ANY stream of that device is being captured in the global capture mode (the
 * re-allocation is a device synchronisation plus an allocation, which such a capture does not survive; a launch on the capturing stream itself
 * that would have to grow the workspace is refused with CCLQR_EINVAL before anything is touched, and so is ANY launch that carries
 * CCLQR_ROLLOUT_NO_ALLOC in cclqr_rollout_opts.flags: cclqr_rollout_ex). */
int cclqr_ctrl_reserve_noise(cclqr_ctrl *c, int64_t n_inst, int32_t steps);

/* The `controlfunction` hook of the reference's controllers (src/control/lqr.jl:14, :56; lqr_tracking.jl:19; pid.jl:16 -- a Julia closure
 * `controlfunction(mechanism, controller, k)` that ends in setForce!(mechanism, eqc, u), e.g. examples/trackingLQR_triple_cartpole.jl:93-117)
 * with the closure on the HOST and the batch on the device: the caller steps the rollout one launch per step (k0 continuation of
 * cclqr_rollout_dev), reads the states, lets its closure compute every instance's joint inputs and hands them over here; the next launch applies
 * them as feed-forward inputs.  Fd: [n_ctrl][nsp][mu] doubles exactly as given to cclqr_ctrl_create (len is checked against that), a HOST
 * pointer (on_device = 0: copied synchronously on the null stream -- the caller must have synchronised every NON-BLOCKING stream on which a launch
 * that reads this controller may still be running, e.g. by reading that launch's states back, as the closure loop does) or a DEVICE pointer
 * (on_device = 1: copied on `stream`, ordered with the launches on it).
 * The controller must have been created with a feed-forward table (Fd != NULL). */
int cclqr_ctrl_set_feedforward(cclqr_ctrl *c, const double *Fd, int64_t len, int32_t on_device, void *stream);

/* kernel launch geometry chosen for a mechanism (for roofline bookkeeping in bench.py; no counterpart in the reference's simulate!,
 * examples/lqr_cartpole.jl:44): lanes per instance and LDS bytes per workgroup; links the chain kernel's LDS image is laid out for
 * (names the instantiation rollout_chain_kernel<lanes, links, law> for forests of chains and rollout_treereg_kernel<lanes, links, law, relax>
 * for branching trees; 0 for closed-loop mechanisms, whose one kernel takes its layout at run time) */
int cclqr_rollout_geometry(const cclqr_mech *m, int32_t *lanes_per_instance, int32_t *lds_bytes_per_workgroup);
int cclqr_rollout_layout_links(const cclqr_mech *m, int32_t *links);
/* lanes that work for ONE link and links per sub-lane group of the chain kernel's instantiation (rollout_chain_kernel<lanes, links, law, relax, lanes_per_link,
 * links_per_group>): a forest of chains that leaves lanes of its lane group idle (1-2 links in 8 lanes: 3 lanes per link; 3-4 in 8, 5-8 in 16, 9-16 in 32: 2) deals
 * the constraint rows of an evaluation to them at unchanged occupancy; 1 and the lane count for longer chains, branching trees and closed loops.  Bookkeeping
 * for bench.py like the two above (no counterpart in the reference's simulate!, examples/lqr_cartpole.jl:44). */
int cclqr_rollout_lanes_per_link(const cclqr_mech *m, int32_t *lanes_per_link, int32_t *links_per_group);
/* instances a launch of n_inst instances x steps steps with these cclqr_rollout_opts.flags puts into one wavefront (fewer than 64 / lanes-per-instance
 * when the batch is spread, see CCLQR_ROLLOUT_PACK_WAVEFRONTS; closed loops: always 1).  Bookkeeping. */
int cclqr_rollout_instances_per_wavefront(const cclqr_mech *m, int64_t n_inst, int32_t steps, int32_t flags, int32_t *instances);

#ifdef __cplusplus
}
#endif
#endif
