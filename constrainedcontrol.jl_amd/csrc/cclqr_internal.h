// cclqr_internal.h -- host-side handles and kernel launch arguments shared by the translation units of libcclqr.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "cclqr_dev.h"

#define CCLQR_ESINGULAR_ (-2)

namespace cclqr {

struct RolloutArgs {
    const MechDev* M;
    const CtrlDev* C;
    int64_t n_inst;
    int steps, k0;
    const double* z0;     // [n_inst][nb][13] user body order
    double* lam;          // [n_inst][5 nb] internal order, or null
    const double* noise;  // [n_inst][noise_stride] or null
    int64_t noise_stride;
    double* pid_state;    // [n_inst][nb][2] integrated / last PID errors carried between launches (opaque link order), or nullptr
    int64_t inst0;        // global index of instance 0 of this launch (Philox stream = global instance index, so shards reproduce the whole batch)
    double* traj;         // [n_inst][steps][nb][13] or null
    double* zT;           // [n_inst][nb][13]
    int* status;          // [n_inst] or null
    double eps_alone;     // measured-error Newton mode (RELAX kernels only): a solve also stops when ||f|| falls below this
    int carry;            // CCLQR_ROLLOUT_CARRY_STATUS: `status` comes in with the instance's status of the launches before (0: none): an instance that was lost stays
                          // frozen and keeps its status, the others merge this launch's Newton count / failure into it
    int ipw;              // chain and tree kernels: instances per wavefront, 1 .. 64 / lanes per instance (lane groups beyond it hold no instance).  The caller of
                          // launch_rollout_chain / launch_rollout_treereg passes 0 (the launch chooses: spread_instances_per_wavefront) or nonzero = pack every wavefront full
    const PlantRec* plants;   // per-instance plants (cclqr_rollout_plants): records [n_plant][nb] in link order, or nullptr = every instance runs the mechanism's own plant
    int64_t plant_off;        // instance n of this launch runs plant plant_off + n (= first_instance - the table's first_index; checked against [0, n_plant) on the host)
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel) instead of once per launch: remembers the largest size set so
// far and only calls the runtime when a launch needs more (capi.hip)
hipError_t set_max_dynamic_lds_once(const void* fn, size_t lds);
// The one way a kernel is launched: raise the kernel's dynamic-LDS limit (set_max_dynamic_lds_once), launch through the pointer, report the
// launch error.  The pointer is selected once by the caller, so the kernel whose limit is raised is the kernel that runs.  RAISE_LDS = false
// for the launches that stay under the 48 KB every kernel has: they make no runtime call besides the launch (nothing that a stream capture
// could object to).  The arguments are converted to the kernel's parameter types as a direct call would.
template <bool RAISE_LDS = true, class... P, class... A>
inline hipError_t launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    if (RAISE_LDS) {
        const hipError_t e = set_max_dynamic_lds_once((const void*)kernel, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<P>(args)...);
    return hipGetLastError();
}

// The control law a rollout kernel is instantiated for.  The values are the kernels' template parameter EXTRA (rollout_chain_kernel,
// rollout_treereg_kernel); the closed-loop kernel has every law at run time.
enum class ControlLaw : int {
    Lqr = 0,           // LQR / TrackingLQR alone
    FricNoise = 1,     // + joint friction and / or noise read from an array (the caller's, or a Philox workspace filled before the launch)
    Pid = 2,           // + PID joints (and everything above)
    PhiloxInKernel = 3 // LQR + noise whose samples the kernel generates itself (forests of chains only)
};

// Which kernel a mechanism's rollout runs on and how it is launched.  Filled once per mechanism (cclqr_tables.h rollout_shape_of, kept in
// cclqr_mech); the entry points, the geometry queries and the launchers all read this one copy.
enum class RolloutFamily : int { Chain, Tree, Loop };     // rollout_chain.hip / rollout_treereg.hip / rollout_loop.hip
struct RolloutShape {
    RolloutFamily family;
    int G;             // lanes per instance (loops: the whole wavefront)
    int NBP;           // links the LDS image is laid out for: with G it names the instantiation (loops: 0, one kernel with a run-time layout)
    int KL, NL;        // lanes per link, links per lane group (KL * NL <= G)
    int full;          // instances per full wavefront: 64 / G (loops: 1)
    int NCB;           // loops: column blocks of eight the instantiation holds (loop_col_blocks), else 0
    int pid_slots;     // (integrated, last) PID pairs per instance: one per joint
    int fixed_plan;    // chains: ONE chain from link 0 over all NBP = nb links, 16 or 17 of them (the N-link cartpole): the kernels with the solve plan compiled in
                       // (rollout_chain.hip rollout_chain_fixed_kernel, cclqr_chain.h PlanFixed); 0 = the plan is read at run time
    size_t lds;        // dynamic LDS per workgroup of the rollout kernel, `full` instances
    size_t lin_lds;    // dynamic LDS per workgroup (one knot) of the mechanism's linearisation kernel
};

// zero doubles behind a controller's gain table: the control phase fetches ceil(12 NBP / G) G entries of a row whatever the mechanism's own
// 12 nb, i.e. up to 12 x 64 - 12 past the end of the LAST row when a short chain runs on a long image.  With one table per instance (n_ctrl > 1)
// every instance's table carries its own zero pad of that overrun (gain_table_layout, CtrlDev::K_stride includes it), so that the entries
// past an instance's last row are zeros and never a NEIGHBOUR's gains -- which may be Inf / NaN when that neighbour's recursion diverged, and
// 0 * NaN would poison a healthy instance's input
#define CCLQR_K_PAD 768
// doubles the rollout kernels' control phase fetches past the end of a gain row: they read ceil(12 NBP / G) G entries of a row (G lanes per instance,
// the LDS image laid out for NBP >= nb links) and let the surplus meet a zero factor.  Closed-loop kernel: exact row length.
static inline size_t gain_row_overrun(const RolloutShape& s, int nb) {
    if (s.family == RolloutFamily::Loop) return 0;
    const long long over = (long long)((12 * s.NBP + s.G - 1) / s.G) * s.G - 12LL * nb;
    return over > 0 ? (size_t)((over + 1) & ~1LL) : 0;
}
// A controller's gain tables in device memory: n_tables tables of rows_per_table rows of 12 nb doubles.  Several tables (one per instance) lie
// `stride` apart, each behind its own zero pad; K_stride is what CtrlDev carries (0: one shared table); alloc_doubles ends in CCLQR_K_PAD zeros.
struct GainTableLayout { size_t pad; long long stride, K_stride; size_t alloc_doubles; };
static inline GainTableLayout gain_table_layout(const RolloutShape& s, int nb, long long n_tables, long long rows_per_table) {
    GainTableLayout L;
    L.pad = n_tables > 1 ? gain_row_overrun(s, nb) : 0;
    L.stride = rows_per_table * 12LL * nb + (long long)L.pad;
    L.K_stride = n_tables > 1 ? L.stride : 0;
    L.alloc_doubles = (size_t)(n_tables > 1 ? n_tables : 1) * (size_t)L.stride + CCLQR_K_PAD;
    return L;
}

// Instances per wavefront of a launch.  A wavefront's step is latency -- a chain of dependent 5 x 5 stages -- not lanes, and a lane group without an
// instance is not idle: it evaluates further step lengths of its neighbours' line searches (group_assist / the partner group).  So a batch that would
// leave SIMDs without a wavefront when packed 64 / G to a wavefront is spread: the fewest instances per wavefront that still fit the batch into
// `slots` wavefronts -- slots = every SIMD of the device for a persistent launch (steps >= 8: it has the device to itself), a quarter of them for
// short launches (step-per-launch chains run several to a device, bench.py::_graph_captured_steps: spreading each over the whole device would
// queue them behind one another).  Measured (tools/gpu_batch_density.py, ms per 1000 steps, packed -> spread): 256 tracking triple cartpoles
// 43.7 -> 34.7, 256 cartpoles 24.6 -> 21.5, 256 17-body chains (300 steps) 22.0 -> 20.2, 4096 cartpoles (configs[1]) 24.9 -> 24.0; a batch that
// fills the device is packed as before.  Same arithmetic in the same order either way: results are bitwise those of the packed launch
// (tests/test_gpu_rollout.py::test_spread_and_packed_launches_agree_bitwise).  packed: CCLQR_ROLLOUT_PACK_WAVEFRONTS.  `full` = 64 / lanes per
// instance (RolloutShape::full); simds = SIMDs of the mechanism's device (cclqr_mech::simds).  Chains and branching trees spread by this one rule.
inline int spread_instances_per_wavefront(int full, int64_t n_inst, int steps, bool packed, int simds) {
    if (packed || full == 1) return full;
    const int64_t slots = steps >= 8 ? simds : simds / 4;
    const int64_t ipw = (n_inst + slots - 1) / slots;
    return ipw < 1 ? 1 : (ipw > full ? full : (int)ipw);
}

hipError_t launch_philox_fill(double* out, unsigned key0, long long inst0, long long n_inst, int k0, int steps, hipStream_t stream);
// the three rollout launchers: forests of chains (rollout_chain.hip), branching trees (rollout_treereg.hip; a.M must point at the device image
// [MechDev | TreeRegDev], treereg_of) and closed-loop mechanisms (rollout_loop.hip: every law at run time).  s = the mechanism's shape
// which kernel family launch_rollout_chain takes: the fixed-plan kernels for a shape that has them, unless the caller asked for the general kernel
// (runtime_plan: CCLQR_ROLLOUT_RUNTIME_PLAN).  Stated here, not inside the launcher, so that the CPU suite can ask it (tests/emu/emu_chain_fixed_plan.cpp)
inline bool chain_launch_fixed_plan(const RolloutShape& s, bool runtime_plan) { return s.family == RolloutFamily::Chain && s.fixed_plan != 0 && !runtime_plan; }
hipError_t launch_rollout_chain(const RolloutArgs& a, const RolloutShape& s, int simds, ControlLaw law, int newton_mode, bool runtime_plan, hipStream_t stream);
hipError_t launch_rollout_treereg(const RolloutArgs& a, const RolloutShape& s, int simds, ControlLaw law, int newton_mode, hipStream_t stream);
hipError_t launch_rollout_loop(const RolloutArgs& a, const RolloutShape& s, int newton_mode, hipStream_t stream);

// per-instance plants (plants.hip): pack the caller-order arrays (device pointers; null = the mechanism's own value) into link-order records and
// validate them; *first_err (set to ~0 by the caller) receives the smallest (plant * nb + body) * 4 + kind among the offending entries
enum { PLANT_ERR_NONFINITE = 0, PLANT_ERR_MASS = 1, PLANT_ERR_INERTIA = 2 };
hipError_t launch_plants_pack(const MechDev* M, int nb, long long n_plant, const double* mass, const double* inertia, const double* p1, const double* p2,
                              PlantRec* out, unsigned long long* first_err, hipStream_t stream);

struct LinArgs {
    const MechDev* M;
    int nk, mu;
    int cj[CCLQR_MAXL];      // controlled links (internal)
    const double* zd;        // [nk][nb][13] internal link order
    const double* Fd;        // [nk][mu]
    double *A, *Bu, *Bl, *G; // [nk][...] internal link order
    int* status;             // [nk]
    const PlantRec* plants;  // per-knot plants (cclqr_linearize_plants): records [n_plant][nb] in link order, or nullptr = every knot on the mechanism's own plant
    long long plant_off;     // knot k is linearised on row plant_off + k of the table (checked against [0, n_plant) on the host); chains and trees only
    // whole trajectories per plant (cclqr_ctrl_create_tracking_batch_plants; lin_knot_rows): rows_per_plant = 0 is the map above, one knot = one setpoint row =
    // one plant.  rows_per_plant = N > 0: the launch holds knots_per_plant = N - 1 knots of every problem -- knot q belongs to problem q / (N - 1), reads setpoint
    // and feed-forward row problem * N + q % (N - 1) (the N-th row of a trajectory is not linearised, lqr_tracking.jl:87-88) and plant row plant_off + problem
    int knots_per_plant, rows_per_plant;
};
// which problem (= plant row behind plant_off) and which setpoint / feed-forward row knot q of a linearisation launch reads
HD void lin_knot_rows(int knot, int knots_per_plant, int rows_per_plant, int* problem, long long* row) {
    *problem = knot; *row = knot;
    if (rows_per_plant > 0) {
        const int p = knot / knots_per_plant;
        *problem = p; *row = (long long)p * rows_per_plant + (knot - p * knots_per_plant);
    }
}
// the model with the multipliers exogenous at the knots a.zd, for any mechanism (linearize.hip): linearize_kernel for chains and trees; closed
// loops are handed on to launch_linearize_loop (rollout_loop.hip, linearize_loop_kernel)
hipError_t launch_linearize(const LinArgs& a, const RolloutShape& s, hipStream_t stream);
hipError_t launch_linearize_loop(const LinArgs& a, const RolloutShape& s, hipStream_t stream);
// the rank-revealing projection onto (A', D) (rollout_loop.hip)
size_t project_model_lds_bytes(int mx, int mu, int ml);
bool project_model_fits(int mx, int mu, int ml);      // dynamic + static LDS of project_model_kernel within one CU's 160 KB
hipError_t launch_project_model(int nk, int mx, int mu, int ml, const double* A, const double* Bu, const double* Bl, const double* G, double* Ap, double* D,
                                double* res, int* rank, hipStream_t stream);

struct RicArgs {
    int nprob, mx, mu, ml, N;
    int time_varying;        // 1: A,Bu,Bl,G are [N-1][...] per problem (knot k uses index k-1)
    double tol;
    const double *A, *Bu, *Bl, *G, *Q, *R;
    double* K;               // [nprob][N-1][mu][mx] ([nprob][mu][mx] with keep_last)
    int* kbreak;             // [nprob]
    int* status;             // [nprob]
    double* work;            // ric_total_work_doubles(args) doubles
    int* stop;               // [nprob] scratch flags of the tiled path
    int path;                // 0: chosen by problem size and count, 1 resident, 2 tiled
    int bf16_terms;          // 0: fp64 MFMA; 1..3: split-bf16 products with fp32 accumulation (tiled path)
    int keep_last;           // 1: K is [nprob][mu][mx], the gain of the last executed backward step (= Ku[1] after the back-fill)
    long long kpad = 0;      // doubles left free between the tables of consecutive problems in K (0: contiguous)
    int p_rows = 0;          // 1: Q or R is not symmetric (ric_p_rows on the host arrays): the kernels that assume a symmetric Pk are not used
    long long q_stride = 0, r_stride = 0;      // doubles between the Q / R of consecutive problems: 0 = one pair shared by every problem, or mx*mx / mu*mu = one
                                               // pair per problem (ric_per_problem_weights)
    double* P_out = nullptr; // [nprob][mx][mx] device, or null: the cost-to-go Pkp1 of every problem's last executed backward step (lqr.jl:170; the step the break test
                             // of lqr.jl:172 fired on, else step 1; Q when N = 1), row-major as the recursion holds it; unspecified for a problem whose status is not 0.
                             // 16-byte aligned (the resident kernels store two doubles at a time)
};
// is the n x n row-major host matrix exactly symmetric?
inline bool ric_symmetric(const double* X, int n) {
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (!(X[(size_t)i * n + j] == X[(size_t)j * n + i])) return false;
    return true;
}
// RicArgs.p_rows: the kernels that assume a symmetric Pk run only when Q and R are EXACTLY symmetric (R is not looked at when mu == 0)
static inline int ric_p_rows(const double* Q, int mx, const double* R, int mu) { return (ric_symmetric(Q, mx) && (mu == 0 || ric_symmetric(R, mu))) ? 0 : 1; }
// ... of a batch with one (Q, R) per problem, Q [n][mx][mx], R [n][mu][mu]: p_rows is a property of the LAUNCH (it picks the kernels), so one problem whose
// weights are not symmetric sends the whole batch to the kernels that do not assume a symmetric Pk
static inline int ric_p_rows_batch(const double* Q, int mx, const double* R, int mu, long long n) {
    for (long long p = 0; p < n; p++)
        if (ric_p_rows(Q + p * mx * mx, mx, mu == 0 ? R : R + p * mu * mu, mu)) return 1;
    return 0;
}
// a call's host weights into its launch arguments: n_weights = 1 leaves the shared pair (stride 0, a.p_rows as the caller set it from that pair); n_weights =
// a.nprob gives every problem its own pair and widens a.p_rows to the batch's
static inline void ric_per_problem_weights(RicArgs& a, const double* Q, const double* R, int n_weights) {
    if (n_weights <= 1) return;
    a.q_stride = (long long)a.mx * a.mx;
    a.r_stride = (long long)a.mu * a.mu;
    a.p_rows = ric_p_rows_batch(Q, a.mx, R, a.mu, n_weights);
}
size_t ric_total_work_doubles(const RicArgs& a);
hipError_t launch_riccati(const RicArgs& a, hipStream_t stream);
// the RicArgs.path (1 resident, 2 tiled) launch_riccati takes for these arguments -- a call that runs its problems in several launches (chunks) asks once, with
// the nprob of the WHOLE call, and passes the answer to every launch: a chunk's own problem count must not pick another kernel
int ric_chosen_path(const RicArgs& a);

// What the analysis records below (PolArgs .. PtkArgs) share; capi.hip fills each by one function.  A batch's gain tables (raw_upload, gather_gains):
struct GainTable {
    const double* Kin = nullptr;   // device: tables [n_gains][nK][mu][mx] in the order of the models' states; may be null when mu = 0 or no step runs
    long long k_stride = 0;        // doubles between the tables of consecutive problems: 0 = one table shared by all, or nK * mu * mx
    int nK = 0;                    // rows per table: one per step / knot, or 1 (a stationary gain, used by every step); the doubling records hold 1 and do not read it
};
struct NoiseIn {      // ... its noise (upload_noise)
    const double *Wu = nullptr, *Sigma0 = nullptr;   // device [n_noise][mu][mu], [n_noise][mx][mx]; either may be null (= 0)
    long long wu_stride = 0, s0_stride = 0;          // doubles between consecutive problems' matrices: 0 = one shared by all
};
struct WeightsIn {    // ... its stage-cost weights (upload_weights; where they are the recursion's own, r.Q / r.R, capi.hip's ric_weights copies them into the RicArgs)
    const double *Q = nullptr, *R = nullptr;         // device [n_weights][mx][mx], [n_weights][mu][mu]
    long long q_stride = 0, r_stride = 0;            // 0 = one pair shared by all, or mx * mx / mu * mu
};

// Policy evaluation (policy.hip): dlqr's cost recursion (lqr.jl:147-177) with the gain GIVEN.  r: the problems as launch_riccati takes them -- nprob, mx, mu, ml, N, tol,
// A, Bu, Bl, G (time_varying = 0), Q, R with their strides, kbreak, status, stop, work (ric_total_work_doubles(r) doubles), path, and P_out, which is REQUIRED here;
// bf16_terms = 0; K, keep_last, kpad and p_rows are not read (no kernel here assumes a symmetric Pk).  The launch shape is ric_chosen_path(r).
struct PolArgs {
    RicArgs r;
    GainTable k;             // nK rows per table: N - 1 (row k - 1 = the gain of backward step k) or 1
    double* dnorm;           // device [nprob][2]: norm(Pk - Pkp1) of the last executed step and of the step before it, NaN where no such step ran
};
hipError_t launch_policy(const PolArgs& a, hipStream_t stream);

// A stationary gain's cost-to-go by doubling (policy_doubling.hip): S(a + b) = S(a) + M(a)' S(b) M(a) over the bits of N - 1, or level by level to convergence.
// r: as for launch_policy, with r.N = the knots of a fixed horizon (N - 1 steps exactly; r.tol is not read) or 0 = to convergence (increment < r.tol); kbreak is not
// written.  The launch shape is launch_policy's.
struct DblArgs {
    RicArgs r;
    GainTable k;             // the stationary gains [n_gains][mu][mx], one row each
    int max_levels;          // to convergence: the last level (2^max_levels steps)
    double* work2;           // device: dbl_work_doubles(r) doubles
    int *levels, *reason;    // device [nprob]: doublings made; to convergence, why the last one was the last (0 converged, 1 max_levels, 2 norm(M) > 1e50)
    double *dnorm, *gnorm;   // device [nprob][2]: the increment norms and norm(M) of the last level and of the one before, NaN where no such level ran
};
size_t dbl_work_doubles(const RicArgs& r);
hipError_t launch_policy_doubling(const DblArgs& a, hipStream_t stream);
// ... and its pieces, for a caller that starts the same recursion from a pair of its own (covariance_doubling.hip): dbl_preset clears the flags and presets the
// diagnostics; the caller's setup kernel then writes (M, S)(1) of every problem to dbl_Md / dbl_Sd, [nprob][mx][mx] each, and raises status / stop of a problem whose
// G Bλ is singular; launch_doubling_levels runs everything after that: P_out = S(n) + M(n)' Q M(n) with r.Q the terminal matrix (N = 1: P_out = r.Q, no setup needed)
static inline double* dbl_Md(const DblArgs& a) { return a.work2; }
static inline double* dbl_Sd(const DblArgs& a) { return a.work2 + (size_t)a.r.nprob * a.r.mx * a.r.mx; }
hipError_t dbl_preset(const DblArgs& a, hipStream_t stream);
hipError_t launch_doubling_levels(const DblArgs& a, hipStream_t stream);

// Closed-loop state covariance under input noise, by the same doubling (covariance_doubling.hip): with the one gain K, Δz⁺ = Abar Δz + D w, w ~ (0, Wu), so after n
// steps from a start of covariance Σ0:  Σ_n = C(n) + M(n) Σ0 M(n)',  C(n) = sum_{i<n} Abar^i W (Abar^i)',  W = D Wu D',  M(n) = Abar^n -- the pair recursion above on
// (Abar', W) with Σ0 as the terminal matrix.  d: as for launch_policy_doubling, except that d.r.Q / d.r.R are NOT the caller's: the launch points d.r.Q at its scaled
// copy of Σ0 (q_stride mx^2); d.r.P_out receives Σ.  d.work2 holds cov_work_doubles(d.r) doubles.
struct CovArgs {
    DblArgs d;
    NoiseIn n;
    WeightsIn w;                 // the stage-cost weights; read only when cost is given
    double *cost, *zstd, *ustd;  // device [nprob][2], [nprob][mx], [nprob][mu], each may be null: tr(Q Σ) and tr(R K Σ K'), sqrt(diag Σ), sqrt(diag K Σ K')
};
size_t cov_work_doubles(const RicArgs& r);
hipError_t launch_covariance_doubling(const CovArgs& a, hipStream_t stream);

// The state covariance of a tracked run, knot by knot (covariance_tracking.hip): Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j' with Abar_j = A'_j - D_j K_j
// (lqr_tracking.jl:107), j = 0 .. N-2, and the moments of every Σ_j.  r: nprob, mx, mu, ml, N, A, Bu, Bl, G with time_varying = 1 for N - 1 models per problem (model j =
// knot j) or 0 for one, kbreak (receives the knot of a singular G Bλ, else -1), status, work (ric_total_work_doubles(r) doubles), path (1 resident where it fits, 2
// tiled; 0 = 1); nothing else of r is read.
struct CtkArgs {
    RicArgs r;
    GainTable k;                 // nK rows per table: N - 1 (row j = the gain of knot j) or 1
    NoiseIn n;
    WeightsIn w;                 // the stage-cost weights (zeros when the caller asks for no cost)
    double* mom;                 // device [nprob][N][2 + mx + mu]: per knot cx, cu, zstd [mx], ustd [mu]
    double* total;               // device [nprob][2]
    double *Sigma, *Sigma_all;   // device [nprob][mx][mx], [nprob][N][mx][mx]; each may be null
};
// doubles of one knot's record in CtkArgs.mom
HD int ctk_record(int mx, int mu) { return 2 + mx + mu; }
// the resident kernel's fit rule, and the path a launch takes (1 resident, 2 tiled) -- a property of the shape and of opts->path alone, never of the batch
bool ctk_resident_fits(int mx, int mu);
int ctk_chosen_path(int mx, int mu, int path);
hipError_t launch_covariance_tracking(const CtkArgs& a, hipStream_t stream);

// The cost-to-go of a tracked run, knot by knot (policy_tracking.hip), the adjoint of the recursion above: P_{N-1} = Q, P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j
// (lqr_tracking.jl:108 with the gain given), j = N-2 .. knot, and price_j = tr(Wu D_j' P_{j+1} D_j).  r: as for launch_covariance_tracking, and Q, R with their strides
// (the stage-cost weights, required).
struct PtkArgs {
    RicArgs r;
    GainTable k;                 // nK rows per table: N - 1 (row j = the gain of knot j) or 1
    int knot;                    // in [0, N-1]: the recursion runs from N - 1 down to this knot
    NoiseIn n;                   // Wu, or null: no price is taken; there is no start covariance (Sigma0 stays null)
    double *P, *P_all;           // device [nprob][mx][mx] = P_knot, [nprob][N][mx][mx] (knots below `knot` are not written); each may be null
    double *price, *total;       // device [nprob][N] (zeros below `knot` and at N - 1), [nprob] = the prices summed from N - 2 downwards; both given with Wu, else both null
};
// the resident kernel's fit rule -- the shapes ctk_resident_fits serves --, and the path a launch takes (1 resident, 2 tiled): the shape and opts->path alone decide
size_t ptk_resident_lds_bytes(int mx, int mu);
bool ptk_resident_fits(int mx, int mu);
int ptk_chosen_path(int mx, int mu, int path);
hipError_t launch_policy_tracking(const PtkArgs& a, hipStream_t stream);

// The Riccati map itself by doubling (riccati_doubling.hip): n steps of lqr.jl:151-170 in projected form are the triple (A_n, G_n, H_n) of the map
// X -> H_n + A_n' X (I + G_n X)^-1 A_n; one step is (A', D R^-1 D', Q), and triple 1 applied after triple 2 is
//   W = (I + G1 H2)^-1,  A = A2 W A1,  G = G2 + A2 W G1 A2',  H = H1 + A1' H2 W A1
// r: as for launch_riccati with time_varying = 0, keep_last = 1 (K [nprob][mu][mx] + kpad, device), p_rows = 0 (Q and R symmetric: the caller has refused any other),
// bf16_terms = 0; r.N = the knots of a fixed horizon (N >= 2: N - 1 single-step triples, no stop test; r.tol is not read) or 0 = level by level to convergence
// (increment of H < r.tol); P_out may be null; kbreak is not written.  One launch shape for every mx >= 1.
struct RdbArgs {
    RicArgs r;
    int max_levels;          // to convergence: the last level (2^max_levels triples)
    double* work2;           // device: rdb_work_doubles(nprob, mx) doubles
    int *levels, *reason;    // device [nprob]: doublings made; why the last one was the last (0 converged / fixed horizon, 1 max_levels, 2 norm(A) > 1e50 or a norm that
                             // is not finite, 3 a zero or non-finite pivot of I + G1 H2)
    double *dnorm, *anorm;   // device [nprob][2]: norm(H(2^j) - H(2^(j-1))) and norm(A(2^j)) of the last level and of the one before, NaN where no such level ran
                             // (fixed horizon: anorm[0] = norm(A_n))
};
// the doubles of RdbArgs.work2: two triples, M = I + G1 H2, the solve's result [W A1 | W G1] and two product temporaries, [nprob][mx][mx] each; the per-tile sums of
// a level's two norms; the pivots of M (ints, a double's room for two)
static inline size_t rdb_work_doubles(long long nprob, int mx) {
    const size_t np = (size_t)nprob, mm = (size_t)mx * mx, tm = ((size_t)mx + 31) / 32;
    return 11 * np * mm + 4 * np * tm * tm + (np * (size_t)mx + 1) / 2 + 8;
}
// The schedule of a fixed horizon of n = N - 1 >= 1 single-step triples, square-and-multiply over the bits of n from the least significant: the first set bit copies
// the doubling triple into the accumulated one, every further set bit composes them, and the doubling triple is composed with itself between bits, not after the
// top one.  Writes the operations in order into ops (room for RDB_MAX_OPS) and returns their number; compositions = popcount(n) - 1 + bit_length(n) - 1.
enum { RDB_COPY = 0, RDB_ACCUMULATE = 1, RDB_DOUBLE = 2, RDB_MAX_OPS = 64 };
static inline int rdb_fixed_schedule(unsigned n, unsigned char* ops) {
    int count = 0, top = 0;
    bool have = false;
    while ((n >> (top + 1)) != 0) top++;
    for (int b = 0; n != 0 && b <= top; b++) {
        if ((n >> b) & 1u) { ops[count++] = have ? RDB_ACCUMULATE : RDB_COPY; have = true; }
        if (b < top) ops[count++] = RDB_DOUBLE;
    }
    return count;
}
// do the kernels hold these sizes (their LDS panels)?  The entry points refuse a size that does not fit as CCLQR_EINVAL before anything is allocated
bool riccati_doubling_fits(int mx, int mu);
// (a run to convergence synchronises `stream` every second level to read the stop flags)
hipError_t launch_riccati_doubling(const RdbArgs& a, hipStream_t stream);

// ---- one TrackingLQR per plant or trajectory (cclqr_ctrl_create_tracking_batch_plants): the workspace plan, pure host arithmetic
// Default budget of the call's device workspace.  Per knot a problem holds A (mx^2), Bu (mx mu), Bl and G (mx ml each), [A'|D] (mx (mx + mu)) and the projection
// scratch (ml^2 + ml (mx + mu)) -- triple cartpole, mx 48, mu 1, ml 20: 2304 + 48 + 960 + 960 + 2352 + 1380 doubles = 64 KB --, so its N = 1000 trajectory takes
// 64 MB and 1024 plants would take 65 GB at once.  4 GiB (1.4 % of an MI355X's 288 GB) runs them 64 problems to a chunk; the gain table itself (393 MB) is the
// controller's, not workspace.
#define CCLQR_TRACKING_WORKSPACE_BYTES (4LL << 30)
#define CCLQR_TRACKING_MAX_CHUNK 32768      // problems per launch: they are the y extent of the Riccati grids (at most 65535)
// bytes one problem adds to a chunk: its N - 1 linear models, its share of the recursion's workspace (ric_doubles = what one more problem adds to
// ric_total_work_doubles) and its knots' Newton statuses
inline long long tracking_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) {
    const long long nk = N - 1;
    return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles) + 4 * ((nk + 1) & ~1LL);
}
// problems per chunk: as many as `budget_bytes` (<= 0: CCLQR_TRACKING_WORKSPACE_BYTES) holds next to the call's fixed_bytes, at most CCLQR_TRACKING_MAX_CHUNK, then
// evened out over the resulting number of chunks (so that no chunk is a short tail).  0: not even one problem fits.  Chunk i of tracking_chunk_count() covers
// the problems [i per, min(n_ctrl, (i + 1) per)).
inline long long tracking_chunk_problems(long long n_ctrl, long long per_problem_bytes, long long fixed_bytes, long long budget_bytes) {
    if (budget_bytes <= 0) budget_bytes = CCLQR_TRACKING_WORKSPACE_BYTES;
    if (n_ctrl < 1 || per_problem_bytes < 1 || fixed_bytes < 0 || budget_bytes < fixed_bytes) return 0;
    long long fit = (budget_bytes - fixed_bytes) / per_problem_bytes;
    if (fit < 1) return 0;
    if (fit > CCLQR_TRACKING_MAX_CHUNK) fit = CCLQR_TRACKING_MAX_CHUNK;
    if (fit > n_ctrl) fit = n_ctrl;
    const long long chunks = (n_ctrl + fit - 1) / fit;
    return (n_ctrl + chunks - 1) / chunks;
}
inline long long tracking_chunk_count(long long n_ctrl, long long per_chunk) { return per_chunk < 1 ? 0 : (n_ctrl + per_chunk - 1) / per_chunk; }
// ---- the covariance of tracked runs on a mechanism's plants (cclqr_value_create_covariance_tracking): the same plan with its own bytes per problem.  A problem adds
// to a chunk its N - 1 linear models, its share of the recursion's workspace (ric_doubles, as above) and its knots' Newton statuses; what every problem of the CALL
// holds whatever the chunk -- its N records of ctk_record doubles, its totals, status and knot -- is counted with it, so that the budget bounds the whole
inline long long tracking_cov_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) {
    const long long nk = N - 1;
    return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles + (long long)N * (2 + mx + mu) + 2) + 4 * ((nk + 1) & ~1LL) + 8;
}
// ... and what the call holds once: the recursion's fixed workspace (ric_fixed doubles), the weights and the noise as given
inline long long tracking_cov_fixed_bytes(int mx, int mu, long long ric_fixed, int n_weights, int n_noise) {
    const long long mm = (long long)mx * mx, uu = (long long)mu * mu;
    return 8 * (ric_fixed + (long long)n_weights * (mm + uu + 1) + (long long)n_noise * (mm + uu));
}
// ---- the cost-to-go of tracked runs on a mechanism's plants (cclqr_value_create_policy_tracking): the same plan again.  A problem adds to a chunk its N - 1 linear
// models, its share of the recursion's workspace and its knots' Newton statuses; what every problem of the CALL holds whatever the chunk -- its N prices, its total,
// status and knot -- is counted with it
inline long long tracking_pol_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) {
    const long long nk = N - 1;
    return 8 * (nk * ((long long)mx * mx + (long long)mx * mu + 2LL * mx * ml) + ric_doubles + (long long)N + 1) + 4 * ((nk + 1) & ~1LL) + 8;
}
// ... and what the call holds once: the recursion's fixed workspace (ric_fixed doubles), the weights and the noise as given (Wu only: there is no start covariance)
inline long long tracking_pol_fixed_bytes(int mx, int mu, long long ric_fixed, int n_weights, int n_noise) {
    const long long mm = (long long)mx * mx, uu = (long long)mu * mu;
    return 8 * (ric_fixed + (long long)n_weights * (mm + uu + 1) + (long long)n_noise * uu);
}

}  // namespace cclqr

// opaque handles of include/cclqr.h
struct cclqr_mech {
    cclqr::MechDev host;       // internal link order
    cclqr::MechDev* dev;
    int nb;
    int nj;                    // joints: nb for trees, >= nb for closed-loop mechanisms
    int link_of_body[CCLQR_MAXL];   // user body  -> internal link
    int link_of_joint[CCLQR_MAXL];  // user joint -> internal link (= link of its child body)
    int device;
    int simds;                 // SIMDs of `device` (4 per compute unit): what spread_instances_per_wavefront spreads a small batch over
    cclqr::RolloutShape shape; // the kernel this mechanism's rollouts and linearisations run on
};
struct cclqr_plants {
    cclqr::PlantRec* dev;      // [n_plant][nb] records in the mechanism's link order
    int64_t n_plant, first_index;
    const cclqr_mech* mech;    // the mechanism whose link order and default values the records were packed with
    int nb, device;
};
// the weights a rollout is scored with (cclqr_score_create): blocks in the controller tables' link order
struct cclqr_score {
    double *Qb_dev, *R_dev;    // [nb][12][12] link order, [mu][mu]
    double settle_tol;
    int nb, mu, device;
    const cclqr_mech* mech;    // the mechanism whose link order the blocks were permuted to
};
// the cost-to-go tables of a controller (cclqr_value_create, cclqr_ctrl_create_lqr_batch_value): P in the caller's body order, as the recursion holds it
struct cclqr_value {
    double* P_dev;             // [n_tables][12 nb][12 nb] row-major
    int64_t n_tables;
    int nb, device;
    const cclqr_mech* mech;    // the mechanism whose body order the tables are in
};
struct cclqr_ctrl {
    cclqr::CtrlDev host;
    cclqr::CtrlDev* dev;
    double *K_dev, *zd_dev, *Fd_dev;
    size_t Fd_len;       // doubles in Fd_dev
    int nb;
    int device;           // the device the tables (and the noise workspace) live on = the mechanism's
    // workspace of the counter-based noise of one launch (noise_philox), grown on demand and kept with the handle
    double* noise_ws;
    size_t noise_ws_cap;
};
