// rollout_treereg.hip -- the LQR-controlled rollout kernel for BRANCHING trees (a body with several child joints), persistent over the whole
// horizon and REGISTER-resident like the chain kernel (rollout_chain.hip): lane t of an instance's lane group owns link t and keeps its state,
// multipliers, Jacobians and Newton iterate in registers.  The parent link is any earlier lane, so parent data arrive by ds_bpermute instead of
// a wave shift and child contributions are summed over the child list; LDS holds the 5x5 Schur blocks (one more pair per pair of sibling joints),
// eliminated without fill in a host-made schedule (cclqr_treereg.h, cclqr_treereg_tables.h).
//
// Replaces: ConstrainedDynamics.simulate!/newton! as driven by the reference (examples/lqr_cartpole.jl:44) with
//           control_lqr! (src/control/lqr.jl:89-139) / control_trackinglqr! (src/control/lqr_tracking.jl:46-71), on mechanisms the reference
//           reads from URDF files (examples/examples_files/*.urdf) that branch.
#include "cclqr_treereg.h"
#include "cclqr_internal.h"
#include "cclqr_newton.h"
#include "cclqr_rollout_step.h"

namespace cclqr {

// value of lane `addr / 4` of the wavefront (ds_bpermute: the LDS crossbar, no memory access)
__device__ __forceinline__ double lane_read(double v, int addr) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_ds_bpermute(addr, lo);
    hi = __builtin_amdgcn_ds_bpermute(addr, hi);
    return __hiloint2double(hi, lo);
}
template <int N>
__device__ __forceinline__ void from_lane(const double* in, double* out, int addr) {
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = lane_read(in[i], addr);
}
// sum over the child links of the owned body of what their lanes hold in `in` (gb4 = 4 x first lane of the group)
template <int N>
__device__ __forceinline__ void child_sum(const TreeL& T, int gb4, int maxchild, const double* in, double* out) {
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = 0.0;
    int c0 = T.child[0], c1 = T.child[1], c2 = T.child[2], c3 = T.child[3];      // the list rotates through fixed registers (cclqr_treereg.h tr_schur_rows)
#pragma unroll 1
    for (int k = 0; k < maxchild; k++) {
        const int addr = gb4 + 4 * c0;
        const bool has = k < T.nchild;
#pragma unroll
        for (int i = 0; i < N; i++) { const double v = lane_read(in[i], addr); out[i] += has ? v : 0.0; }
        c0 = c1; c1 = c2; c2 = c3;
    }
}

__device__ __forceinline__ void load_rec(TrRec& K, const TrRec* p) {
    const int4* q = (const int4*)p;
    const int4 a = q[0], b = q[1], c = q[2];
    K.o0 = a.x; K.o1 = a.y; K.ctl = a.z; K.pad = a.w;
    K.a[0] = b.x; K.a[1] = b.y; K.a[2] = b.z; K.a[3] = b.w;
    K.b[0] = c.x; K.b[1] = c.y; K.b[2] = c.z; K.b[3] = c.w;
}

// residual (+ Jacobians when JAC) at the point s - alpha ds with constraint forces C - alpha cd; returns the group's ||f||_2.
// With JAC the Schur complement rows of the point go straight to LDS (tr_schur_rows) -- if a solve may read them: the norm is formed in front of
// the row block and decides it (cclqr_chain.h chain_rows_verdict, as in the chain kernels that split the rows).  rows: the lane's instance is
// evaluated; nf0, nd: ||f|| of the point the step started from and the step's norm (+ infinity at an accepted point: the rows are built).  The rows
// are wavefront-wide work, so they are built unless NO lane says so.  DINV is stored either way, and the caller's jac_ok does not change: an
// instance that goes on at full step has voted for its rows, one that does not never reads them.
template <int G, bool JAC>
__device__ __forceinline__ double tree_eval(LinkC& c, const TreeL& T, LinkS& S, int t, int pa4, int maxchild, int maxsib, const Lay& Y, double* L, double alpha,
                                            bool active, bool rows, double nf0, double nd, double dt PROF_ARG) {
    double part = 0.0, nrm = 0.0;
    double NB[9], g[5], xq[7];
    LINK_FLAGS_FRESH(c);
#pragma unroll
    for (int k = 0; k < 7; k++) xq[k] = S.z[k];
#pragma unroll
    for (int k = 0; k < 9; k++) NB[k] = 0.0;
    if (active) {
        double cf[6], sv[6], cTR[6], DINV[9];
#pragma unroll
        for (int k = 0; k < 6; k++) { cf[k] = L[Y.C + 6 * t + k] - alpha * S.cd[k]; sv[k] = S.s[k] - alpha * S.ds[k]; cTR[k] = L[Y.D + 6 * t + k]; }
        part = ck_body_eval<JAC>(c, S.z, sv, cf, cTR, cTR + 3, dt, xq, S.d, DINV, NB);
        if (JAC) {
#pragma unroll
            for (int k = 0; k < 9; k++) L[Y.DINV + 9 * t + k] = DINV[k];
        }
    }
    STAMP(PF_EVAL_BODY);
    double pxq[7], pNB[9];
    from_lane<7>(xq, pxq, pa4);
    if (JAC) from_lane<9>(NB, pNB, pa4);
    if (!c.has_a()) {
#pragma unroll
        for (int i = 0; i < 7; i++) pxq[i] = (i == 3) ? 1.0 : 0.0;
    }
    double wXT[3][3], wPB[5][3], wPA[5][3];
    if (active) {
        joint_eval_sparse<JAC>(c, pxq, pxq + 3, xq, xq + 3, pNB, NB, g, wXT, wPB, wPA);
#pragma unroll
        for (int i = 0; i < 5; i++) part += g[i] * g[i];
    }
    STAMP(PF_EVAL_JOINT);
    LINK_FLAGS_FRESH(c);
    if constexpr (JAC) {
        nrm = sqrt(group_sum<G>(part));
        STAMP(PF_EVAL_MAP);
        if (__any(chain_rows_verdict(rows, nrm, nf0, nd, NEWTON_EPS))) {
            double pd[6];
            from_lane<6>(S.d, pd, pa4);
            tr_schur_rows(c, T, t, active, maxchild, maxsib, Y, L, wXT, wPB, wPA, g, S.d, pd);
        } else {
            PCOUNT(PF_ROWS_SKIPPED);
        }
        STAMP(PF_SCHUR_S);
    } else {
        nrm = sqrt(group_sum<G>(part));
        STAMP(PF_EVAL_MAP);
    }
    PCOUNT(PF_EVALS);
    return nrm;
}

// line search of the 32-lane instantiations (cclqr_rollout_step.h TrialIn; rollout_chain.hip chain_eval2 / the accept sequence there: unchanged)
template <int G>
__device__ __forceinline__ void tree_eval2(LinkC& c, const TrialIn& T, const double* Lc, int t, int pa4, const Lay& Y, double a1, double a2, bool active, double dt,
                                           double& n1, double& n2) {
    double part1 = 0.0, part2 = 0.0, xq1[7], xq2[7];
    LINK_FLAGS_FRESH(c);
#pragma unroll
    for (int k = 0; k < 7; k++) { xq1[k] = T.z[k]; xq2[k] = T.z[k]; }
    if (active) {
        double cf1[6], cf2[6], sv1[6], sv2[6], cTR[6], d1[6], d2[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const double cc = Lc[Y.C + 6 * t + k];
            cTR[k] = Lc[Y.D + 6 * t + k];
            cf1[k] = cc - a1 * T.cd[k]; cf2[k] = cc - a2 * T.cd[k];
            sv1[k] = T.s[k] - a1 * T.ds[k]; sv2[k] = T.s[k] - a2 * T.ds[k];
        }
        part1 = ck_body_eval<false>(c, T.z, sv1, cf1, cTR, cTR + 3, dt, xq1, d1, nullptr, nullptr);
        part2 = ck_body_eval<false>(c, T.z, sv2, cf2, cTR, cTR + 3, dt, xq2, d2, nullptr, nullptr);
    }
    double p1[7], p2[7];
    from_lane<7>(xq1, p1, pa4);
    from_lane<7>(xq2, p2, pa4);
    if (!c.has_a()) {
#pragma unroll
        for (int i = 0; i < 7; i++) { p1[i] = (i == 3) ? 1.0 : 0.0; p2[i] = p1[i]; }
    }
    if (active) {
        double g1[5], g2[5];
        joint_eval_sparse<false>(c, p1, p1 + 3, xq1, xq1 + 3, nullptr, nullptr, g1, (double(*)[3]) nullptr, (double(*)[3]) nullptr, (double(*)[3]) nullptr);
        joint_eval_sparse<false>(c, p2, p2 + 3, xq2, xq2 + 3, nullptr, nullptr, g2, (double(*)[3]) nullptr, (double(*)[3]) nullptr, (double(*)[3]) nullptr);
#pragma unroll
        for (int i = 0; i < 5; i++) { part1 += g1[i] * g1[i]; part2 += g2[i] * g2[i]; }
    }
    n1 = sqrt(group_sum<G>(part1));
    n2 = sqrt(group_sum<G>(part2));
}

// G lanes per instance (16 / 32), NBP links the LDS image is laid out for, EXTRA / RELAX as in rollout_chain_kernel
template <int G, int NBP, int EXTRA, bool RELAX = false>
__global__ __launch_bounds__(64) void rollout_treereg_kernel(RolloutArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, t = lane % G, grp = lane / G;
    const int gb4 = 4 * (lane - t);
    const int64_t inst = (int64_t)blockIdx.x * a.ipw + grp;      // (a.ipw instances per wavefront: cclqr_internal.h)
    const MechDev* M = a.M;
    const TreeRegDev* R = treereg_of(M);
    const CtrlDev* CT = a.C;       // the controller's tables; what a step reads of them is the record C below
    const int nb = M->nb;
    const double dt = M->dt;
    const int nss = R->nss;
    Lay Y = make_treereg_layout(NBP, 0);
    const int total = (Y.SS + 25 * nss) | 1;
    Y.total = total;
    double* L = lds + grp * total;
    const int nz = 13 * nb;
    const int maxchild = R->maxchild, maxsib = R->maxsib;

    LinkC c;
    // the lane's link constants, from the records of the plant its instance runs on: the mechanism's own, or -- per-instance plants, a wavefront-uniform
    // branch -- the row of the launch's table (a lane group without an instance reads the first instance's, as it does with controller tables)
    const PlantRec* plant = M->rec;
    const bool have = grp < a.ipw && inst < a.n_inst;      // the lane's instance exists
    if (a.plants) plant = a.plants + ((unsigned)a.plant_off + (have ? (unsigned)inst : 0u)) * (unsigned)nb;      // (a table holds fewer than 2^31 records: cclqr_plants_create)
    link_load_consts_rec(c, M, plant, t, nb, dt);
    TreeL T;
    tree_load(T, M, R, t, nb);
    const int pa4 = gb4 + 4 * T.par;
    if (T.nchild > 0) c.flags |= 4;          // "has a child link" (link_load_consts reads the chains' single-child table)
    if (EXTRA && CT->has_fric && c.on()) { c.fric = CT->fric[t]; if (c.fric != 0.0) c.flags |= LinkC::FRIC; }
    c.set_valid(have);
    const long long ginst = a.inst0 + inst;
    const int ut = c.on() ? M->perm[t] : 0;

    LinkS S;
    double pid_int = 0.0, pid_last = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) S.z[i] = c.live() ? a.z0[inst * nz + ut * 13 + i] : ((i == 3) ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 6; i++) S.s[i] = c.live() ? a.z0[inst * nz + ut * 13 + 7 + i] : 0.0;
    if (EXTRA >= 2 && a.pid_state && a.k0 > 1 && c.live()) { pid_int = a.pid_state[(inst * nb + t) * 2]; pid_last = a.pid_state[(inst * nb + t) * 2 + 1]; }
#pragma unroll
    for (int i = 0; i < 6; i++) { S.cd[i] = 0.0; S.d[i] = 0.0; S.ds[i] = 0.0; }
    // as in rollout_chain.hip: the multiplier block is all a Newton phase reads before writing it (tests/emu/emu_treereg.cpp poisons the rest of the image with
    // signalling NaNs; on the hardware tests/test_gpu_lds_poison.py does), so the image is not cleared -- zero, or the caller's warm start
    if (c.on()) {
        const bool warm = c.live() && a.lam && a.k0 > 1;
#pragma unroll
        for (int i = 0; i < 5; i++) L[Y.LAM + 5 * t + i] = warm ? a.lam[inst * 5 * nb + 5 * t + i] : 0.0;
    }

#ifdef CCLQR_PROFILE
    Prof prof;
    prof.start();
#endif
    int worst = 0;
    if (a.carry && a.status && c.valid()) {      // CCLQR_ROLLOUT_CARRY_STATUS (rollout_chain.hip)
        const NewtonStatus st = status_decode(a.status[inst]);
        worst = st.worst;
        if (st.bad) c.flags |= LinkC::BAD;
        if (st.dead) c.flags |= LinkC::DEAD;
    }
    typedef const __attribute__((address_space(4))) RolloutArgs* KernArgs;
    KernArgs ap = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int k0 = a.k0;
    int nsteps = a.steps;
    for (int kk = 0; kk < nsteps; kk++) {
        const int k = k0 + kk;
        asm volatile("" : "+s"(ap));
        LINK_FLAGS_FRESH(c);
        // ---------------- the launch-invariant data of the step comes first: the controller's record (CtrlDev::hot: one scalar load; the rows of this
        // step's tables follow from it without another load) and gravity.  The setpoint row and the gain rows are read where the feedback law uses
        // them, and the trajectory row is stored BEHIND the law: the memory counter runs over loads and stores in one order, so a load requested
        // behind the stores would wait for their acknowledgement too.
        CtrlHotK C = ctrl_hot_of(CT);
        asm volatile("" : "+s"(C));
        const long long gi = c.valid() ? ginst : a.inst0;      // (a lane of an instance that does not exist reads the first instance's tables; its result is never used)
        const int ne = 12 * nb;
        const int mu = C->mu;
        const CtrlRows rows = ctrl_step_rows(C, k, gi, nz, ne);
        const bool gate = rows.gate;
        const GlobalD Kp = global_table(C->K) + rows.K + t;      // the lane's first entry of the step's first gain row
        const GlobalD Fp = C->Fd ? global_table(C->Fd) + rows.Fd : (GlobalD)0;
        double grav = M->g;
        unsigned long long zd_base = C->zd;
        asm volatile("" : "+s"(zd_base));      // (read with the rest of the record, not on its own where the setpoint row is formed)
        double* const traj_out = ap->traj;
        if (traj_out) {     // Storage row of this step, staged through LDS in user body order so that the HBM stores coalesce
            if (c.live()) {
#pragma unroll
                for (int i = 0; i < 7; i++) L[Y.Z + 13 * ut + i] = S.z[i];
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.Z + 13 * ut + 7 + i] = S.s[i];
            }
        }
        STAMP(PF_IO);
        // ---------------- feedback law (lqr.jl:89-139 / lqr_tracking.jl:46-71)
        double uj = 0.0;
        double zf[13], za[13];
#pragma unroll
        for (int i = 0; i < 7; i++) zf[i] = S.z[i];
#pragma unroll
        for (int i = 0; i < 6; i++) zf[7 + i] = S.s[i];
        from_lane<7>(zf, za, pa4);                      // parent pose (every joint evaluation needs it)
        if (EXTRA) from_lane<6>(zf + 7, za + 7, pa4);   // parent velocities (friction, PID)
        if (!c.has_a()) {
#pragma unroll
            for (int i = 0; i < 13; i++) za[i] = (i == 3) ? 1.0 : 0.0;
        }
        if (gate) {
            if (c.live()) {
                double dz[12], zdv[13];
                const GlobalD zp = global_table(zd_base) + rows.zd + 13 * t;
#pragma unroll
                for (int i = 0; i < 13; i++) zdv[i] = zp[i];
                ck_control_error(zf, zdv, dz);
#pragma unroll
                for (int i = 0; i < 12; i++) L[Y.DZ + 12 * t + i] = dz[i];
                if (EXTRA && (C->flags & CtrlHot::FRIC) && c.has_fric()) uj = ck_friction(c, zf, za);
            }
        }
        // ONE barrier for the staged row and the control error: they lie side by side in the image (Y.Z, Y.DZ), which nothing writes again before the
        // barrier in front of the Newton solve -- the forces phase writes GKA / D / C only
        __syncthreads();
        if (gate) {     // u_i = Fd_i - K_i . dz for the mu inputs (feedback_inputs, cclqr_rollout_step.h)
            constexpr int NE = GainRows<G, NBP>::NE;
            double unoise = 0.0;                    // noise: injected by the caller, or generated for this launch by philox_fill_kernel (rollout_chain.hip)
            if (EXTRA) {
                const double* noise = ap->noise;
                if ((C->flags & CtrlHot::NOISE) && c.valid() && noise) unoise = C->noise_scale * noise[(size_t)inst * ap->noise_stride + (k - 1)];
            }
            double dzv[NE];
            int tf = t;
            asm volatile("" : "+v"(tf));            // the entries' range tests are made here, every step -- not once per launch and kept as NE lane masks
#pragma unroll
            for (int q = 0; q < NE; q++) { const int e = tf + q * G; dzv[q] = (c.valid() && e < ne) ? L[Y.DZ + e] : 0.0; }
            feedback_inputs<G, NBP, EXTRA>(C, Kp, Fp, mu, ne, dzv, unoise, t, uj);
        }
        STAMP(PF_CONTROL);
        asm volatile("" : "+v"(grav));      // the last of the step's loads is waited for HERE, in front of the stores (behind them the wait would be for the stores too)
        if (traj_out) {     // the row leaves behind everything the step had to read: no load waits for the acknowledgement of these stores
            if (c.valid()) {
                int kr = kk, nzr = nz;
                asm volatile("" : "+s"(kr), "+s"(nzr));   // keeps the row address a product computed here (not a running pointer + a 64-bit stride kept in registers)
                double* dst = traj_out + ((size_t)inst * ap->steps + kr) * nzr;
                int e0 = t;
                asm volatile("" : "+v"(e0));      // the loop's entry test is made here, not once per launch and kept as a lane mask
                for (int e = e0; e < nz; e += G) dst[e] = L[Y.Z + e];
            }
        }
        STAMP(PF_IO);
        if (EXTRA >= 2 && (C->flags & CtrlHot::PID)) {
            if (c.live() && CT->pid_on[t]) uj += ck_pid(c, zf, za, CT->pid_P[t], CT->pid_I[t], CT->pid_D[t], CT->pid_goal[t], dt, k == 1, pid_int, pid_last);
        }
        STAMP(PF_CONTROL);
        LINK_FLAGS_FRESH(c);
        // ---------------- joint inputs -> wrenches, per-step invariants, constraint Jacobians at the current knot, force map
        {
            double F[3], tau[3], W6[6], cW6[6];
            ck_joint_wrench(c, uj, zf + 3, za + 3, F, tau, W6, W6 + 3);
            child_sum<6>(T, gb4, maxchild, W6, cW6);
#pragma unroll
            for (int i = 0; i < 3; i++) { F[i] += cW6[i]; tau[i] += cW6[3 + i]; }
            double cTR[6];
            ck_step_invariants(c, zf, F, tau, dt, grav, cTR, cTR + 3);
            double gk[5], kXT[3][3], kPB[5][3], kPA[5][3], lam[5];
            joint_eval_sparse<true>(c, za, za + 3, zf, zf + 3, nullptr, nullptr, gk, kXT, kPB, kPA);
#pragma unroll
            for (int i = 0; i < 5; i++) lam[i] = L[Y.LAM + 5 * t + i];
            if (c.live()) {
                gk_store(t, Y, L, kXT, kPB, kPA);
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.D + 6 * t + i] = cTR[i];
            }
            double own[6], par[6], cpar[6];
            jac_t_apply(c, kXT, kPB, kPA, lam, own, par);
            child_sum<6>(T, gb4, maxchild, par, cpar);
#pragma unroll
            for (int i = 0; i < 6; i++) S.cd[i] = 0.0;
            if (c.live()) {
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.C + 6 * t + i] = own[i] + cpar[i];
            }
        }
        __syncthreads();

        STAMP(PF_FORCES);
        PCOUNT(PF_STEPS);
        // ---------------- newton! (tolerances and line search: SURVEY 8a-bis)
        const bool go = c.valid() && !c.dead();
        bool done = !go, failed = false;
        int its = 0;
        double normf0 = tree_eval<G, true>(c, T, S, t, pa4, maxchild, maxsib, Y, L, 0.0, c.live() && !done, !done, __builtin_huge_val(), __builtin_huge_val(), dt PROF_PASS);
        __syncthreads();
        const int ne_steps = R->ne_steps, nb_steps = R->nb_steps;
        for (int iter = 1; iter <= NEWTON_MAXIT; iter++) {
            if (!__any(!done)) break;
            PCOUNT(PF_NEWTON_ITERS);
            const bool active = c.live() && !done;
            // scheduled no-fill elimination (leaves towards the roots), then the multiplier steps (roots towards the leaves)
            {   // the record of a step is fetched from the tables one step AHEAD (an L2 round trip costs as much as the step's arithmetic)
                const TrRec* rec = &R->el[0][t];
                TrRec K, Kn;
                load_rec(K, rec);
                for (int s = 0; s < ne_steps; s++) {
                    load_rec(Kn, s + 1 < ne_steps ? rec + (s + 1) * TR_LANES : &R->bk[0][t]);
                    if (done) K.ctl = 0;
                    tr_elim(K, L);
                    __syncthreads();
                    K = Kn;
                }
                STAMP(PF_TRI_FWD);
                rec = &R->bk[0][t];
                for (int s = 0; s < nb_steps; s++) {
                    load_rec(Kn, rec + (s + 1 < nb_steps ? s + 1 : s) * TR_LANES);
                    if (done) K.ctl = 0;
                    tr_back(K, L);
                    __syncthreads();
                    K = Kn;
                }
                STAMP(PF_TRI_BWD);
            }
            double nd;
            LINK_FLAGS_FRESH(c);
            {   // multiplier step from LDS, body solve
                double own[6], par[6], cpar[6], dl[5], pdn = 0.0;
#pragma unroll
                for (int r = 0; r < 5; r++) dl[r] = L[Y.DL + 5 * t + r];
                gk_t_apply(c, t, Y, L, dl, own, par);
                child_sum<6>(T, gb4, maxchild, par, cpar);
                if (active) {
                    double DINV[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) DINV[i] = L[Y.DINV + 9 * t + i];
#pragma unroll
                    for (int i = 0; i < 6; i++) S.cd[i] = own[i] + cpar[i];
                    ck_body_solve(c, S.d, S.cd, DINV, S.ds);
#pragma unroll
                    for (int i = 0; i < 6; i++) pdn += S.ds[i] * S.ds[i];
#pragma unroll
                    for (int i = 0; i < 5; i++) pdn += dl[i] * dl[i];
                }
                nd = sqrt(group_sum<G>(pdn));
            }
            __syncthreads();
            STAMP(PF_BODY_SOLVE);
            // line search: halve while ||f|| grows; the full-step trial also evaluates the Jacobians and the Schur blocks (rollout_chain.hip)
            double alpha = 1.0, normf1 = 0.0;
            bool ls_done = done, jac_ok = true;
            {
                const double nf = tree_eval<G, true>(c, T, S, t, pa4, maxchild, maxsib, Y, L, 1.0, active, !done, normf0, nd, dt PROF_PASS);
                if (!ls_done) {
                    normf1 = nf;
                    if (!(normf1 > normf0)) ls_done = true;
                }
            }
            if (G == 32) {
                for (int lv = 1; lv <= LINE_MAXIT;) {
                    if (!__any(!ls_done)) break;
                    const bool mine = !ls_done;
                    const bool other = __shfl_xor(mine ? 1 : 0, 32, 64) != 0;
                    const bool solo = ap->plants != nullptr;      // per-instance plants: no group evaluates the other instance's trial (rollout_chain.hip)
                    const bool helping = !mine && other && !solo;
                    TrialIn Tr;
#pragma unroll
                    for (int i = 0; i < 7; i++) Tr.z[i] = S.z[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) { Tr.s[i] = S.s[i]; Tr.ds[i] = S.ds[i]; Tr.cd[i] = S.cd[i]; }
                    if (mine != other) {
#pragma unroll
                        for (int i = 0; i < 7; i++) { const double o = other_half(S.z[i]); Tr.z[i] = helping ? o : Tr.z[i]; }
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            const double o1 = other_half(S.s[i]), o2 = other_half(S.ds[i]), o3 = other_half(S.cd[i]);
                            Tr.s[i] = helping ? o1 : Tr.s[i]; Tr.ds[i] = helping ? o2 : Tr.ds[i]; Tr.cd[i] = helping ? o3 : Tr.cd[i];
                        }
                    }
                    const double* Lc = helping ? lds + (1 - grp) * total : L;
                    const int l0 = helping ? lv + 2 : lv;
                    double n1, n2;
                    tree_eval2<G>(c, Tr, Lc, t, pa4, Y, ldexp(1.0, -l0), ldexp(1.0, -(l0 + 1)), c.on() && (mine || helping) && l0 <= LINE_MAXIT, dt, n1, n2);
                    PCOUNT(PF_EVALS);
                    const double h1 = other_half(n1), h2 = other_half(n2);
                    if (mine) {
                        const double cand[4] = {n1, n2, h1, h2};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int l = lv + i;
                            if (!ls_done && l <= LINE_MAXIT && (i < 2 || !(other || solo))) {
                                normf1 = cand[i]; alpha = ldexp(1.0, -l); jac_ok = false;
                                if (!(cand[i] > normf0) || l == LINE_MAXIT) ls_done = true;
                            }
                        }
                    }
                    lv += (solo || (mine && other)) ? 2 : 4;
                }
            } else {
                for (int lv = 1; lv <= LINE_MAXIT; lv++) {
                    if (!__any(!ls_done)) break;
                    const double a_l = ldexp(1.0, -lv);
                    const double nf = tree_eval<G, false>(c, T, S, t, pa4, maxchild, maxsib, Y, L, a_l, c.live() && !ls_done, false, 0.0, 0.0, dt PROF_PASS);
                    if (!ls_done) {
                        normf1 = nf; alpha = a_l; jac_ok = false;
                        if (!(nf > normf0) || lv == LINE_MAXIT) ls_done = true;
                    }
                }
            }
            bool need_jac = false;
            if (!done) {
                if (c.live()) {
#pragma unroll
                    for (int i = 0; i < 6; i++) { S.s[i] -= alpha * S.ds[i]; L[Y.C + 6 * t + i] -= alpha * S.cd[i]; S.cd[i] = 0.0; S.ds[i] = 0.0; }
#pragma unroll
                    for (int i = 0; i < 5; i++) L[Y.LAM + 5 * t + i] -= alpha * L[Y.DL + 5 * t + i];
                }
                its = iter;
                if (normf1 < NEWTON_EPS && alpha * nd < NEWTON_EPS) done = true;
                if (RELAX && normf1 < ap->eps_alone) done = true;      // measured-error mode: the residual alone
                if (!(normf1 < 1e300)) { done = true; failed = true; }
                normf0 = normf1;
                need_jac = !done && !jac_ok;
            }
            STAMP(PF_ACCEPT);
            if (__any(need_jac)) tree_eval<G, true>(c, T, S, t, pa4, maxchild, maxsib, Y, L, 0.0, c.live() && need_jac, need_jac, __builtin_huge_val(), __builtin_huge_val(), dt PROF_PASS);
            __syncthreads();
        }
        const bool conv = done && !failed;
        if (go) {
            if (!conv) c.flags |= LinkC::BAD;
            if (its > worst) worst = its;
            if (!conv && its < NEWTON_MAXIT) {   // stopped early on a non-finite residual: freeze the instance at its last pose, at rest
                c.flags |= LinkC::DEAD;
#pragma unroll
                for (int i = 0; i < 6; i++) S.s[i] = 0.0;
            } else if (c.live()) {
                double xq[7];
                ck_next_pose(S.z, S.s, dt, xq);
#pragma unroll
                for (int i = 0; i < 7; i++) S.z[i] = xq[i];
            }
        }
        asm volatile("" : "+s"(ap));
        nsteps = ap->steps;
    }
#ifdef CCLQR_PROFILE
    prof.stamp(PF_IO);
    prof.flush();
#endif
    // ---------------- final state, multipliers, status
    __syncthreads();
    if (c.live()) {
#pragma unroll
        for (int i = 0; i < 7; i++) L[Y.Z + 13 * ut + i] = S.z[i];
#pragma unroll
        for (int i = 0; i < 6; i++) L[Y.Z + 13 * ut + 7 + i] = S.s[i];
    }
    __syncthreads();
    asm volatile("" : "+s"(ap));
    LINK_FLAGS_FRESH(c);
    if (c.valid()) {
        double* zT = ap->zT;
        int* status = ap->status;
        for (int e = t; e < nz; e += G) zT[inst * nz + e] = L[Y.Z + e];
        if (status && t == 0) status[inst] = status_encode(worst, c.bad(), c.dead(), ap->carry);
    }
    if (c.live()) {
        const int nbT = ap->M->nb;
        double* lam = ap->lam;
        if (lam) {
#pragma unroll
            for (int i = 0; i < 5; i++) lam[inst * 5 * nbT + 5 * t + i] = L[Y.LAM + 5 * t + i];
        }
        if (EXTRA >= 2) {
            double* pid_state = ap->pid_state;
            if (pid_state) { pid_state[(inst * nbT + t) * 2] = pid_int; pid_state[(inst * nbT + t) * 2 + 1] = pid_last; }
        }
    }
}

#ifdef CCLQR_PROFILE
extern "C" int cclqr_prof_read_treereg(unsigned long long* out, int reset) {
    return prof_read(out, PF_READ_N, reset);
}
extern "C" int cclqr_prof_read_treereg_n(unsigned long long* out, int cap, int reset) {      // (up to cap words: PF_ROWS_SKIPPED is word 16)
    return prof_read(out, cap, reset);
}
#endif

template <int G, int NBP>
static hipError_t launch_treereg_one(const RolloutArgs& a, ControlLaw law, bool relax, unsigned grid, size_t lds, hipStream_t stream) {
    void (*kern)(RolloutArgs) = nullptr;
    switch (law) {
        case ControlLaw::Lqr: kern = relax ? rollout_treereg_kernel<G, NBP, 0, true> : rollout_treereg_kernel<G, NBP, 0>; break;
        case ControlLaw::FricNoise: kern = rollout_treereg_kernel<G, NBP, 1>; break;
        case ControlLaw::Pid: kern = rollout_treereg_kernel<G, NBP, 2>; break;
        case ControlLaw::PhiloxInKernel: break;      // chains only: a tree's Philox noise is filled into a workspace before the launch (capi.hip)
    }
    if (!kern) return hipErrorInvalidValue;
    return launch_lds(kern, dim3(grid), dim3(64), lds, stream, a);
}

// a.M must be the device image [MechDev | TreeRegDev] of capi.hip (treereg_of)
hipError_t launch_rollout_treereg(const RolloutArgs& a_in, const RolloutShape& s, int simds, ControlLaw law, int newton_mode, hipStream_t stream) {
    RolloutArgs a = a_in;
    a.ipw = spread_instances_per_wavefront(s.full, a.n_inst, a.steps, a_in.ipw != 0, simds);
    const unsigned grid = (unsigned)((a.n_inst + a.ipw - 1) / a.ipw);
    if (grid == 0) return hipSuccess;
    if (s.pid_slots > s.G || s.pid_slots > s.NBP) return hipErrorInvalidValue;      // (a tree has a joint, hence a PID slot, per link)
    const bool relax = newton_mode != 0;      // (the residual-only stop exists under the plain law only: launch_treereg_one)
    if (s.G == 16) return s.NBP == 4 ? launch_treereg_one<16, 4>(a, law, relax, grid, s.lds, stream) : launch_treereg_one<16, 8>(a, law, relax, grid, s.lds, stream);
    if (s.G == 64) return s.NBP == 48 ? launch_treereg_one<64, 48>(a, law, relax, grid, s.lds, stream) : launch_treereg_one<64, 64>(a, law, relax, grid, s.lds, stream);
    switch (s.NBP) {
        case 8: return launch_treereg_one<32, 8>(a, law, relax, grid, s.lds, stream);
        case 10: return launch_treereg_one<32, 10>(a, law, relax, grid, s.lds, stream);
        case 12: return launch_treereg_one<32, 12>(a, law, relax, grid, s.lds, stream);
        case 14: return launch_treereg_one<32, 14>(a, law, relax, grid, s.lds, stream);
        case 16: return launch_treereg_one<32, 16>(a, law, relax, grid, s.lds, stream);
        case 24: return launch_treereg_one<32, 24>(a, law, relax, grid, s.lds, stream);
        default: return launch_treereg_one<32, 32>(a, law, relax, grid, s.lds, stream);
    }
}

}  // namespace cclqr
