// rollout_chain.hip -- the LQR-controlled rollout kernel for forests of chains (all five BASELINE configs), persistent over
// the whole horizon and REGISTER-resident: lane t of an instance's lane group owns link t and keeps its state, multipliers,
// Jacobians and Newton iterate in registers; neighbour links talk through whole-wave DPP shifts; LDS holds only the 5x5
// Schur blocks of the block-tridiagonal solve (cclqr_chain.h).  HBM sees one state load, one gain row per step, one
// trajectory row per step (if recorded) and the final state.
//
// Replaces: ConstrainedDynamics.simulate!/newton! as driven by the reference (examples/lqr_cartpole.jl:44) with
//           control_lqr! (src/control/lqr.jl:89-139) / control_trackinglqr! (src/control/lqr_tracking.jl:46-71).
#ifndef CHAIN_KERNEL_TEXT       // (everything but the kernel's text: see the inclusions below)
#include "cclqr_chain.h"
#include "cclqr_internal.h"
#include "cclqr_newton.h"
#include "cclqr_rollout_step.h"

namespace cclqr {

// lane i <- lane i-1 / lane i+1 of the wavefront (DPP wave shifts; lanes shifted in from outside read 0)
__device__ __forceinline__ double wave_from_prev(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true);   // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_from_next(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);   // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int N>
__device__ __forceinline__ void from_prev(const double* in, double* out) {
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = wave_from_prev(in[i]);
}
template <int N>
__device__ __forceinline__ void from_next(const double* in, double* out) {
#pragma unroll
    for (int i = 0; i < N; i++) out[i] = wave_from_next(in[i]);
}

// ---- the middle link of a TWO-FRONT sweep, solved from registers by the sweep lanes (the 16-, 32- and 64-lane instantiations; cclqr_chain.h has the
// one-lane solve out of LDS, ck_tri_mid, which the 8-lane kernels keep).  When the last sweep step ends, the lanes that ran it hold every word of the
// middle system in their target registers: lane (t & 7) = c < 5 of a front column c of the updated block, lane 5 the right-hand side, and the two
// fronts of an instance share a 16-lane DPP row.  So nothing of it goes through LDS: the two shares are merged by one row rotation (own + row_ror:8
// of the other's -- the same bits in either operand order, and the same as ck_tri_mid's A + (merge ? As : 0.0), the + 0.0 of a plan that does not
// merge included), lane k's column goes to every lane of the row by row_newbcast:k (30 doubles, 60 moves; no ds_bpermute / ds_swizzle, which come
// back through lgkmcnt and would add full drains), and every lane factorises and solves redundantly, as tri_step does.  dl of the middle link is then
// in the registers of the lanes of the first back step (ck_tri_back0_store).
// K: the lane's cursor behind the sweep (K.n = 0 for a lane that takes no part and for a `done` instance); tg: its target registers of the last
// step.  A front that did not run the plan's last step (the shorter one of a plan that does not merge) contributes zeros by a select: its tg is
// stale.  A chain without a sweep step takes front 0's share from the reads of ck_tri_back0_load, behind a wavefront-uniform BRANCH: as a select
// it would make every solve wait for those reads in front of the pivot chain.  Called by ALL lanes in wavefront-uniform control flow (a DPP
// move reads lanes, so none of the row may be masked off); the result is garbage, and unused, outside the sweep lanes of instances that solve.
// B64 (the fixed-plan kernels): each broadcast is ONE 64-bit DPP move (v_mov_b64_dpp; row_newbcast is the control of this kernel that is legal on a
// 64-bit operand) instead of one per dword -- 30 moves for 60 between the last sweep step and the pivot chain.  The same bits land in the same lanes.
template <int CTRL>
__device__ __forceinline__ double dpp_b64(double v) {
    return __longlong_as_double(__builtin_amdgcn_update_dpp(0ll, __double_as_longlong(v), CTRL, 0xf, 0xf, true));
}
template <bool B64 = false>
__device__ __forceinline__ void ck_tri_mid_regs(int t, bool done, const TriPlanB& B, const TriCur& K, const Lay& Y, const double* L, const double* tg, double* dl, TriBack0& Q) {
    const TriPlan& P = B.P;
    ck_tri_back0_load(Q, t, done, B, K, Y, L);
    double m[5];
    const bool ran = K.n == P.steps;
#pragma unroll
    for (int r = 0; r < 5; r++) m[r] = ran ? tg[r] : 0.0;
    if (P.steps == 0) {
        asm volatile("");      // (keeps the branch a branch)
        const bool f0 = (t & 8) == 0;
#pragma unroll
        for (int r = 0; r < 5; r++) m[r] = f0 ? Q.z[r] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 5; r++) m[r] = m[r] + dpp_row_ror<8>(m[r]);      // the other front's lane of the same column
    double A[25];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        if constexpr (B64) {
            A[i * 5 + 0] = dpp_b64<0x150>(m[i]); A[i * 5 + 1] = dpp_b64<0x151>(m[i]); A[i * 5 + 2] = dpp_b64<0x152>(m[i]);
            A[i * 5 + 3] = dpp_b64<0x153>(m[i]); A[i * 5 + 4] = dpp_b64<0x154>(m[i]);
            dl[i] = dpp_b64<0x155>(m[i]);
        } else {
        A[i * 5 + 0] = dpp_f64<0x150>(m[i]); A[i * 5 + 1] = dpp_f64<0x151>(m[i]); A[i * 5 + 2] = dpp_f64<0x152>(m[i]);      // row_newbcast:k
        A[i * 5 + 3] = dpp_f64<0x153>(m[i]); A[i * 5 + 4] = dpp_f64<0x154>(m[i]);
        dl[i] = dpp_f64<0x155>(m[i]);
        }
    }
    lu5_factor(A);
    lu5_solve(A, dl);
}

// ---- the cross-lane part of the Schur rows split by block (cclqr_chain.h ck_schur_rows_split; the 32-lane kernels of at most 17 links): lane 16 + l
// of a group takes a value of lane l.  One swap of DPP rows per dword (v_permlane16_swap_b32 exchanges the odd rows of its first operand with the
// even rows of its second): with both operands the same value, the first result is rows (0, 0, 2, 2) of it and the second rows (1, 1, 3, 3).  A
// vector-ALU instruction: no LDS queue slot, nothing to wait for.  KEEP: lanes with `keep` (lane 16 of a 17-link group, which owns the leaf) hold on
// to their own value, which for a lane of an odd row is the second result.  Called by ALL lanes in wavefront-uniform control flow.
__device__ __forceinline__ auto swap_rows_b32(unsigned first, unsigned second) { return __builtin_amdgcn_permlane16_swap(first, second, false, false); }
// N doubles at a time: the copies that the swaps consume are all made first (one 64-bit move per double), so that no swap reads a register the
// instruction in front of it wrote (which costs two wait states each).
template <bool KEEP, int N>
__device__ __forceinline__ void from_row_below(double* v, bool keep) {
    double cp[N];
#pragma unroll
    for (int i = 0; i < N; i++) { cp[i] = v[i]; asm volatile("" : "+v"(cp[i])); }
#pragma unroll
    for (int i = 0; i < N; i++) {
        const auto a = swap_rows_b32((unsigned)__double2loint(cp[i]), (unsigned)__double2loint(v[i]));
        const auto b = swap_rows_b32((unsigned)__double2hiint(cp[i]), (unsigned)__double2hiint(v[i]));
        const unsigned lo = KEEP ? (keep ? a[1] : a[0]) : a[0], hi = KEEP ? (keep ? b[1] : b[0]) : b[0];
        v[i] = __hiloint2double((int)hi, (int)lo);
    }
}
// group_sum<32> with the two DPP rows of a group combined by the same swap instead of a ds_bpermute: the sum whose result a BRANCH waits for (the
// norm in front of the row block, chain_eval) pays no LDS round trip and no drain of the LDS queue.  The two results of the swap are the sums of
// the group's even and odd row on every lane, where group_sum adds own + other: the same two addends, in either order -- the same bits.
__device__ __forceinline__ double group_sum_rows32(double v) {
    v += dpp_row_ror<8>(v);
    v += dpp_row_ror<4>(v);
    v += dpp_row_ror<2>(v);
    v += dpp_row_ror<1>(v);
    const auto lo = swap_rows_b32((unsigned)__double2loint(v), (unsigned)__double2loint(v));
    const auto hi = swap_rows_b32((unsigned)__double2hiint(v), (unsigned)__double2hiint(v));
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// (as the SUM of feedback_inputs, cclqr_rollout_step.h: the control law's one sum per input and step)
struct GroupSumRows32 { static __device__ __forceinline__ double of(double v) { return group_sum_rows32(v); } };
// ---- the two 32-lane halves of the wavefront exchange values the same way: v_permlane32_swap_b32 exchanges lanes 32-63 of its first operand with
// lanes 0-31 of its second.  With both operands copies of one value, the first result holds the own value on lanes 0-31 and the lower half's on lanes
// 32-63, the second result the upper half's on lanes 0-31 and the own on lanes 32-63.  Called by ALL lanes in wavefront-uniform control flow.
__device__ __forceinline__ auto swap_halves_b32(unsigned first, unsigned second) { return __builtin_amdgcn_permlane32_swap(first, second, false, false); }
// N doubles at a time: out[i] is the first result of v[i]'s swap on the lanes with `first`, the second on the others (v itself is left alone: a swap
// overwrites both its operands).  The two copies that a swap consumes are made ahead of the swaps, as in from_row_below, and the second FROM THE FIRST:
// the iterate lives in accumulation registers, and two reads of it per dword instead of a read and a 64-bit move were 76 instructions more in the
// 17-link kernel and a second value for the allocator to park after its first pass.
template <int N>
__device__ __forceinline__ void halves_pick(const double* v, double* out, bool first) {
    double ca[N], cb[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        ca[i] = v[i]; asm volatile("" : "+v"(ca[i]));
        cb[i] = ca[i]; asm volatile("" : "+v"(cb[i]));
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        const auto a = swap_halves_b32((unsigned)__double2loint(ca[i]), (unsigned)__double2loint(cb[i]));
        const auto b = swap_halves_b32((unsigned)__double2hiint(ca[i]), (unsigned)__double2hiint(cb[i]));
        out[i] = __hiloint2double((int)(first ? b[0] : b[1]), (int)(first ? a[0] : a[1]));
    }
}
// which kernels split the rows, and whether link 0 is without a helper (17 links: lane 16 owns the leaf)
template <int G, int NBP, int KL> struct SchurSplit { static const bool ON = G == 32 && NBP <= 17 && KL == 1, R0 = NBP == 17; };
// once per launch: the helper lanes' flags and scale (schur_split_helper).  M->childl is read at an index below 16.
template <int NBP>
__device__ __forceinline__ void schur_split_setup(LinkC& c, int t, const MechDev* M, int nb) {
    const int l = t & 15;
    const bool help = t >= 16 && !c.on();
    double sl = c.sxb;
    from_row_below<false, 1>(&sl, false);
    if (help) schur_split_helper(c, l < nb && M->childl[l] >= 0, sl);
}
// the helper lanes take wXT and wPB of their link IN PLACE: their own are dead values (they evaluate no joint)
template <bool R0>
__device__ __forceinline__ void schur_split_take(const LinkC& c, int t, double (*wXT)[3], double (*wPB)[3]) {
    const bool keep = R0 && t >= 16 && !c.help();
#pragma unroll
    for (int r = 0; r < 3; r++) from_row_below<R0, 3>(wXT[r], keep);
#pragma unroll
    for (int r = 0; r < 5; r++) from_row_below<R0, 3>(wPB[r], keep);
}

// residual (+ Jacobians when JAC) at the point s - alpha ds with constraint forces C - alpha cd; returns the group's ||f||_2.
// With JAC the Schur complement rows of the point go straight to LDS: W = G_v D^-1 only lives inside this function.
// (The full-step trial is evaluated with JAC on the speculation that it is accepted; if it is not, the accepted point is
// evaluated again, which overwrites these rows.)
// rows: the lane's instance may still read the Schur rows and DINV of this point.  They are built and stored unless NO lane of the wavefront
// says so (a vote: the rows are wavefront-wide work); the residual, the Jacobian code in front of them and the norm are the same either way.
// KL > 1 (several lanes per link, cclqr_chain.h): t is the LINK of the lane (its sub-lane is Q.w); with Jacobians the lane evaluates the rows of its slots only
// and builds their Schur rows, the body's share of the norm comes from the primary sub-lane alone.  KL = 1: the code of rounds 2-4, unchanged.
// SP: the Schur rows are split by block with the lanes sixteen above (1; 2 = in a 17-link group: SchurSplit); inst_on: the lane's instance is evaluated
// (`active` without the lane's own link: what a helper lane stores by).
// SP != 0 only: the norm is formed IN FRONT of the row block, and the lane's `rows` is narrowed by it before the vote (cclqr_chain.h chain_rows_verdict:
// nf0, nd = ||f|| of the point the step started from and the step's norm; + infinity at an accepted point) -- a trial that is rejected, or that ends
// its instance's solve, builds no rows unless the wavefront's other instance needs its own.  The group sum is the same on all 32 lanes of a group, so
// the helper lanes vote as their links' lanes do.  DINV is stored before the norm exists and goes by the caller's `rows`, as jac_ok does there.
template <int G, bool JAC, int KL = 1, int SP = 0>
__device__ __forceinline__ double chain_eval(LinkC& c, LinkS& S, int t, const Lay& Y, double* L, double alpha, bool active, bool inst_on, bool rows, double nf0, double nd, double dt,
                                             const SubSel& Q PROF_ARG) {
    double part = 0.0, nrm = 0.0;
    double NB[9], g[5], xq[7];
    const bool store_dinv = JAC && __any(rows);
    LINK_FLAGS_FRESH(c);
#pragma unroll
    for (int k = 0; k < 7; k++) xq[k] = S.z[k];
    if (active) {
        double cf[6], sv[6], cTR[6], DINV[9];
#pragma unroll
        for (int k = 0; k < 6; k++) { cf[k] = L[Y.C + 6 * t + k] - alpha * S.cd[k]; sv[k] = S.s[k] - alpha * S.ds[k]; cTR[k] = L[Y.D + 6 * t + k]; }
        part = ck_body_eval<JAC>(c, S.z, sv, cf, cTR, cTR + 3, dt, xq, S.d, DINV, NB);
        if (KL > 1 && !c.prim()) part = 0.0;
        if (store_dinv && (KL == 1 || c.prim())) {
#pragma unroll
            for (int k = 0; k < 9; k++) L[Y.DINV + 9 * t + k] = DINV[k];
        }
    }
    STAMP(PF_EVAL_BODY);
    double pxq[7], pNB[9];
    from_prev<7>(xq, pxq);
    if (JAC) from_prev<9>(NB, pNB);
    if (!c.has_a()) {
#pragma unroll
        for (int i = 0; i < 7; i++) pxq[i] = (i == 3) ? 1.0 : 0.0;
    }
    if (JAC && KL > 1) {
        constexpr int NR = SubRows<KL>::NR;
        double gs[NR], sXT[NR][3], sPB[NR][3], sPA[NR][3];
        if (active) {
            joint_eval_rows<KL>(c, Q, pxq, pxq + 3, xq, xq + 3, pNB, NB, gs, sXT, sPB, sPA);
#pragma unroll
            for (int i = 0; i < NR; i++) part += gs[i] * gs[i];
        }
        STAMP(PF_EVAL_JOINT);
        LINK_FLAGS_FRESH(c);
        if (__any(rows)) {
            double pd[6];
            from_prev<6>(S.d, pd);
            // (the next column's operands are requested ahead on the three-lane shape, which has the registers: cartpole 160.0 -> 163.0 M; measured 0 / - 0.3 % on the
            // one-lane 8- and 16-lane kernels -- tracking cfg5, Sawyer -- which therefore keep the plain form)
            ck_schur_rows_sub<KL, (KL == 3)>(c, Q, t, active, Y, L, gs, sXT, sPB, sPA, S.d, pd);
        } else {
            PCOUNT(PF_ROWS_SKIPPED);
        }
        STAMP(PF_SCHUR_S);
    } else {
        double wXT[3][3], wPB[5][3], wPA[5][3];
        if constexpr (JAC && SP != 0) {
            // a lane that evaluates no joint hands whatever its registers hold to the swap (schur_split_take), which overwrites it there: said here, so
            // that the compiler does not set 24 doubles to zero for those lanes first
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) asm volatile("" : "=v"(wXT[r][k]));
#pragma unroll
            for (int r = 0; r < 5; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) asm volatile("" : "=v"(wPB[r][k]));
        }
        if (active) {
            joint_eval_sparse<JAC>(c, pxq, pxq + 3, xq, xq + 3, pNB, NB, g, wXT, wPB, wPA);
            if (KL == 1) {
#pragma unroll
                for (int i = 0; i < 5; i++) part += g[i] * g[i];
            } else {                                     // (residual-only evaluation with several lanes per link: every lane computes all rows, one counts)
                double pj = 0.0;
#pragma unroll
                for (int i = 0; i < 5; i++) pj += g[i] * g[i];
                part += c.prim() ? pj : 0.0;
            }
        }
        STAMP(PF_EVAL_JOINT);
        LINK_FLAGS_FRESH(c);
        if constexpr (JAC && SP != 0) {
            static_assert(G == 32, "the rows are split in 32-lane groups");
            nrm = sqrt(group_sum_rows32(part));
            rows = chain_rows_verdict(rows, nrm, nf0, nd, NEWTON_EPS);
            STAMP(PF_EVAL_MAP);
        }
        if (JAC) {
            if (__any(rows)) {
                double pd[6];
                from_prev<6>(S.d, pd);
                if constexpr (SP != 0) {
                    schur_split_take<SP == 2>(c, t, wXT, wPB);
                    ck_schur_rows_split<SP == 2>(c, t, active, inst_on, Y, L, wXT, wPB, wPA, g, S.d, pd);
                } else {
                    ck_schur_rows(c, t, active, Y, L, wXT, wPB, wPA, g, S.d, pd);
                }
            } else {
                PCOUNT(PF_ROWS_SKIPPED);
            }
            STAMP(PF_SCHUR_S);
        }
    }
    if constexpr (!(JAC && SP != 0)) nrm = sqrt(group_sum<G>(part));
    STAMP(PF_EVAL_MAP);
    PCOUNT(PF_EVALS);
    return nrm;
}

// line search of the 32-lane instantiations (cclqr_rollout_step.h TrialIn): ||f|| of the owning group at the trial points s - a ds (constraint forces C - a cd) for a = a1 and a = a2; Lc = LDS image of the instance
// SP != 0 (the kernels that split the Schur rows): the two sums combine their rows by the swap (group_sum_rows32) -- the accept sequence waits for them
template <int G, int KL = 1, int SP = 0>
__device__ __forceinline__ void chain_eval2(LinkC& c, const TrialIn& T, const double* Lc, int t, const Lay& Y, double a1, double a2, bool active, double dt,
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
    from_prev<7>(xq1, p1);
    from_prev<7>(xq2, p2);
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
    if (KL > 1 && !c.prim()) { part1 = 0.0; part2 = 0.0; }      // (several lanes per link: every lane of a link has evaluated the same residual, one counts)
    if constexpr (SP != 0) {
        static_assert(G == 32, "the rows are split in 32-lane groups");
        n1 = sqrt(group_sum_rows32(part1));
        n2 = sqrt(group_sum_rows32(part2));
    } else {
        n1 = sqrt(group_sum<G>(part1));
        n2 = sqrt(group_sum<G>(part2));
    }
}

// ---- line search of the 8- and 16-lane instantiations (eight / four instances per wavefront): a wavefront pays the LONGEST of its instances'
// searches, and with eight heavy-tailed searches per wavefront somebody nearly always runs deep (53 % of the noise-floor iterations of a
// wavefront of eight see a search go to the 10th halving) while the groups whose search has ended sit idle.  So the idle groups evaluate
// further step lengths of the instances still searching (group_assist below): ||f|| at ONE step length, for any group's lanes, of the
// instance whose trial state is T and whose LDS image is Lc.  Same functions, same order as chain_eval<G, false>.
template <int G, int KL = 1>
__device__ __forceinline__ double chain_eval1(LinkC& c, const TrialIn& T, const double* Lc, int t, const Lay& Y, double a1, bool active, double dt) {
    double part1 = 0.0, xq1[7];
    LINK_FLAGS_FRESH(c);
#pragma unroll
    for (int k = 0; k < 7; k++) xq1[k] = T.z[k];
    if (active) {
        double cf1[6], sv1[6], cTR[6], d1[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            cTR[k] = Lc[Y.D + 6 * t + k];
            cf1[k] = Lc[Y.C + 6 * t + k] - a1 * T.cd[k];
            sv1[k] = T.s[k] - a1 * T.ds[k];
        }
        part1 = ck_body_eval<false>(c, T.z, sv1, cf1, cTR, cTR + 3, dt, xq1, d1, nullptr, nullptr);
    }
    double p1[7];
    from_prev<7>(xq1, p1);
    if (!c.has_a()) {
#pragma unroll
        for (int i = 0; i < 7; i++) p1[i] = (i == 3) ? 1.0 : 0.0;
    }
    if (active) {
        double g1[5];
        joint_eval_sparse<false>(c, p1, p1 + 3, xq1, xq1 + 3, nullptr, nullptr, g1, (double(*)[3]) nullptr, (double(*)[3]) nullptr, (double(*)[3]) nullptr);
#pragma unroll
        for (int i = 0; i < 5; i++) part1 += g1[i] * g1[i];
    }
    if (KL > 1 && !c.prim()) part1 = 0.0;
    return sqrt(group_sum<G>(part1));
}
// value of lane `addr / 4` of the wavefront (ds_bpermute: the LDS crossbar, no memory access)
__device__ __forceinline__ double lane_fetch(double v, int addr) {
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(addr, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(addr, __double2loint(v)));
}

// Counter-based noise (noise_philox): the samples of a launch are generated by this kernel into a workspace and the rollout
// reads them like an injected array -- sqrt/log/cos inside the persistent kernel cost it ~20 scalar registers of polynomial
// constants for its whole lifetime.  sample (instance n, step k) = Box-Muller of Philox-4x32-10 keyed by the GLOBAL instance index.
// Short launches (the step-per-launch / hipGraph form of BASELINE configs[4], cclqr.h CCLQR_PHILOX_INKERNEL_STEPS) generate the sample inside the
// rollout kernel instead (EXTRA = 3): no fill launch in front of every step, no workspace.  ONE compiled body serves both (not inlined), so
// that a sample has the same bits wherever it is generated.
__device__ __attribute__((noinline)) double philox_normal_dev(unsigned key0, unsigned long long instance, int k) { return philox_normal(key0, instance, k); }
__global__ __launch_bounds__(256) void philox_fill_kernel(double* out, unsigned key0, long long inst0, long long n_inst, int k0, int steps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_inst * steps) return;
    const long long n = i / steps;
    const int kk = (int)(i - n * steps);
    out[i] = philox_normal_dev(key0, (unsigned long long)(inst0 + n), k0 + kk);
}
hipError_t launch_philox_fill(double* out, unsigned key0, long long inst0, long long n_inst, int k0, int steps, hipStream_t stream) {
    const long long total = n_inst * steps;
    if (total <= 0) return hipSuccess;
    return launch_lds<false>(philox_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, key0, inst0, n_inst, k0, steps);
}

// NBP: links the LDS image is laid out for (>= nb): a compile-time layout turns every LDS offset into an immediate instead
// of a live scalar register and index arithmetic.
// EXTRA: 0 = plain LQR / TrackingLQR feedback; 1 = + joint friction and noise (examples/trackingLQR_triple_cartpole.jl:93-111);
// 2 = + the PID law of src/control/pid.jl; 3 = 1 with the noise sample of (instance, step) generated HERE (Philox, philox_normal_dev) instead of read
// from an array: the launches of a few steps that a hipGraph replays.  The plain instantiations carry none of that code (nor its registers).
// RELAX: the measured-error Newton mode of cclqr_rollout_opts.newton_mode = 1 -- a solve also stops on ||f|| < eps_alone, whatever the step.  A template
// parameter (plain law only), not a launch argument: the exact-rule kernels sit at 486-502 of 512 registers and any extra live value
// moves them across the line (a scalar mode flag read in the accept phase cost the 17-link instantiations 2 VGPR spills).
// KL, NL: several lanes per link (cclqr_chain.h "SEVERAL LANES PER LINK"): lane t of a group is sub-lane w = t / NL of link tl = t % NL; a mechanism of at most NL
// links whose lane group has KL NL <= G lanes.  KL = 1 (NL = G): one lane per link, the kernels of rounds 2-4, bit for bit.
// ---- The kernel's text follows ONCE in this file and is compiled TWICE: the file includes itself with CHAIN_KERNEL_TEXT defined, which selects the text alone.
// CHAIN_PLAN_FIXED 0: rollout_chain_kernel<G, NBP, EXTRA, RELAX, KL, NL> -- any forest of chains, the plan of the solve read from the plan word on every Newton
// iteration.  CHAIN_PLAN_FIXED 1: rollout_chain_fixed_kernel<NBP, EXTRA, RELAX> (G = 32, KL = 1, NL = 32) -- the mechanisms that are ONE chain over all NBP
// links from link 0 (NBP = 16, 17: RolloutShape::fixed_plan, the N-link cartpole), the chain a constant of the kernel (PlanFixed<NBP>, cclqr_chain.h) instead of
// ~200 scalar selects and lane reads per iteration.  One text, the same functions on the same operands in the same order: the same bits, with the plan's selects
// folded by the compiler.  Two inclusions and the preprocessor -- not one __device__ body with a policy parameter that both kernels call -- because the existing
// kernels' code is pinned (tests/test_chain_*_isa.py): handing the kernel arguments to a function, or restating the lines that read the plan word, moved the
// code of every instantiation.  With CHAIN_PLAN_FIXED 0 the text is what it was.  And in THIS file, not in a file of its own: the source-level rules
// (tests/test_static_kernel_rules.py) and the benchmark's source fingerprint read rollout_chain.hip.
#define CHAIN_KERNEL_TEXT
#define CHAIN_PLAN_FIXED 0
#include "rollout_chain.hip"
#undef CHAIN_PLAN_FIXED
#define CHAIN_PLAN_FIXED 1
#include "rollout_chain.hip"
#undef CHAIN_PLAN_FIXED
#undef CHAIN_KERNEL_TEXT
#else       // CHAIN_KERNEL_TEXT: the kernel's text, for the two inclusions above
#if CHAIN_PLAN_FIXED
template <int NBP, int EXTRA, bool RELAX = false>
__global__ __launch_bounds__(WAVE_BLOCK) void rollout_chain_fixed_kernel(RolloutArgs a)
#else
template <int G, int NBP, int EXTRA, bool RELAX = false, int KL = 1, int NL = G>
__global__ __launch_bounds__(WAVE_BLOCK) void rollout_chain_kernel(RolloutArgs a)
#endif
{
#if CHAIN_PLAN_FIXED
    constexpr int G = 32, KL = 1, NL = 32;
    typedef PlanFixed<NBP> PLAN;
#endif
    extern __shared__ double lds[];
    static_assert(WAVE_BLOCK == 64, "WAVE_HANDOVER orders the phases of ONE wavefront: the workgroup is exactly 64 threads");
    static_assert(KL >= 1 && KL <= 3 && KL * NL <= G && (KL > 1 || NL == G) && (KL == 1 || NL <= NBP), "lane group too small for KL lanes per link");
    const int lane = threadIdx.x, t = lane % G, grp = lane / G;
    const int w = KL > 1 ? t / NL : 0;                      // sub-lane of the lane's link
    const int tl = KL > 1 ? t - NL * w : t;                 // the link the lane works for (LDS slots, tables)
    const int tc = KL > 1 ? (w < KL ? tl : -2) : t;         // ... for comparisons with a link number (no match on a lane without a link)
    const int64_t inst = (int64_t)blockIdx.x * a.ipw + grp;
    const MechDev* M = a.M;
    const CtrlDev* CT = a.C;       // the controller's tables; what a step reads of them is the record C below
    const int nb = M->nb;
    const double dt = M->dt;
    const Lay Y = make_chain_layout(NBP);
    double* L = lds + grp * Y.total;
    const int nz = 13 * nb;

    LinkC c;
    // the lane's link constants, from the records of the plant its instance runs on: the mechanism's own, or -- per-instance plants, a wavefront-uniform
    // branch -- the row of the launch's table (a lane group without an instance reads the first instance's, as it does with controller tables)
    const PlantRec* plant = M->rec;
    const bool have = grp < a.ipw && inst < a.n_inst;      // the lane's instance exists
    if (a.plants) plant = a.plants + ((unsigned)a.plant_off + (have ? (unsigned)inst : 0u)) * (unsigned)nb;      // (a table holds fewer than 2^31 records: cclqr_plants_create)
    link_load_consts_rec(c, M, plant, (KL > 1 && w >= KL) ? CCLQR_MAXL : tl, nb, dt);
    if (KL == 1 || w == 0) c.flags |= LinkC::PRIM;
    constexpr int SP = SchurSplit<G, NBP, KL>::ON ? (SchurSplit<G, NBP, KL>::R0 ? 2 : 1) : 0;
    if constexpr (SP != 0) schur_split_setup<NBP>(c, t, M, nb);
    SubSel Q;
    if (KL > 1) sub_setup<KL>(c, w < KL ? w : 0, Q);
    if (EXTRA && CT->has_fric && c.on()) { c.fric = CT->fric[tl]; if (c.fric != 0.0) c.flags |= LinkC::FRIC; }
    c.set_valid(have);
    const long long ginst = a.inst0 + inst;     // global instance index: selects the controller table when there is one per instance
    const int ut = c.on() ? M->perm[tl] : 0;      // user body index of the owned link
    // The chains of the forest, fetched once: lane ci of the wavefront keeps (start, length) of chain ci, every lane the number of chains
    // (chain_plan_pack, cclqr_chain.h), and the Newton loop reads them with v_readlane instead of going to M->chain_start / M->chain_len (two
    // dependent memory round trips per iteration).  No scalar register holds any of it, and no new vector register: the word shares the register
    // of the lane's user body index (bits 24-29), which the launch keeps anyway.
    // (PlanFixed: the word carries the user body index alone -- nobody reads the chains from it)
    int plan;
#if CHAIN_PLAN_FIXED
    plan = ut << 24;
#else
    {
        const int nch = M->nchains;
        const int cs = M->chain_start[lane], cn = M->chain_len[lane];      // (64 lanes, CCLQR_MAXL = 64 entries: every lane's read is inside the table)
        plan = chain_plan_pack(nch, lane < nch ? cs : 0, lane < nch ? cn : 0) | (ut << 24);
    }
#endif

    LinkS S;
    double pid_int = 0.0, pid_last = 0.0;
#pragma unroll
    for (int i = 0; i < 7; i++) S.z[i] = c.live() ? a.z0[inst * nz + ut * 13 + i] : ((i == 3) ? 1.0 : 0.0);
#pragma unroll
    for (int i = 0; i < 6; i++) S.s[i] = c.live() ? a.z0[inst * nz + ut * 13 + 7 + i] : 0.0;
    if (EXTRA == 2 && a.pid_state && a.k0 > 1 && c.live()) { pid_int = a.pid_state[(inst * nb + tl) * 2]; pid_last = a.pid_state[(inst * nb + tl) * 2 + 1]; }
#pragma unroll
    for (int i = 0; i < 6; i++) { S.cd[i] = 0.0; S.d[i] = 0.0; S.ds[i] = 0.0; }
    // What the Newton phases read before they have written it is the multiplier block only (tests/emu/emu_chain.cpp runs every phase function on an
    // LDS image poisoned with signalling NaNs but for LAM): zero, or the caller's warm start.  Everything else in the image is discarded by a
    // select wherever a phase reads past what was produced (ck_tri_back / cr_back), so it is not cleared: at one step per launch (configs[4]'s
    // graph mode) clearing 601 doubles per instance was 2.3 of the launch's 6.5 us (profiles/r05/launch_overhead.txt).
    if (c.on() && (KL == 1 || c.prim())) {
        const bool warm = c.live() && a.lam && a.k0 > 1;
#pragma unroll
        for (int i = 0; i < 5; i++) L[Y.LAM + 5 * tl + i] = warm ? a.lam[inst * 5 * nb + 5 * tl + i] : 0.0;
    }
    WAVE_HANDOVER();

#ifdef CCLQR_PROFILE
    Prof prof;
    prof.start();
#endif
    int worst = 0;
    // "bad" (a step did not converge) and "dead" (a step produced a non-finite residual; the instance is frozen from then on) are
    // bits of the lane flags, not 64-bit lane masks held in scalar registers through the launch
    if (a.carry && a.status && c.valid()) {      // CCLQR_ROLLOUT_CARRY_STATUS: the launches before this one count (step-per-launch chains)
        const NewtonStatus st = status_decode(a.status[inst]);
        worst = st.worst;
        if (st.bad) c.flags |= LinkC::BAD;
        if (st.dead) c.flags |= LinkC::DEAD;      // lost in an earlier launch: it stays frozen
    }
    // Launch arguments that are only needed once per step or at the end are read from the kernel-argument segment where they are
    // used, through a pointer the optimiser cannot see through, instead of sitting in scalar registers for the whole launch.
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
            if (c.live() && (KL == 1 || c.prim())) {
                LANE_INT_FRESH(plan);
                const int ub = plan >> 24;      // user body index of the owned link
#pragma unroll
                for (int i = 0; i < 7; i++) L[Y.Z + 13 * ub + i] = S.z[i];
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.Z + 13 * ub + 7 + i] = S.s[i];
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
        from_prev<7>(zf, za);                   // parent pose (every joint evaluation needs it)
        if (EXTRA) from_prev<6>(zf + 7, za + 7);   // parent velocities (friction, PID)
        if (!c.has_a()) {
#pragma unroll
            for (int i = 0; i < 13; i++) za[i] = (i == 3) ? 1.0 : 0.0;
        }
        if (gate) {
            if (c.live()) {
                double dz[12], zdv[13];
                const GlobalD zp = global_table(zd_base) + rows.zd + 13 * tl;
#pragma unroll
                for (int i = 0; i < 13; i++) zdv[i] = zp[i];
                ck_control_error(zf, zdv, dz);
                if (KL == 1 || c.prim()) {
#pragma unroll
                    for (int i = 0; i < 12; i++) L[Y.DZ + 12 * tl + i] = dz[i];
                }
                if (EXTRA && (C->flags & CtrlHot::FRIC) && c.has_fric()) uj = ck_friction(c, zf, za);
            }
        }
        // ONE hand-over for the staged row and the control error: they lie side by side in the image (Y.Z, Y.DZ), which nothing writes again before the
        // hand-over in front of the Newton solve -- the forces phase writes GKA / D / C only
        WAVE_HANDOVER();
        if (gate) {     // u_i = Fd_i - K_i . dz for the mu inputs (feedback_inputs, cclqr_rollout_step.h)
            constexpr int NE = GainRows<G, NBP>::NE;
            double unoise = 0.0;                    // noise: injected by the caller, or generated for this launch by philox_fill_kernel
            if (EXTRA == 3) {
                if (C->flags & CtrlHot::NOISE) unoise = C->noise_scale * philox_normal_dev(C->noise_key0, (unsigned long long)gi, k);
            } else if (EXTRA) {
                const double* noise = ap->noise;
                if ((C->flags & CtrlHot::NOISE) && c.valid() && noise) unoise = C->noise_scale * noise[(size_t)inst * ap->noise_stride + (k - 1)];
            }
            double dzv[NE];
            int tf = t;
            asm volatile("" : "+v"(tf));            // the entries' range tests are made here, every step -- not once per launch and kept as NE lane masks
#pragma unroll
            for (int q = 0; q < NE; q++) { const int e = tf + q * G; dzv[q] = (c.valid() && e < ne) ? L[Y.DZ + e] : 0.0; }
            feedback_inputs<G, NBP, EXTRA, std::conditional_t<SP != 0, GroupSumRows32, GroupSum<G>>>(C, Kp, Fp, mu, ne, dzv, unoise, tc, uj);
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
        if (EXTRA == 2 && (C->flags & CtrlHot::PID)) {
            if (c.live() && CT->pid_on[tl]) uj += ck_pid(c, zf, za, CT->pid_P[tl], CT->pid_I[tl], CT->pid_D[tl], CT->pid_goal[tl], dt, k == 1, pid_int, pid_last);
        }
        STAMP(PF_CONTROL);
        LINK_FLAGS_FRESH(c);
        // ---------------- joint inputs -> wrenches, per-step invariants, constraint Jacobians at the current knot, force map
        {
            double F[3], tau[3], W6[6], cW6[6];
            ck_joint_wrench(c, uj, zf + 3, za + 3, F, tau, W6, W6 + 3);
            from_next<6>(W6, cW6);
            if (c.has_c()) {
#pragma unroll
                for (int i = 0; i < 3; i++) { F[i] += cW6[i]; tau[i] += cW6[3 + i]; }
            }
            double cTR[6];
            ck_step_invariants(c, zf, F, tau, dt, grav, cTR, cTR + 3);
            double gk[5], kXT[3][3], kPB[5][3], kPA[5][3], lam[5];
            joint_eval_sparse<true>(c, za, za + 3, zf, zf + 3, nullptr, nullptr, gk, kXT, kPB, kPA);
#pragma unroll
            for (int i = 0; i < 5; i++) lam[i] = L[Y.LAM + 5 * tl + i];
            if (c.live() && (KL == 1 || c.prim())) {
                gk_store(tl, Y, L, kXT, kPB, kPA);
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.D + 6 * tl + i] = cTR[i];
            }
            double own[6], par[6], cpar[6];
            jac_t_apply(c, kXT, kPB, kPA, lam, own, par);
            from_next<6>(par, cpar);
#pragma unroll
            for (int i = 0; i < 6; i++) S.cd[i] = 0.0;
            if (c.live() && (KL == 1 || c.prim())) {
#pragma unroll
                for (int i = 0; i < 6; i++) L[Y.C + 6 * tl + i] = own[i] + (c.has_c() ? cpar[i] : 0.0);
            }
        }
        WAVE_HANDOVER();

        STAMP(PF_FORCES);
        PCOUNT(PF_STEPS);
        // ---------------- newton! (tolerances and line search: SURVEY 8a-bis)
        const bool go = c.valid() && !c.dead();
        bool done = !go, failed = false;
        int its = 0;
        double normf0 = 0.0;
#if CHAIN_PLAN_FIXED
        constexpr int nchains = PLAN::nchains;
#else
        LANE_INT_FRESH(plan);      // (read here, every step: not once per launch and kept in a scalar register)
        const int nchains = chain_plan_count(__builtin_amdgcn_readfirstlane(plan));
#endif
        // ONE evaluation with Jacobians at the accepted point serves the start of the step (every instance that solves: its norm is the
        // solve's first ||f||) and the iterations whose full-step trial was not the point accepted (need_jac, set where the step is accepted)
        bool need_jac = !done;
        for (int iter = 1; iter <= NEWTON_MAXIT; iter++) {
            if (__any(need_jac)) {
                const double nf = chain_eval<G, true, KL, SP>(c, S, tl, Y, L, 0.0, c.live() && need_jac, need_jac, need_jac, __builtin_huge_val(), __builtin_huge_val(), dt, Q PROF_PASS);
                if (iter == 1) normf0 = nf;
            }
            WAVE_HANDOVER();
            if (!__any(!done)) break;
            PCOUNT(PF_NEWTON_ITERS);
            const bool active = c.live() && !done;
            // block-tridiagonal solve along each chain, swept from both ends (cclqr_chain.h)
            for (int ci = 0; ci < nchains; ci++) {
#if CHAIN_PLAN_FIXED
                constexpr int cs = PLAN::cs, cn = PLAN::cn;
                // With the plan a constant, everything the solve derives from the lane number alone (cursors, flags, offsets) is invariant over the launch, and
                // the compiler would keep it in registers that the kernel does not have.  So the solve reads the lane number afresh every iteration, as the
                // run-time kernel reads the plan word: `t` below is this copy (it shadows the kernel's).
                int t_solve = t;
                LANE_INT_FRESH(t_solve);
                const int t = t_solve & (G - 1);      // (the same lane number; said with its range, which the functions below are compiled with: cclqr_chain.h PlanFixed)
#else
                const int pw = __builtin_amdgcn_readlane(plan, ci);
                const int cs = chain_plan_start(pw), cn = chain_plan_len(pw);
#endif
                // long chains: every second link is eliminated first, all at once (cr_level, cclqr_chain.h), and the two-front sweep
                // runs over the half that is left
                constexpr int CRW = 4;
                constexpr bool CR = G == 32 && NBP <= 17;    // 4 lanes for each of up to 8 odd links
                const bool cr = CR && cn >= CR_MIN_LINKS;
                if (CR && cr) {
                    CrLane<CRW> CK;
#if CHAIN_PLAN_FIXED
                    // each pass's arithmetic and stores unfenced, on columns of its own, z of pass B from LDS (cclqr_chain.h cr_level_a): nothing of a pass is
                    // parked in accumulation registers on its way to LDS
                    cr_setup<CRW>(CK, t, cs, cn, 1, Y, done);
                    CR_FLAGS_FRESH(CK);
                    cr_level_a<CRW>(CK, L);
                    WAVE_HANDOVER();
                    CR_FLAGS_FRESH(CK);
                    cr_level_b<CRW>(CK, L);
                    WAVE_HANDOVER();
#else
                    double tc[CrLane<CRW>::NS][5];
                    cr_setup<CRW>(CK, t, cs, cn, 1, Y, done);
                    CR_FLAGS_FRESH(CK);
                    cr_phase_a<CRW>(CK, L, tc);
                    CR_FLAGS_FRESH(CK);
                    cr_store_a<CRW>(CK, L, tc);
                    WAVE_HANDOVER();
                    CR_FLAGS_FRESH(CK);
                    cr_phase_b<CRW>(CK, L, tc);
                    CR_FLAGS_FRESH(CK);
                    cr_store_b<CRW>(CK, L, tc);
                    WAVE_HANDOVER();
#endif
                }
                STAMP(PF_SCHUR_W);
                const TriPlanB PB = cr ? tri_plan_balanced(cs, (cn + 1) / 2, 2) : tri_plan_balanced(cs, cn, 1, G >= 16 ? 2 : 1);
                const TriPlan& P = PB.P;
                TriCur K = tri_cursor(t, PB, Y);
                if (done) K.n = 0;
                if constexpr (G >= 16) {
                    // two fronts: the middle link never goes through LDS.  The last sweep step leaves its update in the sweep lanes' registers, the
                    // middle solve runs there (ck_tri_mid_regs: all lanes, no hand-over in front of it), and the first back step takes dl of the
                    // middle link from the same registers -- two store -> load round trips fewer per Newton iteration on the dependent path
                    double tg[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, dlm[5];
#if CHAIN_PLAN_FIXED
#pragma unroll 1      // (a constant trip count: rolled, as the run-time kernel's loop is)
#endif
                    for (int i = 0; i < P.steps; i++) {
                        double zy[5];
                        int otg = 0, oout = 0;
                        int left = P.steps - 1 - i;
                        LANE_INT_FRESH(left);      // (a per-lane test made here: as a scalar one it has the compiler clone the whole step for the last pass)
                        if (tri_step(K, i, L, tg, zy, &otg, &oout)) tri_step_store_fold(L, otg, oout, tg, zy, left == 0);
                        WAVE_HANDOVER();
                    }
                    STAMP(PF_TRI_FWD);
                    TriBack0 B0;
#if CHAIN_PLAN_FIXED
                    ck_tri_mid_regs<true>(t, done, PB, K, Y, L, tg, dlm, B0);      // (64-bit broadcasts)
#else
                    ck_tri_mid_regs(t, done, PB, K, Y, L, tg, dlm, B0);
#endif
                    ck_tri_back0_store(B0, t, Y, L, dlm);
                    WAVE_HANDOVER();
#if CHAIN_PLAN_FIXED
#pragma unroll 1      // (a constant trip count: rolled, as the run-time kernel's loop is)
#endif
                    for (int j = 1; j < P.steps; j++) {
                        if (!done) ck_tri_back(t, j, PB, Y, L);
                        WAVE_HANDOVER();
                    }
                    // dl of the middle link for the phases behind the solve (cr_back, the body solve, the accept phase): no back step reads it from
                    // LDS, so the five stores queue behind the back substitution, not in front of its first reads
                    if (!done && t == 0) {
#pragma unroll
                        for (int i = 0; i < 5; i++) L[Y.DL + 5 * P.mid + i] = dlm[i];
                    }
                    WAVE_HANDOVER();
                } else {      // 8 lanes: one front, which sweeps to the chain's first link; one lane solves it out of LDS
                    for (int i = 0; i < P.steps; i++) {
                        double tg[5], zy[5];
                        int otg = 0, oout = 0;
                        if (tri_step(K, i, L, tg, zy, &otg, &oout)) tri_step_store(L, otg, oout, tg, zy);
                        WAVE_HANDOVER();
                    }
                    STAMP(PF_TRI_FWD);
                    if (!done) ck_tri_mid<false>(t, PB, Y, L);
                    WAVE_HANDOVER();
                    for (int j = 0; j < P.steps; j++) {
                        if (!done) ck_tri_back(t, j, PB, Y, L);
                        WAVE_HANDOVER();
                    }
                }
                if (CR && cr) {
                    cr_back<CRW>(t, cs, cn, 1, Y, L, done);
                    WAVE_HANDOVER();
                }
                STAMP(PF_TRI_BWD);
            }
            double nd;
            LINK_FLAGS_FRESH(c);
            {   // multiplier step from LDS, body solve
                double own[6], par[6], cpar[6], dl[5], pdn = 0.0;
#pragma unroll
                for (int r = 0; r < 5; r++) dl[r] = L[Y.DL + 5 * tl + r];
                gk_t_apply<true>(c, tl, Y, L, dl, own, par);
                from_next<6>(par, cpar);
                if (active) {
                    double DINV[9];
#pragma unroll
                    for (int i = 0; i < 9; i++) DINV[i] = L[Y.DINV + 9 * tl + i];
#pragma unroll
                    for (int i = 0; i < 6; i++) S.cd[i] = own[i] + (c.has_c() ? cpar[i] : 0.0);
                    ck_body_solve(c, S.d, S.cd, DINV, S.ds);
#pragma unroll
                    for (int i = 0; i < 6; i++) pdn += S.ds[i] * S.ds[i];
#pragma unroll
                    for (int i = 0; i < 5; i++) pdn += dl[i] * dl[i];
                    if (KL > 1 && !c.prim()) pdn = 0.0;
                }
                if constexpr (SP != 0) nd = sqrt(group_sum_rows32(pdn));      // (the trial's row verdict and the accept phase wait for it: no LDS round trip)
                else nd = sqrt(group_sum<G>(pdn));
            }
            WAVE_HANDOVER();
            STAMP(PF_BODY_SOLVE);
            // line search: halve while ||f|| grows.  The first (full-step) trial also evaluates the Jacobians and the Schur blocks,
            // speculating that it is accepted and the solve goes on; later trials evaluate the residual only.
            // An instance whose ||f|| and step are both below eps already is in its last iteration if the trial's ||f|| is below eps too -- alpha nd < eps
            // holds for every alpha <= 1 -- and then nothing reads the rows of the trial: the next step's first evaluation overwrites them.  When
            // every instance of the wavefront that still solves is there, the trial builds none (same code for the residual: the same ||f||); one that
            // goes on after all gets its rows from the evaluation at the top of the next iteration (jac_ok).  (A weaker predictor, ||f|| < eps alone
            // with a residual-only trial, fires in iterations that are not the last: priced in round 3 at 0.5 % of a step, DESIGN_HISTORY.)
            // The kernels that split the rows (SP != 0) ask again inside the trial, once its ||f|| exists (chain_eval, chain_rows_verdict): no rows either for a
            // trial that ends its instance's solve or whose full step is rejected.  jac_ok and DINV go by the predictor here all the same: an instance
            // that is done reads neither, and a rejected full step sets jac_ok = false below.
            double alpha = 1.0, normf1 = 0.0;
            const bool want_rows = !done && !(normf0 < NEWTON_EPS && nd < NEWTON_EPS);
            bool ls_done = done, jac_ok = __any(want_rows);
            {
                const double nf = chain_eval<G, true, KL, SP>(c, S, tl, Y, L, 1.0, active, !done, want_rows, normf0, nd, dt, Q PROF_PASS);
                if (!ls_done) {
                    normf1 = nf;
                    if (!(normf1 > normf0)) ls_done = true;
                }
            }
            if (G == 32) {
                for (int lv = 1; lv <= LINE_MAXIT;) {
                    if (!__any(!ls_done)) break;
                    const bool mine = !ls_done;                                   // uniform over the group
                    bool other;                                                   // the wavefront's other instance is searching too
                    if constexpr (SP != 0) {      // one vote, the other half's bits of it (`mine` is uniform over a half): scalar, no LDS round trip
                        const unsigned long long searching = __ballot(mine);
                        other = (unsigned)(grp != 0 ? searching : searching >> 32) != 0u;
                    } else {
                        other = __shfl_xor(mine ? 1 : 0, 32, 64) != 0;
                    }
                    // per-instance plants: a group holds the constants of its own instance's plant only, so it evaluates no trial of the other instance --
                    // nobody helps, and a searcher advances its own two levels per pass.  Read from the kernel arguments here, not kept through the launch
                    const bool solo = ap->plants != nullptr;
                    const bool helping = !mine && other && !solo;                 // this group's lanes evaluate two more levels of the other's search
                    TrialIn T;
#pragma unroll
                    for (int i = 0; i < 7; i++) T.z[i] = S.z[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) { T.s[i] = S.s[i]; T.ds[i] = S.ds[i]; T.cd[i] = S.cd[i]; }
                    if (mine != other) {       // (symmetric in the two groups: a wavefront-uniform branch) one searches, one helps: hand the trial over
                        if constexpr (SP != 0) {
                            // by half swaps: of a swap's two results the first is the own value on the lower half and the lower half's on the upper, so a
                            // helper of the upper half and a lane of the lower half that keeps its own (the searcher; everybody when solo) take the first
                            const bool first = (grp != 0) == helping;
                            halves_pick<7>(S.z, T.z, first);
                            halves_pick<6>(S.s, T.s, first);
                            halves_pick<6>(S.ds, T.ds, first);
                            halves_pick<6>(S.cd, T.cd, first);
                        } else {
#pragma unroll
                            for (int i = 0; i < 7; i++) { const double o = other_half(S.z[i]); T.z[i] = helping ? o : T.z[i]; }
#pragma unroll
                            for (int i = 0; i < 6; i++) {
                                const double o1 = other_half(S.s[i]), o2 = other_half(S.ds[i]), o3 = other_half(S.cd[i]);
                                T.s[i] = helping ? o1 : T.s[i]; T.ds[i] = helping ? o2 : T.ds[i]; T.cd[i] = helping ? o3 : T.cd[i];
                            }
                        }
                    }
                    const double* Lc = helping ? lds + (1 - grp) * Y.total : L;
                    const int l0 = helping ? lv + 2 : lv;
                    double n1, n2;
                    chain_eval2<G, KL, SP>(c, T, Lc, tl, Y, ldexp(1.0, -l0), ldexp(1.0, -(l0 + 1)), c.on() && (mine || helping) && l0 <= LINE_MAXIT, dt, n1, n2);
                    PCOUNT(PF_EVALS);
                    double h1, h2;                                                // the other half's two norms
                    if constexpr (SP != 0) {
                        const double own[2] = {n1, n2};
                        double oth[2];
                        halves_pick<2>(own, oth, grp != 0);                       // (the lower half's value is the first result on the upper half)
                        h1 = oth[0]; h2 = oth[1];
                    } else {
                        h1 = other_half(n1); h2 = other_half(n2);
                    }
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
                // group assist: the NG = 64 / G groups of the wavefront are dealt to the `count` instances that are still searching -- group g
                // works for the (g mod count)-th of them at level lv + g / count -- so that a pass covers NG / count levels of every search
                // (all of them searching: one level each, as before; one straggler: NG levels at once).  Same accept sequence: the first
                // level that does not grow, level LINE_MAXIT at the latest.
                constexpr int NG = 64 / G;
                for (int lv = 1; lv <= LINE_MAXIT;) {
                    if (!__any(!ls_done)) break;
                    const bool mine = !ls_done;                                                   // uniform over the group
                    const unsigned long long heads = __ballot(mine && t == 0);                    // bit g G: group g is searching
                    // per-instance plants: a group holds its own instance's plant only, so every group works for itself -- the count == NG form below
                    const bool solo = ap->plants != nullptr;
                    const int count = solo ? NG : __builtin_popcountll(heads);                    // >= 1 behind the vote above
                    const int per = NG / count;                                                   // levels of every search this pass (>= 1)
                    const int kq = grp % count, off = grp / count;                                // this group works for the kq-th searcher, level lv + off
                    unsigned long long hm = heads;
                    for (int i = 0; i < kq; i++) hm &= hm - 1;                                    // (kq < count: the kq-th set bit exists)
                    const int src = solo ? grp : __builtin_ctzll(hm) / G;                         // that searcher's group
                    int myrank = 0;                                                               // rank of this group among the searchers
                    for (int g2 = 0; g2 < NG; g2++) myrank += (g2 < grp && ((heads >> (g2 * G)) & 1ull)) ? 1 : 0;
                    const int l0 = lv + off;
                    const bool work = off < per && l0 <= LINE_MAXIT;
                    const int fa = (src * G + t) * 4;
                    TrialIn T;
#pragma unroll
                    for (int i = 0; i < 7; i++) T.z[i] = S.z[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) { T.s[i] = S.s[i]; T.ds[i] = S.ds[i]; T.cd[i] = S.cd[i]; }
                    if (count < NG) {                                                             // (uniform) somebody has lanes to spare: hand the trials over
#pragma unroll
                        for (int i = 0; i < 7; i++) T.z[i] = lane_fetch(S.z[i], fa);
#pragma unroll
                        for (int i = 0; i < 6; i++) { T.s[i] = lane_fetch(S.s[i], fa); T.ds[i] = lane_fetch(S.ds[i], fa); T.cd[i] = lane_fetch(S.cd[i], fa); }
                    }
                    const double nf = chain_eval1<G, KL>(c, T, lds + src * Y.total, tl, Y, ldexp(1.0, -l0), c.on() && work, dt);
                    PCOUNT(PF_EVALS);
                    if (count == NG) {                                                            // (uniform) everybody searches: one level each, the group's own result
                        if (mine) {
                            normf1 = nf; alpha = ldexp(1.0, -lv); jac_ok = false;
                            if (!(nf > normf0) || lv == LINE_MAXIT) ls_done = true;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NG; i++) {                                            // the searcher collects its levels in order
                            const double ci = lane_fetch(nf, ((myrank + i * count) % NG) * G * 4);
                            const int l = lv + i;
                            if (mine && !ls_done && i < per && l <= LINE_MAXIT) {
                                normf1 = ci; alpha = ldexp(1.0, -l); jac_ok = false;
                                if (!(ci > normf0) || l == LINE_MAXIT) ls_done = true;
                            }
                        }
                    }
                    lv += per;
                }
            }
            need_jac = false;
            if (!done) {
                if (c.live()) {
                    if (KL == 1) {
#pragma unroll
                        for (int i = 0; i < 6; i++) { S.s[i] -= alpha * S.ds[i]; L[Y.C + 6 * t + i] -= alpha * S.cd[i]; S.cd[i] = 0.0; S.ds[i] = 0.0; }
#pragma unroll
                        for (int i = 0; i < 5; i++) L[Y.LAM + 5 * t + i] -= alpha * L[Y.DL + 5 * t + i];
                    } else {      // every lane of a link moves its own copy of the iterate; the link's LDS slots are the primary lane's to update
#pragma unroll
                        for (int i = 0; i < 6; i++) { S.s[i] -= alpha * S.ds[i]; if (c.prim()) L[Y.C + 6 * tl + i] -= alpha * S.cd[i]; S.cd[i] = 0.0; S.ds[i] = 0.0; }
                        if (c.prim()) {
#pragma unroll
                            for (int i = 0; i < 5; i++) L[Y.LAM + 5 * tl + i] -= alpha * L[Y.DL + 5 * tl + i];
                        }
                    }
                }
                its = iter;
                if (normf1 < NEWTON_EPS && alpha * nd < NEWTON_EPS) done = true;
                if (RELAX && normf1 < ap->eps_alone) done = true;      // measured-error mode: the residual alone
                if (!(normf1 < 1e300)) { done = true; failed = true; }   // non-finite residual: the instance has left the domain of the integrator
                normf0 = normf1;
                need_jac = !done && !jac_ok;
            }
            STAMP(PF_ACCEPT);
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
        nsteps = ap->steps;      // read again rather than kept in a scalar register through the step
    }
#ifdef CCLQR_PROFILE
    prof.stamp(PF_IO);
    prof.flush();
#endif
    // ---------------- final state, multipliers, status
    WAVE_HANDOVER();
    if (c.live() && (KL == 1 || c.prim())) {
        const int ub = plan >> 24;
#pragma unroll
        for (int i = 0; i < 7; i++) L[Y.Z + 13 * ub + i] = S.z[i];
#pragma unroll
        for (int i = 0; i < 6; i++) L[Y.Z + 13 * ub + 7 + i] = S.s[i];
    }
    WAVE_HANDOVER();
    asm volatile("" : "+s"(ap));
    LINK_FLAGS_FRESH(c);
    if (c.valid()) {
        double* zT = ap->zT;
        int* status = ap->status;
        for (int e = t; e < nz; e += G) zT[inst * nz + e] = L[Y.Z + e];
        if (status && t == 0) status[inst] = status_encode(worst, c.bad(), c.dead(), ap->carry);
    }
    if (c.live() && (KL == 1 || c.prim())) {
        const int nbT = ap->M->nb;      // read again here rather than kept in a scalar register through the launch
        double* lam = ap->lam;
        if (lam) {
#pragma unroll
            for (int i = 0; i < 5; i++) lam[inst * 5 * nbT + 5 * tl + i] = L[Y.LAM + 5 * tl + i];
        }
        if (EXTRA == 2) {
            double* pid_state = ap->pid_state;
            if (pid_state) { pid_state[(inst * nbT + tl) * 2] = pid_int; pid_state[(inst * nbT + tl) * 2 + 1] = pid_last; }
        }
    }
}
#endif      // CHAIN_KERNEL_TEXT
#ifndef CHAIN_KERNEL_TEXT

#ifdef CCLQR_PROFILE
extern "C" int cclqr_prof_read_chain(unsigned long long* out, int reset) {
    return prof_read(out, PF_READ_N, reset);
}
extern "C" int cclqr_prof_read_chain_n(unsigned long long* out, int cap, int reset) {      // (up to cap words: PF_ROWS_SKIPPED is word 16)
    return prof_read(out, cap, reset);
}
#endif

template <int G, int NBP, int KL = 1, int NL = G>
static hipError_t launch_chain_one(const RolloutArgs& a, ControlLaw law, bool relax, bool fixed, unsigned grid, size_t lds, hipStream_t stream) {
    void (*kern)(RolloutArgs) = nullptr;
    switch (law) {
        case ControlLaw::Lqr: kern = relax ? rollout_chain_kernel<G, NBP, 0, true, KL, NL> : rollout_chain_kernel<G, NBP, 0, false, KL, NL>; break;
        case ControlLaw::FricNoise: kern = rollout_chain_kernel<G, NBP, 1, false, KL, NL>; break;
        case ControlLaw::Pid: kern = rollout_chain_kernel<G, NBP, 2, false, KL, NL>; break;
        case ControlLaw::PhiloxInKernel: kern = rollout_chain_kernel<G, NBP, 3, false, KL, NL>; break;
    }
    if constexpr (G == 32 && (NBP == 16 || NBP == 17) && KL == 1) {
        if (fixed) {      // one full-length chain: the same kernel with the plan compiled in
            switch (law) {
                case ControlLaw::Lqr: kern = relax ? rollout_chain_fixed_kernel<NBP, 0, true> : rollout_chain_fixed_kernel<NBP, 0, false>; break;
                case ControlLaw::FricNoise: kern = rollout_chain_fixed_kernel<NBP, 1, false>; break;
                case ControlLaw::Pid: kern = rollout_chain_fixed_kernel<NBP, 2, false>; break;
                case ControlLaw::PhiloxInKernel: kern = rollout_chain_fixed_kernel<NBP, 3, false>; break;
            }
        }
    } else if (fixed) {
        return hipErrorInvalidValue;      // (no fixed-plan kernel of this shape: rollout_shape_of never says so)
    }
    if (!kern) return hipErrorInvalidValue;
    return launch_lds(kern, dim3(grid), dim3(WAVE_BLOCK), lds, stream, a);      // (one wavefront: what WAVE_HANDOVER rests on)
}

hipError_t launch_rollout_chain(const RolloutArgs& a_in, const RolloutShape& s, int simds, ControlLaw law, int newton_mode, bool runtime_plan, hipStream_t stream) {
    RolloutArgs a = a_in;
    a.ipw = spread_instances_per_wavefront(s.full, a.n_inst, a.steps, a_in.ipw != 0, simds);
    const unsigned grid = (unsigned)((a.n_inst + a.ipw - 1) / a.ipw);
    if (grid == 0) return hipSuccess;
    {   // the reduction level's back substitution reads DL / R of one link past the chain and selects the value away (cclqr_chain.h cr_back): that
        // read must stay inside the instance's image whatever order a later re-cut of the layout puts the arrays in
        const Lay Y = make_chain_layout(s.NBP);
        if (Y.DL + 5 * (s.NBP + 1) > Y.total || Y.R + 5 * (s.NBP + 1) > Y.total) return hipErrorInvalidValue;
        // the middle solve reads the scratch block (25 + 5 words) of every plan of the 16- and 32-lane instantiations, merging or not, and selects it away (ck_tri_mid): furthest out
        // for a one-link chain that is the forest's last link
        const TriPlanB B = tri_plan_balanced(s.NBP - 1, 1);
        if (tri_scratch_S(B, Y) + 25 > Y.total || tri_scratch_R(B, Y) + 5 > Y.total) return hipErrorInvalidValue;
    }
    const bool relax = newton_mode != 0;      // (the residual-only stop exists under the plain law only: launch_chain_one)
    const bool fixed = chain_launch_fixed_plan(s, runtime_plan);
    switch (s.NBP) {
        case 4: return s.KL == 3 ? launch_chain_one<8, 4, 3, 2>(a, law, relax, fixed, grid, s.lds, stream) : launch_chain_one<8, 4>(a, law, relax, fixed, grid, s.lds, stream);
        case 8: return launch_chain_one<16, 8>(a, law, relax, fixed, grid, s.lds, stream);
        case 16: return launch_chain_one<32, 16>(a, law, relax, fixed, grid, s.lds, stream);
        case 17: return launch_chain_one<32, 17>(a, law, relax, fixed, grid, s.lds, stream);
        case 32: return launch_chain_one<32, 32>(a, law, relax, fixed, grid, s.lds, stream);
        default: return launch_chain_one<64, 64>(a, law, relax, fixed, grid, s.lds, stream);
    }
}

}  // namespace cclqr
#endif      // !CHAIN_KERNEL_TEXT
