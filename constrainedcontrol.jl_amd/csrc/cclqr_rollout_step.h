// cclqr_rollout_step.h -- what the chain kernel (rollout_chain.hip) and the branching-tree kernel (rollout_treereg.hip) share of a rollout step:
// the per-lane state of the owned link, the trial point a lane group hands to another in the line search, and the feedback law's memory side -- the
// controller's hot record read through the constant address space, its tables as global memory, the gain rows of a step.  Device only; included by
// those two kernels alone.
#pragma once
#include "cclqr_chain.h"
#include "cclqr_newton.h"

namespace cclqr {

// ---- hand-over of the LDS image from one phase of a step to the next, for kernels whose workgroup is ONE wavefront (WAVE_BLOCK threads).
// Sufficient because the LDS executes one wavefront's instructions in issue order: a read issued behind a store sees the stored data whichever lane
// stored it, and a store issued behind a read cannot overtake it.  So the hand-over is a compiler ordering point only -- a wavefront-scope fence emits
// no instruction and no memory operation is moved across it -- where __syncthreads() also drains the LDS queue (s_waitcnt lgkmcnt(0)) before the
// next phase may issue its first read.  Kernels with more than one wavefront per workgroup need the real barrier and never use this.
// Nothing on the host, where builds of these headers run one lane at a time.  (An inlined function, not the builtin written in place: the two compile to
// different schedules of the headline kernel -- 72 full drains and 9 176 instructions this way, 73 and 9 193 the other -- and this one is the one measured.)
constexpr int WAVE_BLOCK = 64;
__device__ __forceinline__ void wave_handover() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#endif
}
#define WAVE_HANDOVER() wave_handover()

// dynamic per-lane data of the owned link.  The velocity part of the state is s itself: the solution (v+, w+) of one step is
// the state's (v, w) at the next knot and the Newton start of the next step.
struct LinkS {
    double z[7], s[6];
    double ds[6], cd[6], d[6];
};

// ---- line search of the 32-lane instantiations (two instances per wavefront): TWO step lengths per pass in a group's own lanes, and when
// only ONE of the wavefront's two instances is still searching the other group's idle lanes evaluate two more for it.  The noise-floor
// searches of the exact stopping rule are heavy-tailed (9 % of them run to the 10th halving), and a wavefront pays the longer of its two:
// the accept sequence -- first level that does not grow, level LINE_MAXIT at the latest -- and every bit of the result are unchanged.
// TrialIn is the trial point handed over (the chain's 8- and 16-lane group assist hands it to any group).
struct TrialIn { double z[7], s[6], ds[6], cd[6]; };
__device__ __forceinline__ double other_half(double v) { return __shfl_xor(v, 32, 64); }

// ---- the controller as a step reads it: the record CtrlDev::hot (cclqr_dev.h) through the CONSTANT address space -- a uniform read of it is a
// scalar load, the fields a step needs come in one wide one, and they are read where they are used (behind an opaque copy of the pointer, as the
// launch arguments are) instead of living in scalar registers through the launch.  The tables the record points at are GLOBAL memory and typed so:
// the rows of a step come out as global_load (counted by vmcnt alone; a flat_load also ties its wait to lgkmcnt).
typedef const __attribute__((address_space(4))) CtrlHot* CtrlHotK;
typedef const __attribute__((address_space(1))) double* GlobalD;
__device__ __forceinline__ CtrlHotK ctrl_hot_of(const CtrlDev* C) { return (CtrlHotK)(uintptr_t)&C->hot; }
__device__ __forceinline__ GlobalD global_table(unsigned long long base) { return (GlobalD)(uintptr_t)base; }

// ---- the gain rows of a step.  u_i = Fd_i - K_i . dz for the mu inputs: the gain entries of a lane -- NE per input, read from HBM / L2 -- are ALL
// requested before the first one is used, CH inputs at a time, together with the inputs' feed-forward values: as a loop "load, multiply-add, next
// entry" every entry paid its own memory round trip (6 round trips per input and lane; 25 % of a step of the seven-input Sawyer arm, 2.4 % of the
// headline's).  No predicate lives across the loads (each would be a 64-bit lane mask in scalar registers): an entry past the end of a row is
// fetched all the same -- it is the next row's, or the zero padding behind the table (CCLQR_K_PAD) -- and meets a zero in dz.
// (The rows live inside the loop over the inputs and are requested behind the barrier that publishes dz: requested at the top of the step, with the
// setpoint row, they are live across the whole control phase -- 14 to 112 registers that the 16- and 32-lane kernels do not have)
template <int G, int NBP>
struct GainRows {
    static constexpr int NE = (12 * NBP + G - 1) / G;
    static constexpr int CH = (G == 16) ? 8 : 1;       // (16 lanes = 5 .. 8 links: the multi-input arms, all their inputs at once; the others usually have one input)
    double kv[CH][NE], fd[CH];
    // Kp: the lane's first entry of the step's first row; Fp: the step's feed-forward row (null: none); inputs i0 .. i0 + CH - 1 (clamped to mu, uniform)
    __device__ __forceinline__ void request(GlobalD Kp, GlobalD Fp, int i0, int mu, int ne) {
#pragma unroll
        for (int j = 0; j < CH; j++) {
            const int ij = (i0 + j < mu) ? i0 + j : i0;
#pragma unroll
            for (int q = 0; q < NE; q++) kv[j][q] = Kp[(size_t)ij * ne + q * G];
            fd[j] = Fp ? Fp[ij] : 0.0;
        }
    }
};
// adds to uj the joint input of the lane whose link number is tc (-2: none) under the record C; Kp = the lane's first entry of the step's first gain
// row, Fp = the step's feed-forward row (null: none), dzv = the lane's NE entries of the control error.  Same products, same order of summation
// as one input at a time.  SUM::of: the sum over the lanes of a group (a kernel may bring its own form of group_sum<G>: same addends, same bits).
template <int G> struct GroupSum { static __device__ __forceinline__ double of(double v) { return group_sum<G>(v); } };
template <int G, int NBP, int EXTRA, class SUM = GroupSum<G>>
__device__ __forceinline__ void feedback_inputs(CtrlHotK C, GlobalD Kp, GlobalD Fp, int mu, int ne, const double* dzv, double unoise, int tc, double& uj) {
    constexpr int NE = GainRows<G, NBP>::NE, CH = GainRows<G, NBP>::CH;
    if (C->K) {                                  // (uniform) LQR / TrackingLQR
        for (int i0 = 0; i0 < mu; i0 += CH) {
            GainRows<G, NBP> rows;
            int cjv[CH];
            rows.request(Kp, Fp, i0, mu, ne);
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const bool ok = i0 + j < mu;         // (uniform)
                const int ij = ok ? i0 + j : i0;
                cjv[j] = ok ? ctrl_hot_cj(C->cj4[ij >> 2], ij) : -1;
            }
#pragma unroll
            for (int j = 0; j < CH; j++) {
                double part = 0.0;
#pragma unroll
                for (int q = 0; q < NE; q++) part += rows.kv[j][q] * dzv[q];
                const double s = SUM::of(part);
                double u = rows.fd[j] - s;
                if (EXTRA) u += unoise;
                if (tc == cjv[j]) uj += u;
            }
        }
    } else {                                     // feed-forward only (OpenLoop, a host closure's inputs)
        for (int i = 0; i < mu; i++) {
            double u = Fp ? Fp[i] : 0.0;
            if (EXTRA) u += unoise;
            if (tc == ctrl_hot_cj(C->cj4[i >> 2], i)) uj += u;
        }
    }
}

}  // namespace cclqr
