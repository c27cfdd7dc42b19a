// score.hip -- cclqr_rollout_score: the LQR cost, peak stage cost and last step outside a tolerance of every instance of a recorded slab, as a
// reduction on the device.  A streaming kernel of its own: the rollout kernels have no register to spare for it.
//
// A lane group of G = 8 / 16 / 32 / 64 lanes owns one instance, SCORE_WAVES wavefronts share the weights' blocks in LDS.  Per step the group
//   1. stages the 13 nb row it requested one step earlier in LDS (entries t, t + G, ...: coalesced) and requests the next step's row,
//   2. lane t < nb forms link t's error about the step's setpoint and its dz' Qb dz (cclqr_score.h), and publishes dz in link order,
//   3. with the feedback gate on, the group forms du_i = -K_i . dz for the mu inputs (gain rows read as the rollout's control phase reads them),
//   4. sums the stage costs over the group (xor butterfly: every lane holds the same bits) and accumulates them in step order.
// Every cross-lane operation (the butterflies, the wave barriers) sits under control flow that depends on launch arguments and controller constants only.
#include "cclqr_internal.h"
#include "cclqr_score.h"

namespace cclqr {

#define SCORE_WAVES 4

template <int G>
__device__ __forceinline__ double score_group_sum(double v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// row, dz and du of an instance are private to ONE lane group of ONE wavefront: what orders a lane's LDS writes before its neighbours' reads is the wavefront's own
// instruction order (LDS operations of a wavefront complete in issue order) -- the fences keep the compiler from moving LDS accesses across the point, no other
// wavefront is waited for
__device__ __forceinline__ void score_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__global__ __launch_bounds__(64 * SCORE_WAVES) void score_kernel(ScoreArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G;      // instances per wavefront
    const int nb = a.nb, mu = a.mu, nz = 13 * nb, ne = 12 * nb;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G;
    double* Qs = lds;                // block of link l at SCORE_QB_STRIDE l: an odd stride, so that the body lanes' reads of one entry fall on distinct banks
#pragma unroll 4
    for (int e = tid; e < 144 * nb; e += 64 * SCORE_WAVES) Qs[(e / 144) * SCORE_QB_STRIDE + e % 144] = a.Qb[e];
    double* row = lds + SCORE_QB_STRIDE * nb + (size_t)(wave * IPW + grp) * score_instance_doubles(nb, mu);
    double* DZ = row + nz;
    double* DU = DZ + ne;
    const long long inst_raw = ((long long)blockIdx.x * SCORE_WAVES + wave) * IPW + grp;
    const bool valid = inst_raw < a.n_inst;
    const long long inst = valid ? inst_raw : a.n_inst - 1;      // (a lane group without an instance scores the last one again; its result is never written)
    const long long gi = a.inst0 + inst;
    const bool body = t < nb;
    const int ut = body ? a.M->perm[t] : 0;                      // the caller's body that link t is

    double s[CCLQR_SCORE_LEN_];
    score_init(s);
    if (a.k0 > 1) {
#pragma unroll
        for (int i = 0; i < CCLQR_SCORE_LEN_; i++) s[i] = a.score[inst * CCLQR_SCORE_LEN_ + i];
    }
    // the controller's record is launch-invariant: ONE read, the fields the rows are formed from stay in registers (ctrl_step_rows then loads nothing per step)
    CtrlHot H;
    {
        const CtrlHot* Hg = &a.C->hot;
        H.K = Hg->K; H.zd = Hg->zd; H.Fd = 0;
        H.K_stride = Hg->K_stride; H.zd_stride = Hg->zd_stride; H.Fd_stride = 0;
        H.nK = Hg->nK; H.N = Hg->N; H.nsp = Hg->nsp; H.mu = Hg->mu;
    }
    const double* Ktab = (const double*)(uintptr_t)H.K;
    const double* zdtab = (const double*)(uintptr_t)H.zd;
    const bool has_K = Ktab != nullptr && H.nK > 0 && mu > 0;
    const int steps = a.steps, k0 = a.k0;
    const double* p = a.traj + inst * (long long)steps * nz;

    // the first step's row and setpoint row; from then on both are requested one step ahead (the setpoint row only when it changes: never, nsp = 1)
    double nxt[CCLQR_SCORE_ROW_LOADS], zd[13], zdn[13];
#pragma unroll
    for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; nxt[j] = (e < nz) ? p[e] : 0.0; }
    long long zoff = ctrl_step_rows(&H, k0, gi, nz, ne).zd;
#pragma unroll
    for (int i = 0; i < 13; i++) { zd[i] = body ? zdtab[zoff + 13 * t + i] : 0.0; zdn[i] = zd[i]; }
    __syncthreads();      // the weights are staged (the one point where the workgroup's wavefronts meet)
    for (int kk = 0; kk < steps; kk++) {
        const int k = k0 + kk;
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = nxt[j]; }
#pragma unroll
        for (int i = 0; i < 13; i++) zd[i] = zdn[i];
        const CtrlRows rows = ctrl_step_rows(&H, k, gi, nz, ne);
        if (kk + 1 < steps) {      // the next step's rows are on their way while this one is reduced
            const double* pn = p + (long long)(kk + 1) * nz;
#pragma unroll
            for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) nxt[j] = pn[e]; }
            const long long znext = ctrl_step_rows(&H, k + 1, gi, nz, ne).zd;
            if (znext != zoff) {
                if (body) {
#pragma unroll
                    for (int i = 0; i < 13; i++) zdn[i] = zdtab[znext + 13 * t + i];
                }
                zoff = znext;
            }
        }
        score_wave_sync();
        double cxb = 0.0;
        if (body) {
            double z[13], dz[12];
#pragma unroll
            for (int i = 0; i < 13; i++) z[i] = row[13 * ut + i];
            score_body_error(z, zd, dz);
            cxb = score_body_cost(dz, Qs + SCORE_QB_STRIDE * t);
#pragma unroll
            for (int i = 0; i < 12; i++) DZ[12 * t + i] = dz[i];
        }
        const double cx = score_group_sum<G>(cxb);
        double cu = 0.0;
        if (rows.gate && has_K) {
            score_wave_sync();
            const double* Kp = Ktab + rows.K;
            for (int i = 0; i < mu; i++) {
                const double du = -score_group_sum<G>(score_gain_partial(t, G, ne, Kp + (size_t)i * ne, DZ));
                if (t == 0) DU[i] = du;
            }
            score_wave_sync();
            cu = score_group_sum<G>(score_input_cost_partial(t, G, mu, a.R, DU));
        }
        score_accumulate(s, cx, cu, k, a.settle_tol);
        score_wave_sync();      // the next step overwrites the row, dz and du
    }
    if (valid && t == 0) {
#pragma unroll
        for (int i = 0; i < CCLQR_SCORE_LEN_; i++) a.score[inst * CCLQR_SCORE_LEN_ + i] = s[i];
    }
}

hipError_t launch_score(const ScoreArgs& a, hipStream_t stream) {
    const int G = score_group_lanes(a.nb);
    const long long per_block = (long long)SCORE_WAVES * (64 / G);
    const dim3 grid((unsigned)((a.n_inst + per_block - 1) / per_block)), block(64 * SCORE_WAVES);
    const size_t lds = score_lds_bytes(a.nb, a.mu, SCORE_WAVES);
    switch (G) {
        case 8: return launch_lds(score_kernel<8>, grid, block, lds, stream, a);
        case 16: return launch_lds(score_kernel<16>, grid, block, lds, stream, a);
        case 32: return launch_lds(score_kernel<32>, grid, block, lds, stream, a);
        default: return launch_lds(score_kernel<64>, grid, block, lds, stream, a);
    }
}

}  // namespace cclqr
