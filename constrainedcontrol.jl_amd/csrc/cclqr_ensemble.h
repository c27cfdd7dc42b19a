// cclqr_ensemble.h -- the statistics of a batch ACROSS its instances at every row of a recorded slab (cclqr_rollout_ensemble, ensemble.hip): per
// step the mean and the centred sum of squares of every coordinate of x = (dz, du) -- dz the error of lqr.jl:92-103 about the step's setpoint, du = -K dz the
// feedback command of lqr.jl:105-113 under its gate -- and, at the steps the caller lists, the centred co-moment matrix of dz.  The per-row and per-tile arithmetic
// lives here as __host__ __device__ functions so that tests/emu/emu_ensemble.cpp runs it lane by lane on the CPU (test infrastructure only).  None of them contains
// a cross-lane operation: they are called under lane predicates (the rule of tests/test_static_kernel_rules.py); the two __device__ helpers ens_group_sum and
// ens_wave_sync, which are nothing else, are marked as such below.
//
// The ONE summation order, a function of n_inst and of the mechanism alone (never of steps, k0, the chunk or the order workgroups finish in):
//   tile  = ENS_TILE consecutive instances, the last tile short;
//   pass  = ens_pass_instances(nb) consecutive instances of a tile, the last pass of the last tile short: its partial is the two-pass (mean, M2) about the pass's
//           first value (ens_pass_partial);
//   a tile's partial = its passes' partials merged in pass order (ens_merge, the pairwise formula of Chan, Golub and LeVeque);
//   the result       = the tiles' partials merged in tile order (ens_finish_kernel).
#pragma once
#include "cclqr_score.h"

namespace cclqr {

#define ENS_WAVES 4
#define ENS_TILE 64           // instances of one workgroup of the moments kernel
#define ENS_COORDS 4          // coordinates per thread of its reduction stage: 12 * 64 + 64 <= ENS_COORDS * 64 * ENS_WAVES
#define ENS_MAX_COV 64        // listed steps of ONE launch (they travel in the kernel's arguments)
#define ENS_KSPLIT 1024       // instances of one K-split of the co-moment kernel

struct EnsArgs {
    const MechDev* M;
    const CtrlDev* C;
    int nb, mu;
    long long n_inst;
    int steps, k0;
    long long inst0;          // global index of instance 0 (the controller table of an instance is keyed by its global index)
    const double* traj;       // [n_inst][steps][nb][13] caller's body order
    double* part;             // [steps][ntiles][2][nx]: mean, M2 of a tile, coordinates in OUTPUT order (dz in the caller's body order, then du)
    double* dzrows;           // [n_cov][n_inst][12 nb] caller's body order: the errors of the listed rows, or null
    int n_cov;
    int cov_row[ENS_MAX_COV]; // slab rows (k - k0) of the listed steps
};

HD int ens_coords(int nb, int mu) { return 12 * nb + mu; }
HD long long ens_tiles(long long n_inst) { return (n_inst + ENS_TILE - 1) / ENS_TILE; }
// instances the workgroup's lane groups hold at once: ENS_WAVES wavefronts of 64 / G lane groups
HD int ens_pass_instances(int nb) { return ENS_WAVES * (64 / score_group_lanes(nb)); }
// doubles of LDS one lane group takes: the staged row (13 nb), then x = (dz in link order, du), padded to an odd stride
HD int ens_group_doubles(int nb, int mu) { return (13 * nb + 12 * nb + mu) | 1; }
HD size_t ens_lds_bytes(int nb, int mu) { return sizeof(double) * (size_t)ens_pass_instances(nb) * ens_group_doubles(nb, mu); }
// where coordinate c of x (dz in LINK order, then du) goes in the outputs: dz in the caller's body order (perm[l] = the caller's body of link l), du as it is
HD int ens_out_index(int c, int ne, const int* perm) { return c < ne ? 12 * perm[c / 12] + c % 12 : c; }

// a value that is not finite counts as NaN, so that whatever it touches is NaN and nothing else (an Inf would leave a mean of Inf beside an M2 of NaN)
HD double ens_canon(double v) { return (fabs(v) <= 1.7976931348623157e308) ? v : NAN; }
// the error of one body about its setpoint (score_body_error: the rollout's own arithmetic), canonicalised
HD void ens_body_row(const double* z, const double* zd, double* dz) {
    score_body_error(z, zd, dz);
#pragma unroll
    for (int i = 0; i < 12; i++) dz[i] = ens_canon(dz[i]);
}

// ---- the two cross-lane pieces of the front end that forms x (ens_moments_kernel; ens_stage_kernel of quantiles.hip forms the same x with them): device code only,
// called at control flow that depends on launch arguments and controller constants alone
template <int G>
__device__ __forceinline__ double ens_group_sum(double v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the row and x of an instance are private to ONE lane group of ONE wavefront between two workgroup barriers: what orders a lane's LDS writes before its
// neighbours' reads is the wavefront's own instruction order; the fences keep the compiler from moving LDS accesses across the point
__device__ __forceinline__ void ens_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (mean, M2) of cnt >= 1 values x[0], x[stride], ...: two passes, the first about x[0] -- equal values give their own bits as the mean and M2 = 0 exactly
HD void ens_pass_partial(const double* x, int stride, int cnt, double* mean, double* M2) {
    const double x0 = x[0];
    double s = 0.0;
    for (int g = 1; g < cnt; g++) s += x[(size_t)g * stride] - x0;
    const double m = x0 + s / (double)cnt;
    double q = 0.0;
    for (int g = 0; g < cnt; g++) { const double d = x[(size_t)g * stride] - m; q += d * d; }
    *mean = m; *M2 = q;
}
// (na, mean, M2) <- merged with (nb, mean_b, M2b), na, nb >= 1: Chan's pairwise formula.  Equal means leave the mean's bits and add nothing to M2
HD void ens_merge(double na, double* mean, double* M2, double nb, double mean_b, double M2b) {
    const double n = na + nb, d = mean_b - *mean;
    *mean = *mean + d * (nb / n);
    *M2 = (*M2 + M2b) + (d * d) * (na * nb / n);
}

// ---- the co-moment matrices of the listed steps: C = Dc' Dc, Dc = the errors less their mean, one workgroup per lower-triangle 32 x 32 tile and K-split
struct EnsCovArgs {
    int mx, tm;               // tm = ceil(mx / 32)
    long long n_inst;
    int nsplit;               // ceil(n_inst / ENS_KSPLIT)
    int stride;               // doubles between consecutive rows of mean (= 12 nb + mu)
    const double* dzrows;     // [n_cov][n_inst][mx]
    const double* mean;       // [steps][stride]: the finished means
    double* cpart;            // [n_cov][nsplit][tm (tm + 1) / 2][1024]
    double* cov;              // [n_cov][mx][mx]
    int cov_row[ENS_MAX_COV];
};
HD int ens_lower_tiles(int tm) { return tm * (tm + 1) / 2; }
HD long long ens_splits(long long n_inst) { return (n_inst + ENS_KSPLIT - 1) / ENS_KSPLIT; }

// the workspace of one call, in doubles: the tiles' partials, then the listed rows' errors, then the splits' co-moment tiles
HD size_t ens_ws_part_doubles(int nb, int mu, long long n_inst, int steps) { return (size_t)steps * (size_t)ens_tiles(n_inst) * 2 * (size_t)ens_coords(nb, mu); }
HD size_t ens_ws_rows_doubles(int nb, long long n_inst, int n_cov) { return (size_t)n_cov * (size_t)n_inst * 12 * (size_t)nb; }
HD size_t ens_ws_cpart_doubles(int nb, long long n_inst, int n_cov) {
    return (size_t)n_cov * (size_t)ens_splits(n_inst) * (size_t)ens_lower_tiles((12 * nb + 31) / 32) * 1024;
}
HD size_t ens_ws_doubles(int nb, int mu, long long n_inst, int steps, int n_cov) {
    return ens_ws_part_doubles(nb, mu, n_inst, steps) + ens_ws_rows_doubles(nb, n_inst, n_cov) + ens_ws_cpart_doubles(nb, n_inst, n_cov);
}

hipError_t launch_ensemble(const EnsArgs& a, double* mean, double* m2, hipStream_t stream);
hipError_t launch_ensemble_finish(const double* part, long long n_inst, int steps, int nx, double* mean, double* m2, hipStream_t stream);
hipError_t launch_ensemble_cov(const EnsCovArgs& a, int n_cov, hipStream_t stream);

}  // namespace cclqr
