// value.hip -- cclqr_value_eval: V_i = dz_i' P_t dz_i for every instance of a batch, the cost the gains were designed to achieve from the state z_i
// (DESIGN.md 4.5).  P is the cost-to-go the Riccati kernels emit (riccati.hip, RicArgs.P_out), dz the error of lqr.jl:92-103 about setpoint row 0.
//
// A lane group of G = 16 / 32 / 64 lanes owns one instance (cclqr_value.h value_group_lanes), VALUE_WAVES wavefronts make a workgroup.  The group
//   1. stages the instance's 13 nb state entries in LDS (entries t, t + G, ...: coalesced),
//   2. lane l < nb forms link l's error about the controller's setpoint and stores it at its BODY's place: dz is in the caller's order, as P is,
//   3. lane t sums dz_i P_ij dz_j over the columns j = t, t + G, ... of every row i (rows of P are read G consecutive doubles at a time),
//   4. the shares are summed over the group (xor butterfly: every lane holds the same bits).
// With one P per instance the kernel is a stream of 8 mx^2 bytes per instance read once; with a shared P that table stays in L2 and the rest is arithmetic.
// Every cross-lane operation (the butterfly, the wave barriers) sits under control flow that depends on nothing but template parameters.
#include "cclqr_internal.h"
#include "cclqr_value.h"

namespace cclqr {

#define VALUE_WAVES 4

template <int G>
__device__ __forceinline__ double value_group_sum(double v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the staged state and dz of an instance are private to ONE lane group of ONE wavefront: the wavefront's own instruction order is what orders a lane's LDS
// writes before its neighbours' reads (score.hip score_wave_sync)
__device__ __forceinline__ void value_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__global__ __launch_bounds__(64 * VALUE_WAVES) void value_kernel(ValueArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G;      // instances per wavefront
    const int nb = a.nb, nz = 13 * nb, mx = 12 * nb;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G;
    double* row = lds + (size_t)(wave * IPW + grp) * value_instance_doubles(nb);
    double* DZ = row + nz;
    const long long inst_raw = ((long long)blockIdx.x * VALUE_WAVES + wave) * IPW + grp;
    const bool valid = inst_raw < a.n_inst;
    const long long inst = valid ? inst_raw : a.n_inst - 1;      // (a lane group without an instance evaluates the last one again; its result is never written)
    const long long gi = a.inst0 + inst;
    const double* z = a.z + inst * a.z_stride;
    for (int e = t; e < nz; e += G) row[e] = z[e];
    const bool body = t < nb;
    double zd[13];
    int ut = 0;
    if (body) {
        const CtrlHot* Hg = &a.C->hot;
        const double* zdrow = (const double*)(uintptr_t)Hg->zd + gi * Hg->zd_stride + 13 * t;      // setpoint row 0 of the instance's table, link t
        ut = a.M->perm[t];                                                                        // the caller's body that link t is
#pragma unroll
        for (int i = 0; i < 13; i++) zd[i] = zdrow[i];
    }
    value_wave_sync();
    if (body) {
        double zb[13], dz[12];
#pragma unroll
        for (int i = 0; i < 13; i++) zb[i] = row[13 * ut + i];
        value_body_error(zb, zd, dz);
#pragma unroll
        for (int i = 0; i < 12; i++) DZ[12 * ut + i] = dz[i];
    }
    value_wave_sync();
    const double v = value_group_sum<G>(value_lane_partial(t, G, mx, a.P + gi * a.p_stride, DZ));
    if (valid && t == 0) a.out[inst] = v;
}

hipError_t launch_value(const ValueArgs& a, hipStream_t stream) {
    if (a.n_inst <= 0) return hipSuccess;
    const int G = value_group_lanes(a.nb);
    const long long per_block = (long long)VALUE_WAVES * (64 / G);
    const dim3 grid((unsigned)((a.n_inst + per_block - 1) / per_block)), block(64 * VALUE_WAVES);
    const size_t lds = value_lds_bytes(a.nb, VALUE_WAVES);
    switch (G) {
        case 16: return launch_lds(value_kernel<16>, grid, block, lds, stream, a);
        case 32: return launch_lds(value_kernel<32>, grid, block, lds, stream, a);
        default: return launch_lds(value_kernel<64>, grid, block, lds, stream, a);
    }
}

}  // namespace cclqr
