// cclqr_riccati_dev.h -- what the two recursions over a problem's projected model share: the Riccati sweep that solves for the gain (riccati.hip, lqr.jl:141-184)
// and the policy evaluation that is given it (policy.hip).  The launch arguments of the kernels (RicGrid), where a knot's pivots and singular flag lie,
// the MFMA tiles of v_mfma_f64_16x16x4_f64 both build their mx^3 products from, and the host pieces of riccati.hip that policy.hip calls: the workspace
// walk and the one projection onto [A' | D] (ric_project_kernel).
#pragma once
#include "cclqr_internal.h"
#include <type_traits>

namespace cclqr {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) double lds_double;   // explicit LDS address space: ds_read/ds_write instead of flat_*

#define TILE_THREADS 256
struct RicGrid {
    int nprob, mx, mu, ml, N, nlin, na, tm, tn;
    double tol;
    const double *A, *Bu, *Bl, *G, *Q, *R;
    long long q_stride, r_stride;      // doubles between the Q / R of consecutive problems: 0 = one pair shared by all, or mx*mx / mu*mu (RicArgs)
    double *AD, *W, *Abar, *P, *Ku, *KRK, *part, *TSp, *scratch, *K;
    int *stop, *kbreak, *status;
    long long kpad;    // doubles between the gain tables of consecutive problems in K (per-instance controller tables: cclqr_internal.h gain_row_overrun)
    int keep_last;     // 1: only the gain of the last executed backward step is kept (K [nprob][mu][mx] = Ku[1] after the back-fill of
                       // lqr.jl:179-181 = the one gain LQR{T,Inf} keeps, lqr.jl:40-43); 0: the whole table K [nprob][N-1][mu][mx]
    int bf16_terms;    // 0: fp64 MFMA (parity mode); 1..3: the two mx^3 products of a backward step on bf16 MFMA with fp32 accumulation,
                       // every fp64 operand split into that many bf16 terms (measured-error mode, BASELINE configs[3]; tiled path only)
    int p_rows;        // 1: Q or R is not symmetric, so neither is Pk: W = Pk [A'|D] reads Pk by rows (the reference's D'*Pk, lqr.jl:152-158);
                       // 0: by columns (= rows of a symmetric Pk: the layout the MFMA A operand wants)
    unsigned char pp_mask[8];   // resident kernel, register-fragment form: bit ct of pp_mask[w] = wavefront w computes the 16x16 tile (its own
                                // row strip, column tile ct) of the SYMMETRIC Pkp1 and mirrors it (ric_pp_assign)
};

// per knot: the pivots of its G Bλ LU, then [ml] = 1 if G Bλ is singular (set by ric_project_kernel, read when a backward step reaches the knot)
__device__ inline int* ric_knot_piv(const RicGrid& a, size_t lin) {
    const size_t sc = ((size_t)a.ml * a.ml + (size_t)a.ml * a.na + 3) & ~(size_t)1;
    return (int*)(a.scratch + (size_t)a.nprob * a.nlin * sc) + lin * (a.ml + 2);
}
// is G Bλ of the model of backward step k singular?  The reference factors it inside the step (lqr.jl:151, lqr_tracking.jl:89), so a knot the
// sweep never reaches -- below the break, or any knot with N = 1 -- is no error
__device__ inline bool ric_knot_singular(const RicGrid& a, int prob, int k) {
    return ric_knot_piv(a, (size_t)prob * a.nlin + (a.nlin > 1 ? k - 1 : 0))[a.ml] != 0;
}

// Q / R of problem `prob`.  Called once per workgroup with prob = a block index: the result is wave-uniform and stays in scalar registers, and the
// tile loops index it as they indexed the shared matrix (stride 0: the very same addresses)
__device__ inline const double* ric_Q_of(const RicGrid& a, int prob) { return a.Q + (long long)prob * a.q_stride; }
__device__ inline const double* ric_R_of(const RicGrid& a, int prob) { return a.R + (long long)prob * a.r_stride; }

// 32x32 tile of op(A)' B summed over k, split over the four wavefronts of the workgroup (wave w takes the k-groups of 4 with
// index = w mod 4), then reduced through LDS in wave order.  la(k, h) / lb(k, h) return operand elements A[k][i0+16h+li] / B[k][j0+16h+li]
// (already masked to 0 outside the matrix).  On return red[e], e = row*32 + col, holds the tile; all threads have synchronised.
template <class FA, class FB>
__device__ inline void tile_mfma_splitk(int K, FA la, FB lb, double (*red)[1024]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    v4d acc[2][2] = {{{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}};
    const int ngroups = (K + 3) >> 2;
    // CH k-groups per wavefront and pass (4 CH loads in flight before the first MFMA): passes of 8 while they are full, then of 2
    auto pass = [&](auto chtag, int g0) {
        constexpr int CH = decltype(chtag)::value;
        double av[CH][2], bv[CH][2];
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int k = 4 * (g0 + 4 * u) + lk;
            const bool kok = (g0 + 4 * u) < ngroups && k < K;
#pragma unroll
            for (int h = 0; h < 2; h++) { av[u][h] = kok ? la(k, h) : 0.0; bv[u][h] = kok ? lb(k, h) : 0.0; }
        }
#pragma unroll
        for (int u = 0; u < CH; u++)
#pragma unroll
            for (int hi = 0; hi < 2; hi++)
#pragma unroll
                for (int hj = 0; hj < 2; hj++) acc[hi][hj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][hi], bv[u][hj], acc[hi][hj], 0, 0, 0);
    };
    // every pass is one round trip to L2 (its loads are issued together, its MFMAs wait for them), so the tail is covered by the
    // FEWEST passes -- a masked pass of 8 or 4 rather than a string of passes of 2 (mx = 204: 13 k-groups per wavefront = 8 + 8
    // masked instead of 8 + 2 + 2 + 2; the masked groups cost idle MFMAs, not latency)
    int g0 = wave;
    for (; g0 + 4 * 7 < ngroups; g0 += 4 * 8) pass(std::integral_constant<int, 8>{}, g0);
    while (g0 < ngroups) {
        const int left = (ngroups - g0 + 3) >> 2;        // k-groups this wavefront still has
        if (left > 4) { pass(std::integral_constant<int, 8>{}, g0); g0 += 4 * 8; }
        else if (left > 2) { pass(std::integral_constant<int, 4>{}, g0); g0 += 4 * 4; }
        else { pass(std::integral_constant<int, 2>{}, g0); g0 += 4 * 2; }
    }
#pragma unroll
    for (int hi = 0; hi < 2; hi++)
#pragma unroll
        for (int hj = 0; hj < 2; hj++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave][(16 * hi + lk + 4 * r) * 32 + 16 * hj + li] = acc[hi][hj][r];
    __syncthreads();
}

// 16x16 tile of sum_k a(k) b(k) by ONE wavefront (the tile of riccati.hip's wave_tile16), with the operands addressed by pointer and stride (no per-load
// lambdas and predicates) and DOUBLE-BUFFERED: the loads of
// the next four k-groups are in flight while the MFMAs of the current four issue, so a wavefront no longer stops for a full LDS / L2
// round trip in front of every batch of MFMAs (with two wavefronts per SIMD the partner covers part of it; the single-buffered form ran at
// a third of the matrix core's rate).  pa / pb point at the lane's element of k-group 0 (row lk of the group, the lane's column clamped
// into range by the caller: rows / columns past the edge compute garbage that the caller does not store); ga / gb = elements between
// consecutive k-groups.  K must be a multiple of 4 (mx = 12 nb always is; other sizes take wave_tile16).
template <class PA, class PB>
__device__ inline v4d wave_tile16_db(int ngroups, PA pa, int ga, PB pb, int gb) {
    constexpr int CH = 4;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    double a0[CH], b0[CH], a1[CH], b1[CH];
#pragma unroll
    for (int u = 0; u < CH; u++) { const bool ok = u < ngroups; a0[u] = ok ? pa[(size_t)u * ga] : 0.0; b0[u] = ok ? pb[(size_t)u * gb] : 0.0; }
    for (int g0 = 0; g0 < ngroups; g0 += 2 * CH) {
#pragma unroll
        for (int u = 0; u < CH; u++) { const int g = g0 + CH + u; const bool ok = g < ngroups; a1[u] = ok ? pa[(size_t)g * ga] : 0.0; b1[u] = ok ? pb[(size_t)g * gb] : 0.0; }
#pragma unroll
        for (int u = 0; u < CH; u++) if (g0 + u < ngroups) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[u], b0[u], acc, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < CH; u++) { const int g = g0 + 2 * CH + u; const bool ok = g < ngroups; a0[u] = ok ? pa[(size_t)g * ga] : 0.0; b0[u] = ok ? pb[(size_t)g * gb] : 0.0; }
#pragma unroll
        for (int u = 0; u < CH; u++) if (g0 + CH + u < ngroups) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[u], b1[u], acc, 0, 0, 0);
    }
    return acc;
}

// ---- host side, defined in riccati.hip
// The sizes of g from a, and the workspace of one launch walked once: g's arrays are placed one behind the other from `base` (null: nowhere); returns the doubles
// of the whole (= ric_total_work_doubles)
size_t ric_lay_out(RicGrid& g, const RicArgs& a, double* base);
// [A' | D] of every knot of every problem into g.AD, the pivots and the singular flag of every knot behind g.scratch (ric_knot_piv), Pk = Q into buffer 0 of g.P:
// ric_project_kernel, the one projection of the library.  g: laid out by ric_lay_out, with A, Bu, Bl, G, Q and q_stride set
hipError_t launch_ric_project(const RicGrid& g, const RicArgs& a, hipStream_t stream);
// the launch record of the doubling kernels for these arguments (policy_doubling.hip): laid out on a.work, with the models, Q, R and their strides, status and stop
RicGrid dbl_ric_grid(const RicArgs& a);

}  // namespace cclqr
