// covariance_doubling.hip -- the closed-loop state covariance of a STATIONARY gain under input noise, by doubling.  The reference's flagship example drives the
// cart with randn()*2 (examples/trackingLQR_triple_cartpole.jl:98, 125); with the one gain of LQR{T,Inf} (src/control/lqr.jl:40-43) the closed loop on the linear
// model is  Δz⁺ = Abar Δz + D w,  Abar = A' - D K (lqr.jl:169; [A' | D]: ric_project_kernel),  w ~ (0, Wu) in input space, so after n steps from a start of
// covariance Σ0
//   Σ_n = C(n) + M(n) Σ0 M(n)',   C(n) = sum_{i<n} Abar^i W (Abar^i)',   W = D Wu D',   M(n) = Abar^n
//   C(a + b) = C(a) + M(a) C(b) M(a)',   M(a + b) = M(a) M(b)
// which is the pair recursion of policy_doubling.hip on (Abar', W) in place of (Abar, Qbar), with Σ0 in place of the terminal Q: its kernels run it unchanged
// (launch_doubling_levels).  New here are the setup that writes that pair and the moments read off Σ.
// The pair is SCALED: the recursion runs on W / w and Σ0 / w with w = 2^floor(log2 tr W) per problem (exact), so that the tol of a run to convergence is relative
// to the noise and has no units, and a noise four times as strong gives exactly four times the covariance.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>

namespace cclqr {

#define COV_RU 16        // rows of Abar / W per workgroup of the setup kernel (= DBL_RU of policy_doubling.hip: the same grid)

struct CovGrid {
    const double* Kin;         // the stationary gains [n_gains][mu][mx]
    long long k_stride;
    const double *Wu, *S0;     // [n_noise][mu][mu], [n_noise][mx][mx], either may be null
    long long wu_stride, s0_stride;
    double *Md, *Sd;           // [nprob][mx][mx]: Abar' and W / w
    double *S0s, *w;           // [nprob][mx][mx]: Σ0 / w, the recursion's terminal matrix; [nprob]: w
    int scaled;                // 1: the recursion ran on the scaled pair (N != 1); 0: Σ0 was handed through as written and w is not set
    double* stage;             // [nprob][mu mx + mu mu]: K Σ and K Σ K'
    const double *Q, *R;       // the stage-cost weights (read when cost is given)
    long long q_stride, r_stride;
    double *Sigma, *dnorm;     // [nprob][mx][mx], [nprob][2]: the driver's results, rescaled in place
    double *cost, *zstd, *ustd;
};

// =====================================================================================================================
// SETUP: Md = Abar' with Abar = A' - D K formed as dbl_setup_kernel forms it (ric_abar_entry; only the store is transposed), Sd = D Wu D' / w, the
// terminal matrix Σ0 / w, and w.  tr W = tr(Wu D'D) costs mx mu^2: every workgroup of a problem computes it, by the same operations, so all agree on w bitwise
__global__ __launch_bounds__(TILE_THREADS) void cov_setup_kernel(RicGrid a, CovGrid c) {
    extern __shared__ double cl[];      // K [mu][mx] | Wu [mu][mu] | D Wu of this workgroup's rows [COV_RU][mu] | the terms of tr(Wu D'D) [mu][mu]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    double* wl = cl + (size_t)mu * mx;
    double* dw = wl + (size_t)mu * mu;
    double* tt = dw + (size_t)COV_RU * mu;
    if (blockIdx.x == 0 && tid == 0 && ric_knot_singular(a, prob, 1)) { a.status[prob] = CCLQR_ESINGULAR_; a.stop[prob] = 1; }      // lqr.jl:151
    const double* Kp = c.Kin + (long long)prob * c.k_stride;
    const double* Wp = c.Wu ? c.Wu + (long long)prob * c.wu_stride : nullptr;
    for (int e = tid; e < mu * mx; e += TILE_THREADS) cl[e] = Kp[e];
    for (int e = tid; e < mu * mu; e += TILE_THREADS) wl[e] = Wp ? Wp[e] : 0.0;
    __syncthreads();
    const double* AD = a.AD + (size_t)prob * mx * na;
    for (int e = tid; e < mu * mu; e += TILE_THREADS) {
        const int p = e / mu, q = e - p * mu;
        double s = 0.0;
        for (int i = 0; i < mx; i++) s += AD[(size_t)i * na + mx + p] * AD[(size_t)i * na + mx + q];
        tt[e] = wl[e] * s;
    }
    for (int e = tid; e < COV_RU * mu; e += TILE_THREADS) {
        const int r = e / mu, q = e - r * mu, i = blockIdx.x * COV_RU + r;
        double s = 0.0;
        if (i < mx)
            for (int p = 0; p < mu; p++) s += AD[(size_t)i * na + mx + p] * wl[p * mu + q];
        dw[e] = s;
    }
    __syncthreads();
    double tr = 0.0;
    for (int e = 0; e < mu * mu; e++) tr += tt[e];
    double w = 1.0, inv = 1.0;      // w = 2^floor(log2 tr W); 1 when there is no noise to scale by (or the trace is no positive finite number)
    if (mu > 0 && tr > 0.0 && tr < INFINITY) {
        int ex;
        (void)frexp(tr, &ex);       // tr = m 2^ex, 0.5 <= m < 1
        ex = ex - 1 < -1000 ? -1000 : (ex - 1 > 1000 ? 1000 : ex - 1);
        w = ldexp(1.0, ex); inv = ldexp(1.0, -ex);
    }
    if (blockIdx.x == 0 && tid == 0) c.w[prob] = w;
    const double* S0 = c.S0 ? c.S0 + (long long)prob * c.s0_stride : nullptr;
    double* Md = c.Md + (size_t)prob * mx * mx;
    double* Sd = c.Sd + (size_t)prob * mx * mx;
    double* S0s = c.S0s + (size_t)prob * mx * mx;
    for (int r = 0; r < COV_RU; r++) {
        const int i = blockIdx.x * COV_RU + r;
        if (i >= mx) break;
        for (int j = tid; j < mx; j += TILE_THREADS) {
            Md[(size_t)j * mx + i] = ric_abar_entry(AD, na, mx, mu, i, j, cl);        // Abar = A' - D K (lqr.jl:169), stored as Abar'
            double q = 0.0;                                                           // W = D Wu D'
            for (int p = 0; p < mu; p++) q += dw[r * mu + p] * AD[(size_t)j * na + mx + p];
            Sd[(size_t)i * mx + j] = q * inv;
            S0s[(size_t)i * mx + j] = S0 ? S0[(size_t)i * mx + j] * inv : 0.0;
        }
    }
}

// =====================================================================================================================
// MOMENTS: one workgroup per problem, after the recursion.  Σ = w P_out in place (exact), dnorm in Σ's units, and what was asked for of
//   cost[0] = tr(Q Σ)   cost[1] = tr(R K Σ K')   zstd[i] = sqrt(max(Σ_ii, 0))   ustd[j] = sqrt(max((K Σ K')_jj, 0))
// Every sum runs in an order fixed by the sizes alone.  A problem whose G Bλ is singular gets none
__global__ __launch_bounds__(TILE_THREADS) void cov_moments_kernel(RicGrid a, CovGrid c) {
    __shared__ double part[TILE_THREADS];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, mm = mx * mx;
    if (a.status[prob] != 0) return;
    const double w = c.scaled ? c.w[prob] : 1.0;
    double* S = c.Sigma + (size_t)prob * mm;
    for (int e = tid; e < mm; e += TILE_THREADS) S[e] *= w;
    if (tid < 2) c.dnorm[2 * prob + tid] *= w;
    __syncthreads();
    if (c.zstd)
        for (int i = tid; i < mx; i += TILE_THREADS) { const double v = S[(size_t)i * mx + i]; c.zstd[(size_t)prob * mx + i] = v < 0.0 ? 0.0 : sqrt(v); }
    if (c.cost) {
        const double* Qp = c.Q + (long long)prob * c.q_stride;
        double s = 0.0;
        for (int i = tid; i < mx; i += TILE_THREADS)
            for (int j = 0; j < mx; j++) s += Qp[(size_t)i * mx + j] * S[(size_t)j * mx + i];
        part[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int k = 0; k < TILE_THREADS; k++) t += part[k];
            c.cost[2 * prob] = t;
        }
    }
    if (!c.cost && !c.ustd) return;
    const double* Kp = c.Kin + (long long)prob * c.k_stride;
    double* T = c.stage + (size_t)prob * ((size_t)mu * mx + (size_t)mu * mu);      // K Σ [mu][mx]
    double* V = T + (size_t)mu * mx;                                               // K Σ K' [mu][mu]
    for (int e = tid; e < mu * mx; e += TILE_THREADS) {
        const int p = e / mx, j = e - p * mx;
        double s = 0.0;
        for (int k = 0; k < mx; k++) s += Kp[p * mx + k] * S[(size_t)k * mx + j];
        T[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < mu * mu; e += TILE_THREADS) {
        const int p = e / mu, q = e - p * mu;
        double s = 0.0;
        for (int j = 0; j < mx; j++) s += T[p * mx + j] * Kp[q * mx + j];
        V[e] = s;
    }
    __syncthreads();
    if (c.ustd)
        for (int p = tid; p < mu; p += TILE_THREADS) { const double v = V[p * mu + p]; c.ustd[(size_t)prob * mu + p] = v < 0.0 ? 0.0 : sqrt(v); }
    if (c.cost && tid == 0) {
        const double* Rp = c.R + (long long)prob * c.r_stride;
        double t = 0.0;
        for (int p = 0; p < mu; p++)
            for (int q = 0; q < mu; q++) t += Rp[p * mu + q] * V[q * mu + p];
        c.cost[2 * prob + 1] = t;
    }
}

// the doubles of CovArgs.d.work2: the recursion's own, Σ0 / w [nprob][mx][mx], w [nprob], and K Σ and K Σ K' per problem
size_t cov_work_doubles(const RicArgs& r) {
    const size_t np = r.nprob, mx = r.mx, mu = r.mu;
    return dbl_work_doubles(r) + np * mx * mx + np + np * (mu * mx + mu * mu);
}

hipError_t launch_covariance_doubling(const CovArgs& v, hipStream_t stream) {
    DblArgs p = v.d;
    RicArgs& a = p.r;
    if (a.nprob <= 0) return hipSuccess;
    const size_t np = a.nprob, mx = a.mx, mu = a.mu, mm = mx * mx;
    CovGrid c;
    memset(&c, 0, sizeof(c));
    c.S0s = p.work2 + dbl_work_doubles(a); c.w = c.S0s + np * mm; c.stage = c.w + np; c.scaled = 1;
    a.Q = c.S0s; a.q_stride = (long long)mm; a.R = nullptr; a.r_stride = 0;      // the recursion's terminal matrix is the scaled Σ0
    c.Kin = p.k.Kin; c.k_stride = p.k.k_stride; c.Wu = v.n.Wu; c.S0 = v.n.Sigma0; c.wu_stride = v.n.wu_stride; c.s0_stride = v.n.s0_stride;
    c.Md = dbl_Md(p); c.Sd = dbl_Sd(p);
    c.Q = v.w.Q; c.R = v.w.R; c.q_stride = v.w.q_stride; c.r_stride = v.w.r_stride;
    c.Sigma = a.P_out; c.dnorm = p.dnorm; c.cost = v.cost; c.zstd = v.zstd; c.ustd = v.ustd;
    hipError_t e = dbl_preset(p, stream);
    if (e == hipSuccess) e = hipMemsetAsync(c.S0s, 0, np * mm * sizeof(double), stream);      // (the projection copies the terminal matrix before the setup has written it)
    if (a.N == 1) {      // no step: Σ = Σ0 as written (zeros without one) -- no model is read, nothing is scaled
        c.scaled = 0;
        if (v.n.Sigma0) { a.Q = v.n.Sigma0; a.q_stride = v.n.s0_stride; }
    }
    const RicGrid g = ric_grid_of(a);
    if (a.N != 1) {
        if (e == hipSuccess) e = launch_ric_project(g, a, stream);
        const size_t lds = (mu * mx + 2 * mu * mu + (size_t)COV_RU * mu) * sizeof(double);
        if (e == hipSuccess) e = launch_lds(cov_setup_kernel, dim3((a.mx + COV_RU - 1) / COV_RU, a.nprob), dim3(TILE_THREADS), lds, stream, g, c);
    }
    if (e == hipSuccess) e = launch_doubling_levels(p, stream);
    if (e == hipSuccess) e = launch_lds<false>(cov_moments_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, c);
    return e;
}

}  // namespace cclqr
