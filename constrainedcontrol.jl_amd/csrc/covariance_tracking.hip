// covariance_tracking.hip -- the state covariance of a TRACKED run under input noise, knot by knot: the forward dual of policy.hip with a model and a gain per knot.
// The reference's flagship example drives the cart with randn()*2 (examples/trackingLQR_triple_cartpole.jl:98) under a TrackingLQR whose gain row of knot j is
// Ku[j] (src/control/lqr_tracking.jl:65, gated by k < N at line 63) on the model linearised at knot j (lqr_tracking.jl:88-89).  Knots are j = 0 .. N-1, knot j
// being the state the law sees at step j + 1 (the indexing of cclqr_rollout_score and of a recorded rollout).  With [A'_j | D_j] the projected pair of knot j
// (ric_project_kernel -- the one copy, launched from here too) and w ~ (0, Wu) in input space:
//   Abar_j  = A'_j - D_j K_j                       (lqr_tracking.jl:107)
//   Σ_0     = Sigma0 (or 0)
//   Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j'     j = 0 .. N-2
//   cx_j = tr(Q Σ_j)   j = 0 .. N-1;    cu_j = tr(R K_j Σ_j K_j')   j = 0 .. N-2, cu_{N-1} = 0
//   zstd_j = sqrt(max(diag Σ_j, 0));    ustd_j = sqrt(max(diag K_j Σ_j K_j', 0)), ustd_{N-1} = 0
//   total  = (sum_j cx_j, sum_j cu_j) in knot order = E[Jx], E[Ju] of simulate(..., steps = N, score = Score(...))
// Σ is a second moment: a rank-one Sigma0 = δδ' with Wu = 0 is the deterministic perturbed start.  Wu, Sigma0, Q, R are used as written; nothing assumes
// symmetry.  N = 1: Σ = Sigma0 and no model is read.  nlin = 1 (one time-invariant model) and nK = 1 (one stationary gain) are served by the same kernels.
// The products are taken as in policy.hip, with the TRANSPOSE of Abar as the stationary operand:
//   T = Abar Σ     (A operand Abar'[k][i], B operand Σ[k][j]: both read along rows), stored TRANSPOSED, Tt[k][i] = T[i][k]
//   T Abar'        (A operand Tt[k][i], B operand Abar'[k][j]: rows again)
// Two launch shapes: RESIDENT, one workgroup per problem over all knots; TILED, every step as device-wide launches.  Both run on v_mfma_f64_16x16x4_f64
// through the tiles of cclqr_riccati_dev.h.  Every sum is taken in an order fixed by the sizes alone: a result depends neither on scheduling nor on the batch.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>

namespace cclqr {

#define CTK_THREADS 512
#define CTK_WAVES (CTK_THREADS / 64)
#define CTK_TILES 5      // 16x16 tiles one wavefront holds across a barrier (ResTiles of cclqr_riccati_dev.h)
#define CTK_PRE 18       // doubles of the next knot's A' one lane holds while the products run: ceil(96 * 96 / 512)
#define CTK_PRE_S 2      // ... and of its D and of its K: ceil(mu mx / 512) (ctk_resident_fits)

// what the kernels take besides the Riccati launch record
struct CtkGrid {
    const double* Kin;         // gain tables [n_gains][nK][mu][mx], the models' state order
    long long k_stride;        // doubles between the tables of consecutive problems: 0 = one table shared by all
    int nK;                    // rows per table: N - 1 (row j = the gain of knot j) or 1 = a stationary gain
    const double *Wu, *S0;     // [n_noise][mu][mu], [n_noise][mx][mx], either may be null (= 0)
    long long wu_stride, s0_stride;
    const double *Q, *R;       // the stage-cost weights
    long long q_stride, r_stride;
    double* mom;               // [nprob][N] records of ctk_record(mx, mu) doubles: cx, cu, zstd [mx], ustd [mu] of the knot
    double* total;             // [nprob][2]
    double *Sigma, *Sigma_all; // each may be null
};
__device__ inline const double* ctk_gain(const RicGrid& a, const CtkGrid& c, int prob, int j) {
    return c.Kin + (long long)prob * c.k_stride + (size_t)(c.nK > 1 ? j : 0) * a.mu * a.mx;
}
__device__ inline const double* ctk_model(const RicGrid& a, int prob, int j) { return a.AD + ((size_t)prob * a.nlin + (a.nlin > 1 ? j : 0)) * a.mx * a.na; }
// is G Bλ of knot j's model singular (ric_knot_singular counts backward steps: knot j is the model of step j + 1)
__device__ inline bool ctk_singular(const RicGrid& a, int prob, int j) { return ric_knot_singular(a, prob, j + 1); }

// Σ_0 into buffer 0 of the workspace's P (the projection, which copies "Q" there, is pointed at that very buffer), the totals to zero
__global__ __launch_bounds__(TILE_THREADS) void ctk_init_kernel(RicGrid a, CtkGrid c) {
    const int prob = blockIdx.x, tid = threadIdx.x, mm = a.mx * a.mx;
    const double* S0 = c.S0 ? c.S0 + (long long)prob * c.s0_stride : nullptr;
    double* P = a.P + (size_t)prob * mm;
    for (int e = tid; e < mm; e += TILE_THREADS) P[e] = S0 ? S0[e] : 0.0;
    if (tid < 2) c.total[2 * prob + tid] = 0.0;
    if (tid == 0) { a.status[prob] = 0; a.kbreak[prob] = -1; }
}

// =====================================================================================================================
// RESIDENT: one 512-thread workgroup per problem, persistent over all knots, for the shapes policy_resident_kernel serves (ctk_resident_fits).  Operand placement:
//   Ab  [mx][mx]  LDS   Abar_j' -- the A operand of T = Abar Σ and the B operand of T Abar': read by every tile of both products
//   X   [mx][mx]  LDS   ONE buffer: Σ_j (B operand of the first product), then Tt (A operand of the second), then Σ_{j+1}.  A wavefront keeps the accumulators of
//                       its <= CTK_TILES tiles in registers until a barrier says every read of the old content is done.  Two mx^2 buffers are 147 KB at mx = 96
//   Kl  [mu][mx]  LDS   K_j while the moments of Σ_j are taken, then D_j Wu [mx][mu] for the step's noise term
//   Dl  [mx][mu]  LDS   D_j
//   Wl, Vl [mu][mu] LDS Wu; K_j Σ_j K_j'
//   registers            knot j + 1's A' (CTK_PRE doubles per lane), D and K (CTK_PRE_S each): REQUESTED before knot j's products and written to LDS after the
//                        barrier that retires Abar_j': meant to keep the model stream off the critical path (not measured separately).  Lane e owns A'[i][jj], e = jj mx + i: consecutive lanes write
//                        consecutive LDS words of the transposed Abar
// LDS at mx = 84, mu = 7: 2 x 56 448 + 2 x 4 704 + 2 x 392 + 64 = 123 152 B; at mx = 96, mu = 7: 2 x 73 728 + 2 x 5 376 + 2 x 392 + 64 = 159 056 B of 163 840.
size_t ctk_resident_lds_bytes(int mx, int mu) {
    return (2 * (size_t)mx * mx + 2 * (size_t)mu * mx + 2 * (size_t)mu * mu + CTK_WAVES) * sizeof(double);
}
// THE fit rule of the resident kernel: whole k-groups of four, a wavefront's share of the tiles in its registers (mx <= 96), a lane's share of the next knot's
// model in its registers, and the operands in one CU's LDS
bool ctk_resident_fits(int mx, int mu) {
    return res_tiles_serve(mx, CTK_WAVES) && mx * mx <= CTK_PRE * CTK_THREADS && mu * mx <= CTK_PRE_S * CTK_THREADS && ctk_resident_lds_bytes(mx, mu) <= 158 * 1024;
}
int ctk_chosen_path(int mx, int mu, int path) { return (path != 2 && ctk_resident_fits(mx, mu)) ? 1 : 2; }

// a wave-uniform value, hidden from loop-invariant code motion
__device__ __forceinline__ int ctk_opaque_s(int x) { asm volatile("" : "+s"(x)); return x; }

static_assert(CTK_TILES == RES_TILES, "the resident kernel holds its tiles in ResTiles");

// the sizes a knot's code is written in, derived from (mx, mu)
struct CtkSizes {
    int mx, mu, na, mm, ms, t16, ntile, ng;
    lds_double *Ab, *X, *Kl, *Dl, *Wl, *Vl, *red;
    __device__ __forceinline__ CtkSizes(int mx_, int mu_, double* lds) : mx(mx_), mu(mu_), na(mx_ + mu_), mm(mx_ * mx_), ms(mu_ * mx_), t16((mx_ + 15) >> 4), ng(mx_ >> 2) {
        ntile = t16 * t16;
        Ab = (lds_double*)lds; X = Ab + mm; Kl = X + mm; Dl = Kl + ms; Wl = Dl + ms; Vl = Wl + mu * mu; red = Vl + mu * mu;
    }
};

__global__ __launch_bounds__(CTK_THREADS) void ctk_resident_kernel(RicGrid a, CtkGrid c) {
    extern __shared__ double sl[];
    const int prob = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int N = a.N;
    const double* Qp = c.Q + (long long)prob * c.q_stride;
    const double* Rp = c.R + (long long)prob * c.r_stride;
    // what advances from knot to knot is carried as running pointers (a base, a problem offset and a knot stride each would not fit the scalar registers):
    // the model, the gain and the singular flag of the knot REQUESTED next, the record and the Sigma_all block of the knot at hand
    const double *ADn, *Kn;
    const int* sgn = ric_knot_piv(a, (size_t)prob * a.nlin) + a.ml;
    int adstep, kstep;
    const int sgstep = a.nlin > 1 ? a.ml + 2 : 0;
    double *mo, *sa;
    {
        const CtkSizes z(a.mx, a.mu, sl);
        const double* S0 = a.P + (size_t)prob * z.mm;      // Σ_0 (ctk_init_kernel)
        const double* Wp = c.Wu ? c.Wu + (long long)prob * c.wu_stride : nullptr;
        for (int e = tid; e < z.mm; e += CTK_THREADS) z.X[e] = S0[e];
        for (int e = tid; e < z.mu * z.mu; e += CTK_THREADS) z.Wl[e] = Wp ? Wp[e] : 0.0;
        ADn = ctk_model(a, prob, 0);
        Kn = z.mu > 0 ? ctk_gain(a, c, prob, 0) : nullptr;
        adstep = a.nlin > 1 ? z.mx * z.na : 0; kstep = c.nK > 1 ? z.ms : 0;
        mo = c.mom + (size_t)prob * N * ctk_record(z.mx, z.mu);
        sa = c.Sigma_all ? c.Sigma_all + (size_t)prob * N * z.mm : nullptr;
    }
    bool singn = false;
    const bool reform = a.nlin > 1 || c.nK > 1;      // Abar changes from knot to knot
    double pre[CTK_PRE], pd[CTK_PRE_S], pk[CTK_PRE_S];
    int status = 0, knot = -1;
    double tx = 0.0, tu = 0.0;      // thread 0: the totals, in knot order
    __syncthreads();
    for (int j = -1; j < N; j++) {      // (j = -1 only requests knot 0's model)
        // Every size-derived value of the knot's code is derived HERE, from values the compiler cannot see through: held across the knot loop as loop invariants
        // (strides, LDS bases, lane predicates, the index pairs of the unrolled walks) they do not fit the scalar registers; re-derived they are a few dozen
        // scalar operations against a step's thousands of cycles
        const CtkSizes z(ctk_opaque_s(a.mx), ctk_opaque_s(a.mu), sl);
        const int mx = z.mx, mu = z.mu, na = z.na, mm = z.mm, ms = z.ms;
        const ResShape rs = {mx, z.t16, z.ntile, z.ng, wave, li, lk, CTK_WAVES};
        lds_double *const Ab = z.Ab, *const X = z.X, *const Kl = z.Kl, *const Dl = z.Dl, *const Wl = z.Wl, *const Vl = z.Vl, *const red = z.red;
        // this lane's elements of A' / Abar: e = tid + 512 r = jj mx + i, walked by increments (no division per element)
        const int i0 = tid % mx, j0 = tid / mx, di = CTK_THREADS % mx, dj = CTK_THREADS / mx;
        const bool last = j == N - 1;
        if (j >= 0 && !last) {
            if (singn) { status = CCLQR_ESINGULAR_; knot = j; break; }      // G Bλ singular                   lqr_tracking.jl:89
            // knot j's K and D, requested a step ago, into LDS (Kl, Dl and Ab are dead by now), and Abar_j' from its A'
#pragma unroll
            for (int r = 0; r < CTK_PRE_S; r++) {
                const int e = tid + CTK_THREADS * r;
                if (e < ms) { Kl[e] = pk[r]; Dl[e] = pd[r]; }
            }
            __syncthreads();
            if (j == 0 || reform) {
                int i = i0, jj = j0;
#pragma unroll
                for (int r = 0; r < CTK_PRE; r++) {
                    if (jj < mx) {
                        double s = pre[r];                                    // Abar = A' - D K (= A-Bu*Ku-Bλ*Kλ)   lqr_tracking.jl:107
#pragma unroll 1
                        for (int p = 0; p < mu; p++) s -= Dl[i * mu + p] * Kl[p * mx + jj];
                        Ab[jj * mx + i] = s;                                  // stored as Abar'
                    }
                    i += di; jj += dj;
                    if (i >= mx) { i -= mx; jj++; }
                }
            }
            __syncthreads();
        }
        const bool next = j + 1 < N - 1;
        singn = next && *sgn != 0;
        if (next && !singn) {      // REQUEST knot j + 1's K and D, and its A' when Abar is to be formed from it
            if (j + 1 == 0 || reform) {
                int i = i0, jj = j0;
#pragma unroll
                for (int r = 0; r < CTK_PRE; r++) {
                    pre[r] = jj < mx ? ADn[(unsigned)(i * na + jj)] : 0.0;
                    i += di; jj += dj;
                    if (i >= mx) { i -= mx; jj++; }
                }
            }
#pragma unroll
            for (int r = 0; r < CTK_PRE_S; r++) {
                const int e = tid + CTK_THREADS * r;
                const bool ok = e < ms;
                const int i = ok ? e / mu : 0, p = ok ? e - i * mu : 0;
                pd[r] = ok ? ADn[(unsigned)(i * na + mx + p)] : 0.0;
                pk[r] = ok ? Kn[e] : 0.0;
            }
        }
        ADn += adstep; Kn += kstep; sgn += sgstep;
        if (j < 0) continue;
        // ---- the moments of Σ_j (X) under K_j (Kl)
        for (int i = tid; i < mx; i += CTK_THREADS) { const double v = X[i * mx + i]; mo[2 + i] = v < 0.0 ? 0.0 : sqrt(v); }
        if (sa) {
            for (int e = tid; e < mm; e += CTK_THREADS) sa[e] = X[e];
            sa += mm;
        }
        {      // tr(Q Σ) = sum Q[i][jj] Σ[jj][i]: each lane its elements in order, the lanes by the shuffle tree, the wavefronts in index order
            double s = 0.0;
            int i = i0, jj = j0;
#pragma unroll 1
            for (int r = 0; r < CTK_PRE; r++) {
                if (jj < mx) s += Qp[(unsigned)(i * mx + jj)] * X[jj * mx + i];
                i += di; jj += dj;
                if (i >= mx) { i -= mx; jj++; }
            }
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) red[wave] = s;
        }
        if (!last) {      // K Σ K': wavefront p takes row p, a lane the columns lane and lane + 64 of K Σ
#pragma unroll 1
            for (int p = wave; p < mu; p += CTK_WAVES) {
                const int c0 = lane, c1 = lane + 64;
                const bool ok0 = c0 < mx, ok1 = c1 < mx;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 1
                for (int k = 0; k < mx; k++) {
                    const double kv = Kl[p * mx + k];
                    if (ok0) s0 += kv * X[k * mx + c0];
                    if (ok1) s1 += kv * X[k * mx + c1];
                }
#pragma unroll 1
                for (int q = 0; q < mu; q++) {
                    double t = (ok0 ? s0 * Kl[q * mx + c0] : 0.0) + (ok1 ? s1 * Kl[q * mx + c1] : 0.0);
                    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
                    if (lane == 0) Vl[p * mu + q] = t;
                }
            }
        }
        ResTiles acc = res_zero();
        if (!last) acc = res_mul(rs, Ab, X);      // T = Abar Σ: this wavefront's tiles, kept in registers
        __syncthreads();      // every wavefront has read Σ_j and K_j: X may take Tt, Kl may take D Wu; red and Vl are complete
        if (tid == 0) {
            double cx = 0.0, cu = 0.0;
#pragma unroll 1
            for (int w = 0; w < CTK_WAVES; w++) cx += red[w];
            if (!last)
#pragma unroll 1
                for (int p = 0; p < mu; p++)
#pragma unroll 1
                    for (int q = 0; q < mu; q++) cu += Rp[p * mu + q] * Vl[q * mu + p];
            mo[0] = cx; mo[1] = cu;
            tx += cx; tu += cu;
        }
#pragma unroll 1
        for (int p = tid; p < mu; p += CTK_THREADS) { const double v = last ? 0.0 : Vl[p * mu + p]; mo[2 + mx + p] = v < 0.0 ? 0.0 : sqrt(v); }
        mo += ctk_record(mx, mu);
        if (last) break;
        for (int e = tid; e < ms; e += CTK_THREADS) {      // D Wu
            const int i = e / mu, q = e - i * mu;
            double s = 0.0;
#pragma unroll 1
            for (int p = 0; p < mu; p++) s += Dl[i * mu + p] * Wl[p * mu + q];
            Kl[e] = s;
        }
        res_each(rs, acc, [&](int i, int q, double v) { X[q * mx + i] = v; });      // Tt[q][i] = T[i][q]
        __syncthreads();
        acc = res_mul(rs, X, Ab);                                                  // T Abar'
        __syncthreads();      // every wavefront has read Tt: the buffer may take Σ_{j+1}
        res_each(rs, acc, [&](int i, int q, double v) {                             // Σ_{j+1} = Abar Σ_j Abar' + (D Wu) D'
#pragma unroll 1
            for (int p = 0; p < mu; p++) v += Kl[i * mu + p] * Dl[q * mu + p];
            X[i * mx + q] = v;
        });
        __syncthreads();      // Σ_{j+1} is complete; Abar_j', D_j and D_j Wu are retired
    }
    if (status == 0 && c.Sigma) {
        const CtkSizes z(a.mx, a.mu, sl);
        double* So = c.Sigma + (size_t)prob * z.mm;
        for (int e = tid; e < z.mm; e += CTK_THREADS) So[e] = z.X[e];
    }
    if (tid == 0) {
        a.status[prob] = status; a.kbreak[prob] = knot;
        if (status == 0) { c.total[2 * prob] = tx; c.total[2 * prob + 1] = tu; }
    }
}

// =====================================================================================================================
// TILED: every other shape (mx % 4 != 0, mx > 96: any chain of more than 8 bodies) and path = 2.  One step = four launches over the problems:
//   ctk_moments_kernel  the moments of Σ_j, Sigma_all[j]                                                   (one workgroup per problem)
//   ctk_abar_kernel     Abar_j' = (A'_j - D_j K_j)'; a singular G Bλ sets the problem's status, which stops it   (blocks of CTK_RU rows)
//   ctk_t_kernel        Tt = (Abar Σ_j)'                                                                    (32x32 tiles, edge tiles masked)
//   ctk_next_kernel     Σ_{j+1} = T Abar' + (D Wu) D' into the other buffer of P                             (32x32 tiles)
// Σ_j lies in buffer j & 1 of the workspace's P, Tt in W, K Σ in KRK, K Σ K' in TSp (ric_lay_out).
#define CTK_RU 16

__global__ __launch_bounds__(TILE_THREADS) void ctk_moments_kernel(RicGrid a, CtkGrid c, int j) {
    __shared__ double part[TILE_THREADS];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, N = a.N, mm = mx * mx;
    if (a.status[prob] != 0) return;
    const bool last = j == N - 1;
    const double* S = a.P + ((size_t)(j & 1) * a.nprob + prob) * mm;
    if (c.Sigma_all) {
        double* o = c.Sigma_all + ((size_t)prob * N + j) * mm;
        for (int e = tid; e < mm; e += TILE_THREADS) o[e] = S[e];
    }
    if (last && c.Sigma) {
        double* o = c.Sigma + (size_t)prob * mm;
        for (int e = tid; e < mm; e += TILE_THREADS) o[e] = S[e];
    }
    double* mo = c.mom + ((size_t)prob * N + j) * ctk_record(mx, mu);
    for (int i = tid; i < mx; i += TILE_THREADS) { const double v = S[(size_t)i * mx + i]; mo[2 + i] = v < 0.0 ? 0.0 : sqrt(v); }
    double cx = 0.0;
    {
        const double* Qp = c.Q + (long long)prob * c.q_stride;
        double s = 0.0;
        for (int i = tid; i < mx; i += TILE_THREADS)
            for (int k = 0; k < mx; k++) s += Qp[(size_t)i * mx + k] * S[(size_t)k * mx + i];
        part[tid] = s;
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < TILE_THREADS; k++) cx += part[k];
    }
    double* V = a.TSp + (size_t)prob * a.tm * mu * a.na;      // K Σ K' [mu][mu]
    if (!last) {
        const double* Kp = ctk_gain(a, c, prob, j);
        double* T = a.KRK + (size_t)prob * mu * mx;           // K Σ [mu][mx]
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {
            const int p = e / mx, q = e - p * mx;
            double s = 0.0;
            for (int k = 0; k < mx; k++) s += Kp[p * mx + k] * S[(size_t)k * mx + q];
            T[e] = s;
        }
        __syncthreads();
        for (int e = tid; e < mu * mu; e += TILE_THREADS) {
            const int p = e / mu, q = e - p * mu;
            double s = 0.0;
            for (int k = 0; k < mx; k++) s += T[p * mx + k] * Kp[q * mx + k];
            V[e] = s;
        }
        __syncthreads();
    }
    for (int p = tid; p < mu; p += TILE_THREADS) { const double v = last ? 0.0 : V[p * mu + p]; mo[2 + mx + p] = v < 0.0 ? 0.0 : sqrt(v); }
    if (tid == 0) {
        double cu = 0.0;
        if (!last) {
            const double* Rp = c.R + (long long)prob * c.r_stride;
            for (int p = 0; p < mu; p++)
                for (int q = 0; q < mu; q++) cu += Rp[p * mu + q] * V[q * mu + p];
        }
        mo[0] = cx; mo[1] = cu;
        c.total[2 * prob] += cx; c.total[2 * prob + 1] += cu;      // launches of one stream: knot order
    }
}

__global__ __launch_bounds__(TILE_THREADS) void ctk_abar_kernel(RicGrid a, CtkGrid c, int j) {
    extern __shared__ double kl[];      // K_j [mu][mx]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    if (a.status[prob] != 0) return;    // stopped at an earlier knot
    if (ctk_singular(a, prob, j)) {     // G Bλ singular (every workgroup of the problem sees it by itself; the lead records it)      lqr_tracking.jl:89
        if (blockIdx.x == 0 && tid == 0) { a.status[prob] = CCLQR_ESINGULAR_; a.kbreak[prob] = j; }
        return;
    }
    const double* Kp = mu > 0 ? ctk_gain(a, c, prob, j) : nullptr;
    for (int e = tid; e < mu * mx; e += TILE_THREADS) kl[e] = Kp[e];
    __syncthreads();
    const double* AD = ctk_model(a, prob, j);
    double* AbT = a.Abar + (size_t)prob * mx * mx;
    for (int r = 0; r < CTK_RU; r++) {
        const int i = blockIdx.x * CTK_RU + r;
        if (i >= mx) break;
        for (int q = tid; q < mx; q += TILE_THREADS) AbT[(size_t)q * mx + i] = ric_abar_entry(AD, na, mx, mu, i, q, kl);      // Abar = A' - D K (lqr_tracking.jl:107), stored as Abar'
    }
}

__global__ __launch_bounds__(TILE_THREADS) void ctk_t_kernel(RicGrid a, int j) {
    __shared__ double red[4][1024];
    const int prob = blockIdx.y, mx = a.mx;
    if (a.status[prob] != 0 || ctk_singular(a, prob, j)) return;
    const double* S = a.P + ((size_t)(j & 1) * a.nprob + prob) * mx * mx;
    tile32_product_transposed(tile32_at(blockIdx.x, a.tm, mx), mx, a.Abar + (size_t)prob * mx * mx, S, a.W + (size_t)prob * mx * a.na, red);      // Tt = (Abar Σ_j)'
}

__global__ __launch_bounds__(TILE_THREADS) void ctk_next_kernel(RicGrid a, CtkGrid c, int j) {
    __shared__ double red[4][1024];
    extern __shared__ double dt[];      // (D Wu) of the tile's rows [32][mu] | D of the tile's columns [32][mu]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    if (a.status[prob] != 0 || ctk_singular(a, prob, j)) return;
    const Tile32 t = tile32_at(blockIdx.x, a.tm, mx);
    const int i0 = t.i0, j0 = t.j0;
    double* Sn = a.P + ((size_t)((j + 1) & 1) * a.nprob + prob) * mx * mx;
    const double* Tt = a.W + (size_t)prob * mx * na;
    const double* AbT = a.Abar + (size_t)prob * mx * mx;
    const double* AD = ctk_model(a, prob, j);
    const double* Wp = c.Wu ? c.Wu + (long long)prob * c.wu_stride : nullptr;
    double *DWi = dt, *Dj = dt + mu * 32;
    for (int e = tid; e < mu * 32; e += TILE_THREADS) {
        const int x = e / mu, q = e - x * mu;
        double s = 0.0;
        if (Wp && i0 + x < mx)
            for (int p = 0; p < mu; p++) s += AD[(size_t)(i0 + x) * na + mx + p] * Wp[p * mu + q];
        DWi[e] = s;
        Dj[e] = (j0 + x < mx) ? AD[(size_t)(j0 + x) * na + mx + q] : 0.0;
    }
    tile32_product(t, mx, Tt, 1, AbT, 0, red);      // T Abar', T read from its transpose
    for (int e = tid; e < 1024; e += TILE_THREADS) {
        const int ii = e >> 5, jj = e & 31, i = i0 + ii, q = j0 + jj;
        if (i < mx && q < mx) {
            double v = tile32_sum(red, e);                                            // Σ_{j+1} = Abar Σ_j Abar' + (D Wu) D'
            for (int p = 0; p < mu; p++) v += DWi[ii * mu + p] * Dj[jj * mu + p];
            Sn[(size_t)i * mx + q] = v;
        }
    }
}

hipError_t launch_covariance_tracking(const CtkArgs& v, hipStream_t stream) {
    const RicArgs& a = v.r;
    if (a.nprob <= 0) return hipSuccess;
    RicGrid g = ric_grid_of(a);      // (the record also carries a.R, its stride and a.stop: no tracking kernel and no projection kernel reads them)
    g.Q = g.P; g.q_stride = (long long)a.mx * a.mx;      // the projection's "Pk = Q" copies Σ_0 onto itself
    CtkGrid c;
    memset(&c, 0, sizeof(c));
    c.Kin = v.k.Kin; c.k_stride = v.k.k_stride; c.nK = v.k.nK;
    c.Wu = a.mu > 0 ? v.n.Wu : nullptr; c.S0 = v.n.Sigma0; c.wu_stride = v.n.wu_stride; c.s0_stride = v.n.s0_stride;
    c.Q = v.w.Q; c.R = v.w.R; c.q_stride = v.w.q_stride; c.r_stride = v.w.r_stride;
    c.Sigma = v.Sigma; c.Sigma_all = v.Sigma_all; c.mom = v.mom; c.total = v.total;
    hipError_t e = launch_lds<false>(ctk_init_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, c);
    if (e == hipSuccess && a.N > 1) e = launch_ric_project(g, a, stream);      // N = 1: no model is read
    if (e != hipSuccess) return e;
    if (ctk_chosen_path(a.mx, a.mu, a.path) == 1)
        return launch_lds(ctk_resident_kernel, dim3(a.nprob), dim3(CTK_THREADS), ctk_resident_lds_bytes(a.mx, a.mu), stream, g, c);
    const size_t mu = a.mu, mx = a.mx;
    const size_t lds_abar = mu * mx * sizeof(double), lds_next = 2 * mu * 32 * sizeof(double);
    void (*const abar)(RicGrid, CtkGrid, int) = ctk_abar_kernel;
    if (lds_abar > 48 * 1024) {
        e = set_max_dynamic_lds_once((const void*)abar, lds_abar);
        if (e != hipSuccess) return e;
    }
    void (*const next)(RicGrid, CtkGrid, int) = ctk_next_kernel;      // 32 KB of static LDS beside its dynamic 2 mu 32 doubles: raised once per call, whatever mu
    e = set_max_dynamic_lds_once((const void*)next, lds_next);
    if (e != hipSuccess) return e;
    for (int j = 0; j < a.N; j++) {
        e = launch_lds<false>(ctk_moments_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, c, j);
        if (j == a.N - 1 || e != hipSuccess) break;
        e = launch_lds<false>(abar, dim3((a.mx + CTK_RU - 1) / CTK_RU, a.nprob), dim3(TILE_THREADS), lds_abar, stream, g, c, j);
        if (e == hipSuccess) e = launch_lds<false>(ctk_t_kernel, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), 0, stream, g, j);
        if (e == hipSuccess) e = launch_lds<false>(next, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), lds_next, stream, g, c, j);
        if (e != hipSuccess) break;
    }
    return e;
}

}  // namespace cclqr
