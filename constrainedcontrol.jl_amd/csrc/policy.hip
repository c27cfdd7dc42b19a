// policy.hip -- policy evaluation: the cost recursion of dlqr (src/control/lqr.jl:147-177) with the gain GIVEN instead of solved for.  Line 160 (Kk = M\b) is
// replaced by "Kuk = K_t[k]"; the second block row of M Kk = b (lqr.jl:154-160) does not involve Pk, so Kλk = (G Bλ) \ (G (A - Bu Kuk)) whatever the gain, and
//   Abar = A - Bu Kuk - Bλ Kλk = A' - D Kuk          (lqr.jl:169; A', D: the projection of riccati.hip, ric_project_kernel -- the one copy, launched from here too)
//   Pkp1 = Q + Kuk' R Kuk + Abar' Pk Abar            (lqr.jl:170)
//   norm(Pk - Pkp1) < tol -> break                   (lqr.jl:172, Frobenius)
// A step is the two mx^3 products of a Riccati step and a rank-mu term; there is no gain solve.  Nothing here assumes a symmetric Pk: the products are taken as
//   V = Abar' Pk   (A operand Abar[k][i], B operand Pk[k][j]: both read along rows), stored TRANSPOSED, Vt[k][i] = V[i][k]
//   Abar' Pk Abar = V Abar   (A operand V[i][k] = Vt[k][i], B operand Abar[k][j]: rows again)
// so every MFMA operand is addressed with the lane's column contiguous, for symmetric and non-symmetric weights alike, and one kernel serves both.
// The same two launch shapes as riccati.hip, chosen by the same rule (ric_chosen_path): RESIDENT, one workgroup per problem; TILED, every step as device-wide
// launches.  Both run on v_mfma_f64_16x16x4_f64 through the tiles of cclqr_riccati_dev.h.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>

namespace cclqr {

#define POL_THREADS 512
#define POL_WAVES (POL_THREADS / 64)
#define POL_TILES 5      // 16x16 tiles of an mx x mx matrix one wavefront holds in registers across a barrier (ResTiles of cclqr_riccati_dev.h)
static_assert(POL_TILES == RES_TILES, "the resident kernel holds its tiles in ResTiles");

// what the policy kernels take besides the Riccati launch record
struct PolGrid {
    const double* Kin;     // gain tables [n_gains][nK][mu][mx], the caller's body order (the models' order)
    long long k_stride;    // doubles between the tables of consecutive problems: 0 = one table shared by all
    int nK;                // rows per table: N - 1 (row k - 1 is the gain of backward step k), or 1 = a stationary gain
    double* dnorm;         // [nprob][2]: norm(Pk - Pkp1) of the last executed step and of the step before it (preset to NaN by the launch)
};
// the gain of backward step k of problem prob
__device__ inline const double* pol_gain(const RicGrid& a, const PolGrid& q, int prob, int k) {
    return q.Kin + (long long)prob * q.k_stride + (size_t)(q.nK > 1 ? k - 1 : 0) * a.mu * a.mx;
}

// =====================================================================================================================
// RESIDENT: one 512-thread workgroup per problem, for every shape the resident Riccati kernel serves (mx % 4 == 0, up to 96 states).  Operand placement:
//   Ab  [mx][mx]  LDS   Abar = A' - D Kuk.  The A operand of V = Abar' Pk and the B operand of V Abar: read by every tile of both products, so it is the matrix
//                       that must not stream.  [A' | D] is constant over the sweep: a stationary gain (nK = 1) forms Abar once, a table of N - 1 rows re-forms
//                       it per step from the L2-resident [A' | D] (mx^2 loads and mu mx^2 multiply-adds against the step's 4 mx^3)
//   X   [mx][mx]  LDS   ONE buffer that holds Pk (B operand of the first product), then Vt (A operand of the second), then Pkp1.  A wavefront keeps the
//                       accumulators of its <= POL_TILES tiles in registers until a barrier says every read of the buffer's old content is done, and only then
//                       stores them.  Three mx^2 matrices do not fit one CU's 160 KB at mx = 84 .. 96 (3 x 56 .. 74 KB); two do.
//   Pg  [mx][mx]  global (buffer 0 of the workspace's P, preset to Q by ric_project_kernel): Pk a second time, touched only elementwise -- the lane that owns
//                       Pkp1[i][j] reads Pk[i][j] for the norm and writes Pkp1[i][j] over it.  mx^2 loads and stores per step, no MFMA operand.
//   Kl, KR [mu][mx], Rl [mu][mu]  LDS   the step's gain, R Kuk, R
// LDS at mx = 84, mu = 7: 2 x 56 448 + 2 x 4 704 + 392 + 80 = 122 776 B; at mx = 96, mu = 7: 2 x 73 728 + 2 x 5 376 + 392 + 80 = 158 680 B of 163 840.
size_t pol_resident_lds_bytes(int mx, int mu) {
    return (2 * (size_t)mx * mx + 2 * (size_t)mu * mx + (size_t)mu * mu + POL_WAVES + 2) * sizeof(double);
}

__global__ __launch_bounds__(POL_THREADS) void policy_resident_kernel(RicGrid a, PolGrid q, double* P_out) {
    extern __shared__ double pl[];
    const int prob = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int mx = a.mx, mu = a.mu, na = a.na, N = a.N;
    lds_double* Ab = (lds_double*)pl;
    lds_double* X = Ab + (size_t)mx * mx;
    lds_double* Kl = X + (size_t)mx * mx;
    lds_double* KR = Kl + (size_t)mu * mx;
    lds_double* Rl = KR + (size_t)mu * mx;
    lds_double* red = Rl + (size_t)mu * mu;
    const double* Qp = ric_Q_of(a, prob);
    const double* AD = a.AD + (size_t)prob * mx * na;          // time-invariant models: one knot per problem
    double* Pg = a.P + (size_t)prob * mx * mx;
    for (int e = tid; e < mx * mx; e += POL_THREADS) X[e] = Qp[e];        // Pk = Q                                  lqr.jl:147
    {
        const double* Rp = ric_R_of(a, prob);
        for (int e = tid; e < mu * mu; e += POL_THREADS) Rl[e] = Rp[e];
    }
    __syncthreads();
    const int t16 = (mx + 15) >> 4, ntile = t16 * t16, ng = mx >> 2;
    double dn0 = __builtin_nan(""), dn1 = __builtin_nan("");
    int k = 0, status = 0;
    for (k = N - 1; k >= 1; k--) {                                        // for outer k=N-1:-1:1                    lqr.jl:150
        if (ric_knot_singular(a, prob, k)) { status = CCLQR_ESINGULAR_; break; }       // G Bλ singular            lqr.jl:151
        if (k == N - 1 || q.nK > 1) {
            const double* Kp = pol_gain(a, q, prob, k);
            for (int e = tid; e < mu * mx; e += POL_THREADS) Kl[e] = Kp[e];            // Kuk = K_t[k]: the gain is given (in place of lqr.jl:160)
            __syncthreads();
            for (int e = tid; e < mu * mx; e += POL_THREADS) {
                const int r = e / mx, j = e - r * mx;
                KR[e] = ric_rk_entry(Rl, mx, mu, r, j, Kl);
            }
            for (int i = tid >> 5; i < mx; i += POL_THREADS / 32)         // Abar = A' - D Kuk (= A-Bu*Kuk-Bλ*Kλk)   lqr.jl:169
                for (int j = tid & 31; j < mx; j += 32) Ab[i * mx + j] = ric_abar_entry(AD, na, mx, mu, i, j, Kl);
            __syncthreads();
        }
        // The tile loops below are res_mul / res_each of cclqr_riccati_dev.h written out: on those functions this kernel compiled to the same resources and the
        // same MFMA, LDS and memory instructions but 53 more scalar and address instructions, and 4096 problems of 24 states ran 2.7 % slower (profiles/r23)
        ResTiles acc = res_zero();
        // V = Abar' Pk: this wavefront's tiles, kept in registers
#pragma unroll 1
        for (int t = 0; t < POL_TILES && wave + POL_WAVES * t < ntile; t++) {      // (one copy of the tile's loop; the result goes to its register slot by selects)
            const int tile = wave + POL_WAVES * t;
            const int i0 = (tile / t16) << 4, j0 = (tile % t16) << 4;
            const int ic = (i0 + li < mx) ? i0 + li : mx - 1, jc = (j0 + li < mx) ? j0 + li : mx - 1;
            const v4d r = wave_tile16_db(ng, Ab + lk * mx + ic, 4 * mx, X + lk * mx + jc, 4 * mx);
            acc.put(t, r);
        }
        __syncthreads();      // every wavefront has read Pk: the buffer may take Vt
#pragma unroll 1
        for (int t = 0; t < POL_TILES && wave + POL_WAVES * t < ntile; t++) {
            const int tile = wave + POL_WAVES * t;
            const int i0 = (tile / t16) << 4, j = ((tile % t16) << 4) + li;
            const v4d v = acc.pick(t);
            if (j < mx) {
#pragma unroll
                for (int r = 0; r < 4; r++) { const int i = i0 + lk + 4 * r; if (i < mx) X[j * mx + i] = v[r]; }      // Vt[j][i] = V[i][j]
            }
        }
        __syncthreads();
        // Abar' Pk Abar = V Abar
#pragma unroll 1
        for (int t = 0; t < POL_TILES && wave + POL_WAVES * t < ntile; t++) {
            const int tile = wave + POL_WAVES * t;
            const int i0 = (tile / t16) << 4, j0 = (tile % t16) << 4;
            const int ic = (i0 + li < mx) ? i0 + li : mx - 1, jc = (j0 + li < mx) ? j0 + li : mx - 1;
            const v4d r = wave_tile16_db(ng, X + lk * mx + ic, 4 * mx, Ab + lk * mx + jc, 4 * mx);
            acc.put(t, r);
        }
        __syncthreads();      // every wavefront has read Vt: the buffer may take Pkp1
        // Pkp1 = Q + Kuk'*R*Kuk + Abar'*Pk*Abar; |Pk - Pkp1|^2 on the way                                           lqr.jl:170-176
        double nacc = 0.0;
#pragma unroll 1
        for (int t = 0; t < POL_TILES && wave + POL_WAVES * t < ntile; t++) {
            const int tile = wave + POL_WAVES * t;
            const int i0 = (tile / t16) << 4, j = ((tile % t16) << 4) + li;
            const v4d va = acc.pick(t);
            if (j < mx) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = i0 + lk + 4 * r;
                    if (i < mx) {
                        double v = Qp[(size_t)i * mx + j] + va[r];
                        for (int c = 0; c < mu; c++) v += Kl[c * mx + i] * KR[c * mx + j];
                        const double d = Pg[(size_t)i * mx + j] - v;
                        nacc += d * d;
                        Pg[(size_t)i * mx + j] = v;      // Pk = Pkp1 (lqr.jl:176), both copies
                        X[i * mx + j] = v;
                    }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) nacc += __shfl_xor(nacc, o, 64);
        if (lane == 0) red[wave] = nacc;
        __syncthreads();      // (also: Pkp1 is complete; red is not written again before the barriers of the next step's products)
        double tot = 0.0;
        for (int w = 0; w < POL_WAVES; w++) tot += red[w];
        dn1 = dn0; dn0 = sqrt(tot);
        if (dn0 < a.tol) break;                                           // if norm(Pk-Pkp1) < tol  break           lqr.jl:172-174
    }
    if (status == 0) {
        if (k < 1 && N - 1 >= 1) k = 1;   // Julia: after a completed loop the outer k holds its last value
        if (N - 1 < 1) k = 0;
        __syncthreads();
        // the last Pkp1 computed: of the step the test fired on, of step 1 when it never fired, Q when N = 1
        double* Po = P_out + (size_t)prob * mx * mx;
        for (int e = tid; e < mx * mx; e += POL_THREADS) Po[e] = X[e];
    }
    if (tid == 0) { a.kbreak[prob] = k; a.status[prob] = status; q.dnorm[2 * prob] = dn0; q.dnorm[2 * prob + 1] = dn1; }
}

// =====================================================================================================================
// TILED: every other shape (mx % 4 != 0, mx > 96: the 17-body chain's 204 states) and single large problems.  One step = three launches over the problems:
//   pol_abar_kernel   break test of the step before (from its per-tile sums, on the device); Abar = A' - D Kuk, R Kuk     (blocks of POL_RU rows)
//   pol_v_kernel      Vt = (Abar' Pk)'                                                                                  (32x32 tiles, edge tiles masked)
//   pol_pn_kernel     Pkp1 = Q + Kuk' R Kuk + V Abar into the other P buffer; per-tile |Pk - Pkp1|^2                      (32x32 tiles)
// and pol_finish_kernel once.  A problem that has met the break criterion raises its stop flag and its later launches return at once: no host round trip per
// step.  Sums are taken per tile and then over the tiles in index order, so the result does not depend on scheduling.  The workspace is the Riccati's
// (ric_lay_out): W holds Vt, KRK holds R Kuk.
#define POL_RU 16

// has problem `prob` stopped, or does the step before this one (k + 1) meet the break criterion?  Uniform over the workgroup: 0 go on, 1 stopped before,
// 2 the test of step k + 1 fires, 3 the step's G Bλ is singular.  The lead workgroup records the norm it sums
__device__ inline int pol_stopped(const RicGrid& a, const PolGrid& q, int prob, int k, bool lead, int* flag) {
    if (threadIdx.x < 64) {
        const int ntile = a.tm * a.tm;
        int st = a.stop[prob];
        if (!st && k < a.N - 1) {
            const double* part = a.part + ((size_t)((k + 1) & 1) * a.nprob + prob) * ntile;
            double tot = 0.0;
            for (int t = threadIdx.x; t < ntile; t += 64) tot += part[t];
            for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
            const double nrm = sqrt(tot);
            if (lead && threadIdx.x == 0) { q.dnorm[2 * prob + 1] = q.dnorm[2 * prob]; q.dnorm[2 * prob] = nrm; }
            if (nrm < a.tol) st = 2;                                                  // if norm(Pk-Pkp1) < tol  break    lqr.jl:172-174
        }
        if (!st && ric_knot_singular(a, prob, k)) st = 3;                             // G Bλ singular                    lqr.jl:151
        if (threadIdx.x == 0) *flag = st;
    }
    __syncthreads();
    return *flag;
}

__global__ __launch_bounds__(TILE_THREADS) void pol_abar_kernel(RicGrid a, PolGrid q, int k) {
    extern __shared__ double kl[];      // Kuk [mu][mx]
    __shared__ int flag;
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    const bool lead = blockIdx.x == 0;
    const int st = pol_stopped(a, q, prob, k, lead, &flag);
    if (st) {
        if (lead && tid == 0 && st == 2) { a.stop[prob] = 1; a.kbreak[prob] = k + 1; }
        if (lead && tid == 0 && st == 3) { a.status[prob] = CCLQR_ESINGULAR_; a.stop[prob] = 1; a.kbreak[prob] = k; }
        return;
    }
    const double* Kp = pol_gain(a, q, prob, k);
    for (int e = tid; e < mu * mx; e += TILE_THREADS) kl[e] = Kp[e];                  // Kuk = K_t[k]: the gain is given (in place of lqr.jl:160)
    __syncthreads();
    if (lead) {
        const double* Rp = ric_R_of(a, prob);
        double* KR = a.KRK + (size_t)prob * mu * mx;
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {
            const int r = e / mx, j = e - r * mx;
            KR[e] = ric_rk_entry(Rp, mx, mu, r, j, kl);
        }
    }
    const double* AD = a.AD + (size_t)prob * mx * na;
    double* Abar = a.Abar + (size_t)prob * mx * mx;
    for (int r = 0; r < POL_RU; r++) {
        const int i = blockIdx.x * POL_RU + r;
        if (i >= mx) break;
        for (int j = tid; j < mx; j += TILE_THREADS) Abar[(size_t)i * mx + j] = ric_abar_entry(AD, na, mx, mu, i, j, kl);      // Abar = A' - D Kuk   lqr.jl:169
    }
}

__global__ __launch_bounds__(TILE_THREADS) void pol_v_kernel(RicGrid a, int k) {
    __shared__ double red[4][1024];
    const int prob = blockIdx.y, mx = a.mx;
    if (a.stop[prob]) return;           // pol_abar_kernel of this step has evaluated the break test
    const double* P = a.P + ((size_t)((a.N - 1 - k) & 1) * a.nprob + prob) * mx * mx;
    tile32_product_transposed(tile32_at(blockIdx.x, a.tm, mx), mx, a.Abar + (size_t)prob * mx * mx, P, a.W + (size_t)prob * mx * a.na, red);      // Vt = (Abar' Pk)'
}

__global__ __launch_bounds__(TILE_THREADS) void pol_pn_kernel(RicGrid a, PolGrid q, int k) {
    __shared__ double red[4][1024];
    extern __shared__ double kt[];      // KuI [mu][32] | KRJ [mu][32]
    __shared__ double wsum[4];
    const int prob = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int mx = a.mx, mu = a.mu;
    if (a.stop[prob]) return;
    const Tile32 t = tile32_at(blockIdx.x, a.tm, mx);
    const int i0 = t.i0, j0 = t.j0;
    const double* P = a.P + ((size_t)((a.N - 1 - k) & 1) * a.nprob + prob) * mx * mx;
    double* Pn = a.P + ((size_t)((a.N - k) & 1) * a.nprob + prob) * mx * mx;
    const double* Vt = a.W + (size_t)prob * mx * a.na;
    const double* Abar = a.Abar + (size_t)prob * mx * mx;
    const double* Kp = pol_gain(a, q, prob, k);
    const double* KR = a.KRK + (size_t)prob * mu * mx;
    const double* Qp = ric_Q_of(a, prob);
    double *KuI = kt, *KRJ = kt + mu * 32;
    for (int e = tid; e < mu * 32; e += TILE_THREADS) {
        const int c = e >> 5, x = e & 31;
        KuI[e] = (i0 + x < mx) ? Kp[(size_t)c * mx + i0 + x] : 0.0;
        KRJ[e] = (j0 + x < mx) ? KR[(size_t)c * mx + j0 + x] : 0.0;
    }
    tile32_product(t, mx, Vt, 1, Abar, 0, red);      // V Abar, V read from its transpose
    double acc = 0.0;
    for (int e = tid; e < 1024; e += TILE_THREADS) {
        const int ii = e >> 5, jj = e & 31, i = i0 + ii, j = j0 + jj;
        if (i < mx && j < mx) {
            double v = Qp[(size_t)i * mx + j] + tile32_sum(red, e);      // Pkp1 = Q + Kuk'*R*Kuk + Abar'*Pk*Abar   lqr.jl:170
            for (int c = 0; c < mu; c++) v += KuI[c * 32 + ii] * KRJ[c * 32 + jj];
            Pn[(size_t)i * mx + j] = v;
            const double d = P[(size_t)i * mx + j] - v;
            acc += d * d;
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.part[((size_t)(k & 1) * a.nprob + prob) * (a.tm * a.tm) + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// the loop variable's final value, the norm of step 1 (its test has no later launch to be evaluated in) and the cost-to-go of the last executed step:
// pol_pn_kernel of step k wrote buffer (N - k) & 1, and a break is detected by the NEXT step's pol_abar_kernel, which stops the problem before anything
// overwrites that buffer.  N = 1: no step ran, buffer 0 holds Q (ric_project_kernel)
__global__ void pol_finish_kernel(RicGrid a, PolGrid q, double* P_out) {
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, N = a.N;
    __shared__ int kb;
    if (tid < 64) {
        const bool ran_out = !a.stop[prob] && N - 1 >= 1;      // step 1 was executed and its norm not yet summed
        if (ran_out) {
            const int ntile = a.tm * a.tm;
            const double* part = a.part + ((size_t)(1 & 1) * a.nprob + prob) * ntile;
            double tot = 0.0;
            for (int t = tid; t < ntile; t += 64) tot += part[t];
            for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
            if (tid == 0) { q.dnorm[2 * prob + 1] = q.dnorm[2 * prob]; q.dnorm[2 * prob] = sqrt(tot); }
        }
        if (tid == 0) {
            const int k = a.stop[prob] ? a.kbreak[prob] : (N - 1 >= 1 ? 1 : 0);      // (the test after step 1 is a break at k = 1 as well: same index)
            a.kbreak[prob] = k;
            kb = k;
        }
    }
    __syncthreads();
    if (a.status[prob] != 0) return;
    const double* Pl = a.P + ((size_t)(kb >= 1 ? (N - kb) & 1 : 0) * a.nprob + prob) * mx * mx;
    double* Po = P_out + (size_t)prob * mx * mx;
    for (int e = tid; e < mx * mx; e += blockDim.x) Po[e] = Pl[e];
}

hipError_t launch_policy(const PolArgs& p, hipStream_t stream) {
    const RicArgs& a = p.r;
    if (a.nprob <= 0) return hipSuccess;
    RicGrid g = ric_grid_of(a);
    g.tol = a.tol;
    PolGrid q;
    q.Kin = p.k.Kin; q.k_stride = p.k.k_stride; q.nK = p.k.nK; q.dnorm = p.dnorm;
    const size_t np = a.nprob, mu = a.mu, mx = a.mx;
    hipError_t e = hipMemsetAsync(a.stop, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.status, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.kbreak, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.dnorm, 0xff, 2 * np * sizeof(double), stream);      // all bits set: a NaN, "no such step ran"
    if (e == hipSuccess) e = launch_ric_project(g, a, stream);
    if (e != hipSuccess) return e;
    // resident wherever the Riccati is (ric_chosen_path: the same shapes, the same crossover), provided a wavefront's share of the tiles fits its registers -- mx <= 96;
    // the one shape beyond it the Riccati's rule lets through (100 states without inputs) runs tiled
    if (ric_chosen_path(a) == 1 && res_tiles_serve(a.mx, POL_WAVES) && pol_resident_lds_bytes(a.mx, a.mu) <= 158 * 1024)
        return launch_lds(policy_resident_kernel, dim3(a.nprob), dim3(POL_THREADS), pol_resident_lds_bytes(a.mx, a.mu), stream, g, q, a.P_out);
    const size_t lds_abar = mu * mx * sizeof(double), lds_pn = 2 * mu * 32 * sizeof(double);
    void (*const abar)(RicGrid, PolGrid, int) = pol_abar_kernel;
    if (lds_abar > 48 * 1024) {
        e = set_max_dynamic_lds_once((const void*)abar, lds_abar);
        if (e != hipSuccess) return e;
    }
    for (int k = a.N - 1; k >= 1; k--) {                                 // for outer k=N-1:-1:1                    lqr.jl:150
        e = launch_lds<false>(abar, dim3((a.mx + POL_RU - 1) / POL_RU, a.nprob), dim3(TILE_THREADS), lds_abar, stream, g, q, k);
        if (e == hipSuccess) e = launch_lds<false>(pol_v_kernel, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), 0, stream, g, k);
        if (e == hipSuccess) e = launch_lds<false>(pol_pn_kernel, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), lds_pn, stream, g, q, k);
        if (e != hipSuccess) return e;
    }
    return launch_lds<false>(pol_finish_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, q, a.P_out);
}

}  // namespace cclqr
