// policy_tracking.hip -- the cost-to-go of a TRACKED run at every knot: policy.hip's backward recursion with a model and a gain row per knot, the adjoint of
// covariance_tracking.hip.  A TrackingLQR applies the gain row Ku[j] at knot j (src/control/lqr_tracking.jl:65, gated by k < N at line 63) on the model linearised at
// knot j (lqr_tracking.jl:88-89).  Knots are j = 0 .. N-1 as in covariance_tracking.hip.  With [A'_j | D_j] the projected pair of knot j (ric_project_kernel -- the
// one copy, launched from here too) and the gain GIVEN (the Pkp1 of lqr_tracking.jl:108 with the gain of line 98 handed in instead of solved for):
//   Abar_j  = A'_j - D_j K_j                                   (lqr_tracking.jl:107)
//   P_{N-1} = Q
//   P_j     = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j          j = N-2 .. knot                                 (lqr_tracking.jl:108)
//   price_j = tr(Wu D_j' P_{j+1} D_j)                          j = N-2 .. knot;   price_{N-1} = 0, and 0 below `knot`
//   total   = sum_j price_j, in the order the recursion produces them (j = N-2 downwards)
// price_j is what the noise sample w ~ (0, Wu) injected at step j + 1 (examples/trackingLQR_triple_cartpole.jl:98) adds to the expected cost of the rest of the
// run, so that with covariance_tracking.hip's Σ and costs:  sum_j (cx_j + cu_j) = tr(P_0 Σ_0) + sum_j price_j.
// Q, R, Wu are used as written; nothing assumes symmetry.  N = 1: P = Q and no model is read.  nlin = 1 (one time-invariant model) and nK = 1 (one stationary gain)
// are served by the same kernels.  The products are policy.hip's:
//   V = Abar' P    (A operand Abar[k][i], B operand P[k][j]: both read along rows), stored TRANSPOSED, Vt[k][i] = V[i][k]
//   V Abar         (A operand Vt[k][i], B operand Abar[k][j]: rows again)
// Two launch shapes: RESIDENT, one workgroup per problem over all knots; TILED, every step as device-wide launches.  Both run on v_mfma_f64_16x16x4_f64 through
// the tiles of cclqr_riccati_dev.h.  Every sum is taken in an order fixed by the sizes alone: a result depends neither on scheduling nor on the batch, nor on
// which outputs are asked for.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>

namespace cclqr {

#define PTK_THREADS 512
#define PTK_WAVES (PTK_THREADS / 64)
#define PTK_TILES 5      // 16x16 tiles one wavefront holds across a barrier (ResTiles of cclqr_riccati_dev.h)
#define PTK_PRE 18       // doubles of the next knot's A' one lane holds while the products run: ceil(96 * 96 / 512)
#define PTK_PRE_S 2      // ... and of its D, of its K and of R K: ceil(mu mx / 512) (ptk_resident_fits)

// what the kernels take besides the Riccati launch record (whose Q, R and strides are the stage-cost weights here)
struct PtkGrid {
    const double* Kin;         // gain tables [n_gains][nK][mu][mx], the models' state order
    long long k_stride;        // doubles between the tables of consecutive problems: 0 = one table shared by all
    int nK;                    // rows per table: N - 1 (row j = the gain of knot j) or 1 = a stationary gain
    int knot;                  // the recursion stops at this knot: P = P_knot
    const double* Wu;          // [n_noise][mu][mu]; null: no price is taken
    long long wu_stride;
    double *P, *P_all;         // [nprob][mx][mx], [nprob][N][mx][mx]; each may be null
    double *price, *total;     // [nprob][N], [nprob]; both null when Wu is
};
__device__ inline const double* ptk_gain(const RicGrid& a, const PtkGrid& c, int prob, int j) {
    return c.Kin + (long long)prob * c.k_stride + (long long)(c.nK > 1 ? j : 0) * a.mu * a.mx;
}
__device__ inline const double* ptk_model(const RicGrid& a, int prob, int j) {
    return a.AD + ((long long)prob * a.nlin + (a.nlin > 1 ? j : 0)) * a.mx * a.na;
}
// is G Bλ of knot j's model singular (ric_knot_singular counts backward steps: knot j is the model of step j + 1)
__device__ inline bool ptk_singular(const RicGrid& a, int prob, int j) { return ric_knot_singular(a, prob, j + 1); }
// buffer of the workspace's P that holds P_j: P_{N-1} = Q lies in buffer 0 (ric_project_kernel, ptk_init_kernel), every step writes the other one
__device__ inline double* ptk_P_of(const RicGrid& a, int prob, int j) { return a.P + ((size_t)((a.N - 1 - j) & 1) * a.nprob + prob) * a.mx * a.mx; }

// One lane's share of the price of knot j, tr(Wu D' P D) = sum_{i,p} (P D)[i][p] (D Wu')[i][p]: the elements e = i mu + p, e = tid, tid + nthreads, .. in that
// order, each (P D)[i][p] summed over k upwards.  P [mx][mx] and D (row stride ds) are read through pointers of any address space; Wl [mu][mu]
template <class PP, class PD, class PW>
__device__ __forceinline__ double ptk_price_share(int mx, int mu, int ms, int tid, int nthreads, PP P, PD D, int ds, PW Wl) {
    double s = 0.0;
#pragma unroll 1
    for (int e = tid; e < ms; e += nthreads) {
        const int i = e / mu, p = e - i * mu;
        double pd = 0.0, w = 0.0;
#pragma unroll 1
        for (int k = 0; k < mx; k++) pd += P[i * mx + k] * D[k * ds + p];
#pragma unroll 1
        for (int q = 0; q < mu; q++) w += Wl[p * mu + q] * D[i * ds + q];
        s += pd * w;
    }
    return s;
}
// ... summed over a workgroup of nw wavefronts: the lanes by the shuffle tree into red[wave]; after a barrier ptk_price_total adds the wavefronts in index order
__device__ __forceinline__ double ptk_price_wave(double s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
template <class PR>
__device__ __forceinline__ double ptk_price_total(PR red, int nw) {
    double t = 0.0;
#pragma unroll 1
    for (int w = 0; w < nw; w++) t += red[w];
    return t;
}

// =====================================================================================================================
// RESIDENT: one 512-thread workgroup per problem, persistent over all knots j = N-2 .. knot, for exactly the shapes ctk_resident_kernel serves
// (ptk_resident_fits).  Operand placement:
//   Ab  [mx][mx]  LDS   Abar_j -- the A operand of V = Abar' P and the B operand of V Abar: read by every tile of both products
//   X   [mx][mx]  LDS   ONE buffer: P_{j+1} (B operand of the first product), then Vt (A operand of the second), then P_j.  A wavefront keeps the accumulators
//                       of its <= PTK_TILES tiles in registers until a barrier says every read of the old content is done
//   Da  [mx][mu]  LDS   D_j while the price of the knot is taken and Abar_j is formed; then R K_j [mu][mx] for the epilogue.  A third mu mx panel would not fit
//                       beside two mx^2 buffers at (96, 7): 164 432 B of 163 840
//   Kb  [mu][mx]  LDS   K_j
//   Wl, Rl [mu][mu] LDS Wu, R
//   registers           (P_{j+1} D_j)[i][p] of the price, never stored: the lane that owns element (i, p) multiplies it by (D_j Wu')[i][p] at once;
//                       R K_j (PTK_PRE_S per lane) from the barrier that completes K_j to the one that retires D_j;
//                       knot j - 1's A' (PTK_PRE doubles per lane), D and K (PTK_PRE_S each): REQUESTED before knot j's products, after Abar_j has consumed knot
//                       j's, and written to LDS after the barrier that retires Abar_j.  Lane e owns A'[i][jj], e = i mx + jj: consecutive lanes read consecutive
//                       words of the model and write consecutive LDS words of Abar
// Barriers per step: six -- D_j and K_j in place; price shares, Abar_j and R K_j taken (D_j retired); P_{j+1} read; Vt stored; Vt read; P_j stored.
// LDS at mx = 84, mu = 7: 2 x 56 448 + 2 x 4 704 + 2 x 392 + 64 = 123 152 B; at mx = 96, mu = 7: 2 x 73 728 + 2 x 5 376 + 2 x 392 + 64 = 159 056 B of 163 840.
size_t ptk_resident_lds_bytes(int mx, int mu) {
    return (2 * (size_t)mx * mx + 2 * (size_t)mu * mx + 2 * (size_t)mu * mu + PTK_WAVES) * sizeof(double);
}
// THE fit rule of the resident kernel: whole k-groups of four, a wavefront's share of the tiles in its registers (mx <= 96), a lane's share of the next knot's
// model in its registers, and the operands in one CU's LDS
bool ptk_resident_fits(int mx, int mu) {
    return res_tiles_serve(mx, PTK_WAVES) && mx * mx <= PTK_PRE * PTK_THREADS && mu * mx <= PTK_PRE_S * PTK_THREADS && ptk_resident_lds_bytes(mx, mu) <= 158 * 1024;
}
int ptk_chosen_path(int mx, int mu, int path) { return (path != 2 && ptk_resident_fits(mx, mu)) ? 1 : 2; }

// a wave-uniform value, hidden from loop-invariant code motion
__device__ __forceinline__ int ptk_opaque_s(int x) { asm volatile("" : "+s"(x)); return x; }

static_assert(PTK_TILES == RES_TILES, "the resident kernel holds its tiles in ResTiles");

// the sizes a knot's code is written in, derived from (mx, mu)
struct PtkSizes {
    int mx, mu, na, mm, ms, t16, ntile, ng;
    lds_double *Ab, *X, *Da, *Kb, *Wl, *Rl, *red;
    __device__ __forceinline__ PtkSizes(int mx_, int mu_, double* lds) : mx(mx_), mu(mu_), na(mx_ + mu_), mm(mx_ * mx_), ms(mu_ * mx_), t16((mx_ + 15) >> 4), ng(mx_ >> 2) {
        ntile = t16 * t16;
        Ab = (lds_double*)lds; X = Ab + mm; Da = X + mm; Kb = Da + ms; Wl = Kb + ms; Rl = Wl + mu * mu; red = Rl + mu * mu;
    }
};

__global__ __launch_bounds__(PTK_THREADS) void ptk_resident_kernel(RicGrid a, PtkGrid c) {
    extern __shared__ double sl[];
    const int prob = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int N = a.N;
    const double* Qp = ric_Q_of(a, prob);
    // what moves from knot to knot is carried as running pointers, walked DOWNWARDS: the model, the gain and the singular flag of the knot requested next, the
    // P_all block of the knot at hand
    const double *ADn, *Kn;
    const int* sgn;
    int adstep, kstep;
    const int sgstep = a.nlin > 1 ? a.ml + 2 : 0;
    double* pa;
    double* const pr = c.price ? c.price + (size_t)prob * N : nullptr;
    {
        const PtkSizes z(a.mx, a.mu, sl);
        const double* Wp = c.Wu ? c.Wu + (long long)prob * c.wu_stride : nullptr;
        const double* Rp = ric_R_of(a, prob);
        for (int e = tid; e < z.mm; e += PTK_THREADS) z.X[e] = Qp[e];                 // P_{N-1} = Q
        for (int e = tid; e < z.mu * z.mu; e += PTK_THREADS) { z.Wl[e] = Wp ? Wp[e] : 0.0; z.Rl[e] = Rp[e]; }
        const int jl = N - 2;      // the first knot stepped (N = 1: none, and nothing below is dereferenced)
        ADn = ptk_model(a, prob, jl);
        Kn = z.mu > 0 ? ptk_gain(a, c, prob, jl) : nullptr;
        sgn = ric_knot_piv(a, (size_t)prob * a.nlin) + (long long)(a.nlin > 1 ? jl : 0) * (a.ml + 2) + a.ml;
        adstep = a.nlin > 1 ? z.mx * z.na : 0; kstep = c.nK > 1 ? z.ms : 0;
        pa = nullptr;
        if (c.P_all) {
            double* top = c.P_all + ((size_t)prob * N + (N - 1)) * z.mm;
            for (int e = tid; e < z.mm; e += PTK_THREADS) top[e] = Qp[e];
            pa = top - z.mm;
        }
        if (pr)
            for (int j = tid; j < N; j += PTK_THREADS)
                if (j < c.knot || j == N - 1) pr[j] = 0.0;
    }
    bool singn = false;
    const bool reform = a.nlin > 1 || c.nK > 1;      // Abar changes from knot to knot
    double pre[PTK_PRE], pd[PTK_PRE_S], pk[PTK_PRE_S], rk[PTK_PRE_S];
    int status = 0, knot = -1;
    double tn = 0.0;      // thread 0: the prices, in the order the recursion produces them
    __syncthreads();
    for (int j = N - 1; j >= c.knot; j--) {      // (j = N - 1 only requests knot N - 2's model)
        // Every size-derived value of the knot's code is derived HERE, from values the compiler cannot see through (ctk_resident_kernel says why)
        const PtkSizes z(ptk_opaque_s(a.mx), ptk_opaque_s(a.mu), sl);
        const int mx = z.mx, mu = z.mu, na = z.na, ms = z.ms;
        const ResShape rs = {mx, z.t16, z.ntile, z.ng, wave, li, lk, PTK_WAVES};
        lds_double *const Ab = z.Ab, *const X = z.X, *const Da = z.Da, *const Kb = z.Kb, *const Wl = z.Wl, *const Rl = z.Rl, *const red = z.red;
        // this lane's elements of A' / Abar: e = tid + 512 r = i mx + jj, walked by increments (no division per element)
        const int i0 = tid / mx, j0 = tid % mx, di = PTK_THREADS / mx, dj = PTK_THREADS % mx;
        const bool step = j < N - 1;
        if (step) {
            if (singn) { status = CCLQR_ESINGULAR_; knot = j; break; }      // G Bλ singular                   lqr_tracking.jl:89
            const bool form = j == N - 2 || reform;
            // knot j's D and K, requested a step ago (or kept: a stationary pair), into LDS: both panels and Ab are dead by now
#pragma unroll
            for (int r = 0; r < PTK_PRE_S; r++) {
                const int e = tid + PTK_THREADS * r;
                if (e < ms) { Da[e] = pd[r]; Kb[e] = pk[r]; }
            }
            __syncthreads();
            if (pr) {      // the price of knot j while P_{j+1} is still in X
                const double s = ptk_price_wave(ptk_price_share(mx, mu, ms, tid, PTK_THREADS, X, Da, mu, Wl));
                if (lane == 0) red[wave] = s;
            }
            if (form) {
                int i = i0, jj = j0;
#pragma unroll
                for (int r = 0; r < PTK_PRE; r++) {
                    if (i < mx) {
                        double s = pre[r];                                    // Abar = A' - D K (= A-Bu*Ku-Bλ*Kλ)   lqr_tracking.jl:107
#pragma unroll 1
                        for (int p = 0; p < mu; p++) s -= Da[i * mu + p] * Kb[p * mx + jj];
                        Ab[i * mx + jj] = s;
                    }
                    i += di; jj += dj;
                    if (jj >= mx) { jj -= mx; i++; }
                }
#pragma unroll
                for (int r = 0; r < PTK_PRE_S; r++) {
                    const int e = tid + PTK_THREADS * r;
                    const bool ok = e < ms;
                    const int rr = ok ? e / mx : 0, jj2 = ok ? e - rr * mx : 0;
                    rk[r] = ok ? ric_rk_entry(Rl, mx, mu, rr, jj2, Kb) : 0.0;
                }
            }
            __syncthreads();      // D_j is retired: its panel takes R K_j; the price shares are complete
#pragma unroll
            for (int r = 0; r < PTK_PRE_S; r++) {
                const int e = tid + PTK_THREADS * r;
                if (e < ms) Da[e] = rk[r];
            }
            if (pr && tid == 0) { const double t = ptk_price_total(red, PTK_WAVES); pr[j] = t; tn += t; }
        }
        const bool next = j - 1 >= c.knot;
        singn = next && *sgn != 0;
        if (next && !singn && (j == N - 1 || reform)) {      // REQUEST knot j - 1's A', D and K
            int i = i0, jj = j0;
#pragma unroll
            for (int r = 0; r < PTK_PRE; r++) {
                pre[r] = i < mx ? ADn[(unsigned)(i * na + jj)] : 0.0;
                i += di; jj += dj;
                if (jj >= mx) { jj -= mx; i++; }
            }
#pragma unroll
            for (int r = 0; r < PTK_PRE_S; r++) {
                const int e = tid + PTK_THREADS * r;
                const bool ok = e < ms;
                const int i2 = ok ? e / mu : 0, p = ok ? e - i2 * mu : 0;
                pd[r] = ok ? ADn[(unsigned)(i2 * na + mx + p)] : 0.0;
                pk[r] = ok ? Kn[e] : 0.0;
            }
        }
        ADn -= adstep; Kn -= kstep; sgn -= sgstep;
        if (!step) continue;
        ResTiles acc = res_mul(rs, Ab, X);      // V = Abar' P_{j+1}: this wavefront's tiles, kept in registers
        __syncthreads();      // every wavefront has read P_{j+1}: X may take Vt
        res_each(rs, acc, [&](int i, int q, double v) { X[q * mx + i] = v; });      // Vt[q][i] = V[i][q]
        __syncthreads();
        acc = res_mul(rs, X, Ab);                                                  // V Abar
        __syncthreads();      // every wavefront has read Vt: the buffer may take P_j
        res_each(rs, acc, [&](int i, int q, double v) {                             // P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j   lqr_tracking.jl:108
            double s = Qp[(unsigned)(i * mx + q)] + v;
#pragma unroll 1
            for (int p = 0; p < mu; p++) s += Kb[p * mx + i] * Da[p * mx + q];
            X[i * mx + q] = s;
            if (pa) pa[(unsigned)(i * mx + q)] = s;
        });
        if (pa) pa -= z.mm;
        __syncthreads();      // P_j is complete; Abar_j, K_j and R K_j are retired
    }
    if (status == 0 && c.P) {
        const PtkSizes z(a.mx, a.mu, sl);
        double* Po = c.P + (size_t)prob * z.mm;
        for (int e = tid; e < z.mm; e += PTK_THREADS) Po[e] = z.X[e];
    }
    if (tid == 0) {
        a.status[prob] = status; a.kbreak[prob] = knot;
        if (status == 0 && c.total) c.total[prob] = tn;
    }
}

// =====================================================================================================================
// TILED: every other shape (mx % 4 != 0, mx > 96: any chain of more than 8 bodies) and path = 2.  ptk_init_kernel once, then one step = four launches:
//   ptk_abar_kernel     Abar_j = A'_j - D_j K_j and R K_j; a singular G Bλ sets the problem's status, which stops it     (blocks of PTK_RU rows)
//   ptk_price_kernel    price_j from P_{j+1} and D_j, added to the total                                              (one workgroup per problem; only with Wu)
//   ptk_v_kernel        Vt = (Abar' P_{j+1})'                                                                         (32x32 tiles, edge tiles masked)
//   ptk_pn_kernel       P_j = Q + K_j' R K_j + V Abar into the other buffer of P, into P_all[j], and into P at j = knot   (32x32 tiles)
// P_j lies in buffer (N - 1 - j) & 1 of the workspace's P, Vt in W, R K in KRK (ric_lay_out).
#define PTK_RU 16

__global__ __launch_bounds__(TILE_THREADS) void ptk_init_kernel(RicGrid a, PtkGrid c) {
    const int prob = blockIdx.x, tid = threadIdx.x, N = a.N, mm = a.mx * a.mx;
    const double* Qp = ric_Q_of(a, prob);
    double* P0 = a.P + (size_t)prob * mm;                                           // P_{N-1} = Q (N = 1: no projection runs to write it)
    double* top = c.P_all ? c.P_all + ((size_t)prob * N + (N - 1)) * mm : nullptr;
    double* Po = (c.P && c.knot == N - 1) ? c.P + (size_t)prob * mm : nullptr;
    for (int e = tid; e < mm; e += TILE_THREADS) {
        const double v = Qp[e];
        P0[e] = v;
        if (top) top[e] = v;
        if (Po) Po[e] = v;
    }
    if (c.price)
        for (int j = tid; j < N; j += TILE_THREADS) c.price[(size_t)prob * N + j] = 0.0;
    if (tid == 0) {
        a.status[prob] = 0; a.kbreak[prob] = -1;
        if (c.total) c.total[prob] = 0.0;
    }
}

__global__ __launch_bounds__(TILE_THREADS) void ptk_abar_kernel(RicGrid a, PtkGrid c, int j) {
    extern __shared__ double kl[];      // K_j [mu][mx]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    if (a.status[prob] != 0) return;    // stopped at a later knot
    if (ptk_singular(a, prob, j)) {     // G Bλ singular (every workgroup of the problem sees it by itself; the lead records it)      lqr_tracking.jl:89
        if (blockIdx.x == 0 && tid == 0) { a.status[prob] = CCLQR_ESINGULAR_; a.kbreak[prob] = j; }
        return;
    }
    const double* Kp = mu > 0 ? ptk_gain(a, c, prob, j) : nullptr;
    for (int e = tid; e < mu * mx; e += TILE_THREADS) kl[e] = Kp[e];
    __syncthreads();
    if (blockIdx.x == 0) {
        const double* Rp = ric_R_of(a, prob);
        double* KR = a.KRK + (size_t)prob * mu * mx;
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {
            const int r = e / mx, q = e - r * mx;
            KR[e] = ric_rk_entry(Rp, mx, mu, r, q, kl);
        }
    }
    const double* AD = ptk_model(a, prob, j);
    double* Abar = a.Abar + (size_t)prob * mx * mx;
    for (int r = 0; r < PTK_RU; r++) {
        const int i = blockIdx.x * PTK_RU + r;
        if (i >= mx) break;
        for (int q = tid; q < mx; q += TILE_THREADS) Abar[(size_t)i * mx + q] = ric_abar_entry(AD, na, mx, mu, i, q, kl);      // Abar = A' - D K   lqr_tracking.jl:107
    }
}

__global__ __launch_bounds__(PTK_THREADS) void ptk_price_kernel(RicGrid a, PtkGrid c, int j) {
    __shared__ double red[PTK_WAVES];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu;
    if (a.status[prob] != 0 || ptk_singular(a, prob, j)) return;
    const double* Wp = c.Wu + (long long)prob * c.wu_stride;
    const double s = ptk_price_wave(ptk_price_share(mx, mu, mu * mx, tid, PTK_THREADS, (const double*)ptk_P_of(a, prob, j + 1), ptk_model(a, prob, j) + mx, a.na, Wp));
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const double t = ptk_price_total(red, PTK_WAVES);
        c.price[(size_t)prob * a.N + j] = t;
        c.total[prob] += t;      // launches of one stream: the order the recursion produces them
    }
}

__global__ __launch_bounds__(TILE_THREADS) void ptk_v_kernel(RicGrid a, int j) {
    __shared__ double red[4][1024];
    const int prob = blockIdx.y, mx = a.mx;
    if (a.status[prob] != 0 || ptk_singular(a, prob, j)) return;
    tile32_product_transposed(tile32_at(blockIdx.x, a.tm, mx), mx, a.Abar + (size_t)prob * mx * mx, ptk_P_of(a, prob, j + 1), a.W + (size_t)prob * mx * a.na, red);      // Vt = (Abar' P_{j+1})'
}

__global__ __launch_bounds__(TILE_THREADS) void ptk_pn_kernel(RicGrid a, PtkGrid c, int j) {
    __shared__ double red[4][1024];
    extern __shared__ double kt[];      // K_j of the tile's rows [mu][32] | R K_j of the tile's columns [mu][32]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu;
    if (a.status[prob] != 0 || ptk_singular(a, prob, j)) return;
    const Tile32 t = tile32_at(blockIdx.x, a.tm, mx);
    const int i0 = t.i0, j0 = t.j0;
    double* Pn = ptk_P_of(a, prob, j);
    double* Pa = c.P_all ? c.P_all + ((size_t)prob * a.N + j) * mx * mx : nullptr;
    double* Po = (c.P && j == c.knot) ? c.P + (size_t)prob * mx * mx : nullptr;
    const double* Vt = a.W + (size_t)prob * mx * a.na;
    const double* Abar = a.Abar + (size_t)prob * mx * mx;
    const double* Kp = mu > 0 ? ptk_gain(a, c, prob, j) : nullptr;
    const double* KR = a.KRK + (size_t)prob * mu * mx;
    const double* Qp = ric_Q_of(a, prob);
    double *KuI = kt, *KRJ = kt + mu * 32;
    for (int e = tid; e < mu * 32; e += TILE_THREADS) {
        const int p = e >> 5, x = e & 31;
        KuI[e] = (i0 + x < mx) ? Kp[(size_t)p * mx + i0 + x] : 0.0;
        KRJ[e] = (j0 + x < mx) ? KR[(size_t)p * mx + j0 + x] : 0.0;
    }
    tile32_product(t, mx, Vt, 1, Abar, 0, red);      // V Abar, V read from its transpose
    for (int e = tid; e < 1024; e += TILE_THREADS) {
        const int ii = e >> 5, jj = e & 31, i = i0 + ii, q = j0 + jj;
        if (i < mx && q < mx) {
            double v = Qp[(size_t)i * mx + q] + tile32_sum(red, e);      // P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j   lqr_tracking.jl:108
            for (int p = 0; p < mu; p++) v += KuI[p * 32 + ii] * KRJ[p * 32 + jj];
            Pn[(size_t)i * mx + q] = v;
            if (Pa) Pa[(size_t)i * mx + q] = v;
            if (Po) Po[(size_t)i * mx + q] = v;
        }
    }
}

hipError_t launch_policy_tracking(const PtkArgs& v, hipStream_t stream) {
    const RicArgs& a = v.r;
    if (a.nprob <= 0) return hipSuccess;
    const RicGrid g = ric_grid_of(a);      // (the record also carries a.stop: no kernel here and no projection kernel reads it)
    PtkGrid c;
    memset(&c, 0, sizeof(c));
    c.Kin = v.k.Kin; c.k_stride = v.k.k_stride; c.nK = v.k.nK; c.knot = v.knot;
    const bool priced = a.mu > 0 && v.n.Wu && v.price && v.total;
    c.Wu = priced ? v.n.Wu : nullptr; c.wu_stride = v.n.wu_stride;
    c.P = v.P; c.P_all = v.P_all;
    c.price = v.price; c.total = v.total;      // without a priced noise the init kernel still zeroes them
    hipError_t e = launch_lds<false>(ptk_init_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, c);
    if (e == hipSuccess && a.N - 1 > v.knot) e = launch_ric_project(g, a, stream);      // no step: no model is read
    if (e != hipSuccess || a.N - 1 <= v.knot) return e;
    if (!priced) { c.price = nullptr; c.total = nullptr; }
    if (ptk_chosen_path(a.mx, a.mu, a.path) == 1)
        return launch_lds(ptk_resident_kernel, dim3(a.nprob), dim3(PTK_THREADS), ptk_resident_lds_bytes(a.mx, a.mu), stream, g, c);
    const size_t mu = a.mu, mx = a.mx;
    const size_t lds_abar = mu * mx * sizeof(double), lds_pn = 2 * mu * 32 * sizeof(double);
    void (*const abar)(RicGrid, PtkGrid, int) = ptk_abar_kernel;
    if (lds_abar > 48 * 1024) {
        e = set_max_dynamic_lds_once((const void*)abar, lds_abar);
        if (e != hipSuccess) return e;
    }
    void (*const pn)(RicGrid, PtkGrid, int) = ptk_pn_kernel;      // 32 KB of static LDS beside its dynamic 2 mu 32 doubles: raised once per call, whatever mu
    e = set_max_dynamic_lds_once((const void*)pn, lds_pn);
    if (e != hipSuccess) return e;
    for (int j = a.N - 2; j >= v.knot; j--) {
        e = launch_lds<false>(abar, dim3((a.mx + PTK_RU - 1) / PTK_RU, a.nprob), dim3(TILE_THREADS), lds_abar, stream, g, c, j);
        if (e == hipSuccess && c.price) e = launch_lds<false>(ptk_price_kernel, dim3(a.nprob), dim3(PTK_THREADS), 0, stream, g, c, j);
        if (e == hipSuccess) e = launch_lds<false>(ptk_v_kernel, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), 0, stream, g, j);
        if (e == hipSuccess) e = launch_lds<false>(pn, dim3(g.tm * g.tm, a.nprob), dim3(TILE_THREADS), lds_pn, stream, g, c, j);
        if (e != hipSuccess) break;
    }
    return e;
}

}  // namespace cclqr
