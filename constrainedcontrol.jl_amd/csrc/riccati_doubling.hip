// riccati_doubling.hip -- the stationary LQR gain by doubling the Riccati map.  LQR{T,Inf} steps dlqr Ntemp times and keeps Ku[1] (src/control/lqr.jl:25-27, 39-43);
// in projected form ([A' | D]: ric_project_kernel, the one projection of the library) a backward step of lqr.jl:151-170 is
//   Ku = (R + D' P D)^-1 D' P A',   Pkp1 = Q + A'' P (I + G0 P)^-1 A'   with G0 = D R^-1 D'   (Woodbury: exact for any P, for symmetric Q and R)
// and n such steps are the triple (A_n, G_n, H_n) of the map X -> H_n + A_n' X (I + G_n X)^-1 A_n, with H_n = the recursion's Pk after n - 1 steps from Pk = Q.  One
// step is (A', G0, Q); triple 1 applied after triple 2 is
//   W = (I + G1 H2)^-1,   A = A2 W A1,   G = G2 + A2 W G1 A2',   H = H1 + A1' H2 W A1
// one mx-square pivoted solve with 2 mx right-hand sides and five mx^3 products.  The pair of triples (d = the doubling one, 2^level steps; a = the accumulated one)
// is driven as policy_doubling.hip drives its pairs; an accumulation is 1 = a, 2 = d.  Two modes:
//   fixed horizon N >= 2   n = N - 1 single-step triples (rdb_fixed_schedule); then the final step in the recursion's own form gives Ku[1] and the last Pkp1 of
//                          dlqr(.., N) with tol = 0: what cclqr_riccati_value(N, tol = 0, keep_last) returns, to rounding.  No stop test
//   to convergence N == 0  level j = 1, 2, .. doubles to 2^j triples; its increment H(2^j) - H(2^(j-1)) = A1' H2 W A1 comes out of the composition.  Stop after level
//                          j, in this order: reason 0 its Frobenius norm < tol; reason 2 norm(A(2^j)) > 1e50 or a norm that is not finite; reason 3 a zero or
//                          non-finite pivot of I + G1 H2 (found before the level changes anything: the triple of level j - 1 stays); reason 1 j == max_levels
// One launch shape for every mx >= 1: each product a device-wide launch of one masked-edge tile kernel on v_mfma_f64_16x16x4_f64 (the tiles of cclqr_riccati_dev.h),
// the LU of M one workgroup per problem, the substitutions one workgroup per panel of right-hand sides; M lives in LDS up to RDB_LDS_MX states and in global memory
// beyond.  A problem that has stopped is skipped through its flag on the device; every second level the host reads the flags and stops launching once all are raised.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>
#include <utility>
#include <vector>

namespace cclqr {

#define RDB_THREADS 512
#define RDB_LDS_MX 96      // M = I + G1 H2 is factored and read from LDS up to this many states: 73 728 B, beside a 32-column panel of 24 576 B
#define RDB_PANEL 32       // right-hand-side columns per workgroup of the substitution
#define RDB_GROWTH 1e50    // norm(A) beyond which the next level could overflow

struct RdbGrid {
    double *Ad, *Gd, *Hd;      // [nprob][mx][mx] each: the doubling triple
    int N, max_levels;
    double tol;
    int *levels, *reason;      // [nprob]
    double *dnorm, *anorm;     // [nprob][2] (preset to NaN by the launch)
};

// S \ B in LDS by Gaussian elimination with partial pivoting (first row of largest magnitude): S [n][n], B [n][nc], both overwritten, B with the solution.  Called by
// every thread of the workgroup; ends synchronised.  A zero pivot is divided by: the result is not finite and says so
__device__ inline void rdb_small_solve(double* S, double* B, int n, int nc, int* ip) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = 0; k < n; k++) {
        if (tid == 0) {
            int p = k;
            double best = fabs(S[k * n + k]);
            for (int i = k + 1; i < n; i++) { const double v = fabs(S[i * n + k]); if (v > best) { best = v; p = i; } }
            *ip = p;
        }
        __syncthreads();
        const int p = *ip;
        if (p != k)
            for (int j = tid; j < n + nc; j += nt) {
                double* x = j < n ? S + j : B + (j - n);
                const int ld = j < n ? n : nc;
                const double t = x[k * ld]; x[k * ld] = x[p * ld]; x[p * ld] = t;
            }
        __syncthreads();
        const double piv = S[k * n + k];
        const int rows = n - 1 - k, cols = n - 1 - k + nc;      // columns k + 1 .. n - 1 of S, then all of B
        for (int e = tid; e < rows * cols; e += nt) {
            const int i = k + 1 + e / cols, j = e % cols;
            const double l = S[i * n + k] / piv;
            if (j < n - 1 - k) S[i * n + k + 1 + j] -= l * S[k * n + k + 1 + j];
            else B[i * nc + (j - (n - 1 - k))] -= l * B[k * nc + (j - (n - 1 - k))];
        }
        __syncthreads();
    }
    for (int j = tid; j < nc; j += nt)      // back substitution: a column is one thread's
        for (int k = n - 1; k >= 0; k--) {
            double s = B[k * nc + j];
            for (int c = k + 1; c < n; c++) s -= S[k * n + c] * B[c * nc + j];
            B[k * nc + j] = s / S[k * n + k];
        }
    __syncthreads();
}

// =====================================================================================================================
// SETUP: the single-step triple Ad = A', Hd = Q, Gd = G0 = D (R \ D').  One workgroup per problem; it reads the singular flag of its G Bλ (lqr.jl:151).
// LDS: R [mu][mu] | Y [mu][mx] | one int
__global__ __launch_bounds__(TILE_THREADS) void rdb_setup_kernel(RicGrid a, RdbGrid d) {
    extern __shared__ double sl[];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    if (tid == 0 && ric_knot_singular(a, prob, 1)) { a.status[prob] = CCLQR_ESINGULAR_; a.stop[prob] = 1; }
    const double* AD = a.AD + (size_t)prob * mx * na;
    const double* Qp = ric_Q_of(a, prob);
    double* Ad = d.Ad + (size_t)prob * mx * mx;
    double* Gd = d.Gd + (size_t)prob * mx * mx;
    double* Hd = d.Hd + (size_t)prob * mx * mx;
    for (int e = tid; e < mx * mx; e += TILE_THREADS) {
        const int i = e / mx, j = e - i * mx;
        Ad[e] = AD[(size_t)i * na + j];
        Hd[e] = Qp[e];
    }
    double* Rl = sl;
    double* Y = Rl + mu * mu;
    int* ip = (int*)(Y + (size_t)mu * mx);
    if (mu > 0) {
        const double* Rp = ric_R_of(a, prob);
        for (int e = tid; e < mu * mu; e += TILE_THREADS) Rl[e] = Rp[e];
        for (int e = tid; e < mu * mx; e += TILE_THREADS) { const int c = e / mx, j = e - c * mx; Y[e] = AD[(size_t)j * na + mx + c]; }
        __syncthreads();
        rdb_small_solve(Rl, Y, mu, mx, ip);
    }
    for (int e = tid; e < mx * mx; e += TILE_THREADS) {
        const int i = e / mx, j = e - i * mx;
        double s = 0.0;
        for (int c = 0; c < mu; c++) s += AD[(size_t)i * na + mx + c] * Y[c * mx + j];
        Gd[e] = s;
    }
}

// =====================================================================================================================
// One generic product, launched per product over the problems (tile32_product_store of cclqr_riccati_dev.h, which dbl_product_kernel of policy_doubling.hip calls too):
//   C = op(A) op(B) [+ E] [+ I],  32x32 tiles with masked edges, and per tile the sum of squares of op(A) op(B) (the increment of H, or A itself)
// E may be C (the lane that owns an element reads and writes it); A and B may not.  Sums are taken per tile here and over the tiles in index order by the kernel
// that reads them, so nothing depends on scheduling or on the batch.
struct RdbOp {
    const double *A, *B, *E;       // E null: no addend
    double *C, *part;              // part [nprob][tm * tm][2] (SqSum), or null
    long long sb, se;              // doubles between the B / E of consecutive problems (0: one shared by all); A and C lie mx * mx apart
    int ta, tb;                    // 1: the operand is read transposed
    int eye;                       // 1: + I
};

__global__ __launch_bounds__(TILE_THREADS) void rdb_product_kernel(int mx, int tm, const int* stop, RdbOp o) {
    __shared__ double red[4][1024];
    __shared__ double wsum[2][4];
    const int prob = blockIdx.y;
    if (stop && stop[prob]) return;
    tile32_product_store(mx, tm, prob, o.A + (size_t)prob * mx * mx, o.ta, o.B + (long long)prob * o.sb, o.tb, o.E ? o.E + (long long)prob * o.se : nullptr, o.eye,
                         o.C + (size_t)prob * mx * mx, o.part, red, wsum);
}

// =====================================================================================================================
// The solve W [A1 | G1] = M \ [A1 | G1], M = I + G1 H2: a partially pivoted LU of M (rdb_lu_kernel, one workgroup per problem, the unit-lower factor's multipliers
// left below the diagonal with every later row exchange applied to them, as LAPACK's getrf leaves them) and the substitutions (rdb_solve_kernel, one workgroup per
// panel of RDB_PANEL right-hand sides, the panel in LDS).  M is held in LDS (LM = true, mx <= RDB_LDS_MX) or worked on where it lies (LM = false).
struct RdbLu {
    double* M;                 // [nprob][mx][mx]: I + G1 H2 in, its LU out
    int* piv;                  // [nprob][mx]: row k was exchanged with row piv[k] >= k
    const double *B1, *B2;     // [nprob][mx][mx]: the right-hand sides A1, G1
    double *X1, *X2;           // [nprob][mx][mx]: W A1, W G1
    int *stop, *reason;
};

template <bool LM>
__global__ __launch_bounds__(RDB_THREADS) void rdb_lu_kernel(int mx, RdbLu u) {
    extern __shared__ double ml[];
    __shared__ double s_pv, s_kk;
    __shared__ int s_p;
    typedef typename std::conditional<LM, lds_double*, double*>::type PM;
    const int prob = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (u.stop[prob]) return;
    double* Mg = u.M + (size_t)prob * mx * mx;
    int* piv = u.piv + (size_t)prob * mx;
    PM M;
    if constexpr (LM) {
        M = (lds_double*)ml;
        for (int e = tid; e < mx * mx; e += RDB_THREADS) M[e] = Mg[e];
        __syncthreads();
    } else M = Mg;
    const int tx = tid & 31, ty = tid >> 5;      // the update: 16 rows of 32 columns per pass
    for (int k = 0; k < mx; k++) {
        if (tid < 64) {      // the first row of largest magnitude in column k, from the diagonal down
            double best = -1.0;
            int bi = k;
            for (int i = k + lane; i < mx; i += 64) { const double v = fabs(M[i * mx + k]); if (v > best) { best = v; bi = i; } }
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (lane == 0) { s_p = bi; s_pv = M[bi * mx + k]; s_kk = M[k * mx + k]; piv[k] = bi; }
        }
        __syncthreads();
        const int p = s_p;
        const double pv = s_pv, kk = s_kk;
        if (!(fabs(pv) > 0.0) || !(fabs(pv) <= 0x1.fffffffffffffp1023)) {      // zero, Inf or NaN (a column of NaNs leaves best at -1 and the diagonal as the pivot)
            if (tid == 0) { u.reason[prob] = 3; u.stop[prob] = 1; }
            return;
        }
        if (p != k)
            for (int j = tid; j < mx; j += RDB_THREADS)
                if (j != k) { const double t = M[k * mx + j]; M[k * mx + j] = M[p * mx + j]; M[p * mx + j] = t; }
        for (int i = k + 1 + tid; i < mx; i += RDB_THREADS) M[i * mx + k] = (i == p ? kk : M[i * mx + k]) / pv;      // column k: exchanged and scaled by its one owner
        if (tid == 0) M[k * mx + k] = pv;
        __syncthreads();
        for (int i = k + 1 + ty; i < mx; i += RDB_THREADS / 32) {
            const double l = M[i * mx + k];
            for (int j = k + 1 + tx; j < mx; j += 32) M[i * mx + j] -= l * M[k * mx + j];
        }
        __syncthreads();
    }
    if constexpr (LM)
        for (int e = tid; e < mx * mx; e += RDB_THREADS) Mg[e] = M[e];
}

// LDS: [LM: the LU, mx * mx] | the panel [mx][pw] | the pivots [mx] ints.  pw (a power of two <= RDB_PANEL) columns, RDB_THREADS / pw threads to a column
template <bool LM>
__global__ __launch_bounds__(RDB_THREADS) void rdb_solve_kernel(int mx, int pw, RdbLu u) {
    extern __shared__ double sv[];
    typedef typename std::conditional<LM, lds_double*, const double*>::type PM;
    const int prob = blockIdx.y, tid = threadIdx.x;
    if (u.stop[prob]) return;
    const double* Mg = u.M + (size_t)prob * mx * mx;
    const int c = tid & (pw - 1), r = tid / pw, nr = RDB_THREADS / pw;
    const int col = blockIdx.x * pw + c;
    const bool valid = col < 2 * mx;
    const double* src = (col < mx ? u.B1 + col : u.B2 + (col - mx)) + (size_t)prob * mx * mx;
    double* dst = (col < mx ? u.X1 + col : u.X2 + (col - mx)) + (size_t)prob * mx * mx;
    PM M;
    lds_double* Xp;
    if constexpr (LM) {
        M = (lds_double*)sv;
        Xp = (lds_double*)sv + mx * mx;
        for (int e = tid; e < mx * mx; e += RDB_THREADS) M[e] = Mg[e];
    } else { M = Mg; Xp = (lds_double*)sv; }
    __attribute__((address_space(3))) int* pl = (__attribute__((address_space(3))) int*)(Xp + mx * pw);
    for (int i = r; i < mx; i += nr) Xp[i * pw + c] = valid ? src[(size_t)i * mx] : 0.0;
    for (int i = tid; i < mx; i += RDB_THREADS) pl[i] = u.piv[(size_t)prob * mx + i];
    __syncthreads();
    if (r == 0)      // the row exchanges, in the order they were made: a column is one thread's
        for (int k = 0; k < mx; k++) {
            const int p = pl[k];
            if (p != k) { const double t = Xp[k * pw + c]; Xp[k * pw + c] = Xp[p * pw + c]; Xp[p * pw + c] = t; }
        }
    __syncthreads();
    for (int k = 0; k + 1 < mx; k++) {      // L y = P b
        const double xk = Xp[k * pw + c];
        for (int i = k + 1 + r; i < mx; i += nr) Xp[i * pw + c] -= M[i * mx + k] * xk;
        __syncthreads();
    }
    for (int k = mx - 1; k >= 0; k--) {     // U x = y: row k is final when step k reads it, and the steps write rows above it only
        const double xk = Xp[k * pw + c] / M[k * mx + k];
        if (r == 0 && valid) dst[(size_t)k * mx] = xk;
        for (int i = r; i < k; i += nr) Xp[i * pw + c] -= M[i * mx + k] * xk;
        __syncthreads();
    }
}

// after level `level` of the run to convergence: the level's two norms, Ad = the level's A product (T), and the stop tests, per problem on the device.  A problem
// whose pivot failed in this level has been stopped by rdb_lu_kernel (reason 3) and keeps the level before
__global__ __launch_bounds__(TILE_THREADS) void rdb_level_kernel(int mx, int tm, int level, RdbGrid d, int* stop, const double* partH, const double* partA, const double* T) {
    const int prob = blockIdx.x, tid = threadIdx.x, ntile = tm * tm;
    const int stopped = stop[prob];
    __syncthreads();      // every wavefront has read the flag before thread 0 may raise it: the workgroup leaves or stays as one
    if (stopped) return;
    const double* src = T + (size_t)prob * mx * mx;
    double* Ad = d.Ad + (size_t)prob * mx * mx;
    for (int e = tid; e < mx * mx; e += TILE_THREADS) Ad[e] = src[e];
    if (tid < 64) {
        const double inc = sq_tile_total(partH + 2 * (size_t)prob * ntile, ntile), an = sq_tile_total(partA + 2 * (size_t)prob * ntile, ntile);
        if (tid == 0) {
            d.levels[prob] = level;
            d.dnorm[2 * prob + 1] = d.dnorm[2 * prob]; d.dnorm[2 * prob] = inc;
            d.anorm[2 * prob + 1] = d.anorm[2 * prob]; d.anorm[2 * prob] = an;
            const bool finite = fabs(inc) <= 0x1.fffffffffffffp1023 && fabs(an) <= 0x1.fffffffffffffp1023;
            if (inc < d.tol) { d.reason[prob] = 0; stop[prob] = 1; }
            else if (an > RDB_GROWTH || !finite) { d.reason[prob] = 2; stop[prob] = 1; }
            else if (level == d.max_levels) { d.reason[prob] = 1; stop[prob] = 1; }
        }
    }
}

// fixed horizon: the number of doublings and norm(A_n)
__global__ __launch_bounds__(TILE_THREADS) void rdb_fixed_out_kernel(int mx, int top, RdbGrid d, const double* Aa) {
    __shared__ double wsum[2][4];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const double* M = Aa + (size_t)prob * mx * mx;
    SqSum g = {0.0, 0.0};
    for (int e = tid; e < mx * mx; e += TILE_THREADS) g.add(M[e]);
    sq_reduce(g, wsum);
    if (tid == 0) {
        g.mid = sq_wave_sum(wsum, 0); g.big = sq_wave_sum(wsum, 1);
        d.levels[prob] = top;
        if (d.reason[prob] == 0) d.anorm[2 * prob] = g.norm();
    }
}

// =====================================================================================================================
// The final step, in the recursion's own form (lqr.jl:151-170 projected), with X = H_n [nprob][mx][mx]:
//   Ku = (R + D' X D) \ D' X A' -> the caller's table;   Abar = A' - D Ku;   E = Q + Ku' R Ku      (P = E + Abar' X Abar follows as two products)
// One workgroup per problem.  A fixed horizon whose pivot failed has no H_n: its gain and P are NaN.  LDS: W1 [mu][mx] | B [mu][mx] | S [mu][mu] | one int
__global__ __launch_bounds__(TILE_THREADS) void rdb_gain_kernel(RicGrid a, const double* X, double* Abar, double* E, const int* reason, int want_p) {
    extern __shared__ double gl[];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    if (a.status[prob] != 0) return;      // G Bλ singular: the call is refused for this problem
    const double* AD = a.AD + (size_t)prob * mx * na;
    const double* Xp = X + (size_t)prob * mx * mx;
    double* Kout = a.K + (size_t)prob * ((size_t)mu * mx + a.kpad);
    double* Ab = Abar + (size_t)prob * mx * mx;
    double* Ep = E + (size_t)prob * mx * mx;
    if (a.N != 0 && reason[prob] == 3) {
        const double nan = __builtin_nan("");
        for (int e = tid; e < mu * mx; e += TILE_THREADS) Kout[e] = nan;
        if (want_p) for (int e = tid; e < mx * mx; e += TILE_THREADS) { Ab[e] = nan; Ep[e] = nan; }
        return;
    }
    double* W1 = gl;
    double* B = W1 + (size_t)mu * mx;
    double* S = B + (size_t)mu * mx;
    int* ip = (int*)(S + mu * mu);
    const double* Rp = ric_R_of(a, prob);
    if (mu > 0) {
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {      // W1 = D' X
            const int c = e / mx, j = e - c * mx;
            double s = 0.0;
            for (int i = 0; i < mx; i++) s += AD[(size_t)i * na + mx + c] * Xp[(size_t)i * mx + j];
            W1[e] = s;
        }
        __syncthreads();
        for (int e = tid; e < mu * mu; e += TILE_THREADS) {      // S = R + W1 D
            const int c = e / mu, f = e - c * mu;
            double s = 0.0;
            for (int i = 0; i < mx; i++) s += W1[c * mx + i] * AD[(size_t)i * na + mx + f];
            S[e] = Rp[e] + s;
        }
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {      // B = W1 A'
            const int c = e / mx, j = e - c * mx;
            double s = 0.0;
            for (int i = 0; i < mx; i++) s += W1[c * mx + i] * AD[(size_t)i * na + j];
            B[e] = s;
        }
        __syncthreads();
        rdb_small_solve(S, B, mu, mx, ip);                       // B = Ku
        for (int e = tid; e < mu * mx; e += TILE_THREADS) Kout[e] = B[e];
        if (!want_p) return;
        for (int e = tid; e < mu * mx; e += TILE_THREADS) {      // W1 = R Ku
            const int c = e / mx, j = e - c * mx;
            W1[e] = ric_rk_entry(Rp, mx, mu, c, j, B);
        }
        __syncthreads();
    }
    if (!want_p) return;
    const double* Qp = ric_Q_of(a, prob);
    for (int e = tid; e < mx * mx; e += TILE_THREADS) {
        const int i = e / mx, j = e - i * mx;
        Ab[e] = ric_abar_entry(AD, na, mx, mu, i, j, B);
        double q = Qp[e];
        for (int c = 0; c < mu; c++) q += B[c * mx + i] * W1[c * mx + j];
        Ep[e] = q;
    }
}

#define RDB_LDS_BUDGET (150 * 1024)      // dynamic LDS a kernel of this file may ask for, of the 160 KB per CU (the rest is static)
static size_t rdb_solve_lds_bytes(int mx, int pw);
static size_t rdb_gain_lds_bytes(int mx, int mu) { return (2 * (size_t)mu * mx + (size_t)mu * mu + 1) * sizeof(double); }
// can the kernels hold these sizes?  The narrowest substitution panel (one column) and the mu x mx panels of the setup and final-step kernels within the LDS budget
bool riccati_doubling_fits(int mx, int mu) { return rdb_solve_lds_bytes(mx, 1) <= RDB_LDS_BUDGET && rdb_gain_lds_bytes(mx, mu) <= RDB_LDS_BUDGET; }
static size_t rdb_solve_lds_bytes(int mx, int pw) { return ((mx <= RDB_LDS_MX ? (size_t)mx * mx : 0) + (size_t)mx * pw) * sizeof(double) + (size_t)mx * sizeof(int); }

hipError_t launch_riccati_doubling(const RdbArgs& p, hipStream_t stream) {
    const RicArgs& a = p.r;
    if (a.nprob <= 0) return hipSuccess;
    if (a.N == 1 || a.N < 0) return hipErrorInvalidValue;
    RicGrid g = ric_grid_of(a);
    g.K = a.K; g.kpad = a.kpad; g.keep_last = 1;
    const size_t np = a.nprob, mx = a.mx, mm = mx * mx, mu = a.mu;
    const int tm = g.tm;
    const bool lm = a.mx <= RDB_LDS_MX;
    int pw = RDB_PANEL;
    if (!riccati_doubling_fits(a.mx, a.mu)) return hipErrorInvalidValue;      // (the entry points have refused such sizes)
    while (pw > 1 && rdb_solve_lds_bytes(a.mx, pw) > RDB_LDS_BUDGET) pw >>= 1;
    double* w = p.work2;
    double *Ad = w, *Gd = w + np * mm, *Hd = w + 2 * np * mm, *Aa = w + 3 * np * mm, *Ga = w + 4 * np * mm, *Ha = w + 5 * np * mm;
    double *Mb = w + 6 * np * mm, *XA = w + 7 * np * mm, *XG = w + 8 * np * mm, *T1 = w + 9 * np * mm, *T2 = w + 10 * np * mm;
    double *partH = w + 11 * np * mm, *partA = partH + 2 * np * tm * tm;
    int* piv = (int*)(partA + 2 * np * tm * tm);
    RdbGrid d;
    d.Ad = Ad; d.Gd = Gd; d.Hd = Hd; d.N = a.N; d.max_levels = p.max_levels; d.tol = a.tol;
    d.levels = p.levels; d.reason = p.reason; d.dnorm = p.dnorm; d.anorm = p.anorm;
    hipError_t e = hipMemsetAsync(a.stop, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.status, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.levels, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.reason, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.dnorm, 0xff, 2 * np * sizeof(double), stream);      // all bits set: a NaN, "no such level ran"
    if (e == hipSuccess) e = hipMemsetAsync(p.anorm, 0xff, 2 * np * sizeof(double), stream);
    if (e != hipSuccess) return e;
    e = launch_ric_project(g, a, stream);
    if (e == hipSuccess) e = launch_lds(rdb_setup_kernel, dim3(a.nprob), dim3(TILE_THREADS), (mu * mu + mu * mx + 1) * sizeof(double), stream, g, d);
    if (e != hipSuccess) return e;

    const long long sm = (long long)mm;
    auto prod = [&](const double* A, int ta, const double* B, int tb, const double* E, long long se, int eye, double* Cm, double* part, const int* stop) {
        RdbOp o;
        o.A = A; o.B = B; o.E = E; o.C = Cm; o.part = part; o.sb = sm; o.se = se; o.ta = ta; o.tb = tb; o.eye = eye;
        return launch_lds<false>(rdb_product_kernel, dim3(tm * tm, a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, tm, stop, o);
    };
    // triple 1 applied after triple 2; G into Go (G2 itself, or a G1 the solve has consumed), H into H1, the new A into T1
    auto compose = [&](const double* A1, const double* G1, double* H1, const double* A2, const double* G2, const double* H2, double* Go, bool norms) {
        hipError_t r = prod(G1, 0, H2, 0, nullptr, 0, 1, Mb, nullptr, a.stop);                                            // M = I + G1 H2
        RdbLu u;
        u.M = Mb; u.piv = piv; u.B1 = A1; u.B2 = G1; u.X1 = XA; u.X2 = XG; u.stop = a.stop; u.reason = p.reason;
        if (r == hipSuccess) r = lm ? launch_lds(rdb_lu_kernel<true>, dim3(a.nprob), dim3(RDB_THREADS), mm * sizeof(double), stream, (int)mx, u)
                                    : launch_lds<false>(rdb_lu_kernel<false>, dim3(a.nprob), dim3(RDB_THREADS), 0, stream, (int)mx, u);
        const dim3 sgrid((unsigned)((2 * mx + pw - 1) / pw), a.nprob);
        if (r == hipSuccess) r = lm ? launch_lds(rdb_solve_kernel<true>, sgrid, dim3(RDB_THREADS), rdb_solve_lds_bytes(a.mx, pw), stream, (int)mx, pw, u)
                                    : launch_lds(rdb_solve_kernel<false>, sgrid, dim3(RDB_THREADS), rdb_solve_lds_bytes(a.mx, pw), stream, (int)mx, pw, u);
        if (r == hipSuccess) r = prod(A2, 0, XG, 0, nullptr, 0, 0, T1, nullptr, a.stop);                                  // A2 W G1
        if (r == hipSuccess) r = prod(A1, 1, H2, 0, nullptr, 0, 0, T2, nullptr, a.stop);                                  // A1' H2
        if (r == hipSuccess) r = prod(T1, 0, A2, 1, G2, sm, 0, Go, nullptr, a.stop);                                      // G = G2 + (A2 W G1) A2'
        if (r == hipSuccess) r = prod(T2, 0, XA, 0, H1, sm, 0, H1, norms ? partH : nullptr, a.stop);                      // H = H1 + (A1' H2) W A1
        if (r == hipSuccess) r = prod(A2, 0, XA, 0, nullptr, 0, 0, T1, norms ? partA : nullptr, a.stop);                  // A = A2 W A1
        return r;
    };
    const bool conv = a.N == 0;
    int top = 0;
    std::vector<int> stopped;
    if (conv) {
        for (int lvl = 1; lvl <= p.max_levels; lvl++) {      // a stopped problem keeps its triple: the level's A is copied in by the kernel that makes the stop tests
            e = compose(Ad, Gd, Hd, Ad, Gd, Hd, Gd, true);
            if (e == hipSuccess) e = launch_lds<false>(rdb_level_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, tm, lvl, d, a.stop, (const double*)partH, (const double*)partA, (const double*)T1);
            if (e != hipSuccess) return e;
            if ((lvl & 1) == 0 && lvl < p.max_levels) {      // every second level: have all problems stopped?  The levels left would be launches that return at the flags
                stopped.resize(np);
                e = hipMemcpyAsync(stopped.data(), a.stop, np * sizeof(int), hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipStreamSynchronize(stream);
                if (e != hipSuccess) return e;
                bool all = true;
                for (size_t q = 0; q < np && all; q++) all = stopped[q] != 0;
                if (all) break;
            }
        }
    } else {
        unsigned char ops[RDB_MAX_OPS];
        const int nops = rdb_fixed_schedule((unsigned)(a.N - 1), ops);
        for (int i = 0; i < nops; i++) {
            if (ops[i] == RDB_COPY) {
                e = hipMemcpyAsync(Aa, Ad, np * mm * sizeof(double), hipMemcpyDeviceToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(Ga, Gd, np * mm * sizeof(double), hipMemcpyDeviceToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(Ha, Hd, np * mm * sizeof(double), hipMemcpyDeviceToDevice, stream);
            } else if (ops[i] == RDB_ACCUMULATE) {
                e = compose(Aa, Ga, Ha, Ad, Gd, Hd, Ga, false);
                std::swap(Aa, T1);
            } else {
                e = compose(Ad, Gd, Hd, Ad, Gd, Hd, Gd, false);
                std::swap(Ad, T1);
                top++;
            }
            if (e != hipSuccess) return e;
        }
    }
    // the final step on X = H_n
    const double* Xn = conv ? Hd : Ha;
    const int want_p = a.P_out ? 1 : 0;
    e = launch_lds(rdb_gain_kernel, dim3(a.nprob), dim3(TILE_THREADS), rdb_gain_lds_bytes(a.mx, a.mu), stream, g, Xn, Mb, T2, (const int*)p.reason, want_p);
    if (e == hipSuccess && want_p) e = prod(Mb, 1, Xn, 0, nullptr, 0, 0, XA, nullptr, nullptr);          // Abar' X
    if (e == hipSuccess && want_p) e = prod(XA, 0, Mb, 0, T2, sm, 0, a.P_out, nullptr, nullptr);          // P = E + (Abar' X) Abar
    if (e == hipSuccess && !conv) e = launch_lds<false>(rdb_fixed_out_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, top, d, (const double*)Aa);
    return e;
}

}  // namespace cclqr
