// policy_doubling.hip -- the cost-to-go of a STATIONARY gain by doubling.  The reference's default controller LQR{T,Inf} keeps one gain (src/control/lqr.jl:40-43); the
// cost recursion of dlqr with that gain given (lqr.jl:147-177, policy.hip) is then Pkp1 = Qbar + Abar' Pk Abar with constant
//   Abar = A - Bu K - Bλ Kλ = A' - D K   (lqr.jl:169; [A' | D]: ric_project_kernel, the one projection of the library)        Qbar = Q + K' R K   (lqr.jl:170)
// so with S(n) = sum_{i<n} (Abar^i)' Qbar Abar^i and M(n) = Abar^n the cost-to-go after n backward steps is P = S(n) + M(n)' Q M(n), and
//   S(a + b) = S(a) + M(a)' S(b) M(a),   M(a + b) = M(a) M(b)
// gives it for any n by square-and-multiply over the bits of n, least significant first: the pair (Sd, Md) = (S, M)(2^level) is doubled between bits, the pair (Sa, Ma)
// accumulates the set bits (the first set bit is a copy: S(0) = 0, M(0) = I).  Two modes:
//   fixed horizon N >= 1   n = N - 1 steps exactly: what cclqr_policy_value returns for nK = 1, tol = 0 and the same N, to rounding.  No break test, no growth stop
//   to convergence N == 0  level j = 1, 2, .. doubles to 2^j steps; its increment S(2^j) - S(2^(j-1)) = M' S M comes out of the doubling itself.  Stop after level j,
//                          in this order: reason 0 its Frobenius norm < tol; reason 2 norm(M(2^j)) > 1e50 (one more level could overflow); reason 1 j == max_levels
// Two launch shapes, chosen as policy.hip chooses them: RESIDENT, one workgroup per problem over all levels; TILED, every product a device-wide launch.  Every mx^3
// product runs on v_mfma_f64_16x16x4_f64 through the tiles of cclqr_riccati_dev.h.  Nothing assumes a symmetric matrix.
#include "cclqr_internal.h"
#include "cclqr_riccati_dev.h"
#include <math.h>
#include <string.h>
#include <utility>

namespace cclqr {

#define DBL_THREADS 512
#define DBL_WAVES (DBL_THREADS / 64)
#define DBL_TILES 5      // 16x16 tiles of an mx x mx matrix one wavefront holds in registers across a barrier (ResTiles of cclqr_riccati_dev.h)
static_assert(DBL_TILES == RES_TILES, "the resident kernel holds its tiles in ResTiles");
#define DBL_RU 16        // rows of Abar / Qbar per workgroup of the setup kernel
#define DBL_GROWTH 1e50  // norm(M) beyond which the next level could overflow: with norm(M) <= 1e50, S(2n) is about 1e200 |Q| and the final M' Q M stays finite

// what the kernels take besides the Riccati launch record (of which they read the sizes, [A' | D], the singular flags, Q, R and status / stop)
struct DblGrid {
    const double* Kin;         // the stationary gains [n_gains][mu][mx]
    long long k_stride;        // doubles between the gains of consecutive problems: 0 = one gain shared by all
    double *Md, *Sd, *Ma, *Sa; // [nprob][mx][mx] each: the doubling pair and the accumulated pair
    int N;                     // knots: N - 1 steps exactly, or 0 = to convergence
    int max_levels;
    double tol;
    int *levels, *reason;      // [nprob]
    double *dnorm, *gnorm;     // [nprob][2] (preset to NaN by the launch)
    double* P_out;             // [nprob][mx][mx]
};

size_t dbl_resident_lds_bytes(int mx) { return (2 * (size_t)mx * mx + 4 * DBL_WAVES) * sizeof(double); }

// =====================================================================================================================
// SETUP, both shapes: Md = Abar = A' - D K and Sd = Qbar = Q + K' (R K), once.  Abar is formed by the function policy.hip forms it by (ric_abar_entry): the two
// evaluations start from the same matrix.  The lead workgroup of a problem reads the singular flag of its G Bλ (lqr.jl:151)
__global__ __launch_bounds__(TILE_THREADS) void dbl_setup_kernel(RicGrid a, DblGrid d) {
    extern __shared__ double kl[];      // K [mu][mx] | R K [mu][mx]
    const int prob = blockIdx.y, tid = threadIdx.x;
    const int mx = a.mx, mu = a.mu, na = a.na;
    double* KR = kl + (size_t)mu * mx;
    if (blockIdx.x == 0 && tid == 0 && ric_knot_singular(a, prob, 1)) { a.status[prob] = CCLQR_ESINGULAR_; a.stop[prob] = 1; }
    const double* Kp = d.Kin + (long long)prob * d.k_stride;
    for (int e = tid; e < mu * mx; e += TILE_THREADS) kl[e] = Kp[e];
    __syncthreads();
    const double* Rp = ric_R_of(a, prob);
    for (int e = tid; e < mu * mx; e += TILE_THREADS) {
        const int r = e / mx, j = e - r * mx;
        KR[e] = ric_rk_entry(Rp, mx, mu, r, j, kl);
    }
    __syncthreads();
    const double* AD = a.AD + (size_t)prob * mx * na;
    const double* Qp = ric_Q_of(a, prob);
    double* Md = d.Md + (size_t)prob * mx * mx;
    double* Sd = d.Sd + (size_t)prob * mx * mx;
    for (int r = 0; r < DBL_RU; r++) {
        const int i = blockIdx.x * DBL_RU + r;
        if (i >= mx) break;
        for (int j = tid; j < mx; j += TILE_THREADS) {
            Md[(size_t)i * mx + j] = ric_abar_entry(AD, na, mx, mu, i, j, kl);        // Abar = A' - D K (= A-Bu*Kuk-Bλ*Kλk)     lqr.jl:169
            double q = Qp[(size_t)i * mx + j];                                        // Qbar = Q + Kuk'*R*Kuk                    lqr.jl:170
            for (int c = 0; c < mu; c++) q += kl[c * mx + i] * KR[c * mx + j];
            Sd[(size_t)i * mx + j] = q;
        }
    }
}

// N = 1: no backward step -- P = Q (lqr.jl:147), M(0) = I
__global__ void dbl_no_step_kernel(RicGrid a, DblGrid d) {
    const int prob = blockIdx.x, mx = a.mx;
    const double* Qp = ric_Q_of(a, prob);
    double* Po = d.P_out + (size_t)prob * mx * mx;
    for (int e = threadIdx.x; e < mx * mx; e += blockDim.x) Po[e] = Qp[e];
    if (threadIdx.x == 0) { d.levels[prob] = 0; d.reason[prob] = 0; d.gnorm[2 * prob] = sqrt((double)mx); }
}

// =====================================================================================================================
// RESIDENT: one 512-thread workgroup per problem, persistent over all levels, for every shape policy_resident_kernel serves (mx % 4 == 0, up to 96 states).
// The live set is five mx^2 matrices (Md, Sd, Ma, Sa and a product in flight): 282 KB at mx = 84, against 160 KB of LDS.  Placement:
//   U, V  [mx][mx]  LDS     the two MFMA operands of the CURRENT product, both read along rows (C = U' V: A operand U[k][i], B operand V[k][j]).  A wavefront keeps
//                           its <= DBL_TILES result tiles in accumulators until a barrier says every read of the buffer they overwrite is done.
//                           X Y for a product without the transpose is (X')' Y: X' is written by a transposing store (from accumulators) or an LDS-to-LDS transpose
//   Md, Sd, Ma, Sa  global  the problem's workspace, L2-resident: touched elementwise by the lane that owns the element (S += increment, M = product) and streamed
//                           into U / V where a product needs them -- a few mx^2 reads per level against its 3 mx^3
// U holds Md whenever a doubling starts (the doubling leaves the new Md there), so a level stages one matrix (Sd); an accumulation stages three.
// LDS: 2 mx^2 + 32 doubles = 113 152 B at mx = 84, 147 712 B at mx = 96, of 163 840.
__global__ __launch_bounds__(DBL_THREADS) void dbl_resident_kernel(RicGrid a, DblGrid d) {
    extern __shared__ double dl[];
    const int prob = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int mx = a.mx, mm = mx * mx;
    if (a.status[prob] != 0) return;      // G Bλ singular (dbl_setup_kernel)                                        lqr.jl:151
    lds_double* U = (lds_double*)dl;
    lds_double* V = U + mm;
    lds_double* red = V + mm;             // [4][DBL_WAVES]
    double* Md = d.Md + (size_t)prob * mm;
    double* Sd = d.Sd + (size_t)prob * mm;
    double* Ma = d.Ma + (size_t)prob * mm;
    double* Sa = d.Sa + (size_t)prob * mm;
    const int t16 = (mx + 15) >> 4;
    const ResShape rs = {mx, t16, t16 * t16, mx >> 2, wave, li, lk, DBL_WAVES};

    auto stage = [&](lds_double* X, const double* src) { for (int e = tid; e < mm; e += DBL_THREADS) X[e] = src[e]; };
    auto mul = [&](lds_double* A, lds_double* B) { return res_mul(rs, A, B); };                  // C = A' B, this wavefront's tiles
    auto each = [&](const ResTiles& acc, auto f) { res_each(rs, acc, f); };                      // f(i, j, C[i][j]) on every element this lane holds
    // the sandwich A' B A: X = (A' B)' stored over B by the lanes that hold it, then X' A.  B's buffer is overwritten
    auto mul3 = [&](lds_double* A, lds_double* B) {
        ResTiles acc = mul(A, B);
        __syncthreads();      // every wavefront has read B: the buffer may take the transposed product
        each(acc, [&](int i, int j, double v) { B[j * mx + i] = v; });
        __syncthreads();
        return mul(B, A);
    };
    auto transpose_u_to_v = [&]() {
        for (int e = tid; e < mm; e += DBL_THREADS) { const int i = e / mx, k = e - i * mx; V[k * mx + i] = U[e]; }
    };
    // two sums of squares over the workgroup: per lane, per wavefront, then over the wavefronts in index order (the eight-wavefront, two-pair sibling of
    // sq_reduce / sq_wave_sum of cclqr_riccati_dev.h, which serve the 256-thread kernels: a new 256-thread kernel calls those)
    auto total2 = [&](SqSum& x, SqSum& y) {
        for (int o = 32; o > 0; o >>= 1) {
            x.mid += __shfl_xor(x.mid, o, 64); x.big += __shfl_xor(x.big, o, 64);
            y.mid += __shfl_xor(y.mid, o, 64); y.big += __shfl_xor(y.big, o, 64);
        }
        if (lane == 0) { red[wave] = x.mid; red[DBL_WAVES + wave] = x.big; red[2 * DBL_WAVES + wave] = y.mid; red[3 * DBL_WAVES + wave] = y.big; }
        __syncthreads();
        x.mid = 0.0; x.big = 0.0; y.mid = 0.0; y.big = 0.0;
        for (int w = 0; w < DBL_WAVES; w++) { x.mid += red[w]; x.big += red[DBL_WAVES + w]; y.mid += red[2 * DBL_WAVES + w]; y.big += red[3 * DBL_WAVES + w]; }
    };

    const bool conv = d.N == 0;
    const unsigned n = conv ? 0u : (unsigned)(d.N - 1);      // >= 1: N = 1 never comes here (dbl_no_step_kernel)
    const int top = conv ? 0 : 31 - __clz((int)n);
    double dn0 = __builtin_nan(""), dn1 = dn0, gn0 = dn0, gn1 = dn0;
    int lvl = 0, reason = 0;
    bool have_a = false;
    stage(U, Md);
    __syncthreads();
    for (;;) {
        if (!conv) {
            if ((n >> lvl) & 1u) {
                if (!have_a) {      // S(0) + I' Sd I, I Md: a copy
                    for (int e = tid; e < mm; e += DBL_THREADS) { Sa[e] = Sd[e]; Ma[e] = Md[e]; }
                    have_a = true;
                    __syncthreads();
                } else {            // S(a + n) = S(a) + M(a)' S(n) M(a), M(a + n) = M(a) M(n)
                    stage(U, Ma);
                    stage(V, Sd);
                    __syncthreads();
                    ResTiles acc = mul3(U, V);
                    each(acc, [&](int i, int j, double v) { Sa[(size_t)i * mx + j] += v; });
                    __syncthreads();      // every wavefront has read V
                    transpose_u_to_v();
                    __syncthreads();
                    stage(U, Md);
                    __syncthreads();
                    acc = mul(V, U);
                    each(acc, [&](int i, int j, double v) { Ma[(size_t)i * mx + j] = v; });
                    __syncthreads();      // U holds Md again
                }
            }
            if (lvl == top) break;
        }
        // S(2n) = S(n) + M(n)' S(n) M(n), M(2n) = M(n) M(n); U holds Md
        stage(V, Sd);
        __syncthreads();
        ResTiles acc = mul3(U, V);
        SqSum inc = {0.0, 0.0}, g = {0.0, 0.0};
        each(acc, [&](int i, int j, double v) { inc.add(v); Sd[(size_t)i * mx + j] += v; });
        __syncthreads();      // every wavefront has read V
        transpose_u_to_v();
        __syncthreads();
        acc = mul(V, U);
        __syncthreads();      // every wavefront has read U: it may take the new Md
        each(acc, [&](int i, int j, double v) { g.add(v); U[i * mx + j] = v; Md[(size_t)i * mx + j] = v; });
        total2(inc, g);       // (its barrier: the new Md and Sd are complete)
        lvl++;
        if (conv) {
            dn1 = dn0; dn0 = inc.norm(); gn1 = gn0; gn0 = g.norm();
            if (dn0 < d.tol) { reason = 0; break; }
            if (gn0 > DBL_GROWTH) { reason = 2; break; }
            if (lvl == d.max_levels) { reason = 1; break; }
        }
    }
    // P = S(n) + M(n)' Q M(n)
    const double* Sn = conv ? Sd : Sa;
    stage(U, conv ? Md : Ma);
    stage(V, ric_Q_of(a, prob));
    __syncthreads();
    if (!conv) {
        SqSum g = {0.0, 0.0}, none = {0.0, 0.0};
        for (int e = tid; e < mm; e += DBL_THREADS) g.add(U[e]);
        total2(g, none);
        gn0 = g.norm();
    }
    ResTiles acc = mul3(U, V);
    double* Po = d.P_out + (size_t)prob * mm;
    each(acc, [&](int i, int j, double v) { Po[(size_t)i * mx + j] = Sn[(size_t)i * mx + j] + v; });
    if (tid == 0) {
        d.levels[prob] = lvl; d.reason[prob] = reason;
        d.dnorm[2 * prob] = dn0; d.dnorm[2 * prob + 1] = dn1; d.gnorm[2 * prob] = gn0; d.gnorm[2 * prob + 1] = gn1;
    }
}

// =====================================================================================================================
// TILED: every other shape (mx % 4 != 0, mx > 96: the 17-body chain's 204 states) and path = 2.  One generic product, launched per product over the problems:
//   C = op(A) B [+ E],  op(A) = A' or A,  32x32 tiles with masked edges, and per tile the sum of squares of op(A) B (the increment of a doubling, or M itself)
// E may be C (the lane that owns an element reads and writes it); A and B may not.  Sums are taken per tile here and over the tiles in index order by the kernel
// that reads them, so nothing depends on scheduling.  A problem that has stopped (its flag is raised on the device, dbl_level_kernel) is skipped by the gated launches.
struct DblOp {
    const double *A, *B, *E;       // E null: no addend
    double *C, *part;              // part [nprob][tm * tm][2] (SqSum), or null
    long long sa, sb, se, sc;      // doubles between the matrices of consecutive problems (0: one shared by all)
    int ta;                        // 1: C = A' B, 0: C = A B
    int gate;                      // 1: a stopped problem is skipped
};

__global__ __launch_bounds__(TILE_THREADS) void dbl_product_kernel(int mx, int tm, const int* stop, DblOp o) {
    __shared__ double red[4][1024];
    __shared__ double wsum[2][4];
    const int prob = blockIdx.y;
    if (o.gate && stop[prob]) return;
    tile32_product_store(mx, tm, prob, o.A + (long long)prob * o.sa, o.ta, o.B + (long long)prob * o.sb, 0, o.E ? o.E + (long long)prob * o.se : nullptr, 0,
                         o.C + (long long)prob * o.sc, o.part, red, wsum);
}

// after level `level` of the run to convergence: the level's two norms, Md = the level's M product (T2), and the stop tests, per problem on the device
__global__ __launch_bounds__(TILE_THREADS) void dbl_level_kernel(int mx, int tm, int level, DblGrid d, int* stop, const double* partS, const double* partM, const double* T2) {
    const int prob = blockIdx.x, tid = threadIdx.x, ntile = tm * tm;
    if (stop[prob]) return;
    const double* src = T2 + (size_t)prob * mx * mx;
    double* Md = d.Md + (size_t)prob * mx * mx;
    for (int e = tid; e < mx * mx; e += TILE_THREADS) Md[e] = src[e];
    if (tid < 64) {
        const double inc = sq_tile_total(partS + 2 * (size_t)prob * ntile, ntile), g = sq_tile_total(partM + 2 * (size_t)prob * ntile, ntile);
        if (tid == 0) {
            d.levels[prob] = level;
            d.dnorm[2 * prob + 1] = d.dnorm[2 * prob]; d.dnorm[2 * prob] = inc;
            d.gnorm[2 * prob + 1] = d.gnorm[2 * prob]; d.gnorm[2 * prob] = g;
            if (inc < d.tol) { d.reason[prob] = 0; stop[prob] = 1; }
            else if (g > DBL_GROWTH) { d.reason[prob] = 2; stop[prob] = 1; }
            else if (level == d.max_levels) { d.reason[prob] = 1; stop[prob] = 1; }
        }
    }
}

// fixed horizon: the number of doublings and norm(M(n))
__global__ __launch_bounds__(TILE_THREADS) void dbl_fixed_out_kernel(int mx, int top, DblGrid d, const double* Ma) {
    __shared__ double wsum[2][4];
    const int prob = blockIdx.x, tid = threadIdx.x;
    const double* M = Ma + (size_t)prob * mx * mx;
    SqSum g = {0.0, 0.0};
    for (int e = tid; e < mx * mx; e += TILE_THREADS) g.add(M[e]);
    sq_reduce(g, wsum);
    if (tid == 0) {
        g.mid = sq_wave_sum(wsum, 0); g.big = sq_wave_sum(wsum, 1);
        d.levels[prob] = top; d.reason[prob] = 0; d.gnorm[2 * prob] = g.norm();
    }
}

// the doubles of DblArgs.work2: Md, Sd, Ma, Sa and two products in flight, [nprob][mx][mx] each, and the per-tile sums of a level's two norms
size_t dbl_work_doubles(const RicArgs& r) {
    const size_t np = r.nprob, mx = r.mx, tm = (mx + 31) / 32;
    return 6 * np * mx * mx + 4 * np * tm * tm + 8;
}

// the two launch records of a call, from its arguments alone (ric_grid_of: the Riccati record): the pair (Md, Sd) a setup kernel writes lies at dbl_Md / dbl_Sd
// (cclqr_internal.h)
static void dbl_records(const DblArgs& p, RicGrid& g, DblGrid& d) {
    const RicArgs& a = p.r;
    g = ric_grid_of(a);
    const size_t np = a.nprob, mm = (size_t)a.mx * a.mx;
    d.Kin = p.k.Kin; d.k_stride = p.k.k_stride; d.N = a.N; d.max_levels = p.max_levels; d.tol = a.tol;
    d.levels = p.levels; d.reason = p.reason; d.dnorm = p.dnorm; d.gnorm = p.gnorm; d.P_out = a.P_out;
    double* w = p.work2;
    d.Md = dbl_Md(p); d.Sd = dbl_Sd(p); d.Ma = w + 2 * np * mm; d.Sa = w + 3 * np * mm;
}

// before any kernel of a call: flags and diagnostics preset
hipError_t dbl_preset(const DblArgs& p, hipStream_t stream) {
    const RicArgs& a = p.r;
    const size_t np = a.nprob;
    hipError_t e = hipMemsetAsync(a.stop, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.status, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.levels, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.reason, 0, np * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p.dnorm, 0xff, 2 * np * sizeof(double), stream);      // all bits set: a NaN, "no such level ran"
    if (e == hipSuccess) e = hipMemsetAsync(p.gnorm, 0xff, 2 * np * sizeof(double), stream);
    return e;
}

// everything after a setup kernel has written the pair (M, S)(1) of every problem and raised the singular flags (N = 1: no setup is needed, the terminal matrix is
// the answer): the resident-or-tiled choice, the levels, the final sandwich with the terminal matrix a.Q and the fixed horizon's diagnostics
hipError_t launch_doubling_levels(const DblArgs& p, hipStream_t stream) {
    const RicArgs& a = p.r;
    if (a.nprob <= 0) return hipSuccess;
    RicGrid g;
    DblGrid d;
    dbl_records(p, g, d);
    const size_t np = a.nprob, mx = a.mx, mm = mx * mx;
    const int tm = g.tm;
    double* w = p.work2;
    double *T1 = w + 4 * np * mm, *T2 = w + 5 * np * mm, *partS = w + 6 * np * mm, *partM = partS + 2 * np * tm * tm;
    hipError_t e = hipSuccess;
    if (a.N == 1) return launch_lds<false>(dbl_no_step_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, g, d);
    // resident wherever the stepping evaluation is (launch_policy: ric_chosen_path, a wavefront's share of the tiles within its registers, two operands within the LDS)
    if (ric_chosen_path(a) == 1 && res_tiles_serve(a.mx, DBL_WAVES) && dbl_resident_lds_bytes(a.mx) <= 158 * 1024)
        return launch_lds(dbl_resident_kernel, dim3(a.nprob), dim3(DBL_THREADS), dbl_resident_lds_bytes(a.mx), stream, g, d);

    const long long sm = (long long)mm;
    auto prod = [&](const double* A, int ta, const double* B, long long sb, const double* E, double* Cm, double* part, int gate) {
        DblOp o;
        o.A = A; o.B = B; o.E = E; o.C = Cm; o.part = part; o.sa = sm; o.sb = sb; o.se = sm; o.sc = sm; o.ta = ta; o.gate = gate;
        return launch_lds<false>(dbl_product_kernel, dim3(tm * tm, a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, tm, (const int*)a.stop, o);
    };
    // X' S X into Sout (+ E) through T1 = X' S
    auto sandwich = [&](const double* X, const double* S, long long ss, const double* E, double* Sout, double* part, int gate) {
        hipError_t r = prod(X, 1, S, ss, nullptr, T1, nullptr, gate);
        return r == hipSuccess ? prod(T1, 0, X, sm, E, Sout, part, gate) : r;
    };
    const bool conv = a.N == 0;
    const unsigned n = conv ? 0u : (unsigned)(a.N - 1);
    int top = 0;
    while (!conv && (n >> (top + 1)) != 0) top++;
    bool have_a = false;
    for (int lvl = 0;;) {
        if (!conv) {
            if ((n >> lvl) & 1u) {
                if (!have_a) {      // S(0) + I' Sd I, I Md: a copy
                    e = hipMemcpyAsync(d.Sa, d.Sd, np * mm * sizeof(double), hipMemcpyDeviceToDevice, stream);
                    if (e == hipSuccess) e = hipMemcpyAsync(d.Ma, d.Md, np * mm * sizeof(double), hipMemcpyDeviceToDevice, stream);
                    have_a = true;
                } else {            // S(a + n) = S(a) + M(a)' S(n) M(a), M(a + n) = M(a) M(n)
                    e = sandwich(d.Ma, d.Sd, sm, d.Sa, d.Sa, nullptr, 0);
                    if (e == hipSuccess) e = prod(d.Ma, 0, d.Md, sm, nullptr, T2, nullptr, 0);
                    std::swap(d.Ma, T2);
                }
                if (e != hipSuccess) return e;
            }
            if (lvl == top) break;
        }
        // S(2n) = S(n) + M(n)' S(n) M(n), M(2n) = M(n) M(n)
        e = sandwich(d.Md, d.Sd, sm, d.Sd, d.Sd, partS, conv);
        if (e == hipSuccess) e = prod(d.Md, 0, d.Md, sm, nullptr, T2, partM, conv);
        lvl++;
        if (conv) {      // a stopped problem keeps its Md: the level's product is copied in by the kernel that makes the stop tests
            if (e == hipSuccess) e = launch_lds<false>(dbl_level_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, tm, lvl, d, a.stop, (const double*)partS, (const double*)partM, (const double*)T2);
        } else std::swap(d.Md, T2);
        if (e != hipSuccess) return e;
        if (conv && lvl == p.max_levels) break;
    }
    // P = S(n) + M(n)' Q M(n)
    const double *Sn = conv ? d.Sd : d.Sa, *Mn = conv ? d.Md : d.Ma;
    e = sandwich(Mn, a.Q, a.q_stride, Sn, a.P_out, nullptr, 0);
    if (e == hipSuccess && !conv) e = launch_lds<false>(dbl_fixed_out_kernel, dim3(a.nprob), dim3(TILE_THREADS), 0, stream, (int)mx, top, d, Mn);
    return e;
}

hipError_t launch_policy_doubling(const DblArgs& p, hipStream_t stream) {
    const RicArgs& a = p.r;
    if (a.nprob <= 0) return hipSuccess;
    hipError_t e = dbl_preset(p, stream);
    if (e != hipSuccess) return e;
    if (a.N != 1) {
        RicGrid g;
        DblGrid d;
        dbl_records(p, g, d);
        e = launch_ric_project(g, a, stream);
        if (e == hipSuccess) e = launch_lds(dbl_setup_kernel, dim3((a.mx + DBL_RU - 1) / DBL_RU, a.nprob), dim3(TILE_THREADS), 2 * (size_t)a.mu * a.mx * sizeof(double), stream, g, d);
        if (e != hipSuccess) return e;
    }
    return launch_doubling_levels(p, stream);
}

}  // namespace cclqr
