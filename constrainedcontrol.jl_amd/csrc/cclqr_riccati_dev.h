// cclqr_riccati_dev.h -- what the two recursions over a problem's projected model share: the Riccati sweep that solves for the gain (riccati.hip, lqr.jl:141-184)
// and the policy evaluation that is given it (policy.hip).  The launch arguments of the kernels (RicGrid), where a knot's pivots and singular flag lie,
// the MFMA tiles of v_mfma_f64_16x16x4_f64 both build their mx^3 products from, and the host pieces of riccati.hip that policy.hip calls: the workspace
// walk and the one projection onto [A' | D] (ric_project_kernel).
#pragma once
#include "cclqr_internal.h"
#include <math.h>
#include <string.h>
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

// =====================================================================================================================
// The blocks every recursion over [A' | D] is built from (policy.hip, policy_doubling.hip, covariance_doubling.hip, covariance_tracking.hip,
// riccati_doubling.hip).  Each takes its sums in ONE fixed order, and the bitwise properties the tests hold these files to -- independence of batch, sharing,
// chunking and path, the duality of the covariance with the cost recursion -- rest on that order being written once: a new recursion calls these, it does not copy them.

// ---- the register-held tile set of a resident workgroup: the 16x16 tiles of an mx x mx matrix one wavefront holds across a barrier, ceil(6 * 6 / 8) at the
// resident limit of 96 states.  Five named values, tile t put and picked by selects, so that the tile loops stay rolled (one copy of their bodies) and nothing is
// indexed at run time (an array indexed inside a rolled loop is placed in scratch memory)
#define RES_TILES 5
struct ResTiles {
    v4d a0, a1, a2, a3, a4;
    __device__ __forceinline__ void put(int t, v4d r) { if (t == 0) a0 = r; if (t == 1) a1 = r; if (t == 2) a2 = r; if (t == 3) a3 = r; if (t == 4) a4 = r; }
    __device__ __forceinline__ v4d pick(int t) const { return t == 0 ? a0 : (t == 1 ? a1 : (t == 2 ? a2 : (t == 3 ? a3 : a4))); }
};
static_assert(sizeof(ResTiles) == RES_TILES * sizeof(v4d), "ResTiles holds RES_TILES tiles: put and pick name each of them");
// the sizes the tile loops are written in: t16 = ceil(mx / 16), ntile = t16^2, ng = mx / 4 k-groups (mx % 4 == 0), this lane's place, nw wavefronts (wavefront
// `wave` takes the tiles wave, wave + nw, ..).  A kernel may hand in values it re-derives as it goes (ctk_resident_kernel)
struct ResShape { int mx, t16, ntile, ng, wave, li, lk, nw; };
__device__ __forceinline__ ResTiles res_zero() { const v4d zero4 = {0.0, 0.0, 0.0, 0.0}; return {zero4, zero4, zero4, zero4, zero4}; }
// C = A' B for two mx x mx LDS operands, both read along rows: this wavefront's tiles, kept in registers
__device__ __forceinline__ ResTiles res_mul(const ResShape& s, lds_double* A, lds_double* B) {
    ResTiles acc = res_zero();
#pragma unroll 1
    for (int t = 0; t < RES_TILES && s.wave + s.nw * t < s.ntile; t++) {
        const int tile = s.wave + s.nw * t;
        const int i0 = (tile / s.t16) << 4, j0 = (tile % s.t16) << 4;
        const int ic = (i0 + s.li < s.mx) ? i0 + s.li : s.mx - 1, jc = (j0 + s.li < s.mx) ? j0 + s.li : s.mx - 1;
        const v4d r = wave_tile16_db(s.ng, A + s.lk * s.mx + ic, 4 * s.mx, B + s.lk * s.mx + jc, 4 * s.mx);
        acc.put(t, r);
    }
    return acc;
}
// f(i, j, C[i][j]) on every element this lane holds
template <class F>
__device__ __forceinline__ void res_each(const ResShape& s, const ResTiles& acc, F f) {
#pragma unroll 1
    for (int t = 0; t < RES_TILES && s.wave + s.nw * t < s.ntile; t++) {
        const int tile = s.wave + s.nw * t;
        const int i0 = (tile / s.t16) << 4, j = ((tile % s.t16) << 4) + s.li;
        const v4d v = acc.pick(t);
        if (j < s.mx) {
#pragma unroll
            for (int r = 0; r < 4; r++) { const int i = i0 + s.lk + 4 * r; if (i < s.mx) f(i, j, v[r]); }
        }
    }
}

// ---- the 32x32 masked-edge tile of a tiled launch: workgroup `tile` of tm x tm, 256 threads
struct Tile32 {
    int i0, j0;
    bool iok[2], jok[2];      // are this lane's two operand columns (i0 / j0 + 16 h + li) inside the matrix
};
__device__ __forceinline__ Tile32 tile32_at(int tile, int tm, int mx) {
    const int li = threadIdx.x & 15, i0 = (tile / tm) << 5, j0 = (tile % tm) << 5;
    return {i0, j0, {i0 + li < mx, i0 + 16 + li < mx}, {j0 + li < mx, j0 + 16 + li < mx}};
}
// the tile of op(A) op(B) into red (tile_mfma_splitk), A and B mx x mx in global memory.  ta: op(A) = A' (A is read along rows, the lane's column contiguous),
// else A; tb: op(B) = B', else B (read along rows)
__device__ __forceinline__ void tile32_product(const Tile32& t, int mx, const double* A, int ta, const double* B, int tb, double (*red)[1024]) {
    const int li = threadIdx.x & 15;
    tile_mfma_splitk(mx,
        [&](int kk, int h) { return t.iok[h] ? (ta ? A[(size_t)kk * mx + t.i0 + 16 * h + li] : A[(size_t)(t.i0 + 16 * h + li) * mx + kk]) : 0.0; },
        [&](int kk, int h) { return t.jok[h] ? (tb ? B[(size_t)(t.j0 + 16 * h + li) * mx + kk] : B[(size_t)kk * mx + t.j0 + 16 * h + li]) : 0.0; }, red);
}
// the tile at (i0, j0) of Xc' Xc into red, Xc = the K rows of X [K][mx] (global memory) less the row vector mean [mx]: a block of a centred Gram (co-moment) matrix
// (ensemble.hip).  The centring and the edge masking are the operand lambdas'; a K-split of a longer sum hands in its own rows
__device__ __forceinline__ void tile32_gram_centred(int i0, int j0, int mx, int K, const double* X, const double* mean, double (*red)[1024]) {
    const int li = threadIdx.x & 15;
    bool iok[2], jok[2];
    double mi[2], mj[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        iok[h] = i0 + 16 * h + li < mx; jok[h] = j0 + 16 * h + li < mx;
        mi[h] = iok[h] ? mean[i0 + 16 * h + li] : 0.0; mj[h] = jok[h] ? mean[j0 + 16 * h + li] : 0.0;
    }
    tile_mfma_splitk(K,
        [&](int kk, int h) { return iok[h] ? X[(size_t)kk * mx + i0 + 16 * h + li] - mi[h] : 0.0; },
        [&](int kk, int h) { return jok[h] ? X[(size_t)kk * mx + j0 + 16 * h + li] - mj[h] : 0.0; }, red);
}
// element e of the tile: the four wavefronts' partial sums in wave order
__device__ __forceinline__ double tile32_sum(const double (*red)[1024], int e) { return ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]; }
// Ct = (A' B)' for the tile: the product, stored transposed with consecutive threads on consecutive i
__device__ __forceinline__ void tile32_product_transposed(const Tile32& t, int mx, const double* A, const double* B, double* Ct, double (*red)[1024]) {
    tile32_product(t, mx, A, 1, B, 0, red);
    for (int e = threadIdx.x; e < 1024; e += TILE_THREADS) {
        const int jj = e >> 5, ii = e & 31, i = t.i0 + ii, j = t.j0 + jj;
        if (i < mx && j < mx) Ct[(size_t)j * mx + i] = tile32_sum(red, ii * 32 + jj);
    }
}

// ---- a Frobenius norm whose sum of squares must not overflow: before the growth stop of a doubling fires the increments of an unstable closed loop reach 1e200
// (S(2n) is about norm(M)^2 |Q|), and their squares do not exist in fp64.  Two sums, as in Blue's algorithm without its small range: an entry above 2^500 is
// squared after scaling by 2^-600.  (An entry below 2^-511 underflows when squared: such a norm lies far below any tol and is reported as smaller than it is, down to 0.)
struct SqSum {
    double mid, big;
    __device__ __forceinline__ void add(double v) {
        if (fabs(v) > 0x1p500) { const double s = v * 0x1p-600; big += s * s; } else mid += v * v;
    }
    __device__ __forceinline__ double norm() const { return big > 0.0 ? sqrt(big + (mid * 0x1p-600) * 0x1p-600) * 0x1p600 : sqrt(mid); }
};
// the norm from a problem's per-tile sums [ntile][2], added in index order per lane and then over the lanes: the same for every launch.  Valid in the first wavefront
__device__ inline double sq_tile_total(const double* part, int ntile) {
    SqSum tot = {0.0, 0.0};
    for (int t = threadIdx.x; t < ntile; t += 64) { tot.mid += part[2 * t]; tot.big += part[2 * t + 1]; }
    for (int o = 32; o > 0; o >>= 1) { tot.mid += __shfl_xor(tot.mid, o, 64); tot.big += __shfl_xor(tot.big, o, 64); }
    return tot.norm();
}
// a pair over a 256-thread workgroup: the lanes by the shuffle tree, wavefront w's sums into wsum[0 / 1][w]; then sq_wave_sum(wsum, c) is the total of component c
// (0 mid, 1 big), the wavefronts in index order.  Ends synchronised
__device__ __forceinline__ void sq_reduce(SqSum acc, double (*wsum)[4]) {
    for (int s = 32; s > 0; s >>= 1) { acc.mid += __shfl_xor(acc.mid, s, 64); acc.big += __shfl_xor(acc.big, s, 64); }
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = acc.mid; wsum[1][threadIdx.x >> 6] = acc.big; }
    __syncthreads();
}
__device__ __forceinline__ double sq_wave_sum(const double (*wsum)[4], int c) { return ((wsum[c][0] + wsum[c][1]) + wsum[c][2]) + wsum[c][3]; }

// the generic product of the doubling recursions, one 32x32 tile of problem prob:  C = op(A) op(B) [+ E] [+ I]  and, where part [nprob][tm * tm][2] is given, the
// tile's sum of squares of op(A) op(B).  E (null: no addend) may be C -- the lane that owns an element reads and writes it; A and B may not
__device__ __forceinline__ void tile32_product_store(int mx, int tm, int prob, const double* A, int ta, const double* B, int tb, const double* E, int eye, double* Cm,
                                                     double* part, double (*red)[1024], double (*wsum)[4]) {
    const Tile32 t = tile32_at(blockIdx.x, tm, mx);
    tile32_product(t, mx, A, ta, B, tb, red);
    SqSum acc = {0.0, 0.0};
    for (int e = threadIdx.x; e < 1024; e += TILE_THREADS) {
        const int ii = e >> 5, jj = e & 31, i = t.i0 + ii, j = t.j0 + jj;
        if (i < mx && j < mx) {
            const double v = tile32_sum(red, e);
            acc.add(v);
            double c = E ? E[(size_t)i * mx + j] + v : v;
            if (eye && i == j) c += 1.0;
            Cm[(size_t)i * mx + j] = c;
        }
    }
    if (!part) return;
    sq_reduce(acc, wsum);
    if (threadIdx.x < 2) part[2 * ((size_t)prob * (tm * tm) + blockIdx.x) + threadIdx.x] = sq_wave_sum(wsum, threadIdx.x);
}

// ---- entry (i, j) of Abar = A' - D K (= A-Bu*Kuk-Bλ*Kλk, lqr.jl:169) from a knot's [A' | D] [mx][na] and a gain K [mu][mx], and entry (r, j) of R K
template <class PK>
__device__ __forceinline__ double ric_abar_entry(const double* AD, int na, int mx, int mu, int i, int j, PK K) {
    double s = AD[(size_t)i * na + j];
    for (int c = 0; c < mu; c++) s -= AD[(size_t)i * na + mx + c] * K[c * mx + j];
    return s;
}
template <class PR, class PK>
__device__ __forceinline__ double ric_rk_entry(PR R, int mx, int mu, int r, int j, PK K) {
    double s = 0.0;
    for (int c = 0; c < mu; c++) s += R[r * mu + c] * K[c * mx + j];
    return s;
}

// ---- host side
// The sizes of g from a, and the workspace of one launch walked once: g's arrays are placed one behind the other from `base` (null: nowhere); returns the doubles
// of the whole (= ric_total_work_doubles).  Defined in riccati.hip
size_t ric_lay_out(RicGrid& g, const RicArgs& a, double* base);
// [A' | D] of every knot of every problem into g.AD, the pivots and the singular flag of every knot behind g.scratch (ric_knot_piv), Pk = Q into buffer 0 of g.P:
// ric_project_kernel, the one projection of the library (riccati.hip).  g: laid out by ric_lay_out, with A, Bu, Bl, G, Q and q_stride set
hipError_t launch_ric_project(const RicGrid& g, const RicArgs& a, hipStream_t stream);
// the launch record for these arguments: laid out on a.work, with the models, Q, R and their strides, kbreak, status and stop; everything else zero, for the caller to set
inline RicGrid ric_grid_of(const RicArgs& a) {
    RicGrid g;
    memset(&g, 0, sizeof(g));
    (void)ric_lay_out(g, a, a.work);
    g.A = a.A; g.Bu = a.Bu; g.Bl = a.Bl; g.G = a.G; g.Q = a.Q; g.R = a.R; g.q_stride = a.q_stride; g.r_stride = a.r_stride;
    g.kbreak = a.kbreak; g.status = a.status; g.stop = a.stop;
    return g;
}
// does the resident tile set serve mx states on nw wavefronts: whole k-groups of four (wave_tile16_db) and a wavefront's share of the 16x16 tiles within ResTiles
// (mx <= 96 on eight).  Each resident kernel adds its own LDS formula
inline bool res_tiles_serve(int mx, int nw) {
    const int t16 = (mx + 15) / 16;
    return (mx & 3) == 0 && t16 * t16 <= RES_TILES * nw;
}

}  // namespace cclqr
