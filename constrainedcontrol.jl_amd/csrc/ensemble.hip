// ensemble.hip -- cclqr_rollout_ensemble: the mean and the centred sum of squares of every coordinate of x = (dz, du) ACROSS the instances of a recorded slab, per
// step, and the centred co-moment matrix of dz at the steps the caller lists.  Where score.hip reduces a slab along time per instance, these
// kernels reduce it across instances per step; they read the slab once.
//
// ens_moments_kernel<G>: a workgroup owns one slab row and one tile of ENS_TILE instances and takes the tile in passes of ens_pass_instances(nb).  Per pass a lane
// group of G = 8 / 16 / 32 / 64 lanes (score_group_lanes)
//   1. stages the 13 nb row of its instance in LDS (entries t, t + G, ...: coalesced; requested one pass earlier),
//   2. lane t < nb forms link t's error about the step's setpoint (score_body_error) and publishes it in link order,
//   3. with the feedback gate on, the group forms du_i = -K_i . dz (score_gain_partial, the gain rows read as the rollout's control phase reads them),
// then the workgroup's threads turn to the coordinates: thread c takes coordinate c of the pass's instances from LDS, forms the pass's (mean, M2) and merges it into
// the tile's (cclqr_ensemble.h).  At a listed row the same threads write the errors to the workspace in the caller's body order.
// ens_finish_kernel merges the tiles' partials in tile order.  No atomics anywhere: the order of every sum is a function of n_inst and the mechanism alone.
// ens_cov_kernel / ens_cov_finish_kernel: C = Dc' Dc on v_mfma_f64_16x16x4_f64 (tile_mfma_splitk), lower 32 x 32 tiles, ENS_KSPLIT instances per workgroup, the
// splits summed in index order and mirrored.
// Every cross-lane operation (the butterflies, the barriers) sits under control flow that depends on launch arguments and controller constants only.
#include "cclqr_internal.h"
#include "cclqr_ensemble.h"
#include "cclqr_riccati_dev.h"

namespace cclqr {

template <int G>
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_moments_kernel(EnsArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G, P = ENS_WAVES * IPW;      // instances per wavefront and per pass
    const int nb = a.nb, mu = a.mu, nz = 13 * nb, ne = 12 * nb, nx = ne + mu, gd = ens_group_doubles(nb, mu);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G, slot = wave * IPW + grp;
    double* row = lds + (size_t)slot * gd;
    double* X = row + nz;
    const int steps = a.steps, r = (int)(blockIdx.x % (unsigned)steps), k = a.k0 + r;
    const long long tile = blockIdx.x / (unsigned)steps, ntiles = ens_tiles(a.n_inst), tile_base = tile * ENS_TILE;
    const int tile_cnt = (int)((a.n_inst - tile_base < ENS_TILE) ? a.n_inst - tile_base : ENS_TILE), npass = (tile_cnt + P - 1) / P;
    const bool body = t < nb;
    const int ut = body ? a.M->perm[t] : 0;               // the caller's body that link t is
    int cslot = -1;                                       // is this row listed, and where do its errors go
    for (int q = 0; q < a.n_cov; q++) cslot = (a.cov_row[q] == r) ? q : cslot;

    // the controller's record is launch-invariant: ONE read (score_kernel)
    CtrlHot H;
    {
        const CtrlHot* Hg = &a.C->hot;
        H.K = Hg->K; H.zd = Hg->zd; H.Fd = 0;
        H.K_stride = Hg->K_stride; H.zd_stride = Hg->zd_stride; H.Fd_stride = 0;
        H.nK = Hg->nK; H.N = Hg->N; H.nsp = Hg->nsp; H.mu = Hg->mu;
    }
    const double* Ktab = (const double*)(uintptr_t)H.K;
    const double* zdtab = (const double*)(uintptr_t)H.zd;
    const bool has_K = Ktab != nullptr && H.nK > 0 && mu > 0;

    // the coordinates of this thread in the reduction stage, and where they go in the outputs
    int cmap[ENS_COORDS];
    double mean[ENS_COORDS], M2[ENS_COORDS];
#pragma unroll
    for (int j = 0; j < ENS_COORDS; j++) {
        const int c = tid + 64 * ENS_WAVES * j;
        cmap[j] = c < nx ? ens_out_index(c, ne, a.M->perm) : 0;
        mean[j] = 0.0; M2[j] = 0.0;
    }

    // a lane group without an instance (the short last pass) takes the tile's last one again: its x is never read
    auto inst_of = [&](int ps) { const int i = ps * P + slot; return tile_base + (i < tile_cnt ? i : tile_cnt - 1); };
    double nxt[CCLQR_SCORE_ROW_LOADS], zd[13];
    {
        const double* p = a.traj + (inst_of(0) * (long long)steps + r) * nz;
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; nxt[j] = (e < nz) ? p[e] : 0.0; }
    }
#pragma unroll
    for (int i = 0; i < 13; i++) zd[i] = 0.0;
    long long zoff = -1;
    for (int ps = 0; ps < npass; ps++) {
        const long long gi = a.inst0 + inst_of(ps);
        const int cnt = (tile_cnt - ps * P < P) ? tile_cnt - ps * P : P;
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = nxt[j]; }
        if (ps + 1 < npass) {      // the next pass's rows are on their way while this one is reduced
            const double* pn = a.traj + (inst_of(ps + 1) * (long long)steps + r) * nz;
#pragma unroll
            for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) nxt[j] = pn[e]; }
        }
        const CtrlRows rows = ctrl_step_rows(&H, k, gi, nz, ne);
        if (rows.zd != zoff) {     // (one table for all: read once)
            if (body) {
#pragma unroll
                for (int i = 0; i < 13; i++) zd[i] = zdtab[rows.zd + 13 * t + i];
            }
            zoff = rows.zd;
        }
        ens_wave_sync();
        if (body) {
            double z[13], dz[12];
#pragma unroll
            for (int i = 0; i < 13; i++) z[i] = row[13 * ut + i];
            ens_body_row(z, zd, dz);
#pragma unroll
            for (int i = 0; i < 12; i++) X[12 * t + i] = dz[i];
        }
        if (rows.gate && has_K) {
            ens_wave_sync();
            const double* Kp = Ktab + rows.K;
            for (int i = 0; i < mu; i++) {
                const double du = -ens_group_sum<G>(score_gain_partial(t, G, ne, Kp + (size_t)i * ne, X));
                if (t == 0) X[ne + i] = ens_canon(du);
            }
        } else {
            for (int i = t; i < mu; i += G) X[ne + i] = 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < ENS_COORDS; j++) {
            const int c = tid + 64 * ENS_WAVES * j;
            if (c < nx) {
                const double* xc = lds + nz + c;
                double pm, pq;
                ens_pass_partial(xc, gd, cnt, &pm, &pq);
                if (ps == 0) { mean[j] = pm; M2[j] = pq; }
                else ens_merge((double)(ps * P), &mean[j], &M2[j], (double)cnt, pm, pq);
                if (cslot >= 0 && c < ne) {
                    double* out = a.dzrows + ((size_t)cslot * (size_t)a.n_inst + (size_t)(tile_base + ps * P)) * ne + cmap[j];
                    for (int g = 0; g < cnt; g++) out[(size_t)g * ne] = xc[(size_t)g * gd];
                }
            }
        }
        __syncthreads();      // the next pass overwrites the rows and x
    }
    double* part = a.part + ((size_t)r * (size_t)ntiles + (size_t)tile) * 2 * nx;
#pragma unroll
    for (int j = 0; j < ENS_COORDS; j++) {
        const int c = tid + 64 * ENS_WAVES * j;
        if (c < nx) { part[cmap[j]] = mean[j]; part[nx + cmap[j]] = M2[j]; }
    }
}

// the tiles' partials of one row merged in tile order
__global__ __launch_bounds__(TILE_THREADS) void ens_finish_kernel(const double* part, long long ntiles, long long n_inst, int nx, double* mean, double* m2) {
    const size_t r = blockIdx.x;
    const double* p = part + r * (size_t)ntiles * 2 * nx;
    for (int c = threadIdx.x; c < nx; c += TILE_THREADS) {
        double m = p[c], q = p[nx + c];
        for (long long tl = 1; tl < ntiles; tl++) {
            const long long left = n_inst - tl * ENS_TILE;
            const double* pt = p + (size_t)tl * 2 * nx;
            ens_merge((double)(tl * ENS_TILE), &m, &q, (double)(left < ENS_TILE ? left : ENS_TILE), pt[c], pt[nx + c]);
        }
        mean[r * nx + c] = m;
        m2[r * nx + c] = q;
    }
}

// lower-triangle tile lt = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void ens_lower_tile(int lt, int* ti, int* tj) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= lt) i++;
    *ti = i; *tj = lt - i * (i + 1) / 2;
}

// one lower 32 x 32 tile of Dc' Dc over the instances of one K-split of one listed step: the centring and the edge masking are the operand lambdas'
__global__ __launch_bounds__(TILE_THREADS) void ens_cov_kernel(EnsCovArgs a) {
    __shared__ double red[4][1024];
    const int lt = blockIdx.x, split = blockIdx.y, q = blockIdx.z, mx = a.mx;
    int ti, tj;
    ens_lower_tile(lt, &ti, &tj);
    const long long kbase = (long long)split * ENS_KSPLIT;
    const int K = (int)(a.n_inst - kbase < ENS_KSPLIT ? a.n_inst - kbase : ENS_KSPLIT);
    const double* D = a.dzrows + ((size_t)q * (size_t)a.n_inst + (size_t)kbase) * mx;
    tile32_gram_centred(ti << 5, tj << 5, mx, K, D, a.mean + (size_t)a.cov_row[q] * a.stride, red);
    double* out = a.cpart + (((size_t)q * a.nsplit + split) * ens_lower_tiles(a.tm) + lt) * 1024;
    for (int e = threadIdx.x; e < 1024; e += TILE_THREADS) out[e] = tile32_sum(red, e);
}

// the splits of a tile summed in index order; the lower triangle is stored and mirrored, so C is exactly symmetric
__global__ __launch_bounds__(TILE_THREADS) void ens_cov_finish_kernel(EnsCovArgs a) {
    const int lt = blockIdx.x, q = blockIdx.y, mx = a.mx, ntri = ens_lower_tiles(a.tm);
    int ti, tj;
    ens_lower_tile(lt, &ti, &tj);
    double* Cq = a.cov + (size_t)q * mx * mx;
    for (int e = threadIdx.x; e < 1024; e += TILE_THREADS) {
        const int ii = e >> 5, jj = e & 31, i = (ti << 5) + ii, j = (tj << 5) + jj;
        if (i < mx && j < mx && j <= i) {
            double v = 0.0;
            for (int s = 0; s < a.nsplit; s++) v += a.cpart[(((size_t)q * a.nsplit + s) * ntri + lt) * 1024 + e];
            Cq[(size_t)i * mx + j] = v;
            Cq[(size_t)j * mx + i] = v;
        }
    }
}

// ens_finish_kernel over `steps` rows of partials [steps][ntiles][2][nx]: launch_ensemble's second half, and the back end of cclqr_series_ensemble (joints.hip)
hipError_t launch_ensemble_finish(const double* part, long long n_inst, int steps, int nx, double* mean, double* m2, hipStream_t stream) {
    return launch_lds<false>(ens_finish_kernel, dim3((unsigned)steps), dim3(TILE_THREADS), 0, stream, part, ens_tiles(n_inst), n_inst, nx, mean, m2);
}

hipError_t launch_ensemble(const EnsArgs& a, double* mean, double* m2, hipStream_t stream) {
    const int G = score_group_lanes(a.nb);
    const long long ntiles = ens_tiles(a.n_inst);
    const dim3 grid((unsigned)(ntiles * a.steps)), block(64 * ENS_WAVES);
    const size_t lds = ens_lds_bytes(a.nb, a.mu);
    hipError_t e;
    switch (G) {
        case 8: e = launch_lds(ens_moments_kernel<8>, grid, block, lds, stream, a); break;
        case 16: e = launch_lds(ens_moments_kernel<16>, grid, block, lds, stream, a); break;
        case 32: e = launch_lds(ens_moments_kernel<32>, grid, block, lds, stream, a); break;
        default: e = launch_lds(ens_moments_kernel<64>, grid, block, lds, stream, a); break;
    }
    if (e != hipSuccess) return e;
    return launch_ensemble_finish(a.part, a.n_inst, a.steps, ens_coords(a.nb, a.mu), mean, m2, stream);
}

hipError_t launch_ensemble_cov(const EnsCovArgs& a, int n_cov, hipStream_t stream) {
    const int ntri = ens_lower_tiles(a.tm);
    const hipError_t e = launch_lds<false>(ens_cov_kernel, dim3(ntri, a.nsplit, n_cov), dim3(TILE_THREADS), 0, stream, a);
    if (e != hipSuccess) return e;
    return launch_lds<false>(ens_cov_finish_kernel, dim3(ntri, n_cov), dim3(TILE_THREADS), 0, stream, a);
}

}  // namespace cclqr
