// quantiles.hip -- cclqr_rollout_quantiles: the quantiles of every coordinate of x = (dz, du) ACROSS the instances of a recorded slab, per step.
// The slab is read once.
//
// ens_stage_kernel<G>: the front end of ens_moments_kernel<G> (ensemble.hip) -- a workgroup owns one slab row and one tile of ENS_TILE instances, takes it in passes
// of ens_pass_instances(nb), and per pass a lane group stages its instance's row in LDS, forms dz per body lane and du over the group, by the SAME device functions
// (ens_body_row, score_gain_partial, ctrl_step_rows, ens_canon, ens_group_sum), so x is bit for bit the x the moments kernel reduces.  Where that kernel reduces a
// pass, this one copies it into a window [coordinate][W + 1] of LDS; every W instances (a whole tile where the LDS holds it, qnt_stage_window) the window goes
// out transposed: W consecutive threads write the W instances of one coordinate, a contiguous run of 8 W bytes of xt [row][coordinate (output order)][n_pad].
// ens_select_kernel: one workgroup per (row, coordinate).  It loads the coordinate's n_inst contiguous values, maps each to a sortable 64-bit key (qnt_key: a value
// that is not finite takes the largest key), pads to a power of two with that key, sorts the keys by a bitonic network in LDS (the pairs of cclqr_quantiles.h), and
// thread j < n_prob counts the finite keys and forms quantile j (qnt_count_finite, qnt_quantile).  A wavefront's 64 consecutive pairs of a step j <= 64 lie in its
// own 128 keys, so those steps are ordered by the wavefront's instruction order alone; only a step with j >= 128, or the step before one, ends at a workgroup barrier.
// Every barrier sits under control flow that depends on launch arguments only, and every loop has one exit.
#include "cclqr_internal.h"
#include "cclqr_quantiles.h"

namespace cclqr {

template <int G>
__global__ __launch_bounds__(64 * ENS_WAVES) void ens_stage_kernel(QntArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G, P = ENS_WAVES * IPW;      // instances per wavefront and per pass
    const int nb = a.nb, mu = a.mu, nz = 13 * nb, ne = 12 * nb, nx = ne + mu, gd = ens_group_doubles(nb, mu);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G, slot = wave * IPW + grp;
    double* row = lds + (size_t)slot * gd;
    double* X = row + nz;
    const int W = a.W, ws = W + 1;
    double* win = lds + (size_t)P * gd;                   // [nx][W + 1]
    const int steps = a.steps, rr = (int)(blockIdx.x % (unsigned)a.nrows), r = a.row0 + rr, k = a.k0 + r;
    const long long tile = blockIdx.x / (unsigned)a.nrows, tile_base = tile * ENS_TILE;
    const int tile_cnt = (int)((a.n_inst - tile_base < ENS_TILE) ? a.n_inst - tile_base : ENS_TILE), npass = (tile_cnt + P - 1) / P;
    const bool body = t < nb;
    const int ut = body ? a.M->perm[t] : 0;               // the caller's body that link t is

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
    double* xrow = a.xt + (size_t)rr * (size_t)nx * (size_t)a.n_pad;
    for (int ps = 0; ps < npass; ps++) {
        const long long gi = a.inst0 + inst_of(ps);
        const int cnt = (tile_cnt - ps * P < P) ? tile_cnt - ps * P : P;
        const int wbase = (ps * P) & ~(W - 1);            // first instance (of the tile) of the window this pass falls into
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = nxt[j]; }
        if (ps + 1 < npass) {      // the next pass's rows are on their way while this one is formed
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
        // thread c takes coordinate c of the pass's instances into the window
        for (int c = tid; c < nx; c += 64 * ENS_WAVES) {
            const double* xc = lds + nz + c;
            double* wc = win + (size_t)c * ws + (ps * P - wbase);
            for (int g = 0; g < cnt; g++) wc[g] = xc[(size_t)g * gd];
        }
        __syncthreads();      // the next pass overwrites the rows and x; the window is complete for the threads that write it out
        if (ps + 1 == npass || ((ps + 1) * P & (W - 1)) == 0) {
            const int wcnt = ps * P + cnt - wbase;        // instances in the window
            double* out = xrow + (size_t)(tile_base + wbase);
            for (int e = tid; e < nx * W; e += 64 * ENS_WAVES) {
                const int c = e / W, i = e & (W - 1);
                if (i < wcnt) out[(size_t)ens_out_index(c, ne, a.M->perm) * (size_t)a.n_pad + i] = win[(size_t)c * ws + i];
            }
            // (the window is written again only behind the next pass's first barrier)
        }
    }
}

__global__ __launch_bounds__(QNT_MAX_THREADS) void ens_select_kernel(QntArgs a, int n2) {
    extern __shared__ unsigned long long keys[];
    const int nx = ens_coords(a.nb, a.mu), c = blockIdx.x, rr = blockIdx.y, tid = threadIdx.x, T = blockDim.x, half = n2 >> 1;
    const double* x = a.xt + ((size_t)rr * (size_t)nx + (size_t)c) * (size_t)a.n_pad;
    for (int e = tid; e < n2; e += T) keys[e] = (e < a.n_inst) ? qnt_key(x[e]) : QNT_KEY_LAST;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int p = tid; p < half; p += T) qnt_compare_exchange(keys, qnt_pair_low(p, j), j, k);
            // the next step's distance is jn = j / 2 (or k when j = 1).  With j <= 64 AND jn <= 64 the keys a wavefront's pairs read next are the 128 keys its own
            // pairs have just written; otherwise another wavefront wrote some of them
            const int jn = (j > 1) ? (j >> 1) : k;
            if (j > 64 || jn > 64) __syncthreads();
            else ens_wave_sync();
        }
    }
    __syncthreads();
    if (tid < a.n_prob) {
        const int cnt = qnt_count_finite(keys, n2);
        const size_t r = (size_t)(a.row0 + rr);
        a.quant[(r * (size_t)a.n_prob + (size_t)tid) * (size_t)nx + (size_t)c] = qnt_quantile(keys, cnt, a.prob[tid]);
        if (tid == 0 && a.finite != nullptr) a.finite[r * (size_t)nx + (size_t)c] = cnt;
    }
}

// ens_select_kernel over the rows a.row0 .. of a.xt [nrows][ens_coords(a.nb, a.mu)][n_pad]: launch_quantiles' second half, and the back end of cclqr_series_quantiles
// (joints.hip; nb = 0, mu = the series' coordinates).  Reads n_inst, n_pad, nb, mu, row0, nrows, xt, n_prob, prob, quant, finite of a
hipError_t launch_quantile_select(const QntArgs& a, hipStream_t stream) {
    const int n2 = qnt_pow2(a.n_inst), nx = ens_coords(a.nb, a.mu);
    return launch_lds(ens_select_kernel, dim3((unsigned)nx, (unsigned)a.nrows), dim3((unsigned)qnt_select_threads(n2)), sizeof(unsigned long long) * (size_t)n2, stream, a, n2);
}

hipError_t launch_quantiles(const QntArgs& a, hipStream_t stream) {
    const int G = score_group_lanes(a.nb);
    const dim3 grid((unsigned)(ens_tiles(a.n_inst) * a.nrows)), block(64 * ENS_WAVES);
    const size_t lds = qnt_stage_lds_bytes(a.nb, a.mu, a.W);
    hipError_t e;
    switch (G) {
        case 8: e = launch_lds(ens_stage_kernel<8>, grid, block, lds, stream, a); break;
        case 16: e = launch_lds(ens_stage_kernel<16>, grid, block, lds, stream, a); break;
        case 32: e = launch_lds(ens_stage_kernel<32>, grid, block, lds, stream, a); break;
        default: e = launch_lds(ens_stage_kernel<64>, grid, block, lds, stream, a); break;
    }
    if (e != hipSuccess) return e;
    return launch_quantile_select(a, stream);
}

}  // namespace cclqr
