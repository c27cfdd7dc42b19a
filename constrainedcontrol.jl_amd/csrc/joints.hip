// joints.hip -- cclqr_rollout_joints: the joint coordinate and the relative joint velocity of every joint at every row of a recorded slab, and
// the front ends of cclqr_series_ensemble / cclqr_series_quantiles, the statistics of any per-instance series across its instances.  A streaming pass over the
// slab, as score.hip is: the slab is read once.
//
// joints_kernel<G, LOOP>: a lane group of G = 8 / 16 / 32 / 64 lanes (score_group_lanes) owns one instance and walks its steps.  Per step the group
//   1. stages the 13 nb row it requested one step earlier in LDS (entries t, t + G, ...: coalesced) and requests the next step's row,
//   2. lane t takes the joints t, t + G, ... (trees: the joint of link t; closed loops: the joint tables by joint, up to 12 joints on 8 lanes):
//      theta and the rate from the two bodies' entries of the row (cclqr_joints.h), written into the [ne] run of the step's output row.
// (w_prev, turns) of the continuous mode stay in the lane's registers from the first step to the last.  There is no workgroup barrier: a row is private to ONE lane
// group of ONE wavefront, and the only cross-lane operation, the wave barrier around the staged row, sits in the step loop, whose bounds are launch arguments.
// series_moments_kernel: a workgroup owns one row, one tile of ENS_TILE instances and SER_THREADS coordinates; thread c copies its coordinate's values of the tile,
// canonicalised, into its own column of LDS and forms the tile's (mean, M2) by ens_pass_partial.  ens_finish_kernel (ensemble.hip) merges the tiles in tile order.
// series_stage_kernel: ENS_TILE instances x SER_TT coordinates of one row through an LDS tile into xt [row][coordinate][n_pad], reads and writes both coalesced;
// ens_select_kernel (quantiles.hip) sorts each coordinate.  No atomics anywhere.
#include "cclqr_internal.h"
#include "cclqr_joints.h"

namespace cclqr {

// the staged row is private to ONE lane group of ONE wavefront (score_wave_sync: the wavefront's own instruction order orders its LDS operations)
__device__ __forceinline__ void jnt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G, bool LOOP>
__global__ __launch_bounds__(64 * JNT_WAVES) void joints_kernel(JointsArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G, SLOTS = LOOP ? JNT_LOOP_SLOTS : 1;      // instances per wavefront, joints per lane
    const int nb = a.nb, ne = a.ne, nz = 13 * nb;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G;
    double* row = lds + (size_t)(wave * IPW + grp) * jnt_instance_doubles(nb);
    const long long inst_raw = ((long long)blockIdx.x * JNT_WAVES + wave) * IPW + grp;
    const bool valid = inst_raw < a.n_inst;
    const long long inst = valid ? inst_raw : a.n_inst - 1;      // (a lane group without an instance takes the last one again; nothing of it is written)
    const int steps = a.steps, k0 = a.k0, mode = a.mode;
    const bool cont = mode == CCLQR_JOINTS_CONTINUOUS_;
    const PlantRec* P = a.plants ? a.plants + (a.plant_off + inst) * nb : a.M->rec;

    JointConst jc[SLOTS];
    double st[SLOTS][2];
    bool mine[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; sl++) {
        const int j = t + sl * G;
        mine[sl] = j < ne;
        const int jj = mine[sl] ? j : 0;
        if (LOOP) jnt_load_loop(jc[sl], a.M, jj);
        else jnt_load_link(jc[sl], a.M, P, jj);
        jnt_carry_init(st[sl]);
        if (cont && k0 > 1 && mine[sl]) {
            const double* cr = a.carry + (inst * ne + jc[sl].out) * 2;
            st[sl][0] = cr[0]; st[sl][1] = cr[1];
        }
    }
    const double* p = a.traj + inst * (long long)steps * nz;
    double nxt[CCLQR_SCORE_ROW_LOADS];
#pragma unroll
    for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; nxt[j] = (e < nz) ? p[e] : 0.0; }
    double* th_out = a.theta + (inst * a.out_steps + (k0 - 1)) * ne;
    double* rt_out = a.rate ? a.rate + (inst * a.out_steps + (k0 - 1)) * ne : nullptr;
    for (int kk = 0; kk < steps; kk++) {
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = nxt[j]; }
        if (kk + 1 < steps) {      // the next step's row is on its way while this one is turned into joint coordinates
            const double* pn = p + (long long)(kk + 1) * nz;
#pragma unroll
            for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) nxt[j] = pn[e]; }
        }
        jnt_wave_sync();
#pragma unroll
        for (int sl = 0; sl < SLOTS; sl++) {
            if (mine[sl]) {
                double th, rt;
                jnt_step(jc[sl], row, mode, st[sl], &th, &rt);
                if (valid) {
                    th_out[(long long)kk * ne + jc[sl].out] = th;
                    if (rt_out) rt_out[(long long)kk * ne + jc[sl].out] = rt;
                }
            }
        }
        jnt_wave_sync();      // the next step overwrites the row
    }
    if (cont && valid) {
#pragma unroll
        for (int sl = 0; sl < SLOTS; sl++) {
            if (mine[sl]) {
                double* cr = a.carry + (inst * ne + jc[sl].out) * 2;
                cr[0] = st[sl][0]; cr[1] = st[sl][1];
            }
        }
    }
}

hipError_t launch_joints(const JointsArgs& a, hipStream_t stream) {
    const int G = score_group_lanes(a.nb);
    const long long per_block = (long long)JNT_WAVES * (64 / G);
    const dim3 grid((unsigned)((a.n_inst + per_block - 1) / per_block)), block(64 * JNT_WAVES);
    const size_t lds = jnt_lds_bytes(a.nb);
    if (a.loop) return launch_lds(joints_kernel<8, true>, grid, block, lds, stream, a);      // a closed loop: at most 8 bodies
    switch (G) {
        case 8: return launch_lds(joints_kernel<8, false>, grid, block, lds, stream, a);
        case 16: return launch_lds(joints_kernel<16, false>, grid, block, lds, stream, a);
        case 32: return launch_lds(joints_kernel<32, false>, grid, block, lds, stream, a);
        default: return launch_lds(joints_kernel<64, false>, grid, block, lds, stream, a);
    }
}

// ---- the tile partials of a series x [n_inst][steps][nc]: grid (steps * tiles, coordinate blocks)
__global__ __launch_bounds__(SER_THREADS) void series_moments_kernel(long long n_inst, int steps, int nc, const double* x, double* part) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, c = blockIdx.y * SER_THREADS + tid;
    const int r = (int)(blockIdx.x % (unsigned)steps);
    const long long tile = blockIdx.x / (unsigned)steps, ntiles = ens_tiles(n_inst), tile_base = tile * ENS_TILE;
    const int cnt = (int)((n_inst - tile_base < ENS_TILE) ? n_inst - tile_base : ENS_TILE);
    if (c < nc) {
        const double* xc = x + ((size_t)tile_base * (size_t)steps + (size_t)r) * (size_t)nc + (size_t)c;
        double* col = lds + tid;      // this thread's own column: nobody else reads or writes it
        for (int g = 0; g < cnt; g++) col[(size_t)g * SER_THREADS] = ens_canon(xc[(size_t)g * (size_t)steps * (size_t)nc]);
        double m, q;
        ens_pass_partial(col, SER_THREADS, cnt, &m, &q);
        double* out = part + ((size_t)r * (size_t)ntiles + (size_t)tile) * 2 * (size_t)nc;
        out[c] = m; out[nc + c] = q;
    }
}

hipError_t launch_series_moments(long long n_inst, int steps, int nc, const double* x, double* part, hipStream_t stream) {
    const dim3 grid((unsigned)(ens_tiles(n_inst) * steps), (unsigned)((nc + SER_THREADS - 1) / SER_THREADS));
    return launch_lds(series_moments_kernel, grid, dim3(SER_THREADS), ser_moments_lds_bytes(), stream, n_inst, steps, nc, x, part);
}

// ---- rows row0 .. of a series transposed into xt [row][coordinate][n_pad]: grid (coordinate blocks, tiles, rows)
__global__ __launch_bounds__(256) void series_stage_kernel(long long n_inst, long long n_pad, int steps, int nc, const double* x, int row0, double* xt) {
    extern __shared__ double lds[];      // [ENS_TILE][SER_TT + 1]
    const int tid = threadIdx.x, c0 = blockIdx.x * SER_TT, rr = blockIdx.z, r = row0 + rr;
    const long long tile_base = (long long)blockIdx.y * ENS_TILE;
    const int cnt = (int)((n_inst - tile_base < ENS_TILE) ? n_inst - tile_base : ENS_TILE);
    for (int e = tid; e < ENS_TILE * SER_TT; e += 256) {
        const int g = e / SER_TT, cc = e % SER_TT;
        if (g < cnt && c0 + cc < nc) lds[g * (SER_TT + 1) + cc] = x[((size_t)(tile_base + g) * (size_t)steps + (size_t)r) * (size_t)nc + (size_t)(c0 + cc)];
    }
    __syncthreads();
    double* out = xt + (size_t)rr * (size_t)nc * (size_t)n_pad + (size_t)tile_base;
    for (int e = tid; e < ENS_TILE * SER_TT; e += 256) {
        const int cc = e / ENS_TILE, g = e % ENS_TILE;
        if (g < cnt && c0 + cc < nc) out[(size_t)(c0 + cc) * (size_t)n_pad + g] = lds[g * (SER_TT + 1) + cc];
    }
}

hipError_t launch_series_stage(long long n_inst, int steps, int nc, const double* x, int row0, int nrows, double* xt, hipStream_t stream) {
    const dim3 grid((unsigned)((nc + SER_TT - 1) / SER_TT), (unsigned)ens_tiles(n_inst), (unsigned)nrows);
    return launch_lds(series_stage_kernel, grid, dim3(256), sizeof(double) * ENS_TILE * (SER_TT + 1), stream, n_inst, ens_tiles(n_inst) * ENS_TILE, steps, nc, x, row0, xt);
}

}  // namespace cclqr
