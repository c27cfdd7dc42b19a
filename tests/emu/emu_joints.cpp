// emu_joints.cpp -- the per-joint functions of csrc/cclqr_joints.h run lane by lane on the host (test infrastructure only): what joints_kernel (csrc/joints.hip)
// does per instance, step and lane -- the row staged by the lane group's lanes (entries t, t + G, ...), lane t taking the joints t, t + G, ..., (w_prev, turns) kept
// per joint from the first step to the last and carried between calls -- and what series_moments_kernel and ens_finish_kernel do per row, tile and coordinate.
// The joint tables come in the caller's order (the device reads them through perm / jperm; the arithmetic is the same), the axis normalised.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_joints.h"
#include <vector>

using namespace cclqr;

extern "C" int emu_joints(int nb, int ne, long long n_inst, int steps, int k0, int mode, const int* type, const int* parent, const int* child, const double* axis,
                          const double* qoff, const double* p1, const double* p2, const double* traj, long long out_steps, double* theta, double* rate, double* carry) {
    const int G = score_group_lanes(nb), nz = 13 * nb;
    if (nb < 1 || nb > 64 || ne < nb || ne > JNT_LOOP_SLOTS * G || n_inst < 1 || steps < 1 || k0 < 1 || out_steps < k0 + steps - 1) return -1;
    if (mode == CCLQR_JOINTS_CONTINUOUS_ && !carry) return -1;
    std::vector<JointConst> jc(ne);
    for (int j = 0; j < ne; j++) {
        JointConst& c = jc[j];
        c.type = type[j]; c.a = parent[j]; c.b = child[j]; c.out = j;
        for (int i = 0; i < 3; i++) { c.axis[i] = axis[3 * j + i]; c.p1[i] = p1[3 * j + i]; c.p2[i] = p2[3 * j + i]; }
        c.qoc[0] = qoff[4 * j];
        for (int i = 1; i < 4; i++) c.qoc[i] = -qoff[4 * j + i];
    }
    std::vector<double> row(jnt_instance_doubles(nb)), st(2 * (size_t)ne);
    for (long long inst = 0; inst < n_inst; inst++) {
        for (int j = 0; j < ne; j++) {
            jnt_carry_init(&st[2 * j]);
            if (mode == CCLQR_JOINTS_CONTINUOUS_ && k0 > 1) { st[2 * j] = carry[(inst * ne + j) * 2]; st[2 * j + 1] = carry[(inst * ne + j) * 2 + 1]; }
        }
        for (int kk = 0; kk < steps; kk++) {
            const double* p = traj + (inst * steps + kk) * nz;
            for (int t = 0; t < G; t++)
                for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = p[e]; }
            for (int t = 0; t < G; t++)
                for (int j = t; j < ne; j += G) {
                    double th, rt;
                    jnt_step(jc[j], row.data(), mode, &st[2 * j], &th, &rt);
                    theta[(inst * out_steps + (k0 - 1 + kk)) * ne + j] = th;
                    if (rate) rate[(inst * out_steps + (k0 - 1 + kk)) * ne + j] = rt;
                }
        }
        if (mode == CCLQR_JOINTS_CONTINUOUS_)
            for (int j = 0; j < ne; j++) { carry[(inst * ne + j) * 2] = st[2 * j]; carry[(inst * ne + j) * 2 + 1] = st[2 * j + 1]; }
    }
    return 0;
}

// the moments of a series x [n_inst][steps][nc] in the defined order: a tile's partial by ens_pass_partial over the whole tile, the tiles merged in tile order
extern "C" int emu_series_moments(long long n_inst, int steps, int nc, const double* x, double* mean, double* m2) {
    if (n_inst < 1 || steps < 1 || nc < 1) return -1;
    const long long ntiles = ens_tiles(n_inst);
    std::vector<double> col(ENS_TILE), pm(ntiles), pq(ntiles);
    for (int r = 0; r < steps; r++)
        for (int c = 0; c < nc; c++) {
            for (long long tile = 0; tile < ntiles; tile++) {
                const long long base = tile * ENS_TILE;
                const int cnt = (int)(n_inst - base < ENS_TILE ? n_inst - base : ENS_TILE);
                for (int g = 0; g < cnt; g++) col[g] = ens_canon(x[((base + g) * steps + r) * nc + c]);
                ens_pass_partial(col.data(), 1, cnt, &pm[tile], &pq[tile]);
            }
            double m = pm[0], q = pq[0];
            for (long long tl = 1; tl < ntiles; tl++) {
                const long long left = n_inst - tl * ENS_TILE;
                ens_merge((double)(tl * ENS_TILE), &m, &q, (double)(left < ENS_TILE ? left : ENS_TILE), pm[tl], pq[tl]);
            }
            mean[(size_t)r * nc + c] = m;
            m2[(size_t)r * nc + c] = q;
        }
    return 0;
}

// the launch's own arithmetic: the dynamic LDS of joints_kernel for an nb-body mechanism and of the tile-moments kernel
extern "C" long long emu_joints_lds(int nb) { return (long long)jnt_lds_bytes(nb); }
extern "C" long long emu_series_moments_lds() { return (long long)ser_moments_lds_bytes(); }
