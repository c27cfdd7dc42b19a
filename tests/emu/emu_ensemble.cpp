// emu_ensemble.cpp -- the row and tile functions of csrc/cclqr_ensemble.h run lane by lane on the host (test infrastructure only): what ens_moments_kernel and
// ens_finish_kernel (csrc/ensemble.hip) do per slab row, tile, pass and lane group, with the lane group's cross-lane sums taken serially over its lanes, LDS as a
// plain array and the workgroup's threads as a loop over the coordinates.  Table rows come from ctrl_step_rows (cclqr_dev.h), as in the kernel.  Tables in link
// order, the slab in the caller's body order, perm[l] = the caller's body of link l.  The co-moment kernels are MFMA code and have no twin here.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_ensemble.h"
#include <vector>

using namespace cclqr;

extern "C" int emu_ensemble(int nb, int mu, long long n_inst, int steps, int k0, long long inst0, const int* perm, const double* traj, const double* zd, int n_ctrl,
                            int nsp, const double* K, int nK, int N, double* mean, double* m2) {
    const int G = score_group_lanes(nb), nz = 13 * nb, ne = 12 * nb, nx = ens_coords(nb, mu), gd = ens_group_doubles(nb, mu), P = ens_pass_instances(nb);
    if (nb < 1 || nb > G || gd < nz + nx || nx > ENS_COORDS * 64 * ENS_WAVES || n_inst < 1 || steps < 1) return -1;
    CtrlHot H;
    H.K = 0; H.zd = 0; H.Fd = 0;      // the rows are offsets from the tables' bases
    H.K_stride = n_ctrl > 1 ? (long long)nK * mu * ne : 0;
    H.zd_stride = n_ctrl > 1 ? (long long)nsp * nz : 0;
    H.Fd_stride = 0;
    H.nK = nK; H.N = N; H.nsp = nsp; H.mu = mu;
    const bool has_K = K != nullptr && nK > 0 && mu > 0;
    const long long ntiles = ens_tiles(n_inst);
    std::vector<double> lds((size_t)P * gd), part((size_t)ntiles * 2 * nx);
    for (int r = 0; r < steps; r++) {
        const int k = k0 + r;
        for (long long tile = 0; tile < ntiles; tile++) {
            const long long tile_base = tile * ENS_TILE;
            const int tile_cnt = (int)(n_inst - tile_base < ENS_TILE ? n_inst - tile_base : ENS_TILE), npass = (tile_cnt + P - 1) / P;
            std::vector<double> tm(nx), tq(nx);
            for (int ps = 0; ps < npass; ps++) {
                const int cnt = tile_cnt - ps * P < P ? tile_cnt - ps * P : P;
                for (int slot = 0; slot < cnt; slot++) {      // a lane group
                    const long long inst = tile_base + ps * P + slot;
                    double* row = lds.data() + (size_t)slot * gd;
                    double* X = row + nz;
                    const double* p = traj + (inst * steps + r) * nz;
                    for (int t = 0; t < G; t++)
                        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = p[e]; }
                    const CtrlRows rows = ctrl_step_rows(&H, k, inst0 + inst, nz, ne);
                    for (int t = 0; t < nb; t++) ens_body_row(row + 13 * perm[t], zd + rows.zd + 13 * t, X + 12 * t);
                    if (rows.gate && has_K) {
                        for (int i = 0; i < mu; i++) {
                            double d = 0.0;
                            for (int t = 0; t < G; t++) d += score_gain_partial(t, G, ne, K + rows.K + (size_t)i * ne, X);
                            X[ne + i] = ens_canon(-d);
                        }
                    } else {
                        for (int i = 0; i < mu; i++) X[ne + i] = 0.0;
                    }
                }
                for (int c = 0; c < nx; c++) {                // a thread of the reduction stage
                    double pm, pq;
                    ens_pass_partial(lds.data() + nz + c, gd, cnt, &pm, &pq);
                    if (ps == 0) { tm[c] = pm; tq[c] = pq; }
                    else ens_merge((double)(ps * P), &tm[c], &tq[c], (double)cnt, pm, pq);
                }
            }
            for (int c = 0; c < nx; c++) {
                const int o = ens_out_index(c, ne, perm);
                part[(size_t)tile * 2 * nx + o] = tm[c];
                part[(size_t)tile * 2 * nx + nx + o] = tq[c];
            }
        }
        for (int c = 0; c < nx; c++) {                        // ens_finish_kernel
            double m = part[c], q = part[nx + c];
            for (long long tl = 1; tl < ntiles; tl++) {
                const long long left = n_inst - tl * ENS_TILE;
                ens_merge((double)(tl * ENS_TILE), &m, &q, (double)(left < ENS_TILE ? left : ENS_TILE), part[(size_t)tl * 2 * nx + c], part[(size_t)tl * 2 * nx + nx + c]);
            }
            mean[(size_t)r * nx + c] = m;
            m2[(size_t)r * nx + c] = q;
        }
    }
    return 0;
}
