// emu_score.cpp -- the row functions of csrc/cclqr_score.h run lane by lane on the host (test infrastructure only): what score_kernel (csrc/score.hip) does per
// instance and step, with the lane group's cross-lane sums taken serially over its lanes and LDS as plain arrays.  Table rows come from ctrl_step_rows (cclqr_dev.h),
// as in the kernel.  Tables in link order, the slab in the caller's body order, perm[l] = the caller's body of link l.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_score.h"
#include <vector>

using namespace cclqr;

extern "C" int emu_score(int nb, int mu, long long n_inst, int steps, int k0, long long inst0, const int* perm, const double* traj, const double* zd, int n_ctrl,
                         int nsp, const double* K, int nK, int N, const double* Qb, const double* R, double settle_tol, double* score) {
    const int G = score_group_lanes(nb), nz = 13 * nb, ne = 12 * nb;
    if (nb < 1 || nb > G || score_instance_doubles(nb, mu) < nz + ne + mu) return -1;
    CtrlHot H;
    H.K = 0; H.zd = 0; H.Fd = 0;      // the rows are offsets from the tables' bases
    H.K_stride = n_ctrl > 1 ? (long long)nK * mu * ne : 0;
    H.zd_stride = n_ctrl > 1 ? (long long)nsp * nz : 0;
    H.Fd_stride = 0;
    H.nK = nK; H.N = N; H.nsp = nsp; H.mu = mu;
    const bool has_K = K != nullptr && nK > 0 && mu > 0;
    std::vector<double> lds(score_instance_doubles(nb, mu));
    double* row = lds.data();
    double* DZ = row + nz;
    double* DU = DZ + ne;
    for (long long inst = 0; inst < n_inst; inst++) {
        double s[CCLQR_SCORE_LEN_];
        score_init(s);
        if (k0 > 1) for (int i = 0; i < CCLQR_SCORE_LEN_; i++) s[i] = score[inst * CCLQR_SCORE_LEN_ + i];
        const double* p = traj + inst * (long long)steps * nz;
        for (int kk = 0; kk < steps; kk++) {
            const int k = k0 + kk;
            for (int t = 0; t < G; t++)
                for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = p[(long long)kk * nz + e]; }
            const CtrlRows rows = ctrl_step_rows(&H, k, inst0 + inst, nz, ne);
            double cx = 0.0;
            for (int t = 0; t < G; t++) {
                if (t >= nb) continue;
                double dz[12];
                score_body_error(row + 13 * perm[t], zd + rows.zd + 13 * t, dz);
                cx += score_body_cost(dz, Qb + 144 * t);
                for (int i = 0; i < 12; i++) DZ[12 * t + i] = dz[i];
            }
            double cu = 0.0;
            if (rows.gate && has_K) {
                for (int i = 0; i < mu; i++) {
                    double d = 0.0;
                    for (int t = 0; t < G; t++) d += score_gain_partial(t, G, ne, K + rows.K + (size_t)i * ne, DZ);
                    DU[i] = -d;
                }
                for (int t = 0; t < G; t++) cu += score_input_cost_partial(t, G, mu, R, DU);
            }
            score_accumulate(s, cx, cu, k, settle_tol);
        }
        for (int i = 0; i < CCLQR_SCORE_LEN_; i++) score[inst * CCLQR_SCORE_LEN_ + i] = s[i];
    }
    return 0;
}
