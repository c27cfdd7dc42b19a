// cclqr_score.h -- scoring a recorded rollout slab on the device (cclqr_rollout_score, score.hip): the quadratic cost the gains were designed to
// minimise, sum_k dz' Q dz + du' R du with dz the error of lqr.jl:92-103 and the Δt-scaled weights of lqr.jl:18-19, its peak and the last step outside
// a tolerance.  The per-row arithmetic lives here as __host__ __device__ functions so that tests/emu/emu_score.cpp runs it lane by lane on the CPU
// (test infrastructure only).  None of them contains a cross-lane operation: they are called under lane predicates (tests/test_static_kernel_rules.py).
#pragma once
#include "cclqr_dev.h"
#include "cclqr_chain.h"

#define CCLQR_SCORE_LEN_ 4      // include/cclqr.h CCLQR_SCORE_LEN (static_assert in capi.hip)

namespace cclqr {

// launch arguments of score_kernel.  Link order is the controller tables' order (CtrlDev: K columns, zd); traj is in the caller's body order, so
// lane t of a lane group reads body M->perm[t] of the row and the weights' blocks were permuted once, at create time (cclqr_score_create).
struct ScoreArgs {
    const MechDev* M;
    const CtrlDev* C;
    const double* Qb;     // [nb][12][12] per-body blocks, LINK order
    const double* R;      // [mu][mu]
    double settle_tol;
    int nb, mu;
    long long n_inst;
    int steps, k0;
    long long inst0;      // global index of instance 0 (the controller table of an instance is keyed by its global index)
    const double* traj;   // [n_inst][steps][nb][13] caller's body order
    double* score;        // [n_inst][4]: read when k0 > 1, always written
};

// lane group of an nb-body mechanism: the smallest of 8, 16, 32, 64 lanes that gives every body a lane
HD int score_group_lanes(int nb) { return nb <= 8 ? 8 : (nb <= 16 ? 16 : (nb <= 32 ? 32 : 64)); }
// doubles of LDS one instance takes: the staged row (13 nb), the error in link order (12 nb), the inputs (mu), padded to an odd stride
HD int score_instance_doubles(int nb, int mu) { return (13 * nb + 12 * nb + mu) | 1; }
// doubles between the weight blocks of consecutive links in LDS: odd, so that the body lanes' ds_read_b64 of one entry fall on distinct banks (144 would put a lane
// stride of 288 banks = 32 mod 64 between them: two bank pairs for the whole group)
#define SCORE_QB_STRIDE 145
// dynamic LDS of a workgroup of `waves` wavefronts: the weights' blocks once, then the instances
HD size_t score_lds_bytes(int nb, int mu, int waves) {
    return sizeof(double) * ((size_t)SCORE_QB_STRIDE * nb + (size_t)waves * (64 / score_group_lanes(nb)) * score_instance_doubles(nb, mu));
}

// entry e of a 13 nb row as the lane t of a G-lane group fetches it: entries t, t + G, t + 2 G, ... (coalesced over the group); at most 13 per lane
#define CCLQR_SCORE_ROW_LOADS 13

// error of one body about its setpoint, order x, v, qtilde, w (lqr.jl:92-95): ph_control_error's arithmetic (cclqr_dev.h), on registers
HD void score_body_error(const double* z, const double* zd, double* dz) { ck_control_error(z, zd, dz); }

// dz' Qb dz of one body, Qb [12][12] as written (symmetric or not): row by row, each row's dot product first
HD double score_body_cost(const double* dz, const double* Qb) {
    double c = 0.0;
#pragma unroll
    for (int r = 0; r < 12; r++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) s += Qb[12 * r + j] * dz[j];
        c += dz[r] * s;
    }
    return c;
}

// lane t's share of K_i . dz: entries t, t + G, ... of the gain row and of the error (both in link order); the caller sums over the group
HD double score_gain_partial(int t, int G, int ne, const double* Krow, const double* dz) {
    double s = 0.0;
    for (int c = t; c < ne; c += G) s += Krow[c] * dz[c];
    return s;
}

// lane t's share of du' R du: rows t, t + G, ... of R; the caller sums over the group
HD double score_input_cost_partial(int t, int G, int mu, const double* R, const double* du) {
    double c = 0.0;
    for (int i = t; i < mu; i += G) {
        double s = 0.0;
        for (int j = 0; j < mu; j++) s += R[(size_t)i * mu + j] * du[j];
        c += du[i] * s;
    }
    return c;
}

// one step's stage costs into the running score, in step order.  A non-finite cx makes Jx and peak NaN and counts as outside the tolerance:
// the max and the comparison are written so that a NaN propagates (cx > peak is false for a NaN on either side)
HD void score_accumulate(double* s, double cx, double cu, int k, double settle_tol) {
    if (!(fabs(cx) <= 1.7976931348623157e308)) cx = NAN;
    s[0] += cx;
    s[1] += cu;
    s[2] = (cx > s[2] || cx != cx) ? cx : s[2];
    if (!(cx <= settle_tol)) s[3] = (double)k;
}
// the score before the first step (a stage cost may be negative under an indefinite Qb: the peak starts below every number)
HD void score_init(double* s) { s[0] = 0.0; s[1] = 0.0; s[2] = -INFINITY; s[3] = 0.0; }

hipError_t launch_score(const ScoreArgs& a, hipStream_t stream);

}  // namespace cclqr
