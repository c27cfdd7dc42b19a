// cclqr_invariants.h -- the integrator's own invariants of a recorded rollout slab on the device (cclqr_rollout_invariants, invariants.hip): per
// instance and step the kinetic and potential energy, their sum, the largest translational and rotational constraint residual and the largest deviation of a
// quaternion from unit length, and an eight-number verdict per instance that survives a run without a trajectory.  The per-body and per-joint arithmetic lives here
// as __host__ __device__ functions so that tests/emu/emu_invariants.cpp runs it lane by lane on the CPU (test infrastructure only).  None of them contains a
// cross-lane operation: they are called under lane predicates (the rule of tests/test_static_kernel_rules.py); the butterflies are in invariants.hip.
//
// Row r of instance i (absolute step k = k0 + r), 13 entries per body as stored: x 0..2, q 3..6, v 7..9, w 10..12 (body frame).
//   out[0] T     = sum_b ( 0.5 m_b (v_b . v_b) + 0.5 (w_b . (J_b w_b)) )
//   out[1] V     = -g sum_b ( m_b x_b[2] )                 g: the mechanism's signed g
//   out[2] E     = out[0] + out[1]
//   out[3] gap   = max |g_r| over the translational constraint rows of all joints      R(q_a)'(x_b + R(q_b) p2 - x_a) - p1
//   out[4] twist = max |g_r| over the rotational rows                                  vec(conj(q_a) q_b conj(qoff))
//   out[5] quat  = max_b | q_b . q_b - 1 |
// The rows g_r are those of joint_eval<false> (cclqr_dev.h), picked by the mechanism's sel / rotmask tables; the origin is x = 0, q = 1.  A FixedOrientation
// constraint has its rotational rows only: its translational rows are 0 whatever the poses are.
// THE SUMMATION ORDER of T and V: one term per link in link order (MechDev::perm; closed loops: the caller's body order), padded with zeros to the lane-group width,
// added by the xor butterfly with offsets 1, 2, 4, ... (v_t += v_{t ^ o}).  Adding a zero is exact, so the bits depend on the link order alone, not on the width.
// Whatever is not finite counts as NaN (ens_canon): a value that is not finite makes the outputs it enters NaN -- never Inf -- and nothing else.  The max PROPAGATES
// a NaN (inv_max): one row that is not finite makes gap / twist / quat of that step NaN.
// The summary [8] of an instance, folded row by row in step order and carried from launch to launch (inv_summary_fold): 0 E at the first row where it is finite,
// 1, 2 min and max of E over such rows, 3 the max of gap over the rows where gap is finite, 4 the absolute step at which 3 was first reached, 5, 6 the max of twist
// and of quat over their finite rows, 7 the number of rows with any of the six outputs not finite.  0 .. 3, 5, 6 are NaN and 4 is 0 until such a row is seen.
#pragma once
#include "cclqr_ensemble.h"

#define CCLQR_INVARIANTS_LEN_ 6             // include/cclqr.h CCLQR_INVARIANTS_LEN / CCLQR_INVARIANTS_SUMMARY_LEN (static_assert in capi.hip)
#define CCLQR_INVARIANTS_SUMMARY_LEN_ 8

namespace cclqr {

#define INV_WAVES 4
#define INV_LOOP_SLOTS 2      // joints per lane of a closed-loop mechanism: up to CCLQR_LOOP_MAXJ = 12 joints on the 8 lanes of its 8 bodies
#define INV_FIXED_ORIENTATION_ 2

// launch arguments of invariants_kernel
struct InvArgs {
    const MechDev* M;
    const PlantRec* plants;   // per-instance plants: records [n_plant][nb] in link order, or nullptr = the mechanism's
    long long plant_off;      // instance i reads plant plant_off + i (= first_instance - the table's first_index; checked on the host)
    int nb, ne, loop;         // loop: MechDev::loop (ne joints by joint, at most 8 bodies); else ne = nb, the joint of link l
    long long n_inst;
    int steps, k0;
    const double* traj;       // [n_inst][steps][nb][13] caller's body order
    long long out_steps;
    double* inv;              // [n_inst][out_steps][6]: rows k0 - 1 .. k0 + steps - 2 are written; or nullptr
    double* rows;             // [n_inst][out_steps][ne][5] caller's joint order; or nullptr
    double* summary;          // [n_inst][8]: read when k0 > 1, always written; or nullptr
};

// what a lane keeps of one body and of one joint for the whole launch
struct InvBody {
    int b;                    // the body in the CALLER's numbering (the slab's)
    double m, J[9];
};
struct InvJoint {
    int a, b, out, rowmask;   // a, b: parent (-1: the origin) and child body in the caller's numbering; out: the caller's joint index; rowmask: inv_rowmask
    double sel[5][3], qoc[4], p1[3], p2[3];
};

// bit r: row r of the joint is rotational (MechDev::rotmask); bit 8 + r: the joint does not have row r (the translational rows of a FixedOrientation constraint)
HD int inv_rowmask(int type, int rotmask) { return (rotmask & 31) | (type == INV_FIXED_ORIENTATION_ ? (~rotmask & 31) << 8 : 0); }

// link l of a chain or tree; P: the plant's records in link order
HD void inv_load_body_link(InvBody& c, const MechDev* M, const PlantRec* P, int l) {
    c.b = M->perm[l]; c.m = P[l].m;
    for (int i = 0; i < 9; i++) c.J[i] = P[l].J[i];
}
HD void inv_load_joint_link(InvJoint& c, const MechDev* M, const PlantRec* P, int l) {
    c.b = M->perm[l]; c.out = M->jperm[l]; c.rowmask = inv_rowmask(M->type[l], M->rotmask[l]);
    const int pa = M->parent[l];
    c.a = pa >= 0 ? M->perm[pa] : -1;
    for (int i = 0; i < 3; i++) { c.p1[i] = P[l].p1[i]; c.p2[i] = P[l].p2[i]; }
    for (int i = 0; i < 4; i++) c.qoc[i] = M->qoc[l][i];
    for (int r = 0; r < 5; r++)
        for (int i = 0; i < 3; i++) c.sel[r][i] = M->sel[l][r][i];
}
// body b and joint j of a closed-loop mechanism: the tables by body and by joint, in the caller's order
HD void inv_load_body_loop(InvBody& c, const MechDev* M, int b) {
    c.b = b; c.m = M->m[b];
    for (int i = 0; i < 9; i++) c.J[i] = M->J[b][i];
}
HD void inv_load_joint_loop(InvJoint& c, const MechDev* M, int j) {
    c.a = M->parent[j]; c.b = M->jchild[j]; c.out = j; c.rowmask = inv_rowmask(M->type[j], M->rotmask[j]);
    for (int i = 0; i < 3; i++) { c.p1[i] = M->p1[j][i]; c.p2[i] = M->p2[j][i]; }
    for (int i = 0; i < 4; i++) c.qoc[i] = M->qoc[j][i];
    for (int r = 0; r < 5; r++)
        for (int i = 0; i < 3; i++) c.sel[r][i] = M->sel[j][r][i];
}

// the max that propagates a NaN; its arguments are canonical (ens_canon) and not negative, so it is symmetric to the bit
HD double inv_max(double a, double b) { return (a != a || a > b) ? a : b; }

// one body's terms of T and of sum m x_z, and its | q . q - 1 | (canonical)
HD void inv_body_terms(const InvBody& c, const double* row, double* T, double* V, double* quat) {
    const double* z = row + 13 * c.b;
    const double v0 = z[7], v1 = z[8], v2 = z[9], w0 = z[10], w1 = z[11], w2 = z[12];
    const double vv = v0 * v0 + v1 * v1 + v2 * v2;
    const double Jw0 = c.J[0] * w0 + c.J[1] * w1 + c.J[2] * w2, Jw1 = c.J[3] * w0 + c.J[4] * w1 + c.J[5] * w2, Jw2 = c.J[6] * w0 + c.J[7] * w1 + c.J[8] * w2;
    *T = 0.5 * c.m * vv + 0.5 * (w0 * Jw0 + w1 * Jw1 + w2 * Jw2);
    *V = c.m * z[2];
    *quat = ens_canon(fabs((z[3] * z[3] + z[4] * z[4] + z[5] * z[5] + z[6] * z[6]) - 1.0));
}

// the five constraint rows of one joint from one staged row (caller's body order): joint_eval<false>'s arithmetic; a row the joint does not have is 0
HD void inv_joint_rows(const InvJoint& j, const double* row, double* g) {
    const double* za = j.a >= 0 ? row + 13 * j.a : nullptr;
    const double* zb = row + 13 * j.b;
    const double* qa = za ? za + 3 : QID_;
    double Ra[9], Rb[9], rp[3], w[3], gT[3];
    rotmat(qa, Ra); rotmat(zb + 3, Rb);
    mv3(Rb, j.p2, rp);
    for (int i = 0; i < 3; i++) w[i] = zb[i] + rp[i] - (za ? za[i] : 0.0);
    mtv3(Ra, w, gT);
    for (int i = 0; i < 3; i++) gT[i] -= j.p1[i];
    double qac[4] = {qa[0], -qa[1], -qa[2], -qa[3]}, rel[4], e[4];
    qmul(qac, zb + 3, rel);
    qmul(rel, j.qoc, e);
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const bool rot = (j.rowmask >> r) & 1, absent = (j.rowmask >> (8 + r)) & 1;
        const double s0 = j.sel[r][0], s1 = j.sel[r][1], s2 = j.sel[r][2];
        const double v = rot ? (s0 * e[1] + s1 * e[2] + s2 * e[3]) : (s0 * gT[0] + s1 * gT[1] + s2 * gT[2]);
        g[r] = absent ? 0.0 : ens_canon(v);
    }
}
// ... folded into the lane's running gap and twist
HD void inv_joint_max(const InvJoint& j, const double* g, double* gap, double* twist) {
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const bool rot = (j.rowmask >> r) & 1;
        const double c = fabs(g[r]);
        if (rot) *twist = inv_max(*twist, c);
        else *gap = inv_max(*gap, c);
    }
}

// the six outputs of a row from the group's sums and maxima
HD void inv_outputs(double Tsum, double Vsum, double g, double gap, double twist, double quat, double* o) {
    o[0] = ens_canon(Tsum);
    o[1] = ens_canon(-g * Vsum);
    o[2] = ens_canon(o[0] + o[1]);
    o[3] = gap; o[4] = twist; o[5] = quat;
}

// entry i of the summary before the first row
HD double inv_summary_start(int i) { return (i == 4 || i == 7) ? 0.0 : NAN; }
// entry i of the summary after one row's outputs o, k the row's absolute step: sv the entry and gmax entry 3, both as they were BEFORE the row (entry 4, the step
// of the largest gap, is decided by entry 3).  A comparison with a NaN does not hold: `sv != sv` is "nothing seen yet".  On the device lane i of a group keeps entry
// i (and every lane entry 3), so a summary costs a lane two doubles, not eight
HD double inv_summary_entry(int i, double sv, double gmax, const double* o, int k) {
    const double E = o[2], gap = o[3], twist = o[4], quat = o[5];
    const bool none = sv != sv;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < CCLQR_INVARIANTS_LEN_; c++) bad = bad || (o[c] != o[c]);
    const double e0 = (E == E && none) ? E : sv;
    const double e1 = (E == E && (none || E < sv)) ? E : sv;
    const double e2 = (E == E && (none || E > sv)) ? E : sv;
    const double e3 = (gap == gap && (none || gap > sv)) ? gap : sv;
    const double e4 = (gap == gap && (gmax != gmax || gap > gmax)) ? (double)k : sv;
    const double e5 = (twist == twist && (none || twist > sv)) ? twist : sv;
    const double e6 = (quat == quat && (none || quat > sv)) ? quat : sv;
    const double e7 = bad ? sv + 1.0 : sv;
    return i == 0 ? e0 : (i == 1 ? e1 : (i == 2 ? e2 : (i == 3 ? e3 : (i == 4 ? e4 : (i == 5 ? e5 : (i == 6 ? e6 : e7))))));
}
// the whole summary on one lane (the host twin, and the statement of what the lanes do together)
HD void inv_summary_init(double* s) {
    for (int i = 0; i < CCLQR_INVARIANTS_SUMMARY_LEN_; i++) s[i] = inv_summary_start(i);
}
HD void inv_summary_fold(double* s, const double* o, int k) {
    const double gmax = s[3];
    for (int i = 0; i < CCLQR_INVARIANTS_SUMMARY_LEN_; i++) s[i] = inv_summary_entry(i, s[i], gmax, o, k);
}

// doubles of LDS one instance takes: the staged row, padded to an odd stride (as jnt_instance_doubles)
HD int inv_instance_doubles(int nb) { return (13 * nb) | 1; }
HD size_t inv_lds_bytes(int nb) { return sizeof(double) * (size_t)INV_WAVES * (64 / score_group_lanes(nb)) * inv_instance_doubles(nb); }

hipError_t launch_invariants(const InvArgs& a, hipStream_t stream);

}  // namespace cclqr
