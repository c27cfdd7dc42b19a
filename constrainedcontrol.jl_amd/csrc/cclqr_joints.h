// cclqr_joints.h -- the joint coordinates of a recorded rollout slab on the device (cclqr_rollout_joints, joints.hip): per instance, step and
// joint the minimal coordinate theta of pid.jl:43-57 (minimalCoordinates: the angle about / the offset along the joint axis, what ph_pid / lp_pid form inside the
// step) and the relative joint velocity of examples/trackingLQR_triple_cartpole.jl:98-101 (what the friction branches of ph_control_error / lp_friction form).
// The per-joint arithmetic lives here as __host__ __device__ functions so that tests/emu/emu_joints.cpp runs it lane by lane on the CPU (test infrastructure
// only).  None of them contains a cross-lane operation: they are called under lane predicates (the rule of tests/test_static_kernel_rules.py).
//
// Joint j hangs body b (its child) off body a (its parent, or the origin: x = 0, q = 1, velocities 0).
//   revolute   e = conj(q_a) q_b conj(qoff),  s = axis . vec(e),  c = e_0,  theta_raw = 2 atan2(s, c);   rate = axis . w_b - axis . w_a
//   prismatic  theta_raw = axis . (R_a'(x_b + R_b p2 - x_a) - p1);                                       rate = axis . R_a'(v_b - v_a)
//   a FixedOrientation constraint has no coordinate: 0 for both.
// Mode 1 (continuous) of a revolute: the principal value w in [-pi, pi] is 2 atan2(s, c) with (s, c) negated when c < 0 -- q and -q give the same w --, and
// theta_k = w_k + 2 pi turns_k with turns = 0 at step 1, one down where w_k - w_prev > pi and one up where it is < -pi.  A w that is not finite gives NaN and
// leaves (w_prev, turns) as they were; they travel from launch to launch in carry [n_inst][ne][2], so a horizon taken chunk by chunk gives the bits of one call.
// Whatever is not finite counts as NaN (ens_canon): a value that is not finite makes the outputs it enters NaN and nothing else.
#pragma once
#include "cclqr_ensemble.h"

#define CCLQR_JOINTS_RAW_ 0           // include/cclqr.h CCLQR_JOINTS_RAW / CCLQR_JOINTS_CONTINUOUS (static_assert in capi.hip)
#define CCLQR_JOINTS_CONTINUOUS_ 1
#define CCLQR_SERIES_MAX_COORDS_ 1024 // include/cclqr.h CCLQR_SERIES_MAX_COORDS

namespace cclqr {

#define JNT_WAVES 4
#define JNT_LOOP_SLOTS 2      // joints per lane of a closed-loop mechanism: up to CCLQR_LOOP_MAXJ = 12 joints on the 8 lanes of its 8 bodies

// launch arguments of joints_kernel
struct JointsArgs {
    const MechDev* M;
    const PlantRec* plants;   // per-instance plants: records [n_plant][nb] in link order (p1, p2 of a link's own joint), or nullptr = the mechanism's
    long long plant_off;      // instance i reads plant plant_off + i (= first_instance - the table's first_index; checked on the host)
    int nb, ne, loop;         // loop: MechDev::loop (ne joints by joint, at most 8 bodies); else ne = nb, the joint of link l
    long long n_inst;
    int steps, k0;
    const double* traj;       // [n_inst][steps][nb][13] caller's body order
    int mode;
    long long out_steps;
    double* theta;            // [n_inst][out_steps][ne] caller's joint order: rows k0 - 1 .. k0 + steps - 2 are written
    double* rate;             // the same shape, or nullptr
    double* carry;            // [n_inst][ne][2] = (w_prev, turns): read when k0 > 1, always written (mode 1), else nullptr
};

// what a lane keeps of one joint for the whole launch
struct JointConst {
    int type, a, b, out;      // a, b: the parent (-1: the origin) and child body in the CALLER's numbering (the slab's); out: the caller's joint index
    double axis[3], qoc[4], p1[3], p2[3];
};

// joint of link l of a chain or tree (bodies through perm, output index jperm); P: the plant's records in link order
HD void jnt_load_link(JointConst& c, const MechDev* M, const PlantRec* P, int l) {
    c.type = M->type[l]; c.b = M->perm[l]; c.out = M->jperm[l];
    const int pa = M->parent[l];
    c.a = pa >= 0 ? M->perm[pa] : -1;
    for (int i = 0; i < 3; i++) { c.axis[i] = M->axis[l][i]; c.p1[i] = P[l].p1[i]; c.p2[i] = P[l].p2[i]; }
    for (int i = 0; i < 4; i++) c.qoc[i] = M->qoc[l][i];
}
// joint j of a closed-loop mechanism: the joint tables by joint, bodies and joints in the caller's order
HD void jnt_load_loop(JointConst& c, const MechDev* M, int j) {
    c.type = M->type[j]; c.a = M->parent[j]; c.b = M->jchild[j]; c.out = j;
    for (int i = 0; i < 3; i++) { c.axis[i] = M->axis[j][i]; c.p1[i] = M->p1[j][i]; c.p2[i] = M->p2[j][i]; }
    for (int i = 0; i < 4; i++) c.qoc[i] = M->qoc[j][i];
}

HD bool jnt_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (s, c) of a revolute: ph_pid's arithmetic.  za: the parent's 13 entries or nullptr = the origin
HD void jnt_revolute_sc(const JointConst& j, const double* za, const double* zb, double* s, double* c) {
    const double* qa = za ? za + 3 : QID_;
    double qac[4] = {qa[0], -qa[1], -qa[2], -qa[3]}, rel[4], e[4];
    qmul(qac, zb + 3, rel);
    qmul(rel, j.qoc, e);
    *s = j.axis[0] * e[1] + j.axis[1] * e[2] + j.axis[2] * e[3];
    *c = e[0];
}
// the offset of a prismatic: ph_pid's arithmetic
HD double jnt_prismatic(const JointConst& j, const double* za, const double* zb) {
    const double* qa = za ? za + 3 : QID_;
    double Ra[9], Rb[9], rp[3], w[3], gT[3];
    rotmat(qa, Ra); rotmat(zb + 3, Rb);
    mv3(Rb, j.p2, rp);
    for (int i = 0; i < 3; i++) w[i] = zb[i] + rp[i] - (za ? za[i] : 0.0);
    mtv3(Ra, w, gT);
    return j.axis[0] * (gT[0] - j.p1[0]) + j.axis[1] * (gT[1] - j.p1[1]) + j.axis[2] * (gT[2] - j.p1[2]);
}
// the relative joint velocity: the friction law's `rel` (ph_control_error, lp_friction)
HD double jnt_rate(const JointConst& j, const double* za, const double* zb) {
    if (j.type > 1) return 0.0;
    double rel;
    if (j.type == 0) {
        rel = j.axis[0] * zb[10] + j.axis[1] * zb[11] + j.axis[2] * zb[12];
        if (za) rel -= j.axis[0] * za[10] + j.axis[1] * za[11] + j.axis[2] * za[12];
    } else {
        double dv[3], dva[3], Ra[9];
        for (int i = 0; i < 3; i++) dv[i] = zb[7 + i] - (za ? za[7 + i] : 0.0);
        rotmat(za ? za + 3 : QID_, Ra);
        mtv3(Ra, dv, dva);
        rel = j.axis[0] * dva[0] + j.axis[1] * dva[1] + j.axis[2] * dva[2];
    }
    return ens_canon(rel);
}
// mode 0 of a revolute: the number PID sees, NaN where s or c is not finite (atan2 of an infinity is a finite angle)
HD double jnt_raw_angle(double s, double c) { return (jnt_finite(s) && jnt_finite(c)) ? 2.0 * atan2(s, c) : NAN; }
// the principal value in [-pi, pi]: the two quaternions of one rotation give the same w
HD double jnt_principal(double s, double c) {
    if (!(jnt_finite(s) && jnt_finite(c))) return NAN;
    if (c < 0.0) { s = -s; c = -c; }
    return 2.0 * atan2(s, c);
}
// one step of the continuation: st = (w_prev, turns).  Before step 1 st = (NaN, 0): no comparison with a NaN holds, so the first finite w takes turns as it is
HD double jnt_continue(double w, double* st) {
    const double PI = 3.14159265358979323846;
    if (!jnt_finite(w)) return NAN;
    const double d = w - st[0];
    if (d > PI) st[1] -= 1.0;
    else if (d < -PI) st[1] += 1.0;
    st[0] = w;
    return w + (2.0 * PI) * st[1];
}
HD void jnt_carry_init(double* st) { st[0] = NAN; st[1] = 0.0; }

// theta and rate of one joint from one staged row (caller's body order); st: the joint's (w_prev, turns), touched in mode 1 on revolutes only
HD void jnt_step(const JointConst& j, const double* row, int mode, double* st, double* theta, double* rate) {
    const double* za = j.a >= 0 ? row + 13 * j.a : nullptr;
    const double* zb = row + 13 * j.b;
    double th = 0.0;
    if (j.type == 0) {
        double s, c;
        jnt_revolute_sc(j, za, zb, &s, &c);
        th = (mode == CCLQR_JOINTS_CONTINUOUS_) ? jnt_continue(jnt_principal(s, c), st) : jnt_raw_angle(s, c);
    } else if (j.type == 1) {
        th = ens_canon(jnt_prismatic(j, za, zb));
    }
    *theta = th;
    *rate = jnt_rate(j, za, zb);
}

// doubles of LDS one instance takes: the staged row, padded to an odd stride
HD int jnt_instance_doubles(int nb) { return (13 * nb) | 1; }
HD size_t jnt_lds_bytes(int nb) { return sizeof(double) * (size_t)JNT_WAVES * (64 / score_group_lanes(nb)) * jnt_instance_doubles(nb); }

hipError_t launch_joints(const JointsArgs& a, hipStream_t stream);

// ---- the statistics of any per-instance series x [n_inst][steps][nc] ACROSS its instances (cclqr_series_ensemble, cclqr_series_quantiles): the front ends of
// joints.hip feed ens_finish_kernel (ensemble.hip) and ens_select_kernel (quantiles.hip).  The ONE summation order of the moments: a tile = ENS_TILE consecutive
// instances, its partial ens_pass_partial over the whole tile, the tiles merged in tile order by ens_merge.
#define SER_THREADS 128       // coordinates of one workgroup of the tile-moments kernel: a column of ENS_TILE values each in LDS
#define SER_TT 64             // the transposing stage moves SER_TT coordinates x ENS_TILE instances at a time
HD size_t ser_moments_lds_bytes() { return sizeof(double) * (size_t)ENS_TILE * SER_THREADS; }
HD size_t ser_ws_doubles(long long n_inst, int steps, int nc) { return (size_t)steps * (size_t)ens_tiles(n_inst) * 2 * (size_t)nc; }
HD size_t ser_row_doubles(long long n_inst, int nc) { return (size_t)nc * (size_t)(ens_tiles(n_inst) * ENS_TILE); }
// part [steps][ntiles][2][nc]
hipError_t launch_series_moments(long long n_inst, int steps, int nc, const double* x, double* part, hipStream_t stream);
// rows row0 .. row0 + nrows - 1 of x into xt [nrows][nc][n_pad]
hipError_t launch_series_stage(long long n_inst, int steps, int nc, const double* x, int row0, int nrows, double* xt, hipStream_t stream);

}  // namespace cclqr
