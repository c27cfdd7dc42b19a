// cclqr_value.h -- the cost the gains were designed to achieve from a start (cclqr_value_eval, value.hip): V = dz' P dz with P the cost-to-go of the
// Riccati recursion (lqr.jl:170, RicArgs.P_out) and dz the error of lqr.jl:92-103 of a state about setpoint row 0 of its controller table.  The per-row
// arithmetic lives here as __host__ __device__ functions so that tests/emu/emu_value.cpp runs it lane by lane on the CPU (test infrastructure only).  None
// of them contains a cross-lane operation: they are called under lane predicates.
#pragma once
#include "cclqr_dev.h"
#include "cclqr_chain.h"

namespace cclqr {

// launch arguments of value_kernel.  P and the states are in the caller's body order (the models and Q of the recursion are); the controller's zd is in link
// order, so lane l of a lane group forms link l's error from body M->perm[l] of the state and stores it at that body's place.
struct ValueArgs {
    const MechDev* M;
    const CtrlDev* C;
    const double* P;       // [n_tables][mx][mx] row-major, mx = 12 nb
    long long p_stride;    // doubles between the P of consecutive instances: 0 = one P shared by all, or mx * mx
    int nb;
    long long n_inst;
    long long inst0;       // global index of instance 0: the controller table (several) and the P table (several) of instance i are inst0 + i
    const double* z;       // instance i at z + i * z_stride: [nb][13] caller's body order
    long long z_stride;    // doubles, >= 13 nb
    double* out;           // [n_inst]
};

// lane group of an instance: the smallest of 16, 32, 64 lanes that gives every column of P a lane, 64 from three bodies on.  Every body has a lane
// (nb <= mx / 12 <= lanes, and nb <= CCLQR_MAXL = 64)
HD int value_group_lanes(int nb) { return 12 * nb <= 16 ? 16 : (12 * nb <= 32 ? 32 : 64); }
// doubles of LDS one instance takes: the staged state (13 nb) and the error in the caller's order (12 nb), padded to an odd stride
HD int value_instance_doubles(int nb) { return (13 * nb + 12 * nb) | 1; }
HD size_t value_lds_bytes(int nb, int waves) { return sizeof(double) * (size_t)waves * (64 / value_group_lanes(nb)) * value_instance_doubles(nb); }

// error of one body about its setpoint, order x, v, qtilde, w (lqr.jl:92-95): ck_control_error's arithmetic (cclqr_chain.h)
HD void value_body_error(const double* z, const double* zd, double* dz) { ck_control_error(z, zd, dz); }

// lane t's share of dz' P dz: the columns t, t + G, ... of every row, P [mx][mx] as written (symmetric or not).  Row by row, each row's dot product over the
// lane's columns first; four rows' loads are issued together.  The order depends on mx and G alone; the caller sums the shares over the group
HD double value_lane_partial(int t, int G, int mx, const double* P, const double* dz) {
    double acc = 0.0;
    int i = 0;
    for (; i + 4 <= mx; i += 4) {
        const double* Pi = P + (size_t)i * mx;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int j = t; j < mx; j += G) {
            const double d = dz[j];
            s0 += Pi[j] * d; s1 += Pi[mx + j] * d; s2 += Pi[2 * mx + j] * d; s3 += Pi[3 * mx + j] * d;
        }
        acc += dz[i] * s0; acc += dz[i + 1] * s1; acc += dz[i + 2] * s2; acc += dz[i + 3] * s3;
    }
    for (; i < mx; i++) {
        const double* Pi = P + (size_t)i * mx;
        double s = 0.0;
        for (int j = t; j < mx; j += G) s += Pi[j] * dz[j];
        acc += dz[i] * s;
    }
    return acc;
}

hipError_t launch_value(const ValueArgs& a, hipStream_t stream);

}  // namespace cclqr
