// emu_value.cpp -- the row functions of csrc/cclqr_value.h run lane by lane on the host (test infrastructure only): what value_kernel (csrc/value.hip) does per
// instance, with the lane group's cross-lane sum taken serially over its lanes and LDS as plain arrays.  The setpoint table in link order, the states and P in the
// caller's body order, perm[l] = the caller's body of link l.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_value.h"
#include <vector>

using namespace cclqr;

extern "C" int emu_value(int nb, long long n_inst, long long inst0, const int* perm, const double* z, long long z_stride, const double* zd, int n_ctrl, int nsp,
                         const double* P, long long n_tables, double* out) {
    const int G = value_group_lanes(nb), nz = 13 * nb, mx = 12 * nb;
    if (nb < 1 || nb > G || value_instance_doubles(nb) < nz + mx || z_stride < nz) return -1;
    const long long zd_stride = n_ctrl > 1 ? (long long)nsp * nz : 0, p_stride = n_tables > 1 ? (long long)mx * mx : 0;
    std::vector<double> lds(value_instance_doubles(nb));
    double* row = lds.data();
    double* DZ = row + nz;
    for (long long inst = 0; inst < n_inst; inst++) {
        const long long gi = inst0 + inst;
        for (int t = 0; t < G; t++)
            for (int e = t; e < nz; e += G) row[e] = z[inst * z_stride + e];
        for (int t = 0; t < G && t < nb; t++) {
            double dz[12];
            value_body_error(row + 13 * perm[t], zd + gi * zd_stride + 13 * t, dz);
            for (int i = 0; i < 12; i++) DZ[12 * perm[t] + i] = dz[i];
        }
        double part[64];
        for (int t = 0; t < G; t++) part[t] = value_lane_partial(t, G, mx, P + gi * p_stride, DZ);
        for (int o = 1; o < G; o <<= 1) {      // the xor butterfly: every lane ends with the same bits
            double nxt[64];
            for (int t = 0; t < G; t++) nxt[t] = part[t] + part[t ^ o];
            for (int t = 0; t < G; t++) part[t] = nxt[t];
        }
        out[inst] = part[0];
    }
    return 0;
}
