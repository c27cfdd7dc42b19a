// plants.hip -- per-instance plants (cclqr_plants_create): the caller's arrays, in the caller's body / joint order, become the link-order records the
// rollout kernels' prologue reads (cclqr_dev.h PlantRec, cclqr_chain.h link_load_consts_rec), and are validated in the same pass.
//
// Stands for: the numbers that `Box(width, depth, length, mass)`, `Revolute(...; p1, p2)` and `Mechanism(origin, links, constraints; g, Δt)` fix for
// the ONE plant of the reference's examples (examples/lqr_cartpole.jl:21-32), here one set per instance of the batch.
#include "cclqr_internal.h"

namespace cclqr {

// One thread per (plant, link).  An input that is null is the mechanism's own value.  The first offending (plant, body) in the caller's numbering is
// kept as the smallest code ((plant * nb + body) * 4 + kind, PLANT_ERR_*) in *first_err, which the host reads back once.
__global__ __launch_bounds__(256) void plants_pack_kernel(const MechDev* M, int nb, long long n_plant, const double* mass, const double* inertia,
                                                          const double* p1, const double* p2, PlantRec* out, unsigned long long* first_err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_plant * nb) return;
    const long long p = i / nb;
    const int l = (int)(i - p * nb);
    const int b = M->perm[l], j = M->jperm[l];      // the link's body and joint in the caller's numbering
    PlantRec r;
    bool finite = true;
    int kind = -1;
    r.m = mass ? mass[p * nb + b] : M->m[l];
    finite = finite && isfinite(r.m);
    for (int k = 0; k < 9; k++) { r.J[k] = inertia ? inertia[(p * nb + b) * 9 + k] : M->J[l][k]; finite = finite && isfinite(r.J[k]); }
    for (int k = 0; k < 3; k++) {
        r.p1[k] = p1 ? p1[(p * nb + j) * 3 + k] : M->p1[l][k];
        r.p2[k] = p2 ? p2[(p * nb + j) * 3 + k] : M->p2[l][k];
        finite = finite && isfinite(r.p1[k]) && isfinite(r.p2[k]);
    }
    if (!finite) kind = PLANT_ERR_NONFINITE;
    else if (mass && !(r.m > 0.0)) kind = PLANT_ERR_MASS;
    else if (inertia) {
        // symmetric (to rounding of a product of rotations: 1e-12 of the largest entry) and positive definite (leading minors)
        double big = 0.0;
        for (int k = 0; k < 9; k++) big = fmax(big, fabs(r.J[k]));
        const bool sym = fabs(r.J[1] - r.J[3]) <= 1e-12 * big && fabs(r.J[2] - r.J[6]) <= 1e-12 * big && fabs(r.J[5] - r.J[7]) <= 1e-12 * big;
        const double d1 = r.J[0], d2 = r.J[0] * r.J[4] - r.J[1] * r.J[3];
        const double d3 = r.J[0] * (r.J[4] * r.J[8] - r.J[5] * r.J[7]) - r.J[1] * (r.J[3] * r.J[8] - r.J[5] * r.J[6]) + r.J[2] * (r.J[3] * r.J[7] - r.J[4] * r.J[6]);
        if (!(sym && d1 > 0.0 && d2 > 0.0 && d3 > 0.0)) kind = PLANT_ERR_INERTIA;
    }
    if (kind >= 0) atomicMin(first_err, (unsigned long long)((p * nb + b) * 4 + kind));
    out[i] = r;
}

hipError_t launch_plants_pack(const MechDev* M, int nb, long long n_plant, const double* mass, const double* inertia, const double* p1, const double* p2,
                              PlantRec* out, unsigned long long* first_err, hipStream_t stream) {
    const long long total = n_plant * nb;
    if (total <= 0) return hipSuccess;
    return launch_lds<false>(plants_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, M, nb, n_plant, mass, inertia, p1, p2, out, first_err);
}

}  // namespace cclqr
