// emu_weights_host.cpp -- the host rule of the per-problem weights on the CPU, for tests/test_weights_host.py (test infrastructure only): ric_p_rows_batch and
// ric_per_problem_weights of cclqr_internal.h, which decide the weight strides and whether a batch may run on the Riccati kernels of a symmetric Pk.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_internal.h"

using namespace cclqr;

extern "C" int emu_ric_p_rows_batch(const double* Q, int mx, const double* R, int mu, long long n) { return ric_p_rows_batch(Q, mx, R, mu, n); }
// out = {q_stride, r_stride, p_rows} of a launch of nprob problems whose shared-pair rule gave p_rows0
extern "C" void emu_ric_per_problem_weights(int nprob, int mx, int mu, int p_rows0, const double* Q, const double* R, int n_weights, long long* out) {
    RicArgs a = {};
    a.nprob = nprob; a.mx = mx; a.mu = mu; a.p_rows = p_rows0;
    ric_per_problem_weights(a, Q, R, n_weights);
    out[0] = a.q_stride; out[1] = a.r_stride; out[2] = a.p_rows;
}
