// emu_quantiles.cpp -- the per-lane functions of csrc/cclqr_quantiles.h run on the host (test infrastructure only): what ens_select_kernel (csrc/quantiles.hip) does
// for ONE coordinate of ONE row -- the key map, the padding to a power of two, the bitonic network step by step with the workgroup's threads as a loop over the
// pairs, the count of the finite keys and the quantile formula.  LDS is a plain array.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_quantiles.h"
#include <vector>

using namespace cclqr;

extern "C" int emu_quantiles(long long n, const double* x, int n_prob, const double* prob, double* quant, int* finite) {
    if (n < 1 || n > QNT_MAX_INST || n_prob < 1 || n_prob > QNT_MAX_PROBS) return -1;
    const int n2 = qnt_pow2(n), T = qnt_select_threads(n2), half = n2 >> 1;
    std::vector<unsigned long long> keys((size_t)n2);
    for (int e = 0; e < n2; e++) keys[e] = (e < n) ? qnt_key(x[e]) : QNT_KEY_LAST;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1)
            for (int tid = 0; tid < T; tid++)
                for (int p = tid; p < half; p += T) qnt_compare_exchange(keys.data(), qnt_pair_low(p, j), j, k);
    const int cnt = qnt_count_finite(keys.data(), n2);
    for (int j = 0; j < n_prob; j++) quant[j] = qnt_quantile(keys.data(), cnt, prob[j]);
    *finite = cnt;
    return 0;
}

// the key map alone: key[i] of x[i], and the value each key maps back to
extern "C" void emu_quantile_keys(long long n, const double* x, unsigned long long* key, double* back) {
    for (long long i = 0; i < n; i++) { key[i] = qnt_key(x[i]); back[i] = qnt_value(key[i]); }
}

// the launch's own sizes (launch_quantiles): the select kernel's dynamic LDS for n instances; the stage kernel's window and dynamic LDS for a mechanism
extern "C" long long emu_quantile_select_lds(long long n) { return (long long)sizeof(unsigned long long) * qnt_pow2(n); }
extern "C" long long emu_quantile_stage_lds(int nb, int mu, int* W) {
    *W = qnt_stage_window(nb, mu);
    return (long long)qnt_stage_lds_bytes(nb, mu, *W);
}
