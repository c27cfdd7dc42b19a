// emu_capi_host.cpp -- the pure host arithmetic of capi.hip on the CPU, for tests/test_capi_host.py (test infrastructure only): the layout of a controller's
// gain tables (cclqr_internal.h: gain_row_overrun, gain_table_layout, CCLQR_K_PAD) and the rule that picks the Riccati kernels of a symmetric Pk (ric_p_rows).
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_internal.h"

using namespace cclqr;

static RolloutShape shape_of(int loop, int G, int NBP) {
    RolloutShape s = {};
    s.family = loop ? RolloutFamily::Loop : RolloutFamily::Chain;      // (chains and trees share the rule: only the loop family is told apart)
    s.G = G; s.NBP = NBP;
    return s;
}
extern "C" long long emu_k_pad(void) { return CCLQR_K_PAD; }
extern "C" long long emu_gain_row_overrun(int loop, int G, int NBP, int nb) { return (long long)gain_row_overrun(shape_of(loop, G, NBP), nb); }
// out = {pad, stride, K_stride, alloc_doubles}
extern "C" void emu_gain_table_layout(int loop, int G, int NBP, int nb, long long n_tables, long long rows_per_table, long long* out) {
    const GainTableLayout L = gain_table_layout(shape_of(loop, G, NBP), nb, n_tables, rows_per_table);
    out[0] = (long long)L.pad; out[1] = L.stride; out[2] = L.K_stride; out[3] = (long long)L.alloc_doubles;
}
extern "C" int emu_ric_p_rows(const double* Q, int mx, const double* R, int mu) { return ric_p_rows(Q, mx, R, mu); }
