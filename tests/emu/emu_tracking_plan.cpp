// emu_tracking_plan.cpp -- the host arithmetic of cclqr_ctrl_create_tracking_batch_plants on the CPU, for tests/test_plant_tracking_host.py (test
// infrastructure only): the chunk rule the call splits its problems by, and the knot -> (problem, setpoint row) map its linearisation launch reads by
// (cclqr_internal.h: tracking_problem_bytes, tracking_chunk_problems, tracking_chunk_count, lin_knot_rows -- the kernel calls the same lin_knot_rows).
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_internal.h"

using namespace cclqr;

extern "C" long long emu_tracking_default_budget(void) { return CCLQR_TRACKING_WORKSPACE_BYTES; }
extern "C" long long emu_tracking_max_chunk(void) { return CCLQR_TRACKING_MAX_CHUNK; }
extern "C" long long emu_tracking_problem_bytes(int mx, int mu, int ml, int N, long long ric_doubles) { return tracking_problem_bytes(mx, mu, ml, N, ric_doubles); }
extern "C" long long emu_tracking_chunk_problems(long long n_ctrl, long long per_problem_bytes, long long fixed_bytes, long long budget_bytes) {
    return tracking_chunk_problems(n_ctrl, per_problem_bytes, fixed_bytes, budget_bytes);
}
extern "C" long long emu_tracking_chunk_count(long long n_ctrl, long long per_chunk) { return tracking_chunk_count(n_ctrl, per_chunk); }
// knot q of a launch with (knots_per_plant, rows_per_plant): out[0] = problem, out[1] = setpoint / feed-forward row
extern "C" void emu_lin_knot_rows(int knot, int knots_per_plant, int rows_per_plant, long long* out) {
    int problem;
    long long row;
    lin_knot_rows(knot, knots_per_plant, rows_per_plant, &problem, &row);
    out[0] = problem; out[1] = row;
}
