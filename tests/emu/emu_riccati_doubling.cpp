// emu_riccati_doubling.cpp -- the host arithmetic of the Riccati doubling on the CPU, for tests/test_riccati_doubling_host.py (test infrastructure only): the bit
// schedule of a fixed horizon and the workspace size (cclqr_internal.h: rdb_fixed_schedule, rdb_work_doubles -- launch_riccati_doubling walks the same schedule).
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_internal.h"

using namespace cclqr;

extern "C" int emu_rdb_max_ops(void) { return RDB_MAX_OPS; }
// ops[i]: 0 copy, 1 accumulate, 2 double; returns their number
extern "C" int emu_rdb_fixed_schedule(unsigned n, unsigned char* ops) { return rdb_fixed_schedule(n, ops); }
extern "C" long long emu_rdb_work_doubles(long long nprob, int mx) { return (long long)rdb_work_doubles(nprob, mx); }
