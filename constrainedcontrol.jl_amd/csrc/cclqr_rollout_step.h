// cclqr_rollout_step.h -- what the chain kernel (rollout_chain.hip) and the branching-tree kernel (rollout_treereg.hip) share of a rollout step:
// the per-lane state of the owned link and the trial point a lane group hands to another in the line search.  Device only; included by
// those two kernels alone.
#pragma once
#include "cclqr_chain.h"

namespace cclqr {

// dynamic per-lane data of the owned link.  The velocity part of the state is s itself: the solution (v+, w+) of one step is
// the state's (v, w) at the next knot and the Newton start of the next step.
struct LinkS {
    double z[7], s[6];
    double ds[6], cd[6], d[6];
};

// ---- line search of the 32-lane instantiations (two instances per wavefront): TWO step lengths per pass in a group's own lanes, and when
// only ONE of the wavefront's two instances is still searching the other group's idle lanes evaluate two more for it.  The noise-floor
// searches of the exact stopping rule are heavy-tailed (9 % of them run to the 10th halving), and a wavefront pays the longer of its two:
// the accept sequence -- first level that does not grow, level LINE_MAXIT at the latest -- and every bit of the result are unchanged.
// TrialIn is the trial point handed over (the chain's 8- and 16-lane group assist hands it to any group).
struct TrialIn { double z[7], s[6], ds[6], cd[6]; };
__device__ __forceinline__ double other_half(double v) { return __shfl_xor(v, 32, 64); }

}  // namespace cclqr
