// emu_chain_fixed_plan.cpp -- the solve plan of the chain kernel on the CPU, for tests/test_chain_fixed_plan_emu.py (test infrastructure only): what
// rollout_chain_fixed_kernel<NBP, ...> derives from the constants of PlanFixed<NBP> (cclqr_chain.h) next to what rollout_chain_kernel derives from the plan
// word of the same mechanism, lane by lane, and the rule that sends a mechanism to the fixed kernels (cclqr_tables.h rollout_shape_of).
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_chain.h"
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_tables.h"

using namespace cclqr;

#define PLAN_WORDS 35
// the solve's per-lane plan as the kernel text forms it (rollout_chain.hip, the 32-lane instantiations): reduction level, balanced two-front plan of
// the reduced chain, the lane's cursor.  out: TriPlanB [8], TriCur [11], CrLane<4> [2 + 3 + 9], cr
static void plan_words(int cs, int cn, int nbp, int t, int* out) {
    const Lay Y = make_chain_layout(nbp);
    const bool cr = cn >= CR_MIN_LINKS;
    CrLane<4> CK = {};
    if (cr) cr_setup<4>(CK, t, cs, cn, 1, Y, false);
    const TriPlanB B = cr ? tri_plan_balanced(cs, (cn + 1) / 2, 2) : tri_plan_balanced(cs, cn, 1, 2);
    const TriCur K = tri_cursor(t, B, Y);
    int i = 0;
    out[i++] = B.P.cs; out[i++] = B.P.cn; out[i++] = B.P.nA; out[i++] = B.P.nB; out[i++] = B.P.mid; out[i++] = B.P.steps; out[i++] = B.merge; out[i++] = B.st;
    out[i++] = K.oLL; out[i++] = K.oQL; out[i++] = K.oRhs; out[i++] = K.oTgt; out[i++] = K.oOut; out[i++] = K.dblk; out[i++] = K.dvec; out[i++] = K.n;
    out[i++] = K.imerge; out[i++] = K.oScr; out[i++] = K.isy ? 1 : 0;
    out[i++] = CK.fl; out[i++] = CK.w; out[i++] = CK.oLL; out[i++] = CK.oPL; out[i++] = CK.oNL;
    for (int s = 0; s < CrLane<4>::NS; s++) { out[i++] = CK.oRhs[s]; out[i++] = CK.oA[s]; out[i++] = CK.oB[s]; }
    out[i++] = cr ? 1 : 0;
    out[i++] = tri_scratch_S(B, Y);
}
template <int NBP>
static int fixed_words(int t, int* out) {
    typedef PlanFixed<NBP> PLAN;
    constexpr int cs = PLAN::cs, cn = PLAN::cn;
    plan_words(cs, cn, NBP, t, out);
    return PLAN::nchains;
}
extern "C" int emu_plan_words(void) { return PLAN_WORDS; }
// the fixed kernel's plan of lane t; returns its number of chains (-1: no such kernel)
extern "C" int emu_fixed_plan(int nbp, int t, int* out) { return nbp == 16 ? fixed_words<16>(t, out) : (nbp == 17 ? fixed_words<17>(t, out) : -1); }
// the run-time kernel's plan of lane t for a forest of nchains chains whose chain ci is (start, len): from the packed word, as the kernel reads it
extern "C" int emu_runtime_plan(int nbp, int nchains, int start, int len, int t, int* out) {
    const int word = chain_plan_pack(nchains, start, len);
    plan_words(chain_plan_start(word), chain_plan_len(word), nbp, t, out);
    return chain_plan_count(word);
}
// RolloutShape::fixed_plan of a mechanism as libcclqr.so would build it; out3 = {family, lanes per instance, layout links}; < 0: the description was refused
extern "C" int emu_shape_fixed_plan(const cclqr_mech_desc* md, int* out3) {
    static cclqr_mech m;
    std::string err;
    const int rc = build_mech_tables(md, &m, err);
    if (rc) return rc < 0 ? rc : -rc;
    const RolloutShape s = rollout_shape_of(m.host, m.nb, m.nj);
    out3[0] = (int)s.family; out3[1] = s.G; out3[2] = s.NBP;
    return s.fixed_plan;
}
// which kernel family launch_rollout_chain takes for that mechanism (cclqr_internal.h chain_launch_fixed_plan): 1 = the fixed-plan kernels; flags as in cclqr_rollout_opts
extern "C" int emu_launch_takes_fixed_plan(const cclqr_mech_desc* md, int flags) {
    static cclqr_mech m;
    std::string err;
    const int rc = build_mech_tables(md, &m, err);
    if (rc) return rc < 0 ? rc : -rc;
    return chain_launch_fixed_plan(rollout_shape_of(m.host, m.nb, m.nj), (flags & CCLQR_ROLLOUT_RUNTIME_PLAN) != 0) ? 1 : 0;
}
