// emu_schur_split.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libcclqr.so).
// The Schur rows of one evaluation built twice on the CPU, lane by lane, from the same random W = G_v D^-1 and G_k: by ck_schur_rows (every link's own
// lane builds its three blocks) and by ck_schur_rows_split (cclqr_chain.h: the link's lane builds two, the lane sixteen above it the child-side one; what
// the kernel moves to that lane by a swap of DPP rows is copied here from the link's lane).  Both go into LDS images that start as signalling NaNs but
// for G_k of the links that exist, so a word read before it is written poisons a block, and an offset outside the image is an out-of-bounds access.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_chain.h"
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

using namespace cclqr;

namespace {
struct Rng {      // xorshift64*: the same stream on every host
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1DULL; }
    double uni() { return (double)(next() >> 11) / 9007199254740992.0 * 2.0 - 1.0; }
    // zeros: four entries in ten are an exact zero of either sign (axis-aligned Jacobians: products and sums that come out as - 0)
    double val(bool zeros) { if (zeros && next() % 10 < 4) return (next() & 1) ? -0.0 : 0.0; return uni(); }
};
struct LaneW { double wXT[3][3], wPB[5][3], wPA[5][3], g[5], d[6], pd[6]; };
}  // namespace

// chain_len[nchains]: the forest, links numbered chain by chain and root to leaf; nbp: links the image is laid out for (16, or 17 for 17 links).
// ref / split: [total] words each (total = the layout's size, returned).  Returns 0, or -1 on a shape the 32-lane split does not serve.
extern "C" int emu_schur_split_case(const int* chain_len, int nchains, int nbp, uint64_t seed, int zeros, double* ref, double* split, int cap) {
    const int G = 32;
    int nb = 0;
    for (int i = 0; i < nchains; i++) nb += chain_len[i];
    if (nb < 1 || nb > nbp || (nbp != 16 && nbp != 17) || (nbp == 17 && nb != 17)) return -1;
    const Lay Y = make_chain_layout(nbp);
    if (cap < Y.total) return -1;
    const bool r0 = nbp == 17;
    Rng R{seed * 0x9E3779B97F4A7C15ULL + 1};
    std::vector<LinkC> c(G);
    std::vector<LaneW> W(G);
    std::vector<double> img(Y.total, std::numeric_limits<double>::signaling_NaN());
    // topology and scales
    std::vector<int> first(nb, 0), last(nb, 0);
    for (int i = 0, t = 0; i < nchains; i++)
        for (int k = 0; k < chain_len[i]; k++, t++) { first[t] = k == 0; last[t] = k == chain_len[i] - 1; }
    for (int t = 0; t < G; t++) {
        std::memset(&c[t], 0, sizeof(LinkC));
        const bool on = t < nb;
        c[t].flags = on ? (1 | (first[t] ? 0 : 2) | (last[t] ? 0 : 4) | ((R.next() & 1) ? 8 : 0) | 16 | 32 | LinkC::PRIM) : 16;
        c[t].sxb = 0.5 + 0.4 * R.uni();
        c[t].sxa = (on && !first[t]) ? c[t - 1].sxb : 0.0;
    }
    // W, g and the body residuals of every link; G_k of every link into the image
    for (int t = 0; t < nb; t++) {
        LaneW& w = W[t];
        double kXT[3][3], kPB[5][3], kPA[5][3];
        for (int r = 0; r < 5; r++)
            for (int k = 0; k < 3; k++) {
                if (r < 3) { w.wXT[r][k] = R.val(zeros); kXT[r][k] = R.val(zeros); }
                w.wPB[r][k] = R.val(zeros); kPB[r][k] = R.val(zeros);
                w.wPA[r][k] = c[t].has_a() ? R.val(zeros) : 0.0;      // (joint_eval_sparse: + 0 when the parent is the origin)
                kPA[r][k] = c[t].has_a() ? R.val(zeros) : 0.0;
            }
        for (int r = 0; r < 5; r++) w.g[r] = R.val(zeros);
        for (int k = 0; k < 6; k++) w.d[k] = R.val(zeros);
        gk_store(t, Y, img.data(), kXT, kPB, kPA);
    }
    for (int t = 0; t < nb; t++)
        for (int k = 0; k < 6; k++) W[t].pd[k] = c[t].has_a() ? W[t - 1].d[k] : 0.0;      // (the wave shift: a lane without a lane below it reads + 0)
    std::memcpy(ref, img.data(), sizeof(double) * Y.total);
    std::memcpy(split, img.data(), sizeof(double) * Y.total);
    for (int t = 0; t < nb; t++) ck_schur_rows(c[t], t, true, Y, ref, W[t].wXT, W[t].wPB, W[t].wPA, W[t].g, W[t].d, W[t].pd);
    // the split form, all 32 lanes: the helper lanes' flags and scale as the launch sets them, their wXT / wPB as the swap leaves them
    for (int t = 16; t < G; t++) {
        if (c[t].on()) continue;
        const int l = t - 16;
        schur_split_helper(c[t], l < nb && c[l].has_c(), c[l].sxb);
        std::memcpy(W[t].wXT, W[l].wXT, sizeof(W[l].wXT));
        std::memcpy(W[t].wPB, W[l].wPB, sizeof(W[l].wPB));
        const double poison = std::numeric_limits<double>::quiet_NaN();      // (what a helper lane holds besides: anything)
        for (int r = 0; r < 5; r++) { W[t].g[r] = poison; for (int k = 0; k < 3; k++) W[t].wPA[r][k] = poison; }
        for (int k = 0; k < 6; k++) { W[t].d[k] = poison; W[t].pd[k] = poison; }
    }
    for (int t = 0; t < G; t++) {
        if (r0) ck_schur_rows_split<true>(c[t], t, c[t].on(), true, Y, split, W[t].wXT, W[t].wPB, W[t].wPA, W[t].g, W[t].d, W[t].pd);
        else ck_schur_rows_split<false>(c[t], t, c[t].on(), true, Y, split, W[t].wXT, W[t].wPB, W[t].wPA, W[t].g, W[t].d, W[t].pd);
    }
    return Y.total;
}
// where the blocks lie (for the test's own checks): SJJ, SJP, SPJ, R, GKA, total
extern "C" void emu_schur_split_layout(int nbp, int* out) {
    const Lay Y = make_chain_layout(nbp);
    out[0] = Y.SJJ; out[1] = Y.SJP; out[2] = Y.SPJ; out[3] = Y.R; out[4] = Y.GKA; out[5] = Y.total;
}
