// emu_cr_level.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libcclqr.so).
// One reduction level (cclqr_chain.h cr_setup .. cr_store_b, 4 lanes per odd link) of a single chain run twice on the CPU, all 32 lanes of a group, on the
// same random block-tridiagonal system:
//   ref: the phases as rollout_chain_kernel calls them -- ONE column array per lane for both passes, z of pass B from the lane's registers (K.z);
//   neu: as the fixed-plan kernels call them (cr_level_a / cr_level_b) -- columns of its own for each pass, z of pass B read back from LDS
//        (cr_phase_b<W, true>).  Here K.z and the columns are poisoned between the passes, so a form that still read them would show.
// A host build runs the lanes one after another, so each phase runs for every lane before any lane stores -- the order of the wavefront's instruction
// stream.  Both images start as signalling NaNs but for the blocks of the links that exist: a word read before it is written poisons what is stored, and
// an offset outside the image is an out-of-bounds access.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_chain.h"
#include <array>
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
    // zeros: four entries in ten are an exact zero of either sign
    double val(bool zeros) { if (zeros && next() % 10 < 4) return (next() & 1) ? -0.0 : 0.0; return uni(); }
};
constexpr int W = 4, NS = CrLane<W>::NS, G = 32;
typedef std::array<std::array<double, 5>, NS> Cols;
double (*cols(Cols& c))[5] { return reinterpret_cast<double(*)[5]>(c.data()); }
const double (*ccols(const Cols& c))[5] { return reinterpret_cast<const double(*)[5]>(c.data()); }
}  // namespace

// cn: links of the chain (from link 0); nbp: links the image is laid out for (16 or 17); skip: the instance is `done` (no lane takes part).
// ref / neu: [total] words each.  Returns the layout's size, or -1 on a shape the level does not serve.
extern "C" int emu_cr_level_case(int cn, int nbp, uint64_t seed, int zeros, int skip, double* ref, double* neu, double* start, int cap) {
    if ((nbp != 16 && nbp != 17) || cn < CR_MIN_LINKS || cn > nbp) return -1;
    const Lay Y = make_chain_layout(nbp);
    if (cap < Y.total) return -1;
    const double snan = std::numeric_limits<double>::signaling_NaN();
    Rng R{seed * 0x9E3779B97F4A7C15ULL + 1};
    std::vector<double> img(Y.total, snan);
    for (int l = 0; l < cn; l++) {
        for (int e = 0; e < 25; e++) {
            img[Y.SJJ + 25 * l + e] = R.val(zeros) + ((e % 6 == 0) ? 4.0 : 0.0);      // (no pivoting in lu5_factor: a dominant diagonal)
            if (l > 0) img[Y.SJP + 25 * l + e] = R.val(zeros);                          // lower block of l: coupling to l - 1
            if (l + 1 < cn) img[Y.SPJ + 25 * (l + 1) + e] = R.val(zeros);               // upper block of l: coupling to l + 1
        }
        for (int r = 0; r < 5; r++) img[Y.R + 5 * l + r] = R.val(zeros);
    }
    std::memcpy(start, img.data(), sizeof(double) * Y.total);
    std::memcpy(ref, img.data(), sizeof(double) * Y.total);
    std::memcpy(neu, img.data(), sizeof(double) * Y.total);
    {   // today's form
        std::vector<CrLane<W>> K(G);
        std::vector<Cols> tc(G);
        for (int t = 0; t < G; t++) cr_setup<W>(K[t], t, 0, cn, 1, Y, skip != 0);
        for (int t = 0; t < G; t++) cr_phase_a<W>(K[t], ref, cols(tc[t]));
        for (int t = 0; t < G; t++) cr_store_a<W>(K[t], ref, ccols(tc[t]));
        for (int t = 0; t < G; t++) cr_phase_b<W>(K[t], ref, cols(tc[t]));
        for (int t = 0; t < G; t++) cr_store_b<W>(K[t], ref, ccols(tc[t]));
    }
    {   // the fixed-plan kernels' form
        std::vector<CrLane<W>> K(G);
        std::vector<Cols> ta(G), tb(G);
        for (int t = 0; t < G; t++) {
            cr_setup<W>(K[t], t, 0, cn, 1, Y, skip != 0);
            for (int s = 0; s < NS; s++) for (int r = 0; r < 5; r++) { K[t].z[s][r] = snan; ta[t][s][r] = snan; tb[t][s][r] = snan; }
        }
        for (int t = 0; t < G; t++) cr_phase_a<W>(K[t], neu, cols(ta[t]));
        for (int t = 0; t < G; t++) cr_store_a<W>(K[t], neu, ccols(ta[t]));
        for (int t = 0; t < G; t++) for (int s = 0; s < NS; s++) for (int r = 0; r < 5; r++) { K[t].z[s][r] = snan; ta[t][s][r] = snan; }
        for (int t = 0; t < G; t++) cr_phase_b<W, true>(K[t], neu, cols(tb[t]));
        for (int t = 0; t < G; t++) cr_store_b<W>(K[t], neu, ccols(tb[t]));
    }
    return Y.total;
}
// where the blocks lie (for the test's own checks): SJJ, SJP, SPJ, R, DL, total
extern "C" void emu_cr_level_layout(int nbp, int* out) {
    const Lay Y = make_chain_layout(nbp);
    out[0] = Y.SJJ; out[1] = Y.SJP; out[2] = Y.SPJ; out[3] = Y.R; out[4] = Y.DL; out[5] = Y.total;
}
