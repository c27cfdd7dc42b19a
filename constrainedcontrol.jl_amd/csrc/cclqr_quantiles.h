// cclqr_quantiles.h -- the order statistics of a batch ACROSS its instances at every row of a recorded slab (cclqr_rollout_quantiles, quantiles.hip):
// per step and per coordinate of x = (dz, du) -- the x of cclqr_ensemble.h, formed by the same functions -- the quantiles at the listed probabilities and the number
// of finite values.  The key map, the sorting network's partner and direction and the quantile formula live here as __host__ __device__ functions so that
// tests/emu/emu_quantiles.cpp runs them lane by lane on the CPU (test infrastructure only).  None of them contains a cross-lane operation.
//
// The definition.  s_0 <= ... <= s_{cnt-1} are the FINITE values of a coordinate over the instances, sorted as numbers with -0.0 before +0.0; for a probability p
//   h = p (cnt - 1),  lo = floor(h),  g = h - lo,  hi = min(lo + 1, cnt - 1),  q = s_lo + g (s_hi - s_lo)
// in fp64 as written, every operation rounded once (no fused multiply-add); g = 0 returns s_lo itself, bit for bit (so p = 0 is the minimum, p = 1 the maximum and
// a -0.0 stays a -0.0); cnt = 0 gives NaN.  The result is a function of the multiset of values alone.
#pragma once
#include "cclqr_ensemble.h"

namespace cclqr {

#define QNT_MAX_INST 16384    // = CCLQR_QUANTILE_MAX_INST: keys of one coordinate held in LDS (128 KB)
#define QNT_MAX_PROBS 16      // = CCLQR_QUANTILE_MAX_PROBS
#define QNT_MAX_THREADS 1024  // of the select kernel
#define QNT_LDS_BUDGET (144 * 1024)   // dynamic LDS the stage kernel may take: the pass's lane groups and the collected window
#define QNT_KEY_LAST 0xffffffffffffffffull    // the key of a value that is not finite, and of the padding: sorts last

struct QntArgs {
    const MechDev* M;
    const CtrlDev* C;
    int nb, mu;
    long long n_inst, n_pad;  // n_pad = n_inst rounded up to a tile: the instances of one coordinate lie n_pad apart in xt
    int steps, k0;            // the slab's rows (its stride) and the absolute step of its row 0
    long long inst0;
    const double* traj;       // [n_inst][steps][nb][13] caller's body order
    int row0, nrows;          // the rows row0 .. row0 + nrows - 1 of the slab are in this launch
    int W;                    // instances collected in LDS before they are written: a power of two, a multiple of ens_pass_instances(nb), at most ENS_TILE
    double* xt;               // [nrows][12 nb + mu (OUTPUT order)][n_pad]
    int n_prob;
    double prob[QNT_MAX_PROBS];
    double* quant;            // [steps][n_prob][12 nb + mu]
    int* finite;              // [steps][12 nb + mu] or null
};

HD long long qnt_pad(long long n_inst) { return ens_tiles(n_inst) * ENS_TILE; }
// doubles of workspace one slab row takes: every coordinate's instances, contiguous
HD size_t qnt_row_doubles(int nb, int mu, long long n_inst) { return (size_t)ens_coords(nb, mu) * (size_t)qnt_pad(n_inst); }
// keys of the sorting network: the next power of two
HD int qnt_pow2(long long n) { int p = 1; while (p < n) p <<= 1; return p; }
HD int qnt_select_threads(int n2) { const int t = n2 / 2; return t < 64 ? 64 : (t > QNT_MAX_THREADS ? QNT_MAX_THREADS : t); }
// the stage kernel's LDS: the pass's lane groups (as the moments kernel lays them out), then the window [12 nb + mu][W + 1] -- the odd stride puts the
// coordinate threads' 64-bit stores of one instance on distinct banks
HD size_t qnt_stage_lds_bytes(int nb, int mu, int W) { return ens_lds_bytes(nb, mu) + sizeof(double) * (size_t)ens_coords(nb, mu) * (size_t)(W + 1); }
// the widest window that fits: a whole tile where it can (each coordinate then receives a 512-byte run), never less than one pass
HD int qnt_stage_window(int nb, int mu) {
    int W = ENS_TILE;
    const int P = ens_pass_instances(nb);
    while (W > P && qnt_stage_lds_bytes(nb, mu, W) > QNT_LDS_BUDGET) W >>= 1;
    return W;
}

// ---- the key map: unsigned order of the keys = numeric order of the values, -0.0 before +0.0, everything that is not finite last
HD unsigned long long qnt_key(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned long long sign = 0x8000000000000000ull, expo = 0x7ff0000000000000ull;
    const unsigned long long k = (u & sign) ? ~u : (u | sign);
    return ((u & expo) == expo) ? QNT_KEY_LAST : k;
}
HD double qnt_value(unsigned long long k) {
    const unsigned long long sign = 0x8000000000000000ull;
    const unsigned long long u = (k & sign) ? (k ^ sign) : ~k;
    return __builtin_bit_cast(double, u);
}

// ---- the bitonic network on n2 = 2^m keys: for k = 2, 4, .. n2 and j = k / 2, k / 4, .. 1 the n2 / 2 pairs (i, i | j) are compared; pair p's lower element
HD int qnt_pair_low(int p, int j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }
// ... and whether the pair is put in ascending order in the merge of size k
HD bool qnt_pair_ascending(int i, int k) { return (i & k) == 0; }
HD void qnt_compare_exchange(unsigned long long* keys, int i, int j, int k) {
    const int l = i | j;
    const unsigned long long a = keys[i], b = keys[l];
    const bool swap = qnt_pair_ascending(i, k) ? (a > b) : (a < b);
    keys[i] = swap ? b : a;
    keys[l] = swap ? a : b;
}
// The keys lie linearly in LDS.  Consecutive lanes hold consecutive pairs, so with j >= 32 a lane group's lower elements are consecutive keys: no bank conflict;
// below that they all have bit j clear -- half the banks, each met twice (MI355X: a 64-bit load is served per 32 lanes on 32 banks of 8 bytes).  Issuing the upper
// element first in half of each lane group removes the conflict and was measured SLOWER by 23 %: the kernel is bound by its vector ALU work, and the
// selects on addresses and values double that of a compare-exchange.

// the number of finite values among n2 sorted keys: the first index that holds QNT_KEY_LAST (bisection; n2 a power of two)
HD int qnt_count_finite(const unsigned long long* keys, int n2) {
    int lo = 0, hi = n2;      // keys[lo - 1] is finite, keys[hi] is not (or hi = n2)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] == QNT_KEY_LAST) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the quantile at probability p of the cnt finite values at the head of the sorted keys, as the definition writes it
HD double qnt_quantile(const unsigned long long* keys, int cnt, double p) {
#pragma clang fp contract(off)
    if (cnt < 1) return NAN;
    const double h = p * (double)(cnt - 1);
    const double fl = floor(h);
    const double g = h - fl;
    const int lo = (int)fl, hi = (lo + 1 < cnt - 1) ? lo + 1 : cnt - 1;
    const double slo = qnt_value(keys[lo]);
    if (g == 0.0) return slo;
    const double shi = qnt_value(keys[hi]);
    const double d = shi - slo;
    const double gd = g * d;
    return slo + gd;
}

hipError_t launch_quantiles(const QntArgs& a, hipStream_t stream);
hipError_t launch_quantile_select(const QntArgs& a, hipStream_t stream);

}  // namespace cclqr
