// invariants.hip -- cclqr_rollout_invariants: kinetic and potential energy, their sum, the largest translational and rotational constraint residual and the largest
// quaternion norm error at every row of a recorded slab, and an eight-number summary per instance.  A streaming pass over the slab, as score.hip
// and joints.hip are: the slab is read once.
//
// invariants_kernel<G, LOOP>: a lane group of G = 8 / 16 / 32 / 64 lanes (score_group_lanes) owns one instance and walks its steps.  Per step the group
//   1. stages the 13 nb row it requested one step earlier in LDS (entries t, t + G, ...: coalesced) and requests the next step's row,
//   2. lane t forms the energy terms and | q . q - 1 | of link t and the five constraint rows of joint t (closed loops: the tables by body and by joint, up to 12
//      joints on 8 lanes) and writes the raw rows if they are wanted (cclqr_invariants.h),
//   3. five butterflies over the group -- two sums, three NaN-propagating maxima; idle lanes bring the identity 0 -- leave the six outputs in every lane: lanes
//      0 .. 5 write one each, and lane i folds them into entry i of the summary, which lanes 0 .. 7 write when the launch ends.
// m, J and the joint constants stay in the lane's registers from the first step to the last.  There is no workgroup barrier and no atomic: a row is private to ONE
// lane group of ONE wavefront; the cross-lane operations -- the wave barrier around the staged row and the butterflies -- sit in the step loop, whose bounds are
// launch arguments, outside every lane predicate.
#include "cclqr_internal.h"
#include "cclqr_invariants.h"

namespace cclqr {

// the staged row is private to ONE lane group of ONE wavefront (score_wave_sync: the wavefront's own instruction order orders its LDS operations)
__device__ __forceinline__ void inv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the value of lane t ^ O.  Offsets inside a 32-lane half go through ds_swizzle's bit-mask mode (lane (i & 0x1f) ^ O of the lane's own half): the pattern is an
// immediate, where a shuffle by index keeps two address registers per butterfly level alive across the whole step loop
template <int O>
__device__ __forceinline__ double inv_xor_lane(double v) {
    if constexpr (O < 32) {
        constexpr int pattern = 0x1f | (O << 10);
        const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), pattern), hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), pattern);
        return __hiloint2double(hi, lo);
    } else {
        return __shfl_xor(v, O, 64);
    }
}
// THE summation order of T and V (cclqr_invariants.h): the xor butterfly of score_group_sum, offsets 1, 2, 4, ...
template <int G, int O = 1>
__device__ __forceinline__ double inv_group_sum(double v) {
    if constexpr (O < G) return inv_group_sum<G, 2 * O>(v + inv_xor_lane<O>(v));
    else return v;
}
template <int G, int O = 1>
__device__ __forceinline__ double inv_group_max(double v) {
    if constexpr (O < G) return inv_group_max<G, 2 * O>(inv_max(v, inv_xor_lane<O>(v)));
    else return v;
}

template <int G, bool LOOP>
__global__ __launch_bounds__(64 * INV_WAVES, LOOP ? 2 : 3) void invariants_kernel(InvArgs a) {
    extern __shared__ double lds[];
    constexpr int IPW = 64 / G, SLOTS = LOOP ? INV_LOOP_SLOTS : 1;      // instances per wavefront, joints per lane
    const int nb = a.nb, ne = a.ne, nz = 13 * nb;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / G, t = lane % G;
    double* row = lds + (size_t)(wave * IPW + grp) * inv_instance_doubles(nb);
    const long long inst_raw = ((long long)blockIdx.x * INV_WAVES + wave) * IPW + grp;
    const bool valid = inst_raw < a.n_inst;
    const long long inst = valid ? inst_raw : a.n_inst - 1;      // (a lane group without an instance takes the last one again; nothing of it is written)
    const int steps = a.steps, k0 = a.k0;
    const double grav = a.M->g;
    const PlantRec* P = a.plants ? a.plants + (a.plant_off + inst) * nb : a.M->rec;

    const bool mine_b = t < nb;
    InvBody bc;
    if (LOOP) inv_load_body_loop(bc, a.M, mine_b ? t : 0);
    else inv_load_body_link(bc, a.M, P, mine_b ? t : 0);
    InvJoint jc[SLOTS];
    bool mine[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; sl++) {
        const int j = t + sl * G;
        mine[sl] = j < ne;
        const int jj = mine[sl] ? j : 0;
        if (LOOP) inv_load_joint_loop(jc[sl], a.M, jj);
        else inv_load_joint_link(jc[sl], a.M, P, jj);
    }
    const int si = t & (CCLQR_INVARIANTS_SUMMARY_LEN_ - 1);      // lane t keeps entry t of the summary (G >= 8 entries), and every lane entry 3
    double sv = inv_summary_start(si), gmax = inv_summary_start(3);
    if (a.summary && k0 > 1) {
        sv = a.summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + si];
        gmax = a.summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + 3];
    }
    const double* p = a.traj + inst * (long long)steps * nz;
    double nxt[CCLQR_SCORE_ROW_LOADS];
#pragma unroll
    for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; nxt[j] = (e < nz) ? p[e] : 0.0; }
    const long long out0 = inst * a.out_steps + (k0 - 1);      // the output row of this launch's first step
    for (int kk = 0; kk < steps; kk++) {
#pragma unroll
        for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = nxt[j]; }
        if (kk + 1 < steps) {      // the next step's row is on its way while this one is reduced
            const double* pn = p + (long long)(kk + 1) * nz;
#pragma unroll
            for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) nxt[j] = pn[e]; }
        }
        inv_wave_sync();
        double Tt = 0.0, Vt = 0.0, qt = 0.0, gp = 0.0, tw = 0.0;      // an idle lane brings the identity of the sum and of the max
        if (mine_b) inv_body_terms(bc, row, &Tt, &Vt, &qt);
#pragma unroll
        for (int sl = 0; sl < SLOTS; sl++) {
            if (mine[sl]) {
                double g[5];
                inv_joint_rows(jc[sl], row, g);
                inv_joint_max(jc[sl], g, &gp, &tw);
                if (valid && a.rows) {
                    double* ro = a.rows + ((out0 + kk) * ne + jc[sl].out) * 5;
#pragma unroll
                    for (int r = 0; r < 5; r++) ro[r] = g[r];
                }
            }
        }
        const double Tsum = inv_group_sum<G>(Tt), Vsum = inv_group_sum<G>(Vt);
        const double gap = inv_group_max<G>(gp), twist = inv_group_max<G>(tw), quat = inv_group_max<G>(qt);
        double o[CCLQR_INVARIANTS_LEN_];
        inv_outputs(Tsum, Vsum, grav, gap, twist, quat, o);
        if (valid && a.inv && t < CCLQR_INVARIANTS_LEN_) {
            const double ot = t == 0 ? o[0] : (t == 1 ? o[1] : (t == 2 ? o[2] : (t == 3 ? o[3] : (t == 4 ? o[4] : o[5]))));
            a.inv[(out0 + kk) * CCLQR_INVARIANTS_LEN_ + t] = ot;
        }
        sv = inv_summary_entry(si, sv, gmax, o, k0 + kk);
        gmax = inv_summary_entry(3, gmax, gmax, o, k0 + kk);
        inv_wave_sync();      // the next step overwrites the row
    }
    if (valid && a.summary && t < CCLQR_INVARIANTS_SUMMARY_LEN_) a.summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + t] = sv;
}

hipError_t launch_invariants(const InvArgs& a, hipStream_t stream) {
    const int G = score_group_lanes(a.nb);
    const long long per_block = (long long)INV_WAVES * (64 / G);
    const dim3 grid((unsigned)((a.n_inst + per_block - 1) / per_block)), block(64 * INV_WAVES);
    const size_t lds = inv_lds_bytes(a.nb);
    if (a.loop) return launch_lds(invariants_kernel<8, true>, grid, block, lds, stream, a);      // a closed loop: at most 8 bodies
    switch (G) {
        case 8: return launch_lds(invariants_kernel<8, false>, grid, block, lds, stream, a);
        case 16: return launch_lds(invariants_kernel<16, false>, grid, block, lds, stream, a);
        case 32: return launch_lds(invariants_kernel<32, false>, grid, block, lds, stream, a);
        default: return launch_lds(invariants_kernel<64, false>, grid, block, lds, stream, a);
    }
}

}  // namespace cclqr
