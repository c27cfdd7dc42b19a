// emu_invariants.cpp -- the per-body and per-joint functions of csrc/cclqr_invariants.h run lane by lane on the host (test infrastructure only): what
// invariants_kernel (csrc/invariants.hip) does per instance, step and lane -- the row staged by the lane group's lanes (entries t, t + G, ...), lane t taking link
// t's energy terms and joint t's five rows (closed loops: joints t and t + G), the five butterflies in the defined order (offsets 1, 2, 4, ...: v_t op= v_{t ^ o}
// for all lanes at once), lanes 0 .. 5 writing the outputs and lane i keeping entry i of the summary.  The tables are the library's own (cclqr_tables.h
// build_mech_tables, compiled for the host), read through the loaders the kernel uses; `lanes` widens the lane group beyond score_group_lanes(nb) to show that
// the bits do not depend on it.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_invariants.h"
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_tables.h"
#include <string.h>
#include <vector>

using namespace cclqr;

template <class Op>
static double butterfly(std::vector<double> v, int G, Op op) {
    std::vector<double> w(G);
    for (int o = 1; o < G; o <<= 1) {
        for (int t = 0; t < G; t++) w[t] = op(v[t], v[t ^ o]);
        v = w;
    }
    for (int t = 1; t < G; t++)
        if (memcmp(&v[t], &v[0], sizeof(double)) != 0) return -1.0e300;      // every lane must hold the same bits (the tests would see this value)
    return v[0];
}

// plant_rec: [n_plant][nb][16] = (m, J[9], p1[3], p2[3]) in link order (PlantBatch.link_records), or NULL = the mechanism's; instance i reads plant plant_off + i
extern "C" int emu_invariants(const cclqr_mech_desc* md, int lanes, const double* plant_rec, long long plant_off, long long n_inst, int steps, int k0,
                              const double* traj, long long out_steps, double* inv, double* rows, double* summary) {
    cclqr_mech m;
    std::string err;
    const int rc = build_mech_tables(md, &m, err);
    if (rc) return rc;
    const MechDev* M = &m.host;
    const int nb = m.nb, ne = m.nj, loop = M->loop, nz = 13 * nb;
    const int G = lanes ? lanes : score_group_lanes(nb), SLOTS = loop ? INV_LOOP_SLOTS : 1;
    if (G < score_group_lanes(nb) || G > 64 || (G & (G - 1)) || ne > SLOTS * G || n_inst < 1 || steps < 1 || k0 < 1) return -1;
    if ((inv || rows) && out_steps < k0 + steps - 1) return -1;
    if (loop && plant_rec) return -1;
    std::vector<PlantRec> rec(nb);
    std::vector<double> row(inv_instance_doubles(nb));
    std::vector<InvBody> bc(G);
    std::vector<InvJoint> jc((size_t)SLOTS * G);
    for (long long inst = 0; inst < n_inst; inst++) {
        const PlantRec* P = M->rec;
        if (plant_rec) {
            for (int l = 0; l < nb; l++) memcpy(&rec[l], plant_rec + ((plant_off + inst) * nb + l) * 16, 16 * sizeof(double));
            P = rec.data();
        }
        for (int t = 0; t < G; t++) {
            const bool mine_b = t < nb;
            if (loop) inv_load_body_loop(bc[t], M, mine_b ? t : 0);
            else inv_load_body_link(bc[t], M, P, mine_b ? t : 0);
            for (int sl = 0; sl < SLOTS; sl++) {
                const int j = t + sl * G, jj = j < ne ? j : 0;
                if (loop) inv_load_joint_loop(jc[(size_t)sl * G + t], M, jj);
                else inv_load_joint_link(jc[(size_t)sl * G + t], M, P, jj);
            }
        }
        double sv[CCLQR_INVARIANTS_SUMMARY_LEN_], gmax[CCLQR_INVARIANTS_SUMMARY_LEN_];      // lanes 0 .. 7 of the group
        for (int t = 0; t < CCLQR_INVARIANTS_SUMMARY_LEN_; t++) {
            sv[t] = inv_summary_start(t); gmax[t] = inv_summary_start(3);
            if (summary && k0 > 1) { sv[t] = summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + t]; gmax[t] = summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + 3]; }
        }
        for (int kk = 0; kk < steps; kk++) {
            const double* p = traj + (inst * steps + kk) * nz;
            for (int t = 0; t < G; t++)
                for (int j = 0; j < CCLQR_SCORE_ROW_LOADS; j++) { const int e = t + j * G; if (e < nz) row[e] = p[e]; }
            std::vector<double> Tt(G, 0.0), Vt(G, 0.0), qt(G, 0.0), gp(G, 0.0), tw(G, 0.0);
            const long long orow = inst * out_steps + (k0 - 1 + kk);
            for (int t = 0; t < G; t++) {
                if (t < nb) inv_body_terms(bc[t], row.data(), &Tt[t], &Vt[t], &qt[t]);
                for (int sl = 0; sl < SLOTS; sl++) {
                    if (t + sl * G >= ne) continue;
                    const InvJoint& J = jc[(size_t)sl * G + t];
                    double g[5];
                    inv_joint_rows(J, row.data(), g);
                    inv_joint_max(J, g, &gp[t], &tw[t]);
                    if (rows)
                        for (int r = 0; r < 5; r++) rows[(orow * ne + J.out) * 5 + r] = g[r];
                }
            }
            auto add = [](double a, double b) { return a + b; };
            auto mx = [](double a, double b) { return inv_max(a, b); };
            const double Tsum = butterfly(Tt, G, add), Vsum = butterfly(Vt, G, add);
            const double gap = butterfly(gp, G, mx), twist = butterfly(tw, G, mx), quat = butterfly(qt, G, mx);
            double o[CCLQR_INVARIANTS_LEN_];
            inv_outputs(Tsum, Vsum, M->g, gap, twist, quat, o);
            if (inv)
                for (int t = 0; t < CCLQR_INVARIANTS_LEN_; t++) inv[orow * CCLQR_INVARIANTS_LEN_ + t] = o[t];
            for (int t = 0; t < CCLQR_INVARIANTS_SUMMARY_LEN_; t++) {
                sv[t] = inv_summary_entry(t, sv[t], gmax[t], o, k0 + kk);
                gmax[t] = inv_summary_entry(3, gmax[t], gmax[t], o, k0 + kk);
            }
        }
        if (summary)
            for (int t = 0; t < CCLQR_INVARIANTS_SUMMARY_LEN_; t++) summary[inst * CCLQR_INVARIANTS_SUMMARY_LEN_ + t] = sv[t];
    }
    return 0;
}

// the one-lane statement of the summary (inv_summary_init / inv_summary_fold) over a finished series [steps][6]: what the lanes above must agree with
extern "C" void emu_invariants_summary(int steps, int k0, const double* series, double* s) {
    if (k0 == 1) inv_summary_init(s);
    for (int r = 0; r < steps; r++) inv_summary_fold(s, series + (size_t)r * CCLQR_INVARIANTS_LEN_, k0 + r);
}

// the launch's own arithmetic: the dynamic LDS of invariants_kernel for an nb-body mechanism
extern "C" long long emu_invariants_lds(int nb) { return (long long)inv_lds_bytes(nb); }
