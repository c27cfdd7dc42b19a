// emu_plants.cpp -- the per-instance plant loader of the rollout kernels' prologue (cclqr_chain.h link_load_consts_rec) on the CPU, for
// tests/test_plants_host.py (test infrastructure only): the link constants of every lane, once from a MechDev built from a plant's own tables
// and once from the nominal MechDev plus that plant's link-order record; and the link order (perm, jperm) the records are packed in.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_chain.h"
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_tables.h"
#include <string.h>
#include <vector>

using namespace cclqr;

// link order of a mechanism: perm[l] = caller's body of link l, jperm[l] = caller's joint of link l, parent[l] = parent link or -1
extern "C" int emu_plants_link_order(const cclqr_mech_desc* md, int* perm, int* jperm, int* parent) {
    cclqr_mech m;
    std::string err;
    const int rc = build_mech_tables(md, &m, err);
    if (rc) return rc;
    for (int l = 0; l < m.nb; l++) { perm[l] = m.host.perm[l]; jperm[l] = m.host.jperm[l]; parent[l] = m.host.parent[l]; }
    return 0;
}

// records [nb][16] (m, J[9], p1[3], p2[3]) of one plant in the link order of `nominal`, from caller-order arrays -- what plants.hip packs
static void pack_records(const MechDev& H, int nb, const double* mass, const double* inertia, const double* p1, const double* p2, std::vector<PlantRec>& R) {
    R.resize(nb);
    for (int l = 0; l < nb; l++) {
        const int b = H.perm[l], j = H.jperm[l];
        R[l].m = mass[b];
        for (int k = 0; k < 9; k++) R[l].J[k] = inertia[9 * b + k];
        for (int k = 0; k < 3; k++) { R[l].p1[k] = p1[3 * j + k]; R[l].p2[k] = p2[3 * j + k]; }
    }
}

// out_a / out_b [lanes][sizeof(LinkC) / 8 + 1] doubles: every LinkC field of lane t (flags as the last double), (a) link_load_consts on the MechDev of the
// plant's own tables `plant`, (b) link_load_consts_rec on the MechDev of `nominal` with the plant's records.  Returns the
// number of doubles per lane, or a negative error.
extern "C" int emu_plants_link_consts(const cclqr_mech_desc* nominal, const cclqr_mech_desc* plant, int lanes, double* out_a, double* out_b) {
    cclqr_mech mn, mp;
    std::string err;
    int rc = build_mech_tables(nominal, &mn, err);
    if (rc) return rc;
    rc = build_mech_tables(plant, &mp, err);
    if (rc) return rc;
    const int nb = mn.nb;
    std::vector<PlantRec> R;
    pack_records(mn.host, nb, plant->mass, plant->inertia, plant->p1, plant->p2, R);
    const int per = 1 + 9 + 3 + 3 + 6 + 4 + 3 + 1 + 2 + 1 + 1;
    for (int t = 0; t < lanes; t++) {
        LinkC ca, cb;
        link_load_consts(ca, &mp.host, t, nb, mp.host.dt);
        link_load_consts_rec(cb, &mn.host, R.data(), t, nb, mn.host.dt);
        const LinkC* cs[2] = {&ca, &cb};
        double* outs[2] = {out_a + (size_t)t * per, out_b + (size_t)t * per};
        for (int s = 0; s < 2; s++) {
            const LinkC& c = *cs[s];
            double* o = outs[s];
            int n = 0;
            o[n++] = c.m;
            for (int i = 0; i < 9; i++) o[n++] = c.J[i];
            for (int i = 0; i < 3; i++) o[n++] = c.p1[i];
            for (int i = 0; i < 3; i++) o[n++] = c.p2[i];
            for (int i = 0; i < 6; i++) o[n++] = c.V12[i];
            for (int i = 0; i < 4; i++) o[n++] = c.qoc[i];
            for (int i = 0; i < 3; i++) o[n++] = c.axis[i];
            o[n++] = c.dtm; o[n++] = c.sxb; o[n++] = c.sxa; o[n++] = c.fric; o[n++] = (double)c.flags;
        }
    }
    return per;
}
