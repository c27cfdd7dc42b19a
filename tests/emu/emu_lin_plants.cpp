// emu_lin_plants.cpp -- TEST INFRASTRUCTURE ONLY: serial twin of linearize.hip's kernel body for one knot ON A PLANT RECORD (cclqr_linearize_plants), for
// tests/test_plant_lqr_host.py.  The knot's record base is resolved once -- the mechanism's own records or the caller's link-order records [nb][16] = (m, J[9],
// p1[3], p2[3]), what plants.hip packs -- and handed to the three places that read a plant: lane_load_consts, ph_forces and ph_lin_rows_B.
// The Newton solve is the serial twin of emu_rollout.cpp (file-local there, hence the include).
#include "emu_rollout.cpp"

extern "C" int emu_lin_plants(const cclqr_mech_desc* md, const double* rec, const double* zd, int mu, const int* ctrl_joint, const double* Fd, double* A,
                              double* Bu, double* Bl, double* Gm) {
    cclqr_mech m;
    std::string err;
    int rc = build_mech_tables(md, &m, err);
    if (rc) return rc;
    const MechDev* M = &m.host;
    const int nb = M->nb, nz = 13 * nb, mx = 12 * nb, ml = 5 * nb, G = 64;
    const double dt = M->dt;
    std::vector<PlantRec> table(nb);
    for (int l = 0; rec && l < nb; l++) {
        const double* r = rec + 16 * l;
        table[l].m = r[0];
        for (int i = 0; i < 9; i++) table[l].J[i] = r[1 + i];
        for (int i = 0; i < 3; i++) { table[l].p1[i] = r[10 + i]; table[l].p2[i] = r[13 + i]; }
    }
    const PlantRec* plant = M->rec;
    if (rec) plant = table.data();
    const Lay Y = make_layout(nb, M->tree ? 2 * M->npairs : 0);
    const int JB = Y.total;
    std::vector<double> lds(Y.total + LJB * nb, 0.0);
    double* L = lds.data();
    std::vector<LaneRegs> R(G);
    int cj[CCLQR_MAXL];
    for (int i = 0; i < mu; i++) cj[i] = m.link_of_joint[ctrl_joint[i]];
    LinOut O;
    O.A = A; O.Bu = Bu; O.Bl = Bl; O.G = Gm; O.mx = mx; O.mu = mu; O.ml = ml;
    for (int e = 0; e < mx * mx; e++) A[e] = 0;
    for (int e = 0; e < mx * mu; e++) Bu[e] = 0;
    for (int e = 0; e < mx * ml; e++) Bl[e] = 0;
    for (int e = 0; e < ml * mx; e++) Gm[e] = 0;
    const int NLg = newton_level_groups(G, nb);
    for (int t = 0; t < G; t++) lane_load_consts(R[t], M, t / nb < NLg ? t % nb : 0, plant);
    for (int e = 0; e < nz; e++) { int l = e / 13, c = e - 13 * l; L[Y.Z + e] = zd[M->perm[l] * 13 + c]; }
    for (int i = 0; i < mu; i++) L[Y.UJ + cj[i]] += Fd ? Fd[i] : 0.0;
    for (int t = 0; t < G; t++) {
        const int lg = t / nb, tl = t - lg * nb;
        if (lg < NLg) { if (M->tree) ph_forces<true>(tl, nb, Y, L, R[t], M, lg == 0, plant); else ph_forces<false>(tl, nb, Y, L, R[t], M, lg == 0, plant); }
        ph_knot_jac(t, nb, Y, L, R[t]);
    }
    for (int t = 0; t < G; t++) { if (M->tree) ph_force_map_tree(t, G, nb, Y, L, M); else ph_force_map(t, G, nb, Y, L, M->end_mask); }
    bool done = false;
    emu_newton(G, nb, Y, L, R, M, dt, &done);
    if (!done) return -3;
    for (int t = 0; t < G; t++) ph_body_eval<true>(t, nb, Y, L, R[t], dt, Y.S, 0.0);
    for (int t = 0; t < G; t++) ph_lin_joint(t, nb, Y, JB, L, R[t]);
    for (int t = 0; t < G; t++) { ph_lin_rows_A(t, nb, Y, JB, L, R[t], M, O); ph_lin_rows_B(t, nb, Y, L, R[t], M, cj, O, plant); }
    return 0;
}
