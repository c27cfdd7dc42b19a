// emu_chain_rows_verdict.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libcclqr.so).
// The chain kernels that split the Schur rows (and the tree kernel) form a full-step trial's ||f|| IN FRONT of the row block and build the rows only if a
// solve will read them (csrc/cclqr_chain.h chain_rows_verdict; rollout_chain.hip chain_eval, rollout_treereg.hip tree_eval).  A wrongly skipped build
// would not show on the GPU: the solve would read the rows of an earlier point and Newton would still converge.  So this twin runs emu_chain.cpp's
// Newton loop (its phase functions, its order; plain feedback law) in two modes on the same inputs:
//   mode 0  every evaluation with Jacobians builds its rows and stores DINV, as emu_chain.cpp does;
//   mode 1  the kernel's decisions, with ONE instance to a vote (the strictest case: nobody else's verdict builds the rows for it): the predictor
//           want = !(||f0|| < eps && nd < eps) decides DINV and jac_ok, chain_rows_verdict -- the same function the kernels call -- decides the rows;
//           whatever the kernel would NOT have written is overwritten with signalling NaNs (the row blocks and the right-hand side; DINV too when the
//           predictor says no), so that a later read of it poisons the result.
// The caller compares final states, multipliers and the Newton count of every step bit for bit, and reads how often each case occurred.
#include "emu_chain.cpp"

extern "C" int emu_chain_rows_verdict(const cclqr_mech_desc* md, const cclqr_ctrl_desc* cd, int64_t n_inst, int steps, const double* z0, int mode,
                                      double* zT, double* lam, int* its_out, long long* counts) {
    const double EPS = 1e-10;      // (NEWTON_EPS of cclqr_newton.h, a device-only header; emu_chain.cpp writes it out too)
    const double INF = std::numeric_limits<double>::infinity(), POISON = std::numeric_limits<double>::signaling_NaN();
    cclqr_mech m;
    std::string err;
    int rc = build_mech_tables(md, &m, err);
    if (rc) return rc;
    if (m.host.tree) return CCLQR_EUNSUPPORTED;
    CtrlHostTables Tb;
    rc = build_ctrl_tables(&m, cd, Tb, err);
    if (rc) return rc;
    Tb.H.K = Tb.K.empty() ? nullptr : Tb.K.data();
    Tb.H.zd = Tb.zd.data();
    Tb.H.Fd = Tb.Fd.empty() ? nullptr : Tb.Fd.data();
    const MechDev* M = &m.host;
    const CtrlDev* C = &Tb.H;
    if (C->has_fric || C->has_pid || C->noise_scale != 0.0) return CCLQR_EUNSUPPORTED;
    const int nb = M->nb, nz = 13 * nb;
    const double dt = M->dt;
    Inst I;
    I.G = chain_lanes_per_instance(nb);
    I.nb = nb; I.dt = dt;
    I.Y = make_chain_layout(chain_layout_links(nb));
    I.lds.resize(I.Y.total);
    I.L = I.lds.data();
    I.c.resize(I.G); I.S.resize(I.G); I.T.resize(I.G);
    const Lay& Y = I.Y;
    double* L = I.L;
    const int G = I.G;
    for (int t = 0; t < G; t++) link_load_consts(I.c[t], M, t, nb, dt);
    counts[0] = counts[1] = counts[2] = 0;      // trials without rows because the instance finished / because the full step was rejected; trials with rows
    // a full-step trial as the kernel leaves it: ||f||, and in mode 1 poison in place of what the kernel does not write.  *jac_ok = DINV AND the rows are there
    auto trial = [&](double normf0, double nd, bool* jac_ok) {
        const double normf1 = chain_eval<true>(I, 1.0, true);
        *jac_ok = true;
        if (mode == 0) return normf1;
        const bool want = !(normf0 < EPS && nd < EPS);
        const bool built = chain_rows_verdict(want, normf1, normf0, nd, EPS);
        *jac_ok = want;
        if (!want) for (int e = 0; e < 9 * nb; e++) L[Y.DINV + e] = POISON;
        if (!built) for (int e = Y.SJJ; e < Y.DL; e++) L[e] = POISON;      // SJJ, SJP, SPJ, R: consecutive in the image (make_chain_layout), DL behind them
        counts[built ? 2 : (normf1 > normf0 ? 1 : 0)]++;
        return normf1;
    };
    if (!(Y.SJJ < Y.SJP && Y.SJP < Y.SPJ && Y.SPJ < Y.R && Y.R + 5 * chain_layout_links(nb) == Y.DL)) return CCLQR_EINVAL;
    for (int64_t inst = 0; inst < n_inst; inst++) {
        for (int e = 0; e < Y.total; e++) L[e] = POISON;
        for (int t = 0; t < nb; t++) for (int i = 0; i < 5; i++) L[Y.LAM + 5 * t + i] = 0.0;
        for (int t = 0; t < G; t++) {
            const bool on = I.c[t].on();
            const int ut = on ? M->perm[t] : 0;
            for (int i = 0; i < 7; i++) I.S[t].z[i] = on ? z0[inst * nz + ut * 13 + i] : (i == 3 ? 1.0 : 0.0);
            for (int i = 0; i < 6; i++) { I.S[t].s[i] = on ? z0[inst * nz + ut * 13 + 7 + i] : 0.0; I.S[t].cd[i] = 0; I.S[t].d[i] = 0; I.S[t].ds[i] = 0; }
        }
        bool dead = false;
        for (int kk = 0; kk < steps; kk++) {
            const int k = 1 + kk;
            const bool gate = (C->N <= 0) || (k < C->N);
            const int ksp = (C->nsp > 1) ? ((k - 1 < C->nsp) ? k - 1 : C->nsp - 1) : 0;
            const int kidx = (C->N <= 0) ? 0 : ((k - 1 < C->nK) ? k - 1 : C->nK - 1);
            std::vector<double> uj(G, 0.0), zf(13 * G), za(13 * G);
            for (int t = 0; t < G; t++) {
                for (int i = 0; i < 7; i++) zf[13 * t + i] = I.S[t].z[i];
                for (int i = 0; i < 6; i++) zf[13 * t + 7 + i] = I.S[t].s[i];
            }
            for (int t = 0; t < G; t++)
                for (int i = 0; i < 13; i++) za[13 * t + i] = I.c[t].has_a() ? zf[13 * (t - 1) + i] : ORIGIN13[i];
            if (gate) {
                for (int t = 0; t < nb; t++) {
                    double dz[12];
                    ck_control_error(&zf[13 * t], C->zd + (size_t)ksp * nz + 13 * t, dz);
                    for (int i = 0; i < 12; i++) L[Y.DZ + 12 * t + i] = dz[i];
                }
                for (int i = 0; i < C->mu; i++) {
                    double s = 0.0;
                    if (C->K) {
                        const double* Krow = C->K + ((size_t)kidx * C->mu + i) * 12 * nb;
                        for (int e = 0; e < 12 * nb; e++) s += Krow[e] * L[Y.DZ + e];
                    }
                    uj[C->cj[i]] += (C->Fd ? C->Fd[(size_t)ksp * C->mu + i] : 0.0) - s;
                }
            }
            {
                std::vector<double> F(3 * G), tau(3 * G), W6(6 * G), par(6 * G), own(6 * G);
                for (int t = 0; t < G; t++) ck_joint_wrench(I.c[t], uj[t], &zf[13 * t + 3], &za[13 * t + 3], &F[3 * t], &tau[3 * t], &W6[6 * t], &W6[6 * t + 3]);
                for (int t = 0; t < G; t++) {
                    const LinkC& c = I.c[t];
                    if (c.has_c()) for (int i = 0; i < 3; i++) { F[3 * t + i] += W6[6 * (t + 1) + i]; tau[3 * t + i] += W6[6 * (t + 1) + 3 + i]; }
                    double cTR[6], gk[5], kXT[3][3], kPB[5][3], kPA[5][3], lm[5];
                    ck_step_invariants(c, &zf[13 * t], &F[3 * t], &tau[3 * t], dt, M->g, cTR, cTR + 3);
                    joint_eval_sparse<true>(c, &za[13 * t], &za[13 * t + 3], &zf[13 * t], &zf[13 * t + 3], nullptr, nullptr, gk, kXT, kPB, kPA);
                    if (!c.on()) continue;
                    for (int i = 0; i < 5; i++) lm[i] = L[Y.LAM + 5 * t + i];
                    gk_store(t, Y, L, kXT, kPB, kPA);
                    for (int i = 0; i < 6; i++) L[Y.D + 6 * t + i] = cTR[i];
                    jac_t_apply(c, kXT, kPB, kPA, lm, &own[6 * t], &par[6 * t]);
                }
                for (int t = 0; t < nb; t++)
                    for (int i = 0; i < 6; i++) { L[Y.C + 6 * t + i] = own[6 * t + i] + (I.c[t].has_c() ? par[6 * (t + 1) + i] : 0.0); I.S[t].cd[i] = 0.0; }
            }
            // ---- newton (emu_chain.cpp, with the trial above).  An evaluation at an accepted point passes + infinity twice to the rule, which then
            // returns its first argument: those rows are always built
            bool done = dead, failed = false;
            int its = 0;
            double normf0 = chain_eval<true>(I, 0.0, !done);
            if (!chain_rows_verdict(true, normf0, INF, INF, EPS)) return CCLQR_EINVAL;
            for (int iter = 1; iter <= 100 && !done; iter++) {
                for (int ci = 0; ci < M->nchains; ci++) {
                    const int cs = M->chain_start[ci], cn = M->chain_len[ci];
                    const bool cr = G == 32 && nb <= 17 && cn >= CR_MIN_LINKS;
                    if (cr) cr_level_emu<4>(G, cs, cn, Y, L);
                    const TriPlanB PB = cr ? tri_plan_balanced(cs, (cn + 1) / 2, 2) : tri_plan_balanced(cs, cn, 1, G >= 16 ? 2 : 1);
                    const TriPlan& P = PB.P;
                    std::vector<TriCur> K(G);
                    for (int t = 0; t < G; t++) K[t] = tri_cursor(t, PB, Y);
                    for (int i = 0; i < P.steps; i++) {
                        double tg[64][5], zy[64][5];
                        int otg[64], oout[64];
                        bool act[64];
                        for (int t = 0; t < G; t++) act[t] = tri_step(K[t], i, L, tg[t], zy[t], &otg[t], &oout[t]);
                        for (int t = 0; t < G; t++) if (act[t]) tri_step_store(L, otg[t], oout[t], tg[t], zy[t]);
                    }
                    for (int t = 0; t < G; t++) ck_tri_mid(t, PB, Y, L);
                    for (int j = 0; j < P.steps; j++) for (int t = 0; t < G; t++) ck_tri_back(t, j, PB, Y, L);
                    if (cr) for (int t = 0; t < G; t++) cr_back<4>(t, cs, cn, 1, Y, L, false);
                }
                double pdn = 0.0;
                {
                    std::vector<double> own(6 * G), par(6 * G);
                    for (int t = 0; t < nb; t++) gk_t_apply(I.c[t], t, Y, L, L + Y.DL + 5 * t, &own[6 * t], &par[6 * t]);
                    for (int t = 0; t < nb; t++) {
                        double DINV[9];
                        for (int i = 0; i < 9; i++) DINV[i] = L[Y.DINV + 9 * t + i];
                        for (int i = 0; i < 6; i++) I.S[t].cd[i] = own[6 * t + i] + (I.c[t].has_c() ? par[6 * (t + 1) + i] : 0.0);
                        ck_body_solve(I.c[t], I.S[t].d, I.S[t].cd, DINV, I.S[t].ds);
                        for (int i = 0; i < 6; i++) pdn += I.S[t].ds[i] * I.S[t].ds[i];
                        for (int i = 0; i < 5; i++) pdn += L[Y.DL + 5 * t + i] * L[Y.DL + 5 * t + i];
                    }
                }
                const double nd = sqrt(pdn);
                bool jac_ok;
                double alpha = 1.0, normf1 = trial(normf0, nd, &jac_ok);
                if (normf1 > normf0)
                    for (int lv = 1; lv <= 10; lv++) {
                        alpha = ldexp(1.0, -lv);
                        normf1 = chain_eval<false>(I, alpha, true);
                        jac_ok = false;
                        if (!(normf1 > normf0)) break;
                    }
                for (int t = 0; t < nb; t++) {
                    for (int i = 0; i < 6; i++) { I.S[t].s[i] -= alpha * I.S[t].ds[i]; L[Y.C + 6 * t + i] -= alpha * I.S[t].cd[i]; I.S[t].cd[i] = 0.0; I.S[t].ds[i] = 0.0; }
                    for (int i = 0; i < 5; i++) L[Y.LAM + 5 * t + i] -= alpha * L[Y.DL + 5 * t + i];
                }
                its = iter;
                if (normf1 < EPS && alpha * nd < EPS) done = true;
                if (!(normf1 < 1e300)) { done = true; failed = true; }
                normf0 = normf1;
                if (!done && !jac_ok) chain_eval<true>(I, 0.0, true);
            }
            its_out[inst * steps + kk] = (done && !failed) ? its : -its;
            if (!dead) {
                if (!(done && !failed) && its < 100) {
                    dead = true;
                    for (int t = 0; t < nb; t++) for (int i = 0; i < 6; i++) I.S[t].s[i] = 0.0;
                } else
                    for (int t = 0; t < nb; t++) {
                        double xq[7];
                        ck_next_pose(I.S[t].z, I.S[t].s, dt, xq);
                        for (int i = 0; i < 7; i++) I.S[t].z[i] = xq[i];
                    }
            }
        }
        for (int t = 0; t < nb; t++) {
            double* dst = zT + inst * nz + 13 * M->perm[t];
            for (int i = 0; i < 7; i++) dst[i] = I.S[t].z[i];
            for (int i = 0; i < 6; i++) dst[7 + i] = I.S[t].s[i];
            for (int i = 0; i < 5; i++) lam[inst * 5 * nb + 5 * t + i] = L[Y.LAM + 5 * t + i];
        }
    }
    return 0;
}
