// emu_ctrl_hot.cpp -- TEST INFRASTRUCTURE ONLY (never linked into libcclqr.so).
// The controller's hot record (CtrlDev::hot, csrc/cclqr_dev.h) and the chain plan word (csrc/cclqr_chain.h) on the CPU: the record is built
// from host tables exactly as cclqr_ctrl_create builds it, and
//   * its fields are handed out next to the CtrlDev fields they copy (tests/test_ctrl_hot_record.py compares them one by one);
//   * the row addresses a rollout step forms from it (ctrl_step_rows) are compared with the indexing the kernels used before the record
//     existed -- the expressions below are that code, on the CtrlDev fields -- for every step, instance, link, input and lane;
//   * the plan word of every lane is decoded against MechDev::nchains / chain_start / chain_len.
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_tables.h"
#include "../../constrainedcontrol.jl_amd/csrc/cclqr_chain.h"
#include <string.h>
#include <string>

using namespace cclqr;

namespace {
int build(const cclqr_mech_desc* md, const cclqr_ctrl_desc* cd, cclqr_mech& m, CtrlHostTables& T) {
    std::string err;
    int rc = build_mech_tables(md, &m, err);
    if (rc) return rc;
    rc = build_ctrl_tables(&m, cd, T, err);
    if (rc) return rc;
    T.H.K = T.K.empty() ? nullptr : T.K.data();
    T.H.zd = T.zd.data();
    T.H.Fd = T.Fd.empty() ? nullptr : T.Fd.data();
    if (!T.H.Fd) T.H.Fd_stride = 0;      // (as cclqr_ctrl_create does for a table that does not exist)
    if (!T.H.K) T.H.K_stride = 0;
    ctrl_hot_build(T.H);
    return 0;
}
long long bits(double v) { long long b; memcpy(&b, &v, 8); return b; }
}  // namespace

// dev[i] / hot[i]: the i-th field of CtrlDev and the record's copy of it; returns the number of fields (<= cap), or a negative error code
extern "C" int emu_ctrl_hot_fields(const cclqr_mech_desc* md, const cclqr_ctrl_desc* cd, long long* dev, long long* hot, int cap) {
    cclqr_mech m;
    CtrlHostTables T;
    int rc = build(md, cd, m, T);
    if (rc) return rc < 0 ? rc : -rc;
    const CtrlDev& C = T.H;
    const CtrlHot& H = C.hot;
    int n = 0;
    auto put = [&](long long a, long long b) { if (n < cap) { dev[n] = a; hot[n] = b; } n++; };
    put(C.mu, H.mu); put(C.nK, H.nK); put(C.N, H.N); put(C.nsp, H.nsp);
    put((long long)(uintptr_t)C.K, (long long)H.K); put((long long)(uintptr_t)C.zd, (long long)H.zd); put((long long)(uintptr_t)C.Fd, (long long)H.Fd);
    put(C.K_stride, H.K_stride); put(C.zd_stride, H.zd_stride); put(C.Fd_stride, H.Fd_stride);
    put(C.has_fric ? 1 : 0, (H.flags & CtrlHot::FRIC) ? 1 : 0);
    put(C.has_pid ? 1 : 0, (H.flags & CtrlHot::PID) ? 1 : 0);
    put(C.noise_scale != 0.0 ? 1 : 0, (H.flags & CtrlHot::NOISE) ? 1 : 0);
    put(bits(C.noise_scale), bits(H.noise_scale));
    put(C.noise_key0, H.noise_key0);
    for (int i = 0; i < C.mu; i++) put(C.cj[i], ctrl_hot_cj(H.cj4[i >> 2], i));
    return n;
}

// steps k0 .. k0 + steps - 1 of instances inst0 .. inst0 + n_inst - 1 on a lane group of G lanes: how many of the addresses (and gates, and joint
// numbers) that the record gives differ from the ones the CtrlDev indexing gives; *checked = how many were compared
extern "C" long long emu_ctrl_hot_rows(const cclqr_mech_desc* md, const cclqr_ctrl_desc* cd, long long inst0, long long n_inst, int k0, int steps, int G, long long* checked) {
    cclqr_mech m;
    CtrlHostTables T;
    int rc = build(md, cd, m, T);
    if (rc) return rc < 0 ? rc : -rc;
    const CtrlDev* C = &T.H;
    const CtrlHot* H = &T.H.hot;
    const int nb = m.nb, nz = 13 * nb, ne = 12 * nb, mu = C->mu;
    long long bad = 0, cnt = 0;
    for (int k = k0; k < k0 + steps; k++)
        for (long long inst = 0; inst < n_inst; inst++) {
            const long long ginst = inst0 + inst, gi = ginst;
            // ---- the indexing of the rollout kernels before the record (rollout_chain.hip, control phase)
            const bool gate = (C->N <= 0) || (k < C->N);
            const int ksp = (C->nsp > 1) ? ((k - 1 < C->nsp) ? k - 1 : C->nsp - 1) : 0;
            const int kidx = (C->N <= 0) ? 0 : ((k - 1 < C->nK) ? k - 1 : C->nK - 1);
            const double* Fp = C->Fd ? C->Fd + gi * C->Fd_stride + (size_t)ksp * mu : nullptr;
            // ---- the record
            const CtrlRows R = ctrl_step_rows(H, k, gi, nz, ne);
            const double* hFp = H->Fd ? (const double*)(uintptr_t)H->Fd + R.Fd : nullptr;
            bad += (gate != R.gate) + (Fp != hFp) + (mu != H->mu);
            cnt += 3;
            for (int l = 0; l < nb; l++) {
                const double* zd = C->zd + ginst * C->zd_stride + (size_t)ksp * nz + 13 * l;
                bad += zd != (const double*)(uintptr_t)H->zd + R.zd + 13 * l;
                cnt++;
            }
            for (int t = 0; t < G && C->K; t++) {
                const double* Kp = C->K + gi * C->K_stride + (size_t)kidx * mu * ne + t;
                const double* hKp = (const double*)(uintptr_t)H->K + R.K + t;
                for (int ij = 0; ij < mu; ij++) {
                    bad += (&Kp[(size_t)ij * ne] != &hKp[(size_t)ij * ne]) + (C->cj[ij] != ctrl_hot_cj(H->cj4[ij >> 2], ij));
                    cnt += 2;
                }
            }
        }
    if (checked) *checked = cnt;
    return bad;
}

// the plan word of each of the 64 lanes, built as rollout_chain.hip builds it; returns how many decoded fields differ from the mechanism's tables
extern "C" int emu_chain_plan(const cclqr_mech_desc* md, int* words, int* nchains) {
    cclqr_mech m;
    std::string err;
    int rc = build_mech_tables(md, &m, err);
    if (rc) return rc < 0 ? rc : -rc;
    const MechDev* M = &m.host;
    if (M->tree) return -1000;      // (branching trees have no chain plan)
    int bad = 0;
    for (int lane = 0; lane < 64; lane++) {
        const int nch = M->nchains;
        const int cs = M->chain_start[lane], cn = M->chain_len[lane];
        const int w = chain_plan_pack(nch, lane < nch ? cs : 0, lane < nch ? cn : 0) | ((lane & 63) << 24);      // (bits 24-29: the kernel keeps the lane's user body index there)
        words[lane] = w;
        bad += chain_plan_count(w) != M->nchains;
        if (lane < nch) bad += (chain_plan_start(w) != M->chain_start[lane]) + (chain_plan_len(w) != M->chain_len[lane]);
        bad += (w >> 24) != (lane & 63);
    }
    *nchains = M->nchains;
    return bad;
}
