// capi.hip -- the extern "C" boundary of libcclqr.so (include/cclqr.h).  Host-side work here is limited to
// validation, index permutations (user body order <-> breadth-first link order) and device memory plumbing;
// every piece of hot-path arithmetic runs in the HIP kernels.
#include "../../include/cclqr.h"
#include "cclqr_internal.h"
#include "cclqr_tables.h"
#include "cclqr_treereg_tables.h"
#include "cclqr_newton.h"
static_assert(CCLQR_NEWTON_MAXIT == NEWTON_MAXIT, "include/cclqr.h and cclqr_newton.h disagree on the Newton iteration cap");
#include "cclqr_wscache.h"
#include "cclqr_score.h"
static_assert(CCLQR_SCORE_LEN == CCLQR_SCORE_LEN_, "include/cclqr.h and cclqr_score.h disagree on the length of a score");
#include "cclqr_value.h"
#include "cclqr_ensemble.h"
#include "cclqr_quantiles.h"
#include "cclqr_joints.h"
static_assert(CCLQR_JOINTS_RAW == CCLQR_JOINTS_RAW_ && CCLQR_JOINTS_CONTINUOUS == CCLQR_JOINTS_CONTINUOUS_ && CCLQR_SERIES_MAX_COORDS == CCLQR_SERIES_MAX_COORDS_,
              "include/cclqr.h and cclqr_joints.h disagree on the joint modes or the coordinates of a series");
#include "cclqr_invariants.h"
static_assert(CCLQR_INVARIANTS_LEN == CCLQR_INVARIANTS_LEN_ && CCLQR_INVARIANTS_SUMMARY_LEN == CCLQR_INVARIANTS_SUMMARY_LEN_,
              "include/cclqr.h and cclqr_invariants.h disagree on the length of a row of invariants or of a summary");
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

using namespace cclqr;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
// every step of an entry point is a checked call that returns on failure -- HIPTRY with the entry point's own prefix, HIPCHK with the call's text, TRY for a
// step that has set the error itself; what the entry point holds by then is released by its scope guards (Owned, DevBlocks, WsScope)
#define HIPTRY(prefix, x)                                                                                           \
    do {                                                                                                            \
        hipError_t e_ = (x);                                                                                        \
        if (e_ != hipSuccess) return fail(CCLQR_EHIP, std::string(prefix) + ": " + hipGetErrorString(e_));         \
    } while (0)
#define HIPCHK(x) HIPTRY(#x, x)
#define TRY(x)                            \
    do {                                  \
        const int rc_ = (x);              \
        if (rc_ != CCLQR_OK) return rc_;  \
    } while (0)
namespace {
// a handle under construction: destroyed by its own cclqr_*_destroy unless the entry point hands it out
template <class T, int (*Destroy)(T*)>
struct Owned {
    T* p;
    explicit Owned(T* q) : p(q) {}
    Owned(const Owned&) = delete;
    ~Owned() { (void)Destroy(p); }
    T* release() { T* q = p; p = nullptr; return q; }
};
// raw hipMalloc blocks of one call.  A return that has not released them first waits for the call's stream: nothing of the call may still run on what is freed
struct DevBlocks {
    hipStream_t stream;
    void *a = nullptr, *b = nullptr;
    bool released = false;
    explicit DevBlocks(hipStream_t s) : stream(s) {}
    DevBlocks(const DevBlocks&) = delete;
    void release() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); a = b = nullptr; released = true; }
    ~DevBlocks() { if (!released) { (void)hipStreamSynchronize(stream); release(); } }
};
}  // namespace

extern "C" const char* cclqr_last_error(void) { return g_err.c_str(); }

#include <mutex>
namespace cclqr {
hipError_t set_max_dynamic_lds_once(const void* fn, size_t lds) {
    struct Entry { int dev; const void* fn; size_t lds; };
    static std::mutex mu;
    static std::vector<Entry> seen;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (auto& s : seen)
        if (s.dev == dev && s.fn == fn) {
            if (s.lds >= lds) return hipSuccess;
            e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) s.lds = lds;
            return e;
        }
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) seen.push_back({dev, fn, lds});
    return e;
}
}  // namespace cclqr

// Device workspaces of the host-pointer entry points (linearize / riccati / rollout staging) are kept per thread and reused by the
// next call instead of a hipMalloc + hipFree (both synchronise the device) per call; cclqr_release_workspaces() returns them.
static thread_local WsCache g_ws;
static hipError_t ws_get(void** p, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const int rc = ws_get_on(g_ws, dev, p, bytes, [](void** q, size_t n) { return (int)hipMalloc(q, n); }, [](void* q) { return (int)hipFree(q); },
                             [](int d) { (void)hipSetDevice(d); });
    return rc < 0 ? hipErrorInvalidDevice : (hipError_t)rc;
}
namespace { struct WsScope { WsMark mark{g_ws}; }; }     // the blocks the entry point took are free again when it returns
// blocks of a thread that exits without calling this stay allocated until the process ends (thread_local destructors must not call
// into a HIP runtime that may already be shutting down)
extern "C" int cclqr_release_workspaces(void) {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    if (have && g_ws.device >= 0 && g_ws.device != cur) (void)hipSetDevice(g_ws.device);
    for (auto& b : g_ws.blocks) if (b.first) (void)hipFree(b.first);
    if (have && g_ws.device >= 0 && g_ws.device != cur) (void)hipSetDevice(cur);
    g_ws.blocks.clear(); g_ws.used = 0; g_ws.device = -1;
    return CCLQR_OK;
}
// every entry point that takes a handle runs on the device the handle's tables live on
static int check_device(const cclqr_mech* m) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(CCLQR_EHIP, "hipGetDevice failed");
    if (m && m->device != dev) return fail(CCLQR_EINVAL, "the mechanism was created on device " + std::to_string(m->device) + ", the calling thread is on device " + std::to_string(dev));
    return CCLQR_OK;
}
extern "C" int cclqr_version(void) { return CCLQR_ABI_VERSION; }
// sizeof / offsetof of the structs of include/cclqr.h as compiled here (the order is the header's comment): a foreign-language mirror checks itself against it
extern "C" int cclqr_abi_layout(int32_t* out, int32_t n) {
#define OFF(T, f) (int32_t) offsetof(T, f)
    const int32_t v[CCLQR_ABI_LAYOUT_LEN] = {
        (int32_t)sizeof(cclqr_mech_desc), OFF(cclqr_mech_desc, nb), OFF(cclqr_mech_desc, ne), OFF(cclqr_mech_desc, dt), OFF(cclqr_mech_desc, g), OFF(cclqr_mech_desc, mass),
        OFF(cclqr_mech_desc, inertia), OFF(cclqr_mech_desc, parent), OFF(cclqr_mech_desc, child), OFF(cclqr_mech_desc, type), OFF(cclqr_mech_desc, p1), OFF(cclqr_mech_desc, p2),
        OFF(cclqr_mech_desc, axis), OFF(cclqr_mech_desc, qoff),
        (int32_t)sizeof(cclqr_ctrl_desc), OFF(cclqr_ctrl_desc, mu), OFF(cclqr_ctrl_desc, ctrl_joint), OFF(cclqr_ctrl_desc, nK), OFF(cclqr_ctrl_desc, N), OFF(cclqr_ctrl_desc, K),
        OFF(cclqr_ctrl_desc, nsp), OFF(cclqr_ctrl_desc, zd), OFF(cclqr_ctrl_desc, Fd), OFF(cclqr_ctrl_desc, fric), OFF(cclqr_ctrl_desc, noise_scale), OFF(cclqr_ctrl_desc, npid),
        OFF(cclqr_ctrl_desc, pid_joint), OFF(cclqr_ctrl_desc, pid_P), OFF(cclqr_ctrl_desc, pid_I), OFF(cclqr_ctrl_desc, pid_D), OFF(cclqr_ctrl_desc, pid_goal),
        OFF(cclqr_ctrl_desc, noise_philox), OFF(cclqr_ctrl_desc, noise_seed), OFF(cclqr_ctrl_desc, n_ctrl),
        (int32_t)sizeof(cclqr_riccati_opts), OFF(cclqr_riccati_opts, path), OFF(cclqr_riccati_opts, bf16_terms), OFF(cclqr_riccati_opts, keep_last), OFF(cclqr_riccati_opts, reserved),
        (int32_t)sizeof(cclqr_rollout_opts), OFF(cclqr_rollout_opts, first_instance), OFF(cclqr_rollout_opts, pid_state_dev), OFF(cclqr_rollout_opts, pid_state_len),
        OFF(cclqr_rollout_opts, noise_ws_dev), OFF(cclqr_rollout_opts, noise_ws_len), OFF(cclqr_rollout_opts, newton_mode), OFF(cclqr_rollout_opts, flags),
        OFF(cclqr_rollout_opts, newton_eps_alone)};
#undef OFF
    if (n < 0 || (n > 0 && !out)) return fail(CCLQR_EINVAL, "bad argument");
    for (int i = 0; i < n && i < CCLQR_ABI_LAYOUT_LEN; i++) out[i] = v[i];
    return CCLQR_ABI_LAYOUT_LEN;
}
extern "C" int cclqr_device_count(int32_t* n) {
    if (!n) return fail(CCLQR_EINVAL, "null argument");
    const hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; return fail(CCLQR_EHIP, hipGetErrorString(e)); }
    return CCLQR_OK;
}
extern "C" int cclqr_set_device(int32_t dev) { HIPCHK(hipSetDevice(dev)); return CCLQR_OK; }

extern "C" int cclqr_mech_create(const cclqr_mech_desc* d, cclqr_mech** out) {
    if (!d || !out) return fail(CCLQR_EINVAL, "null argument");
    Owned<cclqr_mech, cclqr_mech_destroy> own(new cclqr_mech());
    cclqr_mech* m = own.p;
    std::string err;
    const int rc = build_mech_tables(d, m, err);
    if (rc != CCLQR_OK) return fail(rc, err);
    // branching trees: the tables of the register-resident tree kernel (sibling lists, elimination schedule) ride behind the MechDev in the
    // same allocation (cclqr_treereg.h treereg_of)
    std::vector<char> image(m->host.tree ? treereg_offset() + sizeof(TreeRegDev) : sizeof(MechDev), 0);
    memcpy(image.data(), &m->host, sizeof(MechDev));
    if (m->host.tree && !m->host.loop) {
        TreeRegDev* R = new (image.data() + treereg_offset()) TreeRegDev;
        if (!build_treereg_tables(m->host, *R, err)) return fail(CCLQR_EUNSUPPORTED, err);
    }
    HIPTRY("mechanism upload", hipGetDevice(&m->device));
    HIPTRY("mechanism upload", hipMalloc((void**)&m->dev, image.size()));
    HIPTRY("mechanism upload", hipMemcpy(m->dev, image.data(), image.size(), hipMemcpyHostToDevice));
    // the kernels this mechanism runs on, and the SIMDs of ITS device that a small batch is spread over (spread_instances_per_wavefront): both
    // fixed here, so that no launch queries the runtime (never inside a caller's hipGraph capture)
    m->shape = rollout_shape_of(m->host, m->nb, m->nj);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, m->device) != hipSuccess || cus <= 0) cus = 256;
    m->simds = 4 * cus;
    *out = own.release();
    return CCLQR_OK;
}

extern "C" int cclqr_mech_destroy(cclqr_mech* m) {
    if (!m) return CCLQR_OK;
    if (m->dev) (void)hipFree(m->dev);
    delete m;
    return CCLQR_OK;
}

// one knot of the mechanism's linearisation kernel (launch_linearize) within a CU's 160 KB of LDS
static bool linearize_fits_lds(const cclqr_mech* m) { return m->shape.lin_lds <= 160 * 1024; }

// the controlled joints of a call as the kernels address them: links for chains and trees, the caller's joint numbers for closed loops (their tables keep them)
static int map_ctrl_joints(const cclqr_mech* m, int mu, const int32_t* ctrl_joint, int* cj) {
    const bool loop = m->host.loop != 0;
    const int nj = loop ? m->nj : m->nb;
    for (int i = 0; i < mu; i++) {
        if (ctrl_joint[i] < 0 || ctrl_joint[i] >= nj) return fail(CCLQR_EINVAL, "controlled joint out of range");
        cj[i] = loop ? ctrl_joint[i] : m->link_of_joint[ctrl_joint[i]];
    }
    return CCLQR_OK;
}

// a controller handle under construction (ctrl_new), and its last step (ctrl_publish): the tables' addresses into the host record, the record the rollout
// steps read built from it (after the addresses and strides are final), the whole uploaded
typedef Owned<cclqr_ctrl, cclqr_ctrl_destroy> CtrlOwner;
static cclqr_ctrl* ctrl_new(const cclqr_mech* m) {
    cclqr_ctrl* c = new cclqr_ctrl();
    memset(c, 0, sizeof(*c));
    c->nb = m->nb;
    c->device = m->device;
    return c;
}
static hipError_t ctrl_publish(cclqr_ctrl* c) {
    c->host.K = c->K_dev; c->host.zd = c->zd_dev; c->host.Fd = c->Fd_dev;
    if (!c->Fd_dev) c->host.Fd_stride = 0;
    if (!c->K_dev) c->host.K_stride = 0;
    ctrl_hot_build(c->host);
    const hipError_t e = hipMalloc((void**)&c->dev, sizeof(CtrlDev));
    return e != hipSuccess ? e : hipMemcpy(c->dev, &c->host, sizeof(CtrlDev), hipMemcpyHostToDevice);
}

extern "C" int cclqr_ctrl_create(const cclqr_mech* m, const cclqr_ctrl_desc* d, cclqr_ctrl** out) {
    if (!m || !d || !out) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    CtrlHostTables T;
    std::string err;
    const int rc = build_ctrl_tables(m, d, T, err);
    if (rc != CCLQR_OK) return fail(rc, err);
    CtrlOwner own(ctrl_new(m));
    cclqr_ctrl* c = own.p;
    HIPTRY("controller upload", hipMalloc((void**)&c->zd_dev, T.zd.size() * sizeof(double)));
    HIPTRY("controller upload", hipMemcpy(c->zd_dev, T.zd.data(), T.zd.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!T.K.empty()) {      // one table, or one per instance behind its own zero pad (gain_table_layout)
        const size_t ntab = (size_t)T.H.n_ctrl, per = T.K.size() / ntab;
        const GainTableLayout L = gain_table_layout(m->shape, m->nb, T.H.n_ctrl, (long long)T.H.nK * T.H.mu);
        HIPTRY("controller upload", hipMalloc((void**)&c->K_dev, L.alloc_doubles * sizeof(double)));
        HIPTRY("controller upload", hipMemset(c->K_dev, 0, L.alloc_doubles * sizeof(double)));
        HIPTRY("controller upload", L.pad ? hipMemcpy2D(c->K_dev, (size_t)L.stride * sizeof(double), T.K.data(), per * sizeof(double), per * sizeof(double), ntab, hipMemcpyHostToDevice)
                                          : hipMemcpy(c->K_dev, T.K.data(), T.K.size() * sizeof(double), hipMemcpyHostToDevice));
        if (ntab > 1) T.H.K_stride = L.K_stride;
    }
    if (!T.Fd.empty()) {
        HIPTRY("controller upload", hipMalloc((void**)&c->Fd_dev, T.Fd.size() * sizeof(double)));
        HIPTRY("controller upload", hipMemcpy(c->Fd_dev, T.Fd.data(), T.Fd.size() * sizeof(double), hipMemcpyHostToDevice));
        c->Fd_len = T.Fd.size();
    }
    c->host = T.H;
    HIPTRY("controller upload", ctrl_publish(c));
    *out = own.release();
    return CCLQR_OK;
}

// controlfunction hook (lqr.jl:14, :56): the host's closure has computed the joint inputs of the next step
extern "C" int cclqr_ctrl_set_feedforward(cclqr_ctrl* c, const double* Fd, int64_t len, int32_t on_device, void* stream) {
    if (!c || !Fd) return fail(CCLQR_EINVAL, "null argument");
    if (!c->Fd_dev) return fail(CCLQR_EINVAL, "the controller was created without a feed-forward table");
    if (len < 0 || (size_t)len != c->Fd_len) return fail(CCLQR_EINVAL, "feed-forward table length differs from the one the controller was created with");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != c->device) return fail(CCLQR_EINVAL, "the calling thread is not on the controller's device");
    hipError_t e = on_device ? hipMemcpyAsync(c->Fd_dev, Fd, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream)
                             : hipMemcpy(c->Fd_dev, Fd, (size_t)len * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(CCLQR_EHIP, std::string("feed-forward upload: ") + hipGetErrorString(e));
    return CCLQR_OK;
}

// in-place permutation of the 12-column body blocks of every gain row from the caller's body order to the kernels' link order
// (one workgroup per row, the row staged in LDS); what build_ctrl_tables does on the host for caller-supplied gains
__global__ void k_rows_to_link_order_kernel(double* K, long long nrows, long long rows_per_table, long long table_stride, int nb, const MechDev* M) {
    extern __shared__ double row[];
    const long long r = blockIdx.x;
    if (r >= nrows) return;
    double* p = K + (r / rows_per_table) * table_stride + (r % rows_per_table) * 12 * nb;
    for (int e = threadIdx.x; e < 12 * nb; e += blockDim.x) row[e] = p[e];
    __syncthreads();
    for (int e = threadIdx.x; e < 12 * nb; e += blockDim.x) { const int l = e / 12; p[e] = row[12 * M->perm[l] + (e - 12 * l)]; }
}

// are the n items (`what`: knots = plants of a call, instances of a launch) first .. first + n - 1 all among the table's plants?  Item k runs on the plant with
// global index first + k.  No device work, and no std::string unless the answer is no (cclqr_rollout_plants is on the per-step host path)
static int plants_check_range(const cclqr_mech* m, const cclqr_plants* plants, int64_t first, int64_t n, const char* what, const char* of) {
    if (!plants) return CCLQR_OK;
    if (plants->mech != m) return fail(CCLQR_EINVAL, "the plants were created for another mechanism");
    const int64_t lo = first - plants->first_index;
    if (n > 0 && (lo < 0 || lo + n > plants->n_plant))
        return fail(CCLQR_EINVAL, std::string(what) + " " + std::to_string(first) + " .. " + std::to_string(first + n - 1) + " of the " + of + " are not all among the plants " +
                                  std::to_string(plants->first_index) + " .. " + std::to_string(plants->first_index + plants->n_plant - 1));
    return CCLQR_OK;
}

// ---- linearising nk host knots into the calling thread's workspace: the one sequence behind cclqr_linearize_plants, the analytic cclqr_linearize_projected,
// cclqr_riccati_tracking_ex and cclqr_ctrl_create_lqr_batch_plants
struct LinWs { double *zd, *Fd, *A, *Bu, *Bl, *G; int* status; int cj[CCLQR_MAXL]; };      // cj: the controlled joints as the kernels address them
// what such a call is refused for before anything is allocated; cj = the controlled joints as the kernels address them.  No knots: nothing else is looked at
static int linearize_check(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int nk, int mu, const int32_t* ctrl_joint, int* cj) {
    TRY(check_device(m));
    if (plants && m->host.loop)
        return fail(CCLQR_EUNSUPPORTED, "per-instance plants are for forests of chains and branching trees (closed-loop mechanisms run their own plant)");
    TRY(plants_check_range(m, plants, first_plant, nk, "plants", "call"));
    if (nk == 0) return CCLQR_OK;
    if (!linearize_fits_lds(m)) return fail(CCLQR_EUNSUPPORTED, "instance does not fit LDS");
    return map_ctrl_joints(m, mu, ctrl_joint, cj);
}
// The checks, the blocks (inside the caller's WsScope), the upload of the knots (Fd_host null: w.Fd stays what the caller set -- a device table, or none) and
// the launch on the null stream; the models stay on the device and w.cj keeps the mapped joints for a caller that needs them.  `prefix` words a HIP failure
static int linearize_to_ws(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int nk, const double* zd_host, const double* Fd_host, int mu,
                           const int32_t* ctrl_joint, LinWs& w, const char* prefix) {
    TRY(linearize_check(m, plants, first_plant, nk, mu, ctrl_joint, w.cj));
    if (nk == 0) return CCLQR_OK;
    LinArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.cj, w.cj, sizeof(a.cj));
    const size_t n = (size_t)nk, nz = 13 * (size_t)m->nb, mx = 12 * (size_t)m->nb, ml = 5 * (size_t)(m->host.loop ? m->nj : m->nb), mu1 = (size_t)(mu > 0 ? mu : 1);
    HIPTRY(prefix, ws_get((void**)&w.zd, n * nz * sizeof(double)));
    if (Fd_host && mu > 0) HIPTRY(prefix, ws_get((void**)&w.Fd, n * mu * sizeof(double)));
    HIPTRY(prefix, ws_get((void**)&w.A, n * mx * mx * sizeof(double)));
    HIPTRY(prefix, ws_get((void**)&w.Bu, n * mx * mu1 * sizeof(double)));
    HIPTRY(prefix, ws_get((void**)&w.Bl, n * mx * ml * sizeof(double)));
    HIPTRY(prefix, ws_get((void**)&w.G, n * ml * mx * sizeof(double)));
    HIPTRY(prefix, ws_get((void**)&w.status, n * sizeof(int)));
    HIPTRY(prefix, hipMemcpy(w.zd, zd_host, n * nz * sizeof(double), hipMemcpyHostToDevice));
    if (Fd_host && mu > 0) HIPTRY(prefix, hipMemcpy(w.Fd, Fd_host, n * mu * sizeof(double), hipMemcpyHostToDevice));
    a.M = m->dev; a.nk = nk; a.mu = mu;
    a.plants = plants ? plants->dev : nullptr;
    a.plant_off = plants ? first_plant - plants->first_index : 0;
    a.zd = w.zd; a.Fd = w.Fd; a.A = w.A; a.Bu = w.Bu; a.Bl = w.Bl; a.G = w.G; a.status = w.status;
    HIPTRY(prefix, launch_linearize(a, m->shape, nullptr));
    return CCLQR_OK;
}
// the Newton statuses of nk linearised knots, read back: *bad = the first knot whose setpoint solve did not converge, -1 when all did (the caller words the refusal)
static hipError_t knots_converged(const int* status_dev, size_t nk, long long* bad) {
    std::vector<int> st(nk);
    *bad = -1;
    const hipError_t e = hipMemcpy(st.data(), status_dev, nk * sizeof(int), hipMemcpyDeviceToHost);
    for (size_t k = 0; k < nk && e == hipSuccess && *bad < 0; k++)
        if (st[k] <= 0) *bad = (long long)k;
    return e;
}
static int knot_not_converged(long long k) { return fail(CCLQR_ENOCONV, "Newton did not converge at the setpoint of knot " + std::to_string(k)); }

// the one refusal the per-problem weights add (cclqr_riccati_weights, cclqr_ctrl_create_lqr_batch_weights): before anything is allocated or launched
static int check_n_weights(int n_weights, int nprob, const char* of) {
    if (n_weights == 1 || n_weights == nprob) return CCLQR_OK;
    return fail(CCLQR_EINVAL, "n_weights = " + std::to_string(n_weights) + ": the weights are one pair shared by all (1) or one pair per " + of + " (" + std::to_string(nprob) + ")");
}

// a cost-to-go object under construction: n_tables tables of mx x mx doubles on the mechanism's device, not yet filled
typedef Owned<cclqr_value, cclqr_value_destroy> ValueOwner;
static cclqr_value* value_new(const cclqr_mech* m, int64_t n_tables) {
    cclqr_value* v = new cclqr_value();
    memset(v, 0, sizeof(*v));
    v->n_tables = n_tables; v->nb = m->nb; v->device = m->device; v->mech = m;
    return v;
}
static hipError_t value_alloc(cclqr_value* v) { return hipMalloc((void**)&v->P_dev, (size_t)v->n_tables * 144 * (size_t)v->nb * v->nb * sizeof(double)); }

// what both doubling entry points of the Riccati map refuse about their own arguments, before anything is allocated or launched (riccati_doubling.hip); the
// n_weights pairs Q [mx][mx], R [mu][mu] have been counted by the caller (check_n_weights)
static int riccati_doubling_check(int N, double tol, int max_levels, const cclqr_riccati_opts* opts, int mx, int mu, int n_weights, const double* Q, const double* R) {
    if (N == 1 || N < 0) return fail(CCLQR_EINVAL, "N = " + std::to_string(N) + ": a horizon of N >= 2 knots, or 0 = to convergence");
    if (N == 0 && (max_levels < 1 || max_levels > 60)) return fail(CCLQR_EINVAL, "max_levels = " + std::to_string(max_levels) + ": 1 .. 60 (2^max_levels steps)");
    if (!(tol >= 0.0)) return fail(CCLQR_EINVAL, "tol is negative or not a number");
    if (opts && opts->bf16_terms != 0) return fail(CCLQR_EINVAL, "the Riccati doubling runs in fp64 only (bf16_terms = 0)");
    if (!riccati_doubling_fits(mx, mu)) return fail(CCLQR_EINVAL, "bad sizes: mx = " + std::to_string(mx) + ", mu = " + std::to_string(mu) + " exceed the LDS panels of the doubling kernels");
    for (int p = 0; p < n_weights; p++)
        if (ric_p_rows(Q + (size_t)p * mx * mx, mx, mu == 0 ? R : R + (size_t)p * mu * mu, mu))
            return fail(CCLQR_EINVAL, "Q or R of weight pair " + std::to_string(p) + " is not symmetric: the composition of Riccati maps holds for exactly symmetric weights only");
    return CCLQR_OK;
}

// what cclqr_ctrl_create_lqr_batch_doubling adds to the batched construction: the one gain by doubling the Riccati map (riccati_doubling.hip) in place of the
// stepped recursion, and where its diagnostics go (host, [n_ctrl] / [n_ctrl][2], each may be null)
struct LqrDoubling { int max_levels; int32_t *levels, *reason; double *dnorm, *anorm; };
// The host sequence of the batched LQR constructors, one copy: checks, setpoints, linearisation on the plants, dlqr for every setpoint into the controller's table,
// link order, publication.  dbl null: the stepped recursion (cclqr_ctrl_create_lqr_batch_value); else the doubling, with infinite_horizon = 1 and N = 0 or >= 2
static int lqr_batch_build(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, const double* zd, int32_t mu,
                           const int32_t* ctrl_joint, const double* Fd, int32_t n_weights, const double* Q, const double* R, int32_t N,
                           int32_t infinite_horizon, double tol, int32_t* kbreak, const LqrDoubling* dbl, cclqr_ctrl** out, cclqr_value** value) {
    static const char* const what = "batched LQR construction";
    const bool inf = infinite_horizon != 0;
    if (!m || !zd || !Q || !out || (mu > 0 && (!ctrl_joint || !R))) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (m->host.loop) return fail(CCLQR_EUNSUPPORTED, "batched LQR construction is for tree mechanisms (closed loops: cclqr_linearize_projected)");
    if (n_ctrl < 1 || (!dbl && N < 2) || mu < 1 || mu > m->nb) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_weights(n_weights, n_ctrl, "table"));
    if (dbl) TRY(riccati_doubling_check(N, tol, dbl->max_levels, nullptr, 12 * m->nb, mu, n_weights, Q, R));
    const int nb = m->nb;
    const size_t nz = 13 * (size_t)nb, mx = 12 * (size_t)nb, ml = 5 * (size_t)nb, np = (size_t)n_ctrl, nw = (size_t)n_weights;
    CtrlOwner own(ctrl_new(m));
    cclqr_ctrl* c = own.p;
    CtrlDev& H = c->host;
    ValueOwner vown(value ? value_new(m, n_ctrl) : nullptr);      // (value == NULL: nothing is kept, nothing allocated)
    // LQR{T,Inf} (lqr.jl:25-27, 40-43): the recursion runs its N = Ntemp steps, only Ku[1] is kept and the feedback is never gated
    const size_t nKtab = inf ? 1 : (size_t)(N - 1);
    H.mu = mu; H.nK = (int)nKtab; H.N = inf ? 0 : N; H.nsp = 1; H.n_ctrl = n_ctrl;
    const GainTableLayout L = gain_table_layout(m->shape, nb, n_ctrl, (long long)nKtab * mu);      // every instance's table ends in its own zero pad
    H.K_stride = L.K_stride;
    H.zd_stride = n_ctrl > 1 ? (long long)nz : 0;
    H.Fd_stride = (n_ctrl > 1 && Fd) ? mu : 0;
    // setpoints in link order for the rollout's control law
    std::vector<double> zl(np * nz);
    for (size_t s = 0; s < np; s++)
        for (int l = 0; l < nb; l++) memcpy(&zl[(s * nb + l) * 13], zd + (s * nb + m->host.perm[l]) * 13, 13 * sizeof(double));
    double *dQ = nullptr, *dR = nullptr, *dwork = nullptr;
    int *dkb = nullptr, *dst = nullptr, *dstop = nullptr;
    std::vector<int> kb(np), st(np);
    WsScope scope;
    HIPTRY(what, hipMalloc((void**)&c->zd_dev, np * nz * sizeof(double)));
    HIPTRY(what, hipMemcpy(c->zd_dev, zl.data(), np * nz * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY(what, hipMalloc((void**)&c->K_dev, L.alloc_doubles * sizeof(double)));
    if (vown.p) HIPTRY(what, value_alloc(vown.p));
    if (Fd) {
        HIPTRY(what, hipMalloc((void**)&c->Fd_dev, np * mu * sizeof(double)));
        HIPTRY(what, hipMemcpy(c->Fd_dev, Fd, np * mu * sizeof(double), hipMemcpyHostToDevice));
        c->Fd_len = (size_t)np * mu;
    }
    // linearsystem at every setpoint (lqr.jl:63), one launch, reading the controller's own feed-forward table; the matrices stay on the device
    LinWs w = {};
    w.Fd = c->Fd_dev;
    TRY(linearize_to_ws(m, plants, first_plant, n_ctrl, zd, nullptr, mu, ctrl_joint, w, what));
    memcpy(H.cj, w.cj, sizeof(int) * (size_t)mu);
    // dlqr for every setpoint (lqr.jl:141-184), gains written straight into the controller's table
    RicArgs ra;
    ra.nprob = n_ctrl; ra.mx = (int)mx; ra.mu = mu; ra.ml = (int)ml; ra.N = N; ra.time_varying = 0; ra.tol = tol; ra.path = 0; ra.bf16_terms = 0; ra.keep_last = inf ? 1 : 0;
    ra.kpad = (long long)L.pad;
    ra.p_rows = ric_p_rows(Q, (int)mx, R, mu);
    ric_per_problem_weights(ra, Q, R, n_weights);      // (one pair per table: table p is designed with pair p)
    HIPTRY(what, ws_get((void**)&dQ, nw * mx * mx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dR, (nw * mu * mu + 1) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dwork, ric_total_work_doubles(ra) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dstop, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dkb, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dst, np * sizeof(int)));
    HIPTRY(what, hipMemcpy(dQ, Q, nw * mx * mx * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY(what, hipMemcpy(dR, R, nw * mu * mu * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY(what, hipMemset(c->K_dev, 0, L.alloc_doubles * sizeof(double)));
    ra.stop = dstop; ra.A = w.A; ra.Bu = w.Bu; ra.Bl = w.Bl; ra.G = w.G; ra.Q = dQ; ra.R = dR; ra.K = c->K_dev; ra.kbreak = dkb; ra.status = dst; ra.work = dwork;
    ra.P_out = vown.p ? vown.p->P_dev : nullptr;      // the models and Q are in the caller's body order, so is the cost-to-go: it stays as the recursion leaves it
    RdbArgs da;
    if (dbl) {
        double *dwork2 = nullptr;
        HIPTRY(what, ws_get((void**)&dwork2, rdb_work_doubles(n_ctrl, (int)mx) * sizeof(double)));
        HIPTRY(what, ws_get((void**)&da.levels, np * sizeof(int)));
        HIPTRY(what, ws_get((void**)&da.reason, np * sizeof(int)));
        HIPTRY(what, ws_get((void**)&da.dnorm, 2 * np * sizeof(double)));
        HIPTRY(what, ws_get((void**)&da.anorm, 2 * np * sizeof(double)));
        da.r = ra; da.max_levels = dbl->max_levels; da.work2 = dwork2;
        HIPTRY(what, launch_riccati_doubling(da, nullptr));
    } else
        HIPTRY(what, launch_riccati(ra, nullptr));
    const long long nrows = (long long)np * (long long)nKtab * mu;
    HIPTRY(what, launch_lds<false>(k_rows_to_link_order_kernel, dim3((unsigned)nrows), dim3(128), mx * sizeof(double), nullptr, c->K_dev, nrows, (long long)nKtab * mu, L.stride, nb, m->dev));
    HIPTRY(what, hipDeviceSynchronize());
    long long bad = -1;
    HIPTRY(what, knots_converged(w.status, np, &bad));
    if (!dbl) HIPTRY(what, hipMemcpy(kb.data(), dkb, np * sizeof(int), hipMemcpyDeviceToHost));
    HIPTRY(what, hipMemcpy(st.data(), dst, np * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> lv, rs;
    std::vector<double> dn, an;
    if (dbl) {
        lv.resize(np); rs.resize(np); dn.resize(2 * np); an.resize(2 * np);
        HIPTRY(what, hipMemcpy(lv.data(), da.levels, np * sizeof(int), hipMemcpyDeviceToHost));
        HIPTRY(what, hipMemcpy(rs.data(), da.reason, np * sizeof(int), hipMemcpyDeviceToHost));
        HIPTRY(what, hipMemcpy(dn.data(), da.dnorm, 2 * np * sizeof(double), hipMemcpyDeviceToHost));
        HIPTRY(what, hipMemcpy(an.data(), da.anorm, 2 * np * sizeof(double), hipMemcpyDeviceToHost));
    }
    HIPTRY(what, ctrl_publish(c));
    for (size_t p = 0; p < np; p++) {      // kbreak (the doubling's diagnostics) is filled up to the problem the call is refused for
        if (kbreak && !dbl) kbreak[p] = kb[p];
        if (dbl) {
            if (dbl->levels) dbl->levels[p] = lv[p];
            if (dbl->reason) dbl->reason[p] = rs[p];
            if (dbl->dnorm) { dbl->dnorm[2 * p] = dn[2 * p]; dbl->dnorm[2 * p + 1] = dn[2 * p + 1]; }
            if (dbl->anorm) { dbl->anorm[2 * p] = an[2 * p]; dbl->anorm[2 * p + 1] = an[2 * p + 1]; }
        }
        if ((long long)p == bad) return fail(CCLQR_ENOCONV, "Newton did not converge at setpoint " + std::to_string(p));
        if (st[p] != 0) return fail(CCLQR_ESINGULAR, "G*Bl or M is singular at setpoint " + std::to_string(p));
    }
    *out = own.release();
    if (value) *value = vown.release();
    return CCLQR_OK;
}

extern "C" int cclqr_ctrl_create_lqr_batch_value(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, const double* zd, int32_t mu,
                                                 const int32_t* ctrl_joint, const double* Fd, int32_t n_weights, const double* Q, const double* R, int32_t N,
                                                 int32_t infinite_horizon, double tol, int32_t* kbreak, cclqr_ctrl** out, cclqr_value** value) {
    return lqr_batch_build(m, plants, first_plant, n_ctrl, zd, mu, ctrl_joint, Fd, n_weights, Q, R, N, infinite_horizon, tol, kbreak, nullptr, out, value);
}

// LQR{T,Inf}'s one gain (lqr.jl:25-27, 39-43) by doubling the Riccati map of lqr.jl:141-184: cclqr_ctrl_create_lqr_batch_value with infinite_horizon = 1 and the
// doubling in place of the stepped recursion
extern "C" int cclqr_ctrl_create_lqr_batch_doubling(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, const double* zd, int32_t mu,
                                                    const int32_t* ctrl_joint, const double* Fd, int32_t n_weights, const double* Q, const double* R, int32_t N,
                                                    double tol, int32_t max_levels, int32_t* levels, int32_t* reason, double* dnorm, double* anorm,
                                                    cclqr_ctrl** out, cclqr_value** value) {
    const LqrDoubling dbl = {max_levels, levels, reason, dnorm, anorm};
    return lqr_batch_build(m, plants, first_plant, n_ctrl, zd, mu, ctrl_joint, Fd, n_weights, Q, R, N, 1, tol, nullptr, &dbl, out, value);
}

extern "C" int cclqr_ctrl_create_lqr_batch_weights(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, const double* zd, int32_t mu,
                                                   const int32_t* ctrl_joint, const double* Fd, int32_t n_weights, const double* Q, const double* R, int32_t N,
                                                   int32_t infinite_horizon, double tol, int32_t* kbreak, cclqr_ctrl** out) {
    return cclqr_ctrl_create_lqr_batch_value(m, plants, first_plant, n_ctrl, zd, mu, ctrl_joint, Fd, n_weights, Q, R, N, infinite_horizon, tol, kbreak, out, nullptr);
}

extern "C" int cclqr_ctrl_create_lqr_batch_plants(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, const double* zd, int32_t mu,
                                                  const int32_t* ctrl_joint, const double* Fd, const double* Q, const double* R, int32_t N, int32_t infinite_horizon,
                                                  double tol, int32_t* kbreak, cclqr_ctrl** out) {
    return cclqr_ctrl_create_lqr_batch_weights(m, plants, first_plant, n_ctrl, zd, mu, ctrl_joint, Fd, 1, Q, R, N, infinite_horizon, tol, kbreak, out);
}

extern "C" int cclqr_ctrl_create_lqr_batch(const cclqr_mech* m, int32_t n_ctrl, const double* zd, int32_t mu, const int32_t* ctrl_joint,
                                           const double* Fd, const double* Q, const double* R, int32_t N, int32_t infinite_horizon, double tol,
                                           int32_t* kbreak, cclqr_ctrl** out) {
    return cclqr_ctrl_create_lqr_batch_plants(m, nullptr, 0, n_ctrl, zd, mu, ctrl_joint, Fd, Q, R, N, infinite_horizon, tol, kbreak, out);
}

// in-place permutation of the bodies of every setpoint row [nb][13] from the caller's body order to the kernels' link order (one workgroup per row, the row
// staged in LDS): what build_ctrl_tables does on the host for caller-supplied setpoints, here for trajectories that may never have been on the host
__global__ void sp_rows_to_link_order_kernel(double* zd, long long nrows, int nb, const MechDev* M) {
    extern __shared__ double row[];
    const long long r = blockIdx.x;
    if (r >= nrows) return;
    double* p = zd + r * 13 * nb;
    for (int e = threadIdx.x; e < 13 * nb; e += blockDim.x) row[e] = p[e];
    __syncthreads();
    for (int e = threadIdx.x; e < 13 * nb; e += blockDim.x) { const int l = e / 13; p[e] = row[13 * M->perm[l] + (e - 13 * l)]; }
}

// TrackingLQR(mechanism_k, storage_k, Fτ_k, eqcids, Q, R) (lqr_tracking.jl:17-43) for n_ctrl plants and / or trajectories in one call: linearsystem at the knots
// 1 .. N-1 of every trajectory (lqr_tracking.jl:88) on that trajectory's plant, the recursion of lqr_tracking.jl:73-122 per problem, the gains written into the
// controller's tables.  The problems run in chunks that keep the models and the recursion's scratch within the workspace budget (tracking_chunk_problems).
extern "C" int cclqr_ctrl_create_tracking_batch_plants(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_ctrl, int32_t N,
                                                       const double* zd, const double* Fd, int32_t on_device, int32_t mu, const int32_t* ctrl_joint,
                                                       const double* Q, const double* R, double tol, const cclqr_ctrl_desc* law, int64_t workspace_bytes,
                                                       int32_t* kbreak, void* stream, cclqr_ctrl** out) {
    static const char* const what = "batched TrackingLQR construction";
    if (!m || !zd || !Q || !R || !ctrl_joint || !out) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (m->host.loop) return fail(CCLQR_EUNSUPPORTED, "batched TrackingLQR construction is for tree mechanisms (closed-loop mechanisms: cclqr_linearize_projected + cclqr_riccati_tv)");
    if (n_ctrl < 1 || N < 2 || mu < 1 || mu > m->nb) return fail(CCLQR_EINVAL, "bad sizes");
    const int nb = m->nb;
    const size_t nz = 13 * (size_t)nb, mx = 12 * (size_t)nb, ml = 5 * (size_t)nb, np = (size_t)n_ctrl, nk = (size_t)N - 1;
    LinArgs la;
    memset(&la, 0, sizeof(la));
    la.M = m->dev; la.mu = mu;
    la.plants = plants ? plants->dev : nullptr;
    la.knots_per_plant = (int)nk; la.rows_per_plant = N;
    TRY(linearize_check(m, plants, first_plant, n_ctrl, mu, ctrl_joint, la.cj));
    CtrlDev H;
    memset(&H, 0, sizeof(H));
    H.mu = mu; H.nK = (int)nk; H.N = N; H.nsp = N; H.n_ctrl = n_ctrl;
    memcpy(H.cj, la.cj, sizeof(int) * (size_t)mu);
    if (law) {       // the friction / noise law of examples/trackingLQR_triple_cartpole.jl:93-111, as build_ctrl_tables takes it
        if (law->fric)
            for (int j = 0; j < nb; j++) { H.fric[m->link_of_joint[j]] = law->fric[j]; if (law->fric[j] != 0.0) H.has_fric = 1; }
        H.noise_scale = law->noise_scale;
        H.noise_philox = law->noise_philox ? 1 : 0;
        H.noise_key0 = (unsigned)(law->noise_seed & 0xffffffffu) ^ (unsigned)(law->noise_seed >> 32);
    }
    const GainTableLayout L = gain_table_layout(m->shape, nb, n_ctrl, (long long)nk * mu);      // every table ends in its own zero pad
    H.K_stride = L.K_stride;
    H.zd_stride = n_ctrl > 1 ? (long long)N * (long long)nz : 0;
    H.Fd_stride = (n_ctrl > 1 && Fd) ? (long long)N * mu : 0;
    // one Riccati path for the whole call, chosen from n_ctrl, and the chunks the workspace budget allows: all before anything is allocated
    RicArgs ra;
    ra.nprob = n_ctrl; ra.mx = (int)mx; ra.mu = mu; ra.ml = (int)ml; ra.N = N; ra.time_varying = 1; ra.tol = tol; ra.path = 0; ra.bf16_terms = 0; ra.keep_last = 0;
    ra.kpad = (long long)L.pad;
    ra.p_rows = ric_p_rows(Q, (int)mx, R, mu);
    ra.path = ric_chosen_path(ra);
    RicArgs r1 = ra, r2 = ra;
    r1.nprob = 1; r2.nprob = 2;
    const long long ric_per = (long long)(ric_total_work_doubles(r2) - ric_total_work_doubles(r1)), ric_fixed = (long long)ric_total_work_doubles(r1) - ric_per;
    const long long per_bytes = tracking_problem_bytes((int)mx, mu, (int)ml, N, ric_per);
    const size_t q_doubles = mx * mx, r_doubles = ((size_t)mu * mu + 1) & ~(size_t)1;
    const long long fixed_bytes = 8 * (ric_fixed + (long long)q_doubles + (long long)r_doubles);
    const long long budget = workspace_bytes > 0 ? (long long)workspace_bytes : CCLQR_TRACKING_WORKSPACE_BYTES;
    const long long per_chunk = tracking_chunk_problems(n_ctrl, per_bytes, fixed_bytes, budget);
    if (per_chunk < 1)
        return fail(CCLQR_EINVAL, "workspace_bytes = " + std::to_string(budget) + " does not hold one problem: N = " + std::to_string(N) + " knots of this mechanism need " +
                                  std::to_string(fixed_bytes + per_bytes) + " bytes");
    const size_t pc = (size_t)per_chunk;
    hipStream_t st_ = (hipStream_t)stream;
    CtrlOwner own(ctrl_new(m));      // (declared before the blocks: they are released, after a wait for the stream, before the controller's tables)
    cclqr_ctrl* c = own.p;
    c->host = H;
    DevBlocks blocks(st_);           // a: the slab, b: the statuses
    const size_t nsp_all = np * (size_t)N;
    std::vector<int> kb(np), st(np);
    const hipMemcpyKind up = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    // the setpoints go straight into the controller's table, in the caller's body order while the linearisation reads them (it permutes as it loads); they are
    // taken to link order in place afterwards.  Host arrays are copied synchronously, device arrays on `stream`
    HIPTRY(what, hipMalloc((void**)&c->zd_dev, nsp_all * nz * sizeof(double)));
    HIPTRY(what, on_device ? hipMemcpyAsync(c->zd_dev, zd, nsp_all * nz * sizeof(double), up, st_) : hipMemcpy(c->zd_dev, zd, nsp_all * nz * sizeof(double), up));
    HIPTRY(what, hipMalloc((void**)&c->K_dev, L.alloc_doubles * sizeof(double)));
    if (Fd) {
        HIPTRY(what, hipMalloc((void**)&c->Fd_dev, nsp_all * mu * sizeof(double)));
        HIPTRY(what, on_device ? hipMemcpyAsync(c->Fd_dev, Fd, nsp_all * mu * sizeof(double), up, st_) : hipMemcpy(c->Fd_dev, Fd, nsp_all * mu * sizeof(double), up));
        c->Fd_len = nsp_all * mu;
    }
    HIPTRY(what, hipMalloc(&blocks.a, (size_t)(fixed_bytes + per_bytes * per_chunk)));
    HIPTRY(what, hipMalloc(&blocks.b, (np * nk + 3 * np + pc) * sizeof(int)));
    int *dlst = (int*)blocks.b, *dkb = dlst + np * nk, *dst = dkb + np, *dstop = dst + np;
    // the slab: Q | R | A | Bu | Bl | G of a chunk's knots | the recursion's workspace for a chunk
    double* dQ = (double*)blocks.a;
    double* dR = dQ + q_doubles;
    double* dA = dR + r_doubles;
    double* dBu = dA + pc * nk * mx * mx;
    double* dBl = dBu + pc * nk * mx * mu;
    double* dG = dBl + pc * nk * mx * ml;
    double* dwork = dG + pc * nk * ml * mx;
    HIPTRY(what, hipMemcpy(dQ, Q, mx * mx * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY(what, hipMemcpy(dR, R, (size_t)mu * mu * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY(what, hipMemsetAsync(c->K_dev, 0, L.alloc_doubles * sizeof(double), st_));
    la.A = dA; la.Bu = dBu; la.Bl = dBl; la.G = dG;
    ra.stop = dstop; ra.A = dA; ra.Bu = dBu; ra.Bl = dBl; ra.G = dG; ra.Q = dQ; ra.R = dR; ra.work = dwork;
    for (size_t c0 = 0; c0 < np; c0 += pc) {
        const size_t nc = np - c0 < pc ? np - c0 : pc;
        // linearsystem at the knots 1 .. N-1 of the chunk's trajectories (lqr_tracking.jl:88), one launch; the models stay on the device
        la.nk = (int)(nc * nk);
        la.zd = c->zd_dev + c0 * (size_t)N * nz;
        la.Fd = c->Fd_dev ? c->Fd_dev + c0 * (size_t)N * mu : nullptr;
        la.plant_off = plants ? first_plant - plants->first_index + (long long)c0 : 0;
        la.status = dlst + c0 * nk;
        HIPTRY(what, launch_linearize(la, m->shape, st_));
        // the recursion of lqr_tracking.jl:73-122 for each of them, gains written straight into the controller's tables
        ra.nprob = (int)nc;
        ra.K = c->K_dev + c0 * (size_t)L.stride; ra.kbreak = dkb + c0; ra.status = dst + c0;
        HIPTRY(what, launch_riccati(ra, st_));
    }
    const long long nrows = (long long)np * (long long)nk * mu;
    HIPTRY(what, launch_lds<false>(k_rows_to_link_order_kernel, dim3((unsigned)nrows), dim3(128), mx * sizeof(double), st_, c->K_dev, nrows, (long long)nk * mu, L.stride, nb, m->dev));
    HIPTRY(what, launch_lds<false>(sp_rows_to_link_order_kernel, dim3((unsigned)nsp_all), dim3(64), nz * sizeof(double), st_, c->zd_dev, (long long)nsp_all, nb, m->dev));
    HIPTRY(what, hipStreamSynchronize(st_));
    long long bad = -1;
    HIPTRY(what, knots_converged(dlst, np * nk, &bad));
    HIPTRY(what, hipMemcpy(kb.data(), dkb, np * sizeof(int), hipMemcpyDeviceToHost));
    HIPTRY(what, hipMemcpy(st.data(), dst, np * sizeof(int), hipMemcpyDeviceToHost));
    blocks.release();
    HIPTRY(what, ctrl_publish(c));
    for (size_t p = 0; p < np; p++) if (kbreak) kbreak[p] = kb[p];
    for (size_t p = 0; p < np; p++) {
        if (bad >= 0 && (size_t)bad / nk == p)
            return fail(CCLQR_ENOCONV, "Newton did not converge at the setpoint of knot " + std::to_string((size_t)bad % nk) + " of table " + std::to_string(p));
        if (st[p] != 0) return fail(CCLQR_ESINGULAR, "G*Bl or M is singular in table " + std::to_string(p));
    }
    *out = own.release();
    return CCLQR_OK;
}

// one table's gains back on the host, in the caller's body order (the inverse of k_rows_to_link_order_kernel / build_ctrl_tables)
extern "C" int cclqr_ctrl_get_gains(const cclqr_mech* m, const cclqr_ctrl* c, int64_t table, double* K_host) {
    if (!m || !c || !K_host) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (c->nb != m->nb || c->device != m->device) return fail(CCLQR_EINVAL, "the controller was created for another mechanism");
    if (!c->K_dev || c->host.nK < 1) return fail(CCLQR_EINVAL, "the controller has no gains (open loop / PID)");
    const int64_t ntab = c->host.n_ctrl > 1 ? c->host.n_ctrl : 1;
    if (table < 0 || table >= ntab) return fail(CCLQR_EINVAL, "table " + std::to_string(table) + " is not among the controller's tables 0 .. " + std::to_string(ntab - 1));
    const int nb = m->nb;
    const size_t mx = 12 * (size_t)nb, rows = (size_t)c->host.nK * c->host.mu;
    std::vector<double> Kl(rows * mx);
    HIPCHK(hipMemcpy(Kl.data(), c->K_dev + (size_t)table * (size_t)c->host.K_stride, rows * mx * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; r++)
        for (int l = 0; l < nb; l++) memcpy(K_host + r * mx + 12 * m->host.perm[l], &Kl[r * mx + 12 * l], 12 * sizeof(double));
    return CCLQR_OK;
}

extern "C" int cclqr_ctrl_destroy(cclqr_ctrl* c) {
    if (!c) return CCLQR_OK;
    if (c->K_dev) (void)hipFree(c->K_dev);
    if (c->zd_dev) (void)hipFree(c->zd_dev);
    if (c->Fd_dev) (void)hipFree(c->Fd_dev);
    if (c->noise_ws) (void)hipFree(c->noise_ws);
    if (c->dev) (void)hipFree(c->dev);
    delete c;
    return CCLQR_OK;
}

// the four geometry queries read the mechanism's RolloutShape: what they report is what the launchers launch
extern "C" int cclqr_rollout_layout_links(const cclqr_mech* m, int32_t* links) {
    if (!m || !links) return fail(CCLQR_EINVAL, "null argument");
    // links the rollout kernel's LDS image is laid out for (it names the instantiation): chains rollout_chain_kernel, branching trees
    // rollout_treereg_kernel; 0 for closed-loop mechanisms (one kernel, runtime layout)
    *links = m->shape.NBP;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_lanes_per_link(const cclqr_mech* m, int32_t* lanes_per_link, int32_t* links_per_group) {
    if (!m) return fail(CCLQR_EINVAL, "null argument");
    if (lanes_per_link) *lanes_per_link = m->shape.KL;
    if (links_per_group) *links_per_group = m->shape.NL;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_instances_per_wavefront(const cclqr_mech* m, int64_t n_inst, int32_t steps, int32_t flags, int32_t* instances) {
    if (!m || !instances) return fail(CCLQR_EINVAL, "null argument");
    *instances = spread_instances_per_wavefront(m->shape.full, n_inst, steps, (flags & CCLQR_ROLLOUT_PACK_WAVEFRONTS) != 0, m->simds);
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_geometry(const cclqr_mech* m, int32_t* lanes, int32_t* lds_bytes) {
    if (!m) return fail(CCLQR_EINVAL, "null argument");
    if (lanes) *lanes = m->shape.G;
    if (lds_bytes) *lds_bytes = (int32_t)m->shape.lds;
    return CCLQR_OK;
}

// cclqr_rollout_ex, first part: the arguments as the caller gave them
static int rollout_check_args(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const double* z0, const double* zT,
                              const int32_t* status, const cclqr_rollout_opts* opts) {
    if (!m || !c || !z0 || !zT) return fail(CCLQR_EINVAL, "null argument");
    if (n_inst < 0 || steps < 0 || k0 < 1) return fail(CCLQR_EINVAL, "bad sizes");
    if (c->nb != m->nb) return fail(CCLQR_EINVAL, "controller was built for another mechanism");
    TRY(check_device(m));
    if (m->shape.lds > 160 * 1024) return fail(CCLQR_EUNSUPPORTED, "instance does not fit LDS");
    const int64_t first = opts ? opts->first_instance : 0;
    if (first < 0) return fail(CCLQR_EINVAL, "negative first_instance");
    if (c->host.n_ctrl > 1 && first + n_inst > c->host.n_ctrl) return fail(CCLQR_EINVAL, "more instances than per-instance controller tables");
    // one (integrated, last) pair per joint; never looked at for a controller without a PID law
    if (opts && c->host.has_pid && opts->pid_state_dev && opts->pid_state_len != n_inst * (int64_t)m->shape.pid_slots * 2)
        return fail(CCLQR_EINVAL, "pid_state_len must be n_inst * nb * 2 (closed loops: n_inst * joints * 2)");
    if (opts && (opts->flags & ~(CCLQR_ROLLOUT_NO_ALLOC | CCLQR_ROLLOUT_PACK_WAVEFRONTS | CCLQR_ROLLOUT_CARRY_STATUS | CCLQR_ROLLOUT_RUNTIME_PLAN))) return fail(CCLQR_EINVAL, "unknown bit in cclqr_rollout_opts.flags");
    if (opts && (opts->flags & CCLQR_ROLLOUT_CARRY_STATUS) && !status) return fail(CCLQR_EINVAL, "CCLQR_ROLLOUT_CARRY_STATUS needs the status array (it is read and written)");
    return CCLQR_OK;
}

// cclqr_rollout_ex, second part: where the noise of this launch comes from.  On return *noise is the array the kernel reads (the caller's, or a
// workspace filled here on `stream`; null: none) or *in_kernel says that the kernel draws the samples itself.
// Counter-based noise is generated for this launch into a workspace, read by the rollout like an injected array.  The workspace is the
// caller's (opts->noise_ws_dev: required for launches that share one controller on different streams or threads) or the handle's,
// which only ever grows OUTSIDE stream capture: hipMalloc / hipFree are illegal while a stream is being captured, so a captured
// launch needs the workspace sized beforehand (cclqr_ctrl_reserve_noise) or passed in.
static int rollout_resolve_noise(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const cclqr_rollout_opts* opts, void* stream,
                                 const double** noise, int64_t* noise_stride, bool* in_kernel) {
    const CtrlDev& H = c->host;
    *in_kernel = false;
    if (!(H.noise_scale != 0.0 && H.mu > 0)) { *noise = nullptr; return CCLQR_OK; }
    if (*noise || !H.noise_philox || steps <= 0) return CCLQR_OK;
    // launches of a few steps on forests of chains (the step-per-launch form a hipGraph replays, BASELINE configs[4]) generate their samples inside the
    // rollout kernel (rollout_chain_kernel<.., 3>): one kernel per step instead of two, and no workspace that could have to grow
    if (m->shape.family == RolloutFamily::Chain && !H.has_pid && steps <= CCLQR_PHILOX_INKERNEL_STEPS && !(opts && opts->noise_ws_dev)) { *in_kernel = true; return CCLQR_OK; }
    const size_t need = (size_t)n_inst * steps;
    const int64_t first = opts ? opts->first_instance : 0;
    double* ws = nullptr;
    if (opts && opts->noise_ws_dev) {
        if (opts->noise_ws_len < (int64_t)need) return fail(CCLQR_EINVAL, "noise_ws_len must be at least n_inst * steps");
        ws = opts->noise_ws_dev;
    } else {
        cclqr_ctrl* cm = const_cast<cclqr_ctrl*>(c);
        if (cm->noise_ws_cap < need) {
            // growing = a device synchronisation + an allocation.  A caller who has said CCLQR_ROLLOUT_NO_ALLOC (anybody with a capture open on
            // this device, on whichever stream) is refused outright; without the flag the library can only see a capture of `stream` itself
            if (opts && (opts->flags & CCLQR_ROLLOUT_NO_ALLOC))
                return fail(CCLQR_EINVAL, "CCLQR_ROLLOUT_NO_ALLOC: the Philox noise workspace of this controller holds " + std::to_string(cm->noise_ws_cap) + " samples, the launch needs " +
                                          std::to_string(need) + ": call cclqr_ctrl_reserve_noise(ctrl, n_inst, steps) beforehand or pass cclqr_rollout_opts.noise_ws_dev");
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            if (stream) HIPCHK(hipStreamIsCapturing((hipStream_t)stream, &cap));
            if (cap != hipStreamCaptureStatusNone)
                return fail(CCLQR_EINVAL, "the Philox noise workspace cannot grow during stream capture: call cclqr_ctrl_reserve_noise(ctrl, n_inst, steps) "
                                          "before the capture or pass cclqr_rollout_opts.noise_ws_dev");
            TRY(cclqr_ctrl_reserve_noise(cm, n_inst, steps));
        }
        ws = cm->noise_ws;
    }
    HIPCHK(launch_philox_fill(ws, H.noise_key0, first, n_inst, k0, steps, (hipStream_t)stream));
    *noise = ws - (k0 - 1);      // indexed by the absolute step k-1
    *noise_stride = steps;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_plants(const cclqr_mech* m, const cclqr_plants* plants, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0,
                                    const double* z0, double* lam, const double* noise, int64_t noise_stride, double* traj, double* zT, int32_t* status,
                                    const cclqr_rollout_opts* opts, void* stream) {
    if (m && c && n_inst == 0) return CCLQR_OK;   // empty batch
    TRY(rollout_check_args(m, c, n_inst, steps, k0, z0, zT, status, opts));
    const int64_t first_instance = opts ? opts->first_instance : 0;
    // every instance of the launch must find its plant: refused before anything is launched (the Philox fill included)
    TRY(plants_check_range(m, plants, first_instance, n_inst, "instances", "launch"));
    bool philox_in_kernel = false;
    TRY(rollout_resolve_noise(m, c, n_inst, steps, k0, opts, stream, &noise, &noise_stride, &philox_in_kernel));
    const CtrlDev& H = c->host;
    // the one place a controller's tables become a kernel's law
    const ControlLaw law = H.has_pid ? ControlLaw::Pid : (philox_in_kernel ? ControlLaw::PhiloxInKernel : ((H.has_fric || noise) ? ControlLaw::FricNoise : ControlLaw::Lqr));
    RolloutArgs a;
    a.M = m->dev; a.C = c->dev; a.n_inst = n_inst; a.steps = steps; a.k0 = k0; a.z0 = z0; a.lam = lam; a.noise = noise;
    a.noise_stride = noise_stride; a.traj = traj; a.zT = zT; a.status = status; a.inst0 = opts ? opts->first_instance : 0;
    a.pid_state = (opts && H.has_pid) ? opts->pid_state_dev : nullptr;      // never forwarded to a controller without a PID law
    a.ipw = (opts && (opts->flags & CCLQR_ROLLOUT_PACK_WAVEFRONTS)) ? 1 : 0;
    a.carry = (opts && (opts->flags & CCLQR_ROLLOUT_CARRY_STATUS)) ? 1 : 0;
    const int newton_mode = opts ? opts->newton_mode : 0;
    a.eps_alone = (opts && opts->newton_eps_alone > 0.0) ? opts->newton_eps_alone : 1e-10;
    a.plants = plants ? plants->dev : nullptr;
    a.plant_off = plants ? first_instance - plants->first_index : 0;
    if (newton_mode != 0 && newton_mode != 1) return fail(CCLQR_EINVAL, "newton_mode must be 0 (exact rule) or 1 (residual-only stop)");
    if (m->shape.family == RolloutFamily::Loop) {      // one kernel, every law at run time (LQR / TrackingLQR, friction, noise, PID); newton_mode 1 under any of them
        HIPCHK(launch_rollout_loop(a, m->shape, newton_mode, (hipStream_t)stream));
        return CCLQR_OK;
    }
    if (newton_mode != 0 && law != ControlLaw::Lqr)
        return fail(CCLQR_EUNSUPPORTED, "newton_mode 1 exists under the plain LQR / TrackingLQR law only on chains and branching trees (closed-loop mechanisms: every law)");
    if (m->shape.family == RolloutFamily::Tree) HIPCHK(launch_rollout_treereg(a, m->shape, m->simds, law, newton_mode, (hipStream_t)stream));
    else HIPCHK(launch_rollout_chain(a, m->shape, m->simds, law, newton_mode, opts && (opts->flags & CCLQR_ROLLOUT_RUNTIME_PLAN), (hipStream_t)stream));
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_ex(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const double* z0,
                                double* lam, const double* noise, int64_t noise_stride, double* traj, double* zT, int32_t* status,
                                const cclqr_rollout_opts* opts, void* stream) {
    return cclqr_rollout_plants(m, nullptr, c, n_inst, steps, k0, z0, lam, noise, noise_stride, traj, zT, status, opts, stream);
}

// Per-instance plants: upload (host pointers) or read in place (device pointers) the caller-order arrays, pack and validate them on the device
// (plants.hip), read the first-error word back once.
extern "C" int cclqr_plants_create(const cclqr_mech* m, int64_t n_plant, int64_t first_index, const double* mass, const double* inertia, const double* p1,
                                   const double* p2, int32_t on_device, void* stream, cclqr_plants** out) {
    if (!m || !out) return fail(CCLQR_EINVAL, "null argument");
    if (n_plant < 1 || first_index < 0) return fail(CCLQR_EINVAL, "need n_plant >= 1 and first_index >= 0");
    if (n_plant * (int64_t)(m ? m->nb : 1) >= (int64_t)1 << 31) return fail(CCLQR_EUNSUPPORTED, "a plant table holds fewer than 2^31 (plant, link) records (256 GB)");
    TRY(check_device(m));
    if (m->host.loop) return fail(CCLQR_EUNSUPPORTED, "per-instance plants are for forests of chains and branching trees (closed-loop mechanisms run their own plant)");
    const size_t nb = (size_t)m->nb, np = (size_t)n_plant;
    hipStream_t st = (hipStream_t)stream;
    const double* src[4] = {mass, inertia, p1, p2};
    const size_t per[4] = {nb, 9 * nb, 3 * nb, 3 * nb};
    unsigned long long* derr = nullptr;
    WsScope scope;
    HIPTRY("plants upload", ws_get((void**)&derr, sizeof(unsigned long long)));
    for (int k = 0; k < 4 && !on_device; k++) {
        if (!src[k]) continue;
        double* d = nullptr;
        HIPTRY("plants upload", ws_get((void**)&d, np * per[k] * sizeof(double)));
        HIPTRY("plants upload", hipMemcpyAsync(d, src[k], np * per[k] * sizeof(double), hipMemcpyHostToDevice, st));
        src[k] = d;
    }
    Owned<cclqr_plants, cclqr_plants_destroy> own(new cclqr_plants());
    cclqr_plants* P = own.p;
    P->dev = nullptr; P->n_plant = n_plant; P->first_index = first_index; P->mech = m; P->nb = m->nb; P->device = m->device;
    unsigned long long herr = ~0ull;
    HIPTRY("plants upload", hipMalloc((void**)&P->dev, np * nb * sizeof(PlantRec)));
    HIPTRY("plants upload", hipMemcpyAsync(derr, &herr, sizeof(herr), hipMemcpyHostToDevice, st));
    HIPTRY("plants upload", launch_plants_pack(m->dev, m->nb, n_plant, src[0], src[1], src[2], src[3], P->dev, derr, st));
    HIPTRY("plants upload", hipMemcpyAsync(&herr, derr, sizeof(herr), hipMemcpyDeviceToHost, st));
    HIPTRY("plants upload", hipStreamSynchronize(st));
    if (herr != ~0ull) {
        const unsigned long long pb = herr / 4;
        static const char* what[3] = {"a non-finite value", "mass must be positive", "inertia must be symmetric positive definite"};
        return fail(CCLQR_EINVAL, "plant " + std::to_string(pb / nb) + ", body " + std::to_string(pb % nb) + ": " + what[herr % 4 < 3 ? herr % 4 : 0]);
    }
    *out = own.release();
    return CCLQR_OK;
}

extern "C" int cclqr_plants_destroy(cclqr_plants* p) {
    if (!p) return CCLQR_OK;
    if (p->dev) (void)hipFree(p->dev);
    delete p;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_dev(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const double* z0,
                                 double* lam, const double* noise, int64_t noise_stride, double* traj, double* zT, int32_t* status,
                                 void* stream) {
    return cclqr_rollout_ex(m, c, n_inst, steps, k0, z0, lam, noise, noise_stride, traj, zT, status, nullptr, stream);
}

extern "C" int cclqr_ctrl_reserve_noise(cclqr_ctrl* c, int64_t n_inst, int32_t steps) {
    if (!c || n_inst < 0 || steps < 0) return fail(CCLQR_EINVAL, "bad argument");
    const size_t need = (size_t)n_inst * steps;
    if (c->noise_ws_cap >= need) return CCLQR_OK;
    {   // the block lives on the handle's device: growing it from a thread that is on another one would drain and allocate there
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return fail(CCLQR_EHIP, "hipGetDevice failed");
        if (dev != c->device) return fail(CCLQR_EINVAL, "the controller was created on device " + std::to_string(c->device) + ", the calling thread is on device " + std::to_string(dev));
    }
    // a launch that still reads the old block may be in flight on some stream: the device is drained before the block is replaced
    HIPCHK(hipDeviceSynchronize());
    if (c->noise_ws) HIPCHK(hipFree(c->noise_ws));
    c->noise_ws = nullptr; c->noise_ws_cap = 0;
    HIPCHK(hipMalloc((void**)&c->noise_ws, (need ? need : 1) * sizeof(double)));
    c->noise_ws_cap = need;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_host_ex(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const double* z0,
                                     const double* noise, double* traj, double* zT, int32_t* status, const cclqr_rollout_opts* opts) {
    if (m && c && n_inst == 0) return CCLQR_OK;   // empty batch
    if (!m || !c || !z0 || !zT) return fail(CCLQR_EINVAL, "null argument");
    if (opts && (opts->pid_state_dev || opts->noise_ws_dev)) return fail(CCLQR_EINVAL, "the host-pointer rollout takes no device buffers in its options");
    TRY(check_device(m));
    if (n_inst < 0 || steps < 0 || k0 < 1) return fail(CCLQR_EINVAL, "bad sizes");      // (rollout_check_args' rule: the staging below is sized by them)
    const size_t nz = (size_t)13 * m->nb;
    double *dz0 = nullptr, *dzT = nullptr, *dtraj = nullptr, *dnoise = nullptr;
    int32_t* dst = nullptr;
    WsScope scope;
    HIPTRY("rollout", ws_get((void**)&dz0, n_inst * nz * sizeof(double)));
    HIPTRY("rollout", ws_get((void**)&dzT, n_inst * nz * sizeof(double)));
    HIPTRY("rollout", ws_get((void**)&dst, n_inst * sizeof(int32_t)));
    if (traj) HIPTRY("rollout", ws_get((void**)&dtraj, n_inst * steps * nz * sizeof(double)));
    if (noise) HIPTRY("rollout", ws_get((void**)&dnoise, (size_t)n_inst * steps * sizeof(double)));
    HIPTRY("rollout", hipMemcpy(dz0, z0, n_inst * nz * sizeof(double), hipMemcpyHostToDevice));
    if (noise) HIPTRY("rollout", hipMemcpy(dnoise, noise, (size_t)n_inst * steps * sizeof(double), hipMemcpyHostToDevice));
    // noise is indexed by the absolute step k-1: shift the base so that k0 maps to column 0 of the caller's array
    const double* nbase = dnoise ? dnoise - (k0 - 1) : nullptr;
    TRY(cclqr_rollout_ex(m, c, n_inst, steps, k0, dz0, nullptr, nbase, steps, dtraj, dzT, dst, opts, nullptr));
    HIPTRY("rollout", hipDeviceSynchronize());
    HIPTRY("rollout", hipMemcpy(zT, dzT, n_inst * nz * sizeof(double), hipMemcpyDeviceToHost));
    if (traj) HIPTRY("rollout", hipMemcpy(traj, dtraj, n_inst * steps * nz * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIPTRY("rollout", hipMemcpy(status, dst, n_inst * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CCLQR_OK;
}

extern "C" int cclqr_rollout(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, const double* z0,
                             const double* noise, double* traj, double* zT, int32_t* status) {
    return cclqr_rollout_host_ex(m, c, n_inst, steps, k0, z0, noise, traj, zT, status, nullptr);
}

extern "C" int cclqr_linearize(const cclqr_mech* m, int32_t nk, const double* zd, int32_t mu, const int32_t* ctrl_joint, const double* Fd,
                               double* A, double* Bu, double* Bl, double* G) {
    return cclqr_linearize_plants(m, nullptr, 0, nk, zd, mu, ctrl_joint, Fd, A, Bu, Bl, G);
}

extern "C" int cclqr_linearize_plants(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t nk, const double* zd, int32_t mu,
                                      const int32_t* ctrl_joint, const double* Fd, double* A, double* Bu, double* Bl, double* G) {
    if (!m || !zd || !A || !Bl || !G || (mu > 0 && (!ctrl_joint || !Bu))) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    // a closed-loop mechanism has its own tables (bodies and joints in the caller's order, ml = 5 rows per joint incl. the two null rows of a
    // FixedOrientation); its G*Bl is singular, so the recursion takes the projected pair of cclqr_linearize_projected, not these four
    const int nj = m->host.loop ? m->nj : m->nb;
    const size_t n = (size_t)nk, mx = 12 * (size_t)m->nb, ml = 5 * (size_t)nj;
    if (nk < 0 || mu < 0 || mu > nj) return fail(CCLQR_EINVAL, "Missmatched length for constraints");
    WsScope scope;
    LinWs w = {};
    TRY(linearize_to_ws(m, plants, first_plant, nk, zd, Fd, mu, ctrl_joint, w, "linearize"));
    if (nk == 0) return CCLQR_OK;
    HIPTRY("linearize", hipDeviceSynchronize());
    HIPTRY("linearize", hipMemcpy(A, w.A, n * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    if (mu > 0) HIPTRY("linearize", hipMemcpy(Bu, w.Bu, n * mx * mu * sizeof(double), hipMemcpyDeviceToHost));
    HIPTRY("linearize", hipMemcpy(Bl, w.Bl, n * mx * ml * sizeof(double), hipMemcpyDeviceToHost));
    HIPTRY("linearize", hipMemcpy(G, w.G, n * ml * mx * sizeof(double), hipMemcpyDeviceToHost));
    long long bad = -1;
    HIPTRY("linearize", knots_converged(w.status, n, &bad));
    return bad < 0 ? CCLQR_OK : knot_not_converged(bad);
}

// ---- projected linear model by central differences of the DEVICE step map (any topology; the only linearisation of closed loops)
static inline void h_qmul(const double* a, const double* b, double* o) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
// difference quotients of the perturbed single-step results, on the device: thread = (knot, column, body).  Error coordinates of a
// state about the nominal next state, per body x, v, q~ = vec(q0^-1 q), w  (lqr.jl:92-103)
__global__ void fd_quotient_kernel(const double* zT, int nk, int per, int nb, int mu, double h, double* Ap, double* D) {
    const int mx = 12 * nb, ncol = mx + mu;
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)nk * ncol * nb) return;
    const int b = (int)(id % nb), col = (int)((id / nb) % ncol), k = (int)(id / ((long long)nb * ncol));
    const size_t nz = 13 * (size_t)nb;
    const double* z0 = zT + ((size_t)k * per) * nz + 13 * b;
    const double* zp = zT + ((size_t)k * per + 1 + 2 * col) * nz + 13 * b;
    const double* zm = zp + nz;
    const double qc[4] = {z0[3], -z0[4], -z0[5], -z0[6]};
    double qp[4], qm[4], e[12];
    qmul(qc, zp + 3, qp);
    qmul(qc, zm + 3, qm);
    for (int i = 0; i < 3; i++) {
        e[i] = zp[i] - zm[i]; e[3 + i] = zp[7 + i] - zm[7 + i]; e[6 + i] = qp[1 + i] - qm[1 + i]; e[9 + i] = zp[10 + i] - zm[10 + i];
    }
    for (int i = 0; i < 12; i++) {
        const double v = e[i] / (2.0 * h);
        const int r = 12 * b + i;
        if (col < mx) Ap[((size_t)k * mx + r) * mx + col] = v;
        else D[((size_t)k * mx + r) * mu + (col - mx)] = v;
    }
}
// The projected pair ANALYTICALLY (h <= 0): the exact Jacobians of the one-step map with the multipliers exogenous -- linearize_kernel for
// trees, linearize_loop_kernel (cclqr_lin_loop.h) for closed loops, nothing leaves the device -- and then the multipliers eliminated by
// project_model_kernel, whose complete pivoting stops at the numerical rank of G Bl (singular for a loop: redundant constraint rows).  The caller has
// checked that both kernels fit LDS.
static int linearize_projected_analytic(const cclqr_mech* m, int32_t nk, const double* zd, int32_t mu, const int32_t* ctrl_joint, const double* Fd,
                                        double* Ap, double* D) {
    static const char* const what = "linearize_projected";
    const int mx = 12 * m->nb, ml = 5 * (m->host.loop ? m->nj : m->nb);
    const size_t n = (size_t)nk, mu1 = (size_t)(mu > 0 ? mu : 1);
    double *dAp = nullptr, *dD = nullptr, *dres = nullptr;
    int* drank = nullptr;
    std::vector<double> res(nk);
    WsScope scope;
    HIPTRY(what, ws_get((void**)&dAp, n * mx * mx * sizeof(double)));      // every block before the upload: no allocation between the two launches
    HIPTRY(what, ws_get((void**)&dD, n * mx * mu1 * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dres, n * sizeof(double)));
    HIPTRY(what, ws_get((void**)&drank, n * sizeof(int)));
    LinWs w = {};
    TRY(linearize_to_ws(m, nullptr, 0, nk, zd, Fd, mu, ctrl_joint, w, what));
    HIPTRY(what, launch_project_model(nk, mx, mu, ml, w.A, w.Bu, w.Bl, w.G, dAp, dD, dres, drank, nullptr));
    HIPTRY(what, hipDeviceSynchronize());
    HIPTRY(what, hipMemcpy(Ap, dAp, n * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    if (mu > 0) HIPTRY(what, hipMemcpy(D, dD, n * mx * mu * sizeof(double), hipMemcpyDeviceToHost));
    long long bad = -1;
    HIPTRY(what, knots_converged(w.status, n, &bad));
    HIPTRY(what, hipMemcpy(res.data(), dres, n * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < nk; k++) {
        if (k == bad) return knot_not_converged(k);
        if (!(res[k] < 1e-6)) return fail(CCLQR_ESINGULAR, "the constraint rows of the linear model are inconsistent at knot " + std::to_string(k) + " (G Bl rank-deficient beyond redundancy)");
    }
    return CCLQR_OK;
}

extern "C" int cclqr_linearize_projected(const cclqr_mech* m, int32_t nk, const double* zd, int32_t mu, const int32_t* ctrl_joint, const double* Fd,
                                         double h, double* Ap, double* D) {
    if (!m || !zd || !Ap || (mu > 0 && (!ctrl_joint || !D))) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (nk < 0 || mu < 0 || mu > m->nj) return fail(CCLQR_EINVAL, "Missmatched length for constraints");
    if (nk == 0) return CCLQR_OK;
    static const char* const what = "linearize_projected";
    const int nb = m->nb, mx = 12 * nb;
    if (!(h > 0.0)) {
        // the analytic projection keeps [G Bl | G A | G Bu] of a knot in one CU's LDS (project_model_kernel): 175 KB for a 16-body tree, 198 KB for
        // the 17-body headline chain.  What does not fit is differenced instead (the h > 0 form with its documented step), so that the default
        // call is defined for every mechanism cclqr_mech_create takes
        const int nj = m->host.loop ? m->nj : nb;
        const bool fits = project_model_fits(mx, mu, 5 * nj) && linearize_fits_lds(m);
        if (fits) return linearize_projected_analytic(m, nk, zd, mu, ctrl_joint, Fd, Ap, D);
        h = 1e-6;
    }
    const size_t nz = 13 * (size_t)nb;
    const int per = 1 + 2 * mx + 2 * mu;            // nominal, +-h in every state error coordinate, +-h in every input
    const size_t n = (size_t)nk * per;
    std::vector<double> z0(n * nz), fd(n * (size_t)(mu > 0 ? mu : 1), 0.0), zdum(n * nz, 0.0);
    std::vector<int32_t> st(n);
    for (size_t i = 0; i < n; i++)
        for (int b = 0; b < nb; b++) zdum[i * nz + 13 * b + 3] = 1.0;
    for (int k = 0; k < nk; k++) {
        const double* zk = zd + (size_t)k * nz;
        for (int q = 0; q < per; q++) {
            double* z = &z0[((size_t)k * per + q) * nz];
            memcpy(z, zk, nz * sizeof(double));
            for (int i = 0; i < mu; i++) fd[((size_t)k * per + q) * mu + i] = Fd ? Fd[(size_t)k * mu + i] : 0.0;
            if (q >= 1 && q <= 2 * mx) {
                const int col = (q - 1) >> 1, b = col / 12, e = col % 12;
                const double s = ((q - 1) & 1) ? -h : h;
                double* p = z + 13 * b;
                if (e < 3) p[e] += s;
                else if (e < 6) p[7 + e - 3] += s;
                else if (e < 9) {                       // q = qd (sqrt(1 - s^2), s e_i): vec(qd^-1 q) = s e_i exactly
                    double dq[4] = {sqrt(1.0 - s * s), 0.0, 0.0, 0.0}, qn[4];
                    dq[1 + e - 6] = s;
                    h_qmul(zk + 13 * b + 3, dq, qn);
                    for (int i = 0; i < 4; i++) p[3 + i] = qn[i];
                } else p[10 + e - 9] += s;
            } else if (q > 2 * mx) {
                const int i = (q - 1 - 2 * mx) >> 1;
                fd[((size_t)k * per + q) * mu + i] += ((q - 1) & 1) ? -h : h;
            }
        }
    }
    cclqr_ctrl_desc cd;
    memset(&cd, 0, sizeof(cd));
    cd.mu = mu; cd.ctrl_joint = ctrl_joint; cd.nK = 0; cd.N = 0; cd.K = nullptr; cd.nsp = 1; cd.zd = zdum.data(); cd.Fd = mu > 0 ? fd.data() : nullptr;
    cd.n_ctrl = (int32_t)n;
    cclqr_ctrl* c = nullptr;
    TRY(cclqr_ctrl_create(m, &cd, &c));
    CtrlOwner own(c);
    double *dz0 = nullptr, *dzT = nullptr, *dAp = nullptr, *dD = nullptr;
    int32_t* dst = nullptr;
    WsScope scope;
    HIPTRY(what, ws_get((void**)&dz0, n * nz * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dzT, n * nz * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dst, n * sizeof(int32_t)));
    HIPTRY(what, ws_get((void**)&dAp, (size_t)nk * mx * mx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dD, (size_t)nk * mx * (size_t)(mu > 0 ? mu : 1) * sizeof(double)));
    HIPTRY(what, hipMemcpy(dz0, z0.data(), n * nz * sizeof(double), hipMemcpyHostToDevice));
    TRY(cclqr_rollout_ex(m, c, (int64_t)n, 1, 1, dz0, nullptr, nullptr, 0, nullptr, dzT, dst, nullptr, nullptr));
    const long long work = (long long)nk * (mx + mu) * nb;
    HIPTRY(what, launch_lds<false>(fd_quotient_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, nullptr, dzT, nk, per, nb, mu, h, dAp, dD));
    HIPTRY(what, hipDeviceSynchronize());
    HIPTRY(what, hipMemcpy(st.data(), dst, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPTRY(what, hipMemcpy(Ap, dAp, (size_t)nk * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    if (mu > 0) HIPTRY(what, hipMemcpy(D, dD, (size_t)nk * mx * mu * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        if (st[i] <= 0) return fail(CCLQR_ENOCONV, "Newton did not converge at a perturbed setpoint of knot " + std::to_string(i / per));
    return CCLQR_OK;
}

// shared tail of the dlqr entry points: run the recursion on device-resident (A,Bu,Bl,G) inside the caller's WsScope, download K and kbreak.  Q, R: n_weights = 1
// pair shared by the problems, or nprob pairs (the caller has checked: check_n_weights).  P: host [nprob][mx][mx] for the cost-to-go (RicArgs.P_out), or null
static int run_riccati(int nprob, int mx, int mu, int ml, int N, int time_varying, double tol, const double* dA, const double* dBu,
                       const double* dBl, const double* dG, int n_weights, const double* Q, const double* R, double* K, int32_t* kbreak,
                       const cclqr_riccati_opts* opts, double* P = nullptr) {
    const int keep_last = (opts && opts->keep_last) ? 1 : 0;
    const size_t nK = (size_t)nprob * (N > 1 ? (keep_last ? 1 : N - 1) : 0) * mu * mx;
    const size_t nP = (size_t)nprob * mx * mx;
    double *dQ = nullptr, *dR = nullptr, *dK = nullptr, *dwork = nullptr, *dP = nullptr;
    int *dkb = nullptr, *dst = nullptr, *dstop = nullptr;
    std::vector<int> st(nprob), kb(nprob);
    RicArgs a;
    a.nprob = nprob; a.mx = mx; a.mu = mu; a.ml = ml; a.N = N; a.time_varying = time_varying; a.tol = tol;
    a.path = opts ? opts->path : 0;
    a.bf16_terms = opts ? opts->bf16_terms : 0;
    a.keep_last = keep_last;
    a.p_rows = ric_p_rows(Q, mx, R, mu);
    ric_per_problem_weights(a, Q, R, n_weights);
    const size_t nw = (size_t)n_weights;
    if (a.path < 0 || a.path > 2 || a.bf16_terms < 0 || a.bf16_terms > 3) return fail(CCLQR_EINVAL, "riccati options: path in 0..2, bf16_terms in 0..3");
    HIPTRY("riccati", ws_get((void**)&dQ, nw * mx * mx * sizeof(double)));
    HIPTRY("riccati", ws_get((void**)&dR, (nw * mu * mu + 1) * sizeof(double)));
    HIPTRY("riccati", ws_get((void**)&dK, (nK + 1) * sizeof(double)));
    HIPTRY("riccati", ws_get((void**)&dwork, ric_total_work_doubles(a) * sizeof(double)));
    HIPTRY("riccati", ws_get((void**)&dstop, nprob * sizeof(int)));
    HIPTRY("riccati", ws_get((void**)&dkb, nprob * sizeof(int)));
    HIPTRY("riccati", ws_get((void**)&dst, nprob * sizeof(int)));
    if (P) HIPTRY("riccati", ws_get((void**)&dP, nP * sizeof(double)));
    HIPTRY("riccati", hipMemcpy(dQ, Q, nw * mx * mx * sizeof(double), hipMemcpyHostToDevice));
    if (mu > 0) HIPTRY("riccati", hipMemcpy(dR, R, nw * mu * mu * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY("riccati", hipMemset(dK, 0, (nK + 1) * sizeof(double)));
    a.stop = dstop;
    a.A = dA; a.Bu = dBu; a.Bl = dBl; a.G = dG; a.Q = dQ; a.R = dR; a.K = dK; a.kbreak = dkb; a.status = dst; a.work = dwork;
    a.P_out = dP;
    HIPTRY("riccati", launch_riccati(a, nullptr));
    HIPTRY("riccati", hipDeviceSynchronize());
    if (nK) HIPTRY("riccati", hipMemcpy(K, dK, nK * sizeof(double), hipMemcpyDeviceToHost));
    if (P) HIPTRY("riccati", hipMemcpy(P, dP, nP * sizeof(double), hipMemcpyDeviceToHost));
    HIPTRY("riccati", hipMemcpy(kb.data(), dkb, nprob * sizeof(int), hipMemcpyDeviceToHost));
    HIPTRY("riccati", hipMemcpy(st.data(), dst, nprob * sizeof(int), hipMemcpyDeviceToHost));
    for (int p = 0; p < nprob; p++) {
        if (kbreak) kbreak[p] = kb[p];
        if (st[p] != 0) return fail(CCLQR_ESINGULAR, "G*Bl or M is singular in problem " + std::to_string(p));
    }
    return CCLQR_OK;
}

// `count` host models (A, Bu, Bl, G) into the calling thread's workspace for run_riccati (one per problem, or one per knot of a time-varying problem)
struct RicModels { double *A, *Bu, *Bl, *G; };
static int upload_models(size_t count, size_t mx, size_t mu, size_t ml, const double* A, const double* Bu, const double* Bl, const double* G, RicModels& d) {
    static const char* const what = "riccati upload";
    HIPTRY(what, ws_get((void**)&d.A, count * mx * mx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&d.Bu, (count * mx * mu + 1) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&d.Bl, (count * mx * ml + 1) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&d.G, (count * ml * mx + 1) * sizeof(double)));
    HIPTRY(what, hipMemcpy(d.A, A, count * mx * mx * sizeof(double), hipMemcpyHostToDevice));
    if (mu > 0) HIPTRY(what, hipMemcpy(d.Bu, Bu, count * mx * mu * sizeof(double), hipMemcpyHostToDevice));
    if (ml > 0) HIPTRY(what, hipMemcpy(d.Bl, Bl, count * mx * ml * sizeof(double), hipMemcpyHostToDevice));
    if (ml > 0) HIPTRY(what, hipMemcpy(d.G, G, count * ml * mx * sizeof(double), hipMemcpyHostToDevice));
    return CCLQR_OK;
}

extern "C" int cclqr_riccati(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl,
                             const double* G, const double* Q, const double* R, int32_t N, double tol, double* K, int32_t* kbreak) {
    return cclqr_riccati_ex(nprob, mx, mu, ml, A, Bu, Bl, G, Q, R, N, tol, K, kbreak, nullptr);
}

extern "C" int cclqr_riccati_ex(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl,
                                const double* G, const double* Q, const double* R, int32_t N, double tol, double* K, int32_t* kbreak,
                                const cclqr_riccati_opts* opts) {
    return cclqr_riccati_weights(nprob, mx, mu, ml, A, Bu, Bl, G, 1, Q, R, N, tol, K, kbreak, opts);
}

extern "C" int cclqr_riccati_value(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                   int32_t n_weights, const double* Q, const double* R, int32_t N, double tol, int32_t time_varying, double* K, double* P,
                                   int32_t* kbreak, const cclqr_riccati_opts* opts) {
    const int tv = time_varying != 0;
    if (!A || !Q || (mu > 0 && (!Bu || !R)) || (ml > 0 && (!Bl || !G)) || !K) return fail(CCLQR_EINVAL, "null argument");
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0 || N < (tv ? 2 : 1)) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_weights(n_weights, nprob, "problem"));
    WsScope scope;
    RicModels d = {};
    TRY(upload_models((size_t)nprob * (tv ? (size_t)N - 1 : 1), mx, mu, ml, A, Bu, Bl, G, d));      // one model per problem, or per knot of every problem
    return run_riccati(nprob, mx, mu, ml, N, tv, tol, d.A, d.Bu, d.Bl, d.G, n_weights, Q, R, K, kbreak, opts, P);
}

extern "C" int cclqr_riccati_weights(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl,
                                     const double* G, int32_t n_weights, const double* Q, const double* R, int32_t N, double tol, double* K,
                                     int32_t* kbreak, const cclqr_riccati_opts* opts) {
    return cclqr_riccati_value(nprob, mx, mu, ml, A, Bu, Bl, G, n_weights, Q, R, N, tol, 0, K, nullptr, kbreak, opts);
}

extern "C" int cclqr_riccati_tv(int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                const double* Q, const double* R, int32_t N, double tol, double* K, int32_t* kbreak) {
    return cclqr_riccati_value(1, mx, mu, ml, A, Bu, Bl, G, 1, Q, R, N, tol, 1, K, nullptr, kbreak, nullptr);
}

extern "C" int cclqr_riccati_tracking(const cclqr_mech* m, int32_t mu, const int32_t* ctrl_joint, const double* zd, const double* Fd,
                                      const double* Q, const double* R, int32_t N, double tol, double* K, int32_t* kbreak) {
    return cclqr_riccati_tracking_ex(m, mu, ctrl_joint, zd, Fd, Q, R, N, tol, K, kbreak, nullptr);
}

extern "C" int cclqr_riccati_tracking_ex(const cclqr_mech* m, int32_t mu, const int32_t* ctrl_joint, const double* zd, const double* Fd,
                                         const double* Q, const double* R, int32_t N, double tol, double* K, int32_t* kbreak,
                                         const cclqr_riccati_opts* opts) {
    if (!m || !zd || !Q || !K || (mu > 0 && (!ctrl_joint || !R))) return fail(CCLQR_EINVAL, "null argument");
    if (m->host.loop) return fail(CCLQR_EUNSUPPORTED, "TrackingLQR of a closed-loop mechanism is outside this build's scope");
    if (N < 2 || mu < 0 || mu > m->nb) return fail(CCLQR_EINVAL, "bad sizes");
    // knots 1..N-1 (lqr_tracking.jl:87-88): linearise all of them in one launch, keep the matrices on the device
    WsScope scope;
    LinWs w = {};
    TRY(linearize_to_ws(m, nullptr, 0, N - 1, zd, Fd, mu, ctrl_joint, w, "riccati_tracking"));
    long long bad = -1;
    HIPTRY("riccati_tracking", knots_converged(w.status, (size_t)N - 1, &bad));
    if (bad >= 0) return knot_not_converged(bad);
    return run_riccati(1, 12 * m->nb, mu, 5 * m->nb, N, 1, tol, w.A, w.Bu, w.Bl, w.G, 1, Q, R, K, kbreak, opts);
}

// ---- scoring a rollout on the device (score.hip).  The weights are permuted ONCE, here: traj rows stay in the caller's body order, the controller's K columns
// and setpoints are in link order (build_ctrl_tables), so the per-body blocks go to link order with them (closed loops: perm is the identity)
extern "C" int cclqr_score_create(const cclqr_mech* m, const double* Qb, int32_t mu, const double* R, double settle_tol, cclqr_score** out) {
    if (!m || !Qb || !out || (mu > 0 && !R)) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (mu < 0 || mu > m->nj) return fail(CCLQR_EINVAL, "mu = " + std::to_string(mu) + " is not a number of controlled joints of this mechanism (0 .. " + std::to_string(m->nj) + ")");
    if (!std::isfinite(settle_tol)) return fail(CCLQR_EINVAL, "settle_tol is not finite");
    const int nb = m->nb;
    for (size_t e = 0; e < (size_t)nb * 144; e++)
        if (!std::isfinite(Qb[e])) return fail(CCLQR_EINVAL, "a weight is not finite: Qb of body " + std::to_string(e / 144) + ", entry " + std::to_string(e % 144));
    for (size_t e = 0; e < (size_t)mu * mu; e++)
        if (!std::isfinite(R[e])) return fail(CCLQR_EINVAL, "a weight is not finite: R entry " + std::to_string(e));
    std::vector<double> Ql((size_t)nb * 144);
    for (int l = 0; l < nb; l++) memcpy(&Ql[(size_t)l * 144], Qb + (size_t)m->host.perm[l] * 144, 144 * sizeof(double));
    Owned<cclqr_score, cclqr_score_destroy> own(new cclqr_score());
    cclqr_score* s = own.p;
    memset(s, 0, sizeof(*s));
    s->settle_tol = settle_tol; s->nb = nb; s->mu = mu; s->device = m->device; s->mech = m;
    HIPTRY("score weights upload", hipMalloc((void**)&s->Qb_dev, Ql.size() * sizeof(double)));
    HIPTRY("score weights upload", hipMemcpy(s->Qb_dev, Ql.data(), Ql.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPTRY("score weights upload", hipMalloc((void**)&s->R_dev, ((size_t)mu * mu + 1) * sizeof(double)));
    if (mu > 0) HIPTRY("score weights upload", hipMemcpy(s->R_dev, R, (size_t)mu * mu * sizeof(double), hipMemcpyHostToDevice));
    *out = own.release();
    return CCLQR_OK;
}

extern "C" int cclqr_score_destroy(cclqr_score* s) {
    if (!s) return CCLQR_OK;
    if (s->Qb_dev) (void)hipFree(s->Qb_dev);
    if (s->R_dev) (void)hipFree(s->R_dev);
    delete s;
    return CCLQR_OK;
}

extern "C" int cclqr_rollout_score(const cclqr_mech* m, const cclqr_ctrl* c, const cclqr_score* s, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance,
                                   const double* traj, double* score, void* stream) {
    if (!m || !c || !s) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (s->mech != m || s->nb != m->nb || s->device != m->device) return fail(CCLQR_EINVAL, "the score weights were created for another mechanism or device");
    if (c->nb != m->nb || c->device != m->device) return fail(CCLQR_EINVAL, "the controller was created for another mechanism or device");
    if (steps < 1 || k0 < 1) return fail(CCLQR_EINVAL, "need steps >= 1 and k0 >= 1 (got steps = " + std::to_string(steps) + ", k0 = " + std::to_string(k0) + ")");
    if (n_inst < 0 || first_instance < 0) return fail(CCLQR_EINVAL, "negative n_inst or first_instance");
    if (s->mu != c->host.mu) return fail(CCLQR_EINVAL, "mu of the score weights (" + std::to_string(s->mu) + ") differs from the controller's (" + std::to_string(c->host.mu) + ")");
    if (!c->zd_dev || c->host.nsp < 1) return fail(CCLQR_EINVAL, "the controller has no setpoint table");
    if (c->host.n_ctrl > 1 && first_instance + n_inst > c->host.n_ctrl)
        return fail(CCLQR_EINVAL, "first_instance + n_inst = " + std::to_string(first_instance + n_inst) + " exceeds the controller's n_ctrl = " + std::to_string(c->host.n_ctrl) + " tables");
    if (n_inst == 0) return CCLQR_OK;
    if (!traj || !score) return fail(CCLQR_EINVAL, "null argument");
    ScoreArgs a;
    a.M = m->dev; a.C = c->dev; a.Qb = s->Qb_dev; a.R = s->R_dev; a.settle_tol = s->settle_tol; a.nb = m->nb; a.mu = s->mu;
    a.n_inst = n_inst; a.steps = steps; a.k0 = k0; a.inst0 = first_instance; a.traj = traj; a.score = score;
    HIPCHK(launch_score(a, (hipStream_t)stream));
    return CCLQR_OK;
}

// ---- the statistics of a slab across its instances (ensemble.hip).  Nothing is allocated, copied or synchronised: the listed steps travel in the kernels' arguments
// and everything between the kernels lies in the caller's workspace
static int ensemble_sizes_ok(const cclqr_mech* m, int32_t mu, int64_t n_inst, int32_t steps, int32_t n_cov) {
    if (mu < 0 || mu > m->nj) return fail(CCLQR_EINVAL, "mu = " + std::to_string(mu) + " is not a number of controlled joints of this mechanism (0 .. " + std::to_string(m->nj) + ")");
    if (n_inst < 1) return fail(CCLQR_EINVAL, "n_inst = " + std::to_string(n_inst) + ": an ensemble holds at least one instance");
    if (steps < 1) return fail(CCLQR_EINVAL, "need steps >= 1 (got " + std::to_string(steps) + ")");
    if (n_cov < 0 || n_cov > ENS_MAX_COV) return fail(CCLQR_EINVAL, "n_cov = " + std::to_string(n_cov) + ": one call takes 0 .. " + std::to_string(ENS_MAX_COV) + " listed steps");
    if (ens_tiles(n_inst) * steps > 0x7fffffffLL || ens_splits(n_inst) > 65535) return fail(CCLQR_EINVAL, "n_inst x steps exceeds one launch: call with fewer steps");
    return CCLQR_OK;
}
// the handle, size and index checks every call over a slab's instances makes, in this order (cclqr_rollout_ensemble, cclqr_rollout_quantiles)
static int ensemble_call_ok(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, int32_t n_cov) {
    if (!m || !c) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (c->nb != m->nb || c->device != m->device) return fail(CCLQR_EINVAL, "the controller was created for another mechanism or device");
    TRY(ensemble_sizes_ok(m, c->host.mu, n_inst, steps, n_cov));
    if (k0 < 1 || first_instance < 0) return fail(CCLQR_EINVAL, "need k0 >= 1 and first_instance >= 0 (got k0 = " + std::to_string(k0) + ", first_instance = " + std::to_string(first_instance) + ")");
    if (!c->zd_dev || c->host.nsp < 1) return fail(CCLQR_EINVAL, "the controller has no setpoint table");
    if (c->host.n_ctrl > 1 && first_instance + n_inst > c->host.n_ctrl)
        return fail(CCLQR_EINVAL, "first_instance + n_inst = " + std::to_string(first_instance + n_inst) + " exceeds the controller's n_ctrl = " + std::to_string(c->host.n_ctrl) + " tables");
    return CCLQR_OK;
}
extern "C" int cclqr_rollout_ensemble_ws_bytes(const cclqr_mech* m, int32_t mu, int64_t n_inst, int32_t steps, int32_t n_cov, size_t* bytes) {
    if (!m || !bytes) return fail(CCLQR_EINVAL, "null argument");
    TRY(ensemble_sizes_ok(m, mu, n_inst, steps, n_cov));
    *bytes = sizeof(double) * ens_ws_doubles(m->nb, mu, n_inst, steps, n_cov);
    return CCLQR_OK;
}
extern "C" int cclqr_rollout_ensemble(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, const double* traj,
                                      double* mean, double* m2, int32_t n_cov, const int32_t* cov_steps, double* cov, void* ws, size_t ws_bytes, void* stream) {
    TRY(ensemble_call_ok(m, c, n_inst, steps, k0, first_instance, n_cov));
    if (!traj || !mean || !m2 || (n_cov > 0 && (!cov_steps || !cov))) return fail(CCLQR_EINVAL, "null argument");
    for (int q = 0; q < n_cov; q++)
        if (cov_steps[q] < k0 || cov_steps[q] > k0 + steps - 1)
            return fail(CCLQR_EINVAL, "cov_steps[" + std::to_string(q) + "] = " + std::to_string(cov_steps[q]) + " lies outside the launch's steps " + std::to_string(k0) + " .. " + std::to_string(k0 + steps - 1));
    const int nb = m->nb, mu = c->host.mu;
    const size_t need = sizeof(double) * ens_ws_doubles(nb, mu, n_inst, steps, n_cov);
    if (!ws) return fail(CCLQR_EINVAL, "null workspace: cclqr_rollout_ensemble_ws_bytes says how large it must be (" + std::to_string(need) + " bytes)");
    if (ws_bytes < need) return fail(CCLQR_EINVAL, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, " + std::to_string(need) + " needed (cclqr_rollout_ensemble_ws_bytes)");
    EnsArgs a;
    memset(&a, 0, sizeof(a));
    a.M = m->dev; a.C = c->dev; a.nb = nb; a.mu = mu; a.n_inst = n_inst; a.steps = steps; a.k0 = k0; a.inst0 = first_instance; a.traj = traj;
    a.part = (double*)ws;
    a.dzrows = n_cov > 0 ? a.part + ens_ws_part_doubles(nb, mu, n_inst, steps) : nullptr;
    a.n_cov = n_cov;
    for (int q = 0; q < n_cov; q++) a.cov_row[q] = cov_steps[q] - k0;
    HIPCHK(launch_ensemble(a, mean, m2, (hipStream_t)stream));
    if (n_cov == 0) return CCLQR_OK;
    EnsCovArgs v;
    memset(&v, 0, sizeof(v));
    v.mx = 12 * nb; v.tm = (v.mx + 31) / 32; v.n_inst = n_inst; v.nsplit = (int)ens_splits(n_inst); v.stride = ens_coords(nb, mu);
    v.dzrows = a.dzrows; v.mean = mean; v.cpart = a.dzrows + ens_ws_rows_doubles(nb, n_inst, n_cov); v.cov = cov;
    for (int q = 0; q < n_cov; q++) v.cov_row[q] = a.cov_row[q];
    HIPCHK(launch_ensemble_cov(v, n_cov, (hipStream_t)stream));
    return CCLQR_OK;
}

// ---- the quantiles of a slab across its instances (quantiles.hip).  Nothing is allocated, copied or synchronised: the probabilities travel in the kernels'
// arguments, and the rows are taken in blocks of as many as the caller's workspace holds -- a row's result does not know which block it was in
static int quantile_sizes_ok(const cclqr_mech* m, int32_t mu, int64_t n_inst, int32_t steps) {
    TRY(ensemble_sizes_ok(m, mu, n_inst, steps, 0));
    if (n_inst > CCLQR_QUANTILE_MAX_INST)
        return fail(CCLQR_EUNSUPPORTED, "n_inst = " + std::to_string(n_inst) + ": one call sorts at most CCLQR_QUANTILE_MAX_INST = " + std::to_string(CCLQR_QUANTILE_MAX_INST) + " instances");
    return CCLQR_OK;
}
extern "C" int cclqr_rollout_quantiles_ws_bytes(const cclqr_mech* m, int32_t mu, int64_t n_inst, int32_t steps, size_t* min_bytes, size_t* full_bytes) {
    if (!m || !min_bytes || !full_bytes) return fail(CCLQR_EINVAL, "null argument");
    TRY(quantile_sizes_ok(m, mu, n_inst, steps));
    *min_bytes = sizeof(double) * qnt_row_doubles(m->nb, mu, n_inst);
    *full_bytes = *min_bytes * (size_t)steps;
    return CCLQR_OK;
}
extern "C" int cclqr_rollout_quantiles(const cclqr_mech* m, const cclqr_ctrl* c, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, const double* traj,
                                       int32_t n_prob, const double* prob, double* quant, int32_t* finite, void* ws, size_t ws_bytes, void* stream) {
    TRY(ensemble_call_ok(m, c, n_inst, steps, k0, first_instance, 0));
    if (!traj || !prob || !quant) return fail(CCLQR_EINVAL, "null argument");
    if (n_prob < 1 || n_prob > CCLQR_QUANTILE_MAX_PROBS)
        return fail(CCLQR_EINVAL, "n_prob = " + std::to_string(n_prob) + ": one call takes 1 .. " + std::to_string(CCLQR_QUANTILE_MAX_PROBS) + " probabilities");
    for (int j = 0; j < n_prob; j++)
        if (!(prob[j] >= 0.0 && prob[j] <= 1.0)) return fail(CCLQR_EINVAL, "prob[" + std::to_string(j) + "] = " + std::to_string(prob[j]) + " is not a probability in [0, 1]");
    const int nb = m->nb, mu = c->host.mu;
    TRY(quantile_sizes_ok(m, mu, n_inst, steps));
    const size_t row_bytes = sizeof(double) * qnt_row_doubles(nb, mu, n_inst);
    if (!ws) return fail(CCLQR_EINVAL, "null workspace: cclqr_rollout_quantiles_ws_bytes says how large it must be (at least " + std::to_string(row_bytes) + " bytes)");
    if (ws_bytes < row_bytes) return fail(CCLQR_EINVAL, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, " + std::to_string(row_bytes) + " needed for one row (cclqr_rollout_quantiles_ws_bytes)");
    if (((uintptr_t)ws & 7) != 0) return fail(CCLQR_EINVAL, "the workspace is not 8-byte aligned");
    QntArgs a;
    memset(&a, 0, sizeof(a));
    a.M = m->dev; a.C = c->dev; a.nb = nb; a.mu = mu; a.n_inst = n_inst; a.n_pad = qnt_pad(n_inst); a.steps = steps; a.k0 = k0; a.inst0 = first_instance; a.traj = traj;
    a.W = qnt_stage_window(nb, mu); a.xt = (double*)ws; a.n_prob = n_prob; a.quant = quant; a.finite = finite;
    for (int j = 0; j < n_prob; j++) a.prob[j] = prob[j];
    const size_t fit = ws_bytes / row_bytes;
    const int block = (int)(fit < 65535 ? fit : 65535);      // (rows are the y extent of the select kernel's grid)
    for (int r0 = 0; r0 < steps; r0 += block) {
        a.row0 = r0; a.nrows = steps - r0 < block ? steps - r0 : block;
        HIPCHK(launch_quantiles(a, (hipStream_t)stream));
    }
    return CCLQR_OK;
}

// ---- the passes that turn a slab into per-instance series written at the absolute step (joints.hip, invariants.hip): the ONE sequence of refusals they share.
// slab_series_check: the device, the sizes, and -- where a series output is given -- that out_steps rows hold the steps of this launch
static int slab_series_check(const cclqr_mech* m, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, int64_t out_steps, bool series) {
    if (!m) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (n_inst < 1 || steps < 1 || k0 < 1)
        return fail(CCLQR_EINVAL, "need n_inst >= 1, steps >= 1 and k0 >= 1 (got n_inst = " + std::to_string(n_inst) + ", steps = " + std::to_string(steps) + ", k0 = " + std::to_string(k0) + ")");
    if (first_instance < 0) return fail(CCLQR_EINVAL, "negative first_instance");
    if (series && out_steps < (int64_t)k0 + steps - 1)
        return fail(CCLQR_EINVAL, "out_steps = " + std::to_string(out_steps) + " does not hold the steps " + std::to_string(k0) + " .. " + std::to_string((int64_t)k0 + steps - 1) + " of this launch");
    return CCLQR_OK;
}
// slab_plants_check: the plants are this mechanism's, on its device, and cover the launch's instances
static int slab_plants_check(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_instance, int64_t n_inst) {
    if (plants && (plants->nb != m->nb || plants->device != m->device)) return fail(CCLQR_EINVAL, "the plants were created for another mechanism or device");
    if (plants && m->shape.family == RolloutFamily::Loop) return fail(CCLQR_EINVAL, "the plants were created for another mechanism: a closed-loop mechanism takes none");
    return plants_check_range(m, plants, first_instance, n_inst, "instances", "launch");
}

// ---- the joint coordinates of a slab (joints.hip).  Nothing is allocated, copied or synchronised
extern "C" int cclqr_rollout_joints(const cclqr_mech* m, const cclqr_plants* plants, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, const double* traj,
                                    int32_t mode, int64_t out_steps, double* theta, double* rate, double* carry, void* stream) {
    TRY(slab_series_check(m, n_inst, steps, k0, first_instance, out_steps, true));
    if (mode != CCLQR_JOINTS_RAW && mode != CCLQR_JOINTS_CONTINUOUS) return fail(CCLQR_EINVAL, "mode = " + std::to_string(mode) + " is neither CCLQR_JOINTS_RAW nor CCLQR_JOINTS_CONTINUOUS");
    if (mode == CCLQR_JOINTS_CONTINUOUS && !carry) return fail(CCLQR_EINVAL, "CCLQR_JOINTS_CONTINUOUS needs carry_dev [n_inst][ne][2]: the turn count travels in it from launch to launch");
    if (!traj || !theta) return fail(CCLQR_EINVAL, "null traj_dev or theta_dev");
    TRY(slab_plants_check(m, plants, first_instance, n_inst));
    JointsArgs a;
    memset(&a, 0, sizeof(a));
    a.M = m->dev; a.plants = plants ? plants->dev : nullptr; a.plant_off = plants ? first_instance - plants->first_index : 0;
    a.nb = m->nb; a.ne = m->nj; a.loop = m->host.loop; a.n_inst = n_inst; a.steps = steps; a.k0 = k0; a.traj = traj; a.mode = mode; a.out_steps = out_steps;
    a.theta = theta; a.rate = rate; a.carry = mode == CCLQR_JOINTS_CONTINUOUS ? carry : nullptr;
    HIPCHK(launch_joints(a, (hipStream_t)stream));
    return CCLQR_OK;
}

// ---- the integrator's invariants of a slab (invariants.hip).  Nothing is allocated, copied or synchronised
extern "C" int cclqr_rollout_invariants(const cclqr_mech* m, const cclqr_plants* plants, int64_t n_inst, int32_t steps, int32_t k0, int64_t first_instance, const double* traj,
                                        int64_t out_steps, double* inv, double* rows, double* summary, void* stream) {
    TRY(slab_series_check(m, n_inst, steps, k0, first_instance, out_steps, inv || rows));
    if (!traj) return fail(CCLQR_EINVAL, "null traj_dev");
    if (!inv && !rows && !summary) return fail(CCLQR_EINVAL, "inv_dev, rows_dev and summary_dev are all NULL: the call would compute nothing");
    TRY(slab_plants_check(m, plants, first_instance, n_inst));
    InvArgs a;
    memset(&a, 0, sizeof(a));
    a.M = m->dev; a.plants = plants ? plants->dev : nullptr; a.plant_off = plants ? first_instance - plants->first_index : 0;
    a.nb = m->nb; a.ne = m->nj; a.loop = m->host.loop; a.n_inst = n_inst; a.steps = steps; a.k0 = k0; a.traj = traj; a.out_steps = out_steps;
    a.inv = inv; a.rows = rows; a.summary = summary;
    HIPCHK(launch_invariants(a, (hipStream_t)stream));
    return CCLQR_OK;
}

// ---- the statistics of any per-instance series across its instances (joints.hip in front of ens_finish_kernel / ens_select_kernel).  Nothing is allocated, copied
// or synchronised; the refusals and the workspace block rule are those of cclqr_rollout_ensemble / cclqr_rollout_quantiles
static int series_sizes_ok(int64_t n_inst, int32_t steps, int32_t nc) {
    if (n_inst < 1) return fail(CCLQR_EINVAL, "n_inst = " + std::to_string(n_inst) + ": an ensemble holds at least one instance");
    if (steps < 1) return fail(CCLQR_EINVAL, "need steps >= 1 (got " + std::to_string(steps) + ")");
    if (nc < 1 || nc > CCLQR_SERIES_MAX_COORDS) return fail(CCLQR_EINVAL, "nc = " + std::to_string(nc) + ": a series has 1 .. CCLQR_SERIES_MAX_COORDS = " + std::to_string(CCLQR_SERIES_MAX_COORDS) + " coordinates");
    if (ens_tiles(n_inst) * steps > 0x7fffffffLL) return fail(CCLQR_EINVAL, "n_inst x steps exceeds one launch: call with fewer steps");
    return CCLQR_OK;
}
static int series_quantile_sizes_ok(int64_t n_inst, int32_t steps, int32_t nc) {
    TRY(series_sizes_ok(n_inst, steps, nc));
    if (n_inst > CCLQR_QUANTILE_MAX_INST)
        return fail(CCLQR_EUNSUPPORTED, "n_inst = " + std::to_string(n_inst) + ": one call sorts at most CCLQR_QUANTILE_MAX_INST = " + std::to_string(CCLQR_QUANTILE_MAX_INST) + " instances");
    return CCLQR_OK;
}
extern "C" int cclqr_series_ensemble_ws_bytes(int64_t n_inst, int32_t steps, int32_t nc, size_t* bytes) {
    if (!bytes) return fail(CCLQR_EINVAL, "null argument");
    TRY(series_sizes_ok(n_inst, steps, nc));
    *bytes = sizeof(double) * ser_ws_doubles(n_inst, steps, nc);
    return CCLQR_OK;
}
extern "C" int cclqr_series_ensemble(int64_t n_inst, int32_t steps, int32_t nc, const double* x, double* mean, double* m2, void* ws, size_t ws_bytes, void* stream) {
    TRY(series_sizes_ok(n_inst, steps, nc));
    if (!x || !mean || !m2) return fail(CCLQR_EINVAL, "null argument");
    const size_t need = sizeof(double) * ser_ws_doubles(n_inst, steps, nc);
    if (!ws) return fail(CCLQR_EINVAL, "null workspace: cclqr_series_ensemble_ws_bytes says how large it must be (" + std::to_string(need) + " bytes)");
    if (ws_bytes < need) return fail(CCLQR_EINVAL, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, " + std::to_string(need) + " needed (cclqr_series_ensemble_ws_bytes)");
    if (((uintptr_t)ws & 7) != 0) return fail(CCLQR_EINVAL, "the workspace is not 8-byte aligned");
    HIPCHK(launch_series_moments(n_inst, steps, nc, x, (double*)ws, (hipStream_t)stream));
    HIPCHK(launch_ensemble_finish((const double*)ws, n_inst, steps, nc, mean, m2, (hipStream_t)stream));
    return CCLQR_OK;
}
extern "C" int cclqr_series_quantiles_ws_bytes(int64_t n_inst, int32_t steps, int32_t nc, size_t* min_bytes, size_t* full_bytes) {
    if (!min_bytes || !full_bytes) return fail(CCLQR_EINVAL, "null argument");
    TRY(series_quantile_sizes_ok(n_inst, steps, nc));
    *min_bytes = sizeof(double) * ser_row_doubles(n_inst, nc);
    *full_bytes = *min_bytes * (size_t)steps;
    return CCLQR_OK;
}
extern "C" int cclqr_series_quantiles(int64_t n_inst, int32_t steps, int32_t nc, const double* x, int32_t n_prob, const double* prob, double* quant, int32_t* finite,
                                      void* ws, size_t ws_bytes, void* stream) {
    TRY(series_sizes_ok(n_inst, steps, nc));
    if (!x || !prob || !quant) return fail(CCLQR_EINVAL, "null argument");
    if (n_prob < 1 || n_prob > CCLQR_QUANTILE_MAX_PROBS)
        return fail(CCLQR_EINVAL, "n_prob = " + std::to_string(n_prob) + ": one call takes 1 .. " + std::to_string(CCLQR_QUANTILE_MAX_PROBS) + " probabilities");
    for (int j = 0; j < n_prob; j++)
        if (!(prob[j] >= 0.0 && prob[j] <= 1.0)) return fail(CCLQR_EINVAL, "prob[" + std::to_string(j) + "] = " + std::to_string(prob[j]) + " is not a probability in [0, 1]");
    TRY(series_quantile_sizes_ok(n_inst, steps, nc));
    const size_t row_bytes = sizeof(double) * ser_row_doubles(n_inst, nc);
    if (!ws) return fail(CCLQR_EINVAL, "null workspace: cclqr_series_quantiles_ws_bytes says how large it must be (at least " + std::to_string(row_bytes) + " bytes)");
    if (ws_bytes < row_bytes) return fail(CCLQR_EINVAL, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, " + std::to_string(row_bytes) + " needed for one row (cclqr_series_quantiles_ws_bytes)");
    if (((uintptr_t)ws & 7) != 0) return fail(CCLQR_EINVAL, "the workspace is not 8-byte aligned");
    QntArgs a;      // (the select kernel counts its coordinates as 12 nb + mu: nb = 0, mu = nc)
    memset(&a, 0, sizeof(a));
    a.nb = 0; a.mu = nc; a.n_inst = n_inst; a.n_pad = qnt_pad(n_inst); a.steps = steps; a.k0 = 1;
    a.xt = (double*)ws; a.n_prob = n_prob; a.quant = quant; a.finite = finite;
    for (int j = 0; j < n_prob; j++) a.prob[j] = prob[j];
    const size_t fit = ws_bytes / row_bytes;
    const int block = (int)(fit < 65535 ? fit : 65535);      // (rows are the y extent of the select kernel's grid and the z extent of the stage kernel's)
    for (int r0 = 0; r0 < steps; r0 += block) {
        a.row0 = r0; a.nrows = steps - r0 < block ? steps - r0 : block;
        HIPCHK(launch_series_stage(n_inst, steps, nc, x, a.row0, a.nrows, a.xt, (hipStream_t)stream));
        HIPCHK(launch_quantile_select(a, (hipStream_t)stream));
    }
    return CCLQR_OK;
}

// ---- the cost-to-go of a controller's tables and the cost it predicts (value.hip).  P stays in the caller's body order, as the recursion holds it (the models and Q
// are in that order); the kernel permutes the error, not the table
extern "C" int cclqr_value_create(const cclqr_mech* m, int64_t n_tables, const double* P_host, cclqr_value** out) {
    if (!m || !P_host || !out) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (n_tables < 1) return fail(CCLQR_EINVAL, "n_tables = " + std::to_string(n_tables) + ": a value object holds at least one table");
    ValueOwner own(value_new(m, n_tables));
    HIPTRY("cost-to-go upload", value_alloc(own.p));
    HIPTRY("cost-to-go upload", hipMemcpy(own.p->P_dev, P_host, (size_t)n_tables * 144 * (size_t)m->nb * m->nb * sizeof(double), hipMemcpyHostToDevice));
    *out = own.release();
    return CCLQR_OK;
}

extern "C" int cclqr_value_get(const cclqr_value* v, int64_t table, double* P_host) {
    if (!v || !P_host) return fail(CCLQR_EINVAL, "null argument");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != v->device) return fail(CCLQR_EINVAL, "the calling thread is not on the value object's device");
    if (table < 0 || table >= v->n_tables) return fail(CCLQR_EINVAL, "table " + std::to_string(table) + " is not among the value object's tables 0 .. " + std::to_string(v->n_tables - 1));
    const size_t per = 144 * (size_t)v->nb * v->nb;
    HIPCHK(hipMemcpy(P_host, v->P_dev + (size_t)table * per, per * sizeof(double), hipMemcpyDeviceToHost));
    return CCLQR_OK;
}

extern "C" int cclqr_value_destroy(cclqr_value* v) {
    if (!v) return CCLQR_OK;
    if (v->P_dev) (void)hipFree(v->P_dev);
    delete v;
    return CCLQR_OK;
}

extern "C" int cclqr_value_eval(const cclqr_mech* m, const cclqr_ctrl* c, const cclqr_value* v, int64_t n_inst, int64_t first_instance, const double* z_dev,
                                int64_t z_stride, double* out_dev, void* stream) {
    if (!m || !c || !v) return fail(CCLQR_EINVAL, "null argument");
    TRY(check_device(m));
    if (v->mech != m || v->nb != m->nb || v->device != m->device) return fail(CCLQR_EINVAL, "the value object was created for another mechanism or device");
    if (c->nb != m->nb || c->device != m->device) return fail(CCLQR_EINVAL, "the controller was created for another mechanism or device");
    if (n_inst < 0 || first_instance < 0) return fail(CCLQR_EINVAL, "negative n_inst or first_instance");
    const int64_t ctrl_tables = c->host.n_ctrl > 1 ? c->host.n_ctrl : 1;
    if (v->n_tables != 1 && v->n_tables != ctrl_tables)
        return fail(CCLQR_EINVAL, "the value object holds " + std::to_string(v->n_tables) + " tables: one shared by all (1) or one per controller table (" + std::to_string(ctrl_tables) + ")");
    if (!c->zd_dev || c->host.nsp < 1) return fail(CCLQR_EINVAL, "the controller has no setpoint table");
    const int64_t tables = v->n_tables > 1 ? v->n_tables : ctrl_tables;
    if (tables > 1 && first_instance + n_inst > tables)
        return fail(CCLQR_EINVAL, "first_instance + n_inst = " + std::to_string(first_instance + n_inst) + " exceeds the " + std::to_string(tables) + " tables");
    if (z_stride < 13 * (int64_t)m->nb) return fail(CCLQR_EINVAL, "z_stride = " + std::to_string(z_stride) + " is less than a state's 13 nb = " + std::to_string(13 * m->nb) + " doubles");
    if (n_inst == 0) return CCLQR_OK;
    if (!z_dev || !out_dev) return fail(CCLQR_EINVAL, "null argument");
    ValueArgs a;
    a.M = m->dev; a.C = c->dev; a.P = v->P_dev; a.p_stride = v->n_tables > 1 ? 144LL * m->nb * m->nb : 0; a.nb = m->nb;
    a.n_inst = n_inst; a.inst0 = first_instance; a.z = z_dev; a.z_stride = z_stride; a.out = out_dev;
    HIPCHK(launch_value(a, (hipStream_t)stream));
    return CCLQR_OK;
}

// ---- policy evaluation (policy.hip): dlqr's cost recursion (lqr.jl:147-177) with the gains given
// rows of gain tables from the kernels' link order (a controller's device tables: padded stride between tables) to the caller's body order, packed
// [n_tables][rows_per_table][12 nb] -- the inverse of k_rows_to_link_order_kernel, out of place: the controller's tables are not touched.  One workgroup per row
__global__ void k_rows_to_body_order_kernel(const double* K, long long nrows, long long rows_per_table, long long table_stride, int nb, const MechDev* M, double* out) {
    const long long r = blockIdx.x;
    if (r >= nrows) return;
    const double* p = K + (r / rows_per_table) * table_stride + (r % rows_per_table) * 12 * nb;
    double* o = out + r * 12 * nb;
    for (int e = threadIdx.x; e < 12 * nb; e += blockDim.x) { const int l = e / 12; o[12 * M->perm[l] + (e - 12 * l)] = p[e]; }
}

// ---- the host sequences the analysis entry points below share: a new analysis calls these, it does not copy them under a new name
// the sizes of a launch record: fp64 (bf16_terms = 0), no gain output.  Callers: run_policy, doubling_args, tracking_setup, tracking_value_on_plants, cclqr_riccati_doubling
static void ric_sizes(RicArgs& r, int nprob, int mx, int mu, int ml, int N, int time_varying, double tol, int path, int keep_last = 0) {
    r.nprob = nprob; r.mx = mx; r.mu = mu; r.ml = ml; r.N = N; r.time_varying = time_varying; r.tol = tol; r.path = path; r.bf16_terms = 0; r.keep_last = keep_last; r.K = nullptr;
}
// host weights [n_weights][mx][mx], [n_weights][mu][mu] onto the device with their strides, inside the caller's WsScope.  Callers: run_policy, run_doubling,
// run_covariance, ctk_setup, ptk_setup, cclqr_riccati_doubling
static int upload_weights(int mx, int mu, int n_weights, const double* Q, const double* R, WeightsIn& w, const char* what) {
    const size_t nw = (size_t)n_weights;
    double *dQ = nullptr, *dR = nullptr;
    HIPTRY(what, ws_get((void**)&dQ, nw * mx * mx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dR, (nw * mu * mu + 1) * sizeof(double)));
    HIPTRY(what, hipMemcpy(dQ, Q, nw * mx * mx * sizeof(double), hipMemcpyHostToDevice));
    if (mu > 0) HIPTRY(what, hipMemcpy(dR, R, nw * mu * mu * sizeof(double), hipMemcpyHostToDevice));
    w.Q = dQ; w.R = dR;
    if (n_weights > 1) { w.q_stride = (long long)mx * mx; w.r_stride = (long long)mu * mu; }
    return CCLQR_OK;
}
// ... as the recursion's own weights.  Callers: run_policy, run_doubling, ptk_setup, cclqr_riccati_doubling
static void ric_weights(RicArgs& r, const WeightsIn& w) { r.Q = w.Q; r.R = w.R; r.q_stride = w.q_stride; r.r_stride = w.r_stride; }
// host noise Wu [n_noise][mu][mu] and Sigma0 [n_noise][mx][mx] (each may be null: not given) onto the device with their strides, inside the caller's WsScope.
// Callers: run_covariance, tracking_setup
static int upload_noise(int mx, int mu, int n_noise, const double* Wu, const double* Sigma0, NoiseIn& n, const char* what) {
    const size_t nn = (size_t)n_noise, mm = (size_t)mx * mx, uu = (size_t)mu * mu;
    double *dWu = nullptr, *dS0 = nullptr;
    if (Wu) {
        HIPTRY(what, ws_get((void**)&dWu, nn * uu * sizeof(double)));
        HIPTRY(what, hipMemcpy(dWu, Wu, nn * uu * sizeof(double), hipMemcpyHostToDevice));
        n.Wu = dWu; n.wu_stride = n_noise > 1 ? (long long)uu : 0;
    }
    if (Sigma0) {
        HIPTRY(what, ws_get((void**)&dS0, nn * mm * sizeof(double)));
        HIPTRY(what, hipMemcpy(dS0, Sigma0, nn * mm * sizeof(double), hipMemcpyHostToDevice));
        n.Sigma0 = dS0; n.s0_stride = n_noise > 1 ? (long long)mm : 0;
    }
    return CCLQR_OK;
}
// What a recursion runs on, on the device: the models, the gain tables and the [nprob][mx][mx] matrix it writes (P or Σ).  raw_upload fills it for the entries on
// caller-supplied matrices, policy_models_and_gains for those on a mechanism's plants
struct AnaDev { RicModels m; GainTable k; double* P; };
// the preamble of a raw entry, inside its WsScope: models_per_problem host models of every problem (0: no model is read), n_gains host tables of `rows` rows
// (gains_read = false: no step reads a gain, none is copied) and the matrix the kernels write.  Callers: cclqr_policy_value, cclqr_policy_value_doubling,
// cclqr_covariance_doubling, tracking_raw_upload
static int raw_upload(const char* what, int nprob, int mx, int mu, int ml, int models_per_problem, const double* A, const double* Bu, const double* Bl, const double* G,
                      int n_gains, int rows, bool gains_read, const double* K, AnaDev& d) {
    d = AnaDev{};
    if (models_per_problem > 0) TRY(upload_models((size_t)nprob * models_per_problem, mx, mu, ml, A, Bu, Bl, G, d.m));
    const size_t nKd = (mu > 0 && gains_read) ? (size_t)n_gains * rows * mu * mx : 0;
    double* dK = nullptr;
    HIPTRY(what, ws_get((void**)&dK, (nKd + 1) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&d.P, (size_t)nprob * mx * mx * sizeof(double)));
    if (nKd) HIPTRY(what, hipMemcpy(dK, K, nKd * sizeof(double), hipMemcpyHostToDevice));
    d.k.Kin = dK; d.k.k_stride = n_gains > 1 ? (long long)rows * mu * mx : 0; d.k.nK = rows;
    return CCLQR_OK;
}
// n values from the device into v.  Callers: every read-back of the analyses (run_policy, doubling_read_back, run_covariance, ctk_ / ptk_ / tracking_read_back)
template <class T>
static int download(std::vector<T>& v, const T* dev, size_t n, const char* what) {
    v.resize(n);
    HIPTRY(what, hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
    return CCLQR_OK;
}
// problem p's pair of a [nprob][2] diagnostic into the caller's array (may be null).  Callers: policy_report, doubling_report, covariance_report, tracking_cov_report
static void put_pair(double* out, const std::vector<double>& v, size_t p) {
    if (out) { out[2 * p] = v[2 * p]; out[2 * p + 1] = v[2 * p + 1]; }
}
// the refusal of a singular G Bλ in problem / model / table p, with its knot where the recursion names one.  Callers: policy_report, doubling_report,
// tracking_cov_report, tracking_pol_report
static int singular_in(const char* of, long long p, const int* knot = nullptr) {
    return fail(CCLQR_ESINGULAR, std::string("G*Bl is singular in ") + of + " " + std::to_string(p) + (knot ? " at knot " + std::to_string(*knot) : std::string()));
}
// the refusals several entries word alike, before anything is allocated or launched.  n_gains: tables = whole gain tables, else single stationary gains (always per
// problem).  Callers: cclqr_policy_value, tracking_counts_check / cclqr_policy_value_doubling, cclqr_covariance_doubling
static int check_n_gains(int n_gains, int nprob, bool tables, const char* of) {
    if (n_gains == 1 || n_gains == nprob) return CCLQR_OK;
    return fail(CCLQR_EINVAL, "n_gains = " + std::to_string(n_gains) + (tables ? std::string(": the gains are one table shared by all (1) or one table per ") + of
                                                                               : std::string(": one gain shared by all (1) or one per problem")) + " (" + std::to_string(nprob) + ")");
}
// n_noise: are = "Wu / Sigma0 are" or "Wu is".  Callers: covariance_check, tracking_cov_check, tracking_pol_check
static int check_n_noise(int n_noise, int nprob, const char* are, const char* of) {
    if (n_noise == 1 || n_noise == nprob) return CCLQR_OK;
    return fail(CCLQR_EINVAL, "n_noise = " + std::to_string(n_noise) + ": " + are + " one shared by all (1) or one per " + of + " (" + std::to_string(nprob) + ")");
}
// the options of an analysis that runs in fp64 on path 0..2: what = its name, the = "the " where the sentence takes the article.  Callers: cclqr_policy_value,
// doubling_check, tracking_launch_check
static int check_fp64_path(const cclqr_riccati_opts* opts, const char* what, const char* the) {
    const int path = opts ? opts->path : 0;
    if (path < 0 || path > 2) return fail(CCLQR_EINVAL, std::string(what) + " options: path in 0..2");
    if (opts && opts->bf16_terms != 0) return fail(CCLQR_EINVAL, std::string(the) + what + " runs in fp64 only (bf16_terms = 0)");
    return CCLQR_OK;
}

// ---- policy evaluation's own
// shared tail of the two entry points: the recursion on device-resident models and gains, inside the caller's WsScope; d.P is written by the kernels.  kb, st [nprob]
// and dn [nprob][2] come back on the host
static int run_policy(int nprob, int mx, int mu, int ml, int N, double tol, const AnaDev& d, int n_weights, const double* Q, const double* R, int path,
                      std::vector<int>& kb, std::vector<int>& st, std::vector<double>& dn) {
    static const char* const what = "policy evaluation";
    double *dwork = nullptr, *ddn = nullptr;
    int *dkb = nullptr, *dst = nullptr, *dstop = nullptr;
    const size_t np = (size_t)nprob;
    PolArgs a;
    RicArgs& r = a.r;
    WeightsIn w;
    ric_sizes(r, nprob, mx, mu, ml, N, 0, tol, path);
    TRY(upload_weights(mx, mu, n_weights, Q, R, w, what));
    ric_weights(r, w);
    HIPTRY(what, ws_get((void**)&dwork, ric_total_work_doubles(r) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&ddn, 2 * np * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dstop, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dkb, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dst, np * sizeof(int)));
    r.stop = dstop; r.A = d.m.A; r.Bu = d.m.Bu; r.Bl = d.m.Bl; r.G = d.m.G; r.kbreak = dkb; r.status = dst; r.work = dwork; r.P_out = d.P;
    a.k = d.k; a.dnorm = ddn;
    HIPTRY(what, launch_policy(a, nullptr));
    HIPTRY(what, hipDeviceSynchronize());
    TRY(download(kb, dkb, np, what));
    TRY(download(st, dst, np, what));
    return download(dn, ddn, 2 * np, what);
}
// ... and its diagnostics into the caller's arrays (each may be null), up to the problem the call is refused for
static int policy_report(const std::vector<int>& kb, const std::vector<int>& st, const std::vector<double>& dn, int nprob, int32_t* kbreak, double* dnorm, const char* of) {
    for (int p = 0; p < nprob; p++) {
        if (kbreak) kbreak[p] = kb[p];
        put_pair(dnorm, dn, p);
        if (st[p] != 0) return singular_in(of, p);
    }
    return CCLQR_OK;
}
// what both entry points refuse about the recursion's own sizes, before anything is allocated or launched
static int policy_check(int nprob, int mu, int N, int nK, int n_weights, const char* of) {
    if (N > 1 && mu > 0 && nK != 1 && nK != N - 1)
        return fail(CCLQR_EINVAL, "nK = " + std::to_string(nK) + ": a gain table holds one row (a stationary gain) or N - 1 = " + std::to_string(N - 1) + " rows, one per backward step");
    return check_n_weights(n_weights, nprob, of);
}

extern "C" int cclqr_policy_value(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                  int32_t n_gains, int32_t nK, const double* K, int32_t n_weights, const double* Q, const double* R, int32_t N, double tol,
                                  double* P, int32_t* kbreak, double* dnorm, const cclqr_riccati_opts* opts) {
    static const char* const what = "policy evaluation";
    if (!A || !Q || !P || (mu > 0 && (!Bu || !R)) || (ml > 0 && (!Bl || !G)) || (mu > 0 && N > 1 && !K)) return fail(CCLQR_EINVAL, "null argument");
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0 || N < 1) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_gains(n_gains, nprob, true, "problem"));
    TRY(policy_check(nprob, mu, N, nK, n_weights, "problem"));
    TRY(check_fp64_path(opts, what, ""));
    WsScope scope;
    AnaDev d;
    TRY(raw_upload(what, nprob, mx, mu, ml, 1, A, Bu, Bl, G, n_gains, nK, N > 1, K, d));
    std::vector<int> kb, st;
    std::vector<double> dn;
    TRY(run_policy(nprob, mx, mu, ml, N, tol, d, n_weights, Q, R, opts ? opts->path : 0, kb, st, dn));
    HIPTRY(what, hipMemcpy(P, d.P, (size_t)nprob * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    return policy_report(kb, st, dn, nprob, kbreak, dnorm, "problem");
}

// what the controller entry points of every analysis refuse about the mechanism, the controller and the plants, before anything is allocated or launched; subject:
// the analysis as the closed-loop refusal names it; bad_sizes: the caller's own test of its counts; stationary: the analysis is of time-invariant models only.  cj: the
// controlled links; *tables: the controller's gain tables (1 or n_models).  Callers: cclqr_value_create_policy, _policy_doubling, _covariance_doubling (stationary),
// tracking_value_on_plants
static int policy_ctrl_check(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, int32_t mu, const int32_t* ctrl_joint,
                             const cclqr_ctrl* c, const std::string& subject, bool bad_sizes, bool stationary, int* cj, int64_t* tables) {
    TRY(check_device(m));
    if (m->host.loop) return fail(CCLQR_EUNSUPPORTED, subject + " is for tree mechanisms (closed loops have no multiplier model to evaluate a gain on)");
    if (c->nb != m->nb || c->device != m->device) return fail(CCLQR_EINVAL, "the controller was created for another mechanism or device");
    if (bad_sizes) return fail(CCLQR_EINVAL, "bad sizes");
    const CtrlDev& H = c->host;
    if (!c->K_dev || H.nK < 1) return fail(CCLQR_EINVAL, "the controller has no gains (open loop / PID)");
    if (stationary && H.nsp > 1)
        return fail(CCLQR_EUNSUPPORTED, "tracking controllers (more than one setpoint row per table) are outside policy evaluation's scope: time-invariant models only");
    TRY(linearize_check(m, plants, first_plant, n_models, mu, ctrl_joint, cj));      // the refusals of cclqr_linearize_plants
    bool same = mu == H.mu;
    for (int i = 0; same && i < mu; i++) same = cj[i] == H.cj[i];
    if (!same) return fail(CCLQR_EINVAL, "mu / ctrl_joint are not the controller's: its gains act on other joints");
    *tables = H.n_ctrl > 1 ? H.n_ctrl : 1;
    if (*tables != 1 && *tables != n_models)
        return fail(CCLQR_EINVAL, "the controller holds " + std::to_string(*tables) + " tables: one shared by all models (1) or one per model (" + std::to_string(n_models) + ")");
    return CCLQR_OK;
}
// the controller's gains gathered into the models' body order on `stream`, device to device (they never visit the host), inside the caller's WsScope:
// k.Kin [tables][nK][mu][12 nb].  Callers: policy_models_and_gains, tracking_value_on_plants
static int gather_gains(const cclqr_mech* m, const cclqr_ctrl* c, int mu, int64_t tables, hipStream_t stream, GainTable& k, const char* what) {
    const CtrlDev& H = c->host;
    const long long rows_per_table = (long long)H.nK * mu, nrows = tables * rows_per_table;
    double* dK = nullptr;
    HIPTRY(what, ws_get((void**)&dK, (size_t)nrows * 12 * m->nb * sizeof(double)));
    HIPTRY(what, launch_lds<false>(k_rows_to_body_order_kernel, dim3((unsigned)nrows), dim3(128), 0, stream, c->K_dev, nrows, rows_per_table, (long long)H.K_stride, m->nb,
                                   m->dev, dK));
    k = GainTable{dK, tables > 1 ? rows_per_table * 12 * m->nb : 0, H.nK};
    return CCLQR_OK;
}
// ... and the device sequence the stationary ones share, their counterpart of raw_upload, inside the caller's WsScope: the tables of the value v under construction
// allocated (they are d.P), linearsystem at every setpoint on its plant (lqr.jl:63), and gather_gains.  Callers: cclqr_value_create_policy,
// cclqr_value_create_policy_doubling, cclqr_value_create_covariance_doubling
static int policy_models_and_gains(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, const double* zd, const double* Fd, int32_t mu,
                                   const int32_t* ctrl_joint, const cclqr_ctrl* c, int64_t tables, cclqr_value* v, AnaDev& d, const char* what) {
    LinWs w = {};
    HIPTRY(what, value_alloc(v));
    TRY(linearize_to_ws(m, plants, first_plant, n_models, zd, Fd, mu, ctrl_joint, w, what));
    long long bad = -1;
    HIPTRY(what, knots_converged(w.status, (size_t)n_models, &bad));
    if (bad >= 0) return fail(CCLQR_ENOCONV, "Newton did not converge at setpoint " + std::to_string(bad));
    d.m = RicModels{w.A, w.Bu, w.Bl, w.G};
    d.P = v->P_dev;
    return gather_gains(m, c, mu, tables, nullptr, d.k, what);
}

extern "C" int cclqr_value_create_policy(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, const double* zd, int32_t mu,
                                         const int32_t* ctrl_joint, const double* Fd, const cclqr_ctrl* c, int32_t n_weights, const double* Q, const double* R,
                                         int32_t N, double tol, int32_t* kbreak, double* dnorm, cclqr_value** out) {
    if (!m || !zd || !c || !Q || !out || (mu > 0 && (!ctrl_joint || !R))) return fail(CCLQR_EINVAL, "null argument");
    int cj[CCLQR_MAXL];
    int64_t tables = 1;
    TRY(policy_ctrl_check(m, plants, first_plant, n_models, mu, ctrl_joint, c, "policy evaluation", n_models < 1 || N < 1 || mu < 1 || mu > m->nb, true, cj, &tables));
    const CtrlDev& H = c->host;
    if (H.nK > 1 && N != H.nK + 1)
        return fail(CCLQR_EINVAL, "the controller's tables hold " + std::to_string(H.nK) + " rows, one per backward step: N must be " + std::to_string(H.nK + 1) + " (got " + std::to_string(N) + ")");
    TRY(policy_check(n_models, mu, N, H.nK, n_weights, "model"));
    ValueOwner vown(value_new(m, n_models));
    WsScope scope;
    AnaDev d;
    TRY(policy_models_and_gains(m, plants, first_plant, n_models, zd, Fd, mu, ctrl_joint, c, tables, vown.p, d, "policy evaluation"));
    std::vector<int> kb, st;
    std::vector<double> dn;
    TRY(run_policy(n_models, 12 * m->nb, mu, 5 * m->nb, N, tol, d, n_weights, Q, R, 0, kb, st, dn));
    TRY(policy_report(kb, st, dn, n_models, kbreak, dnorm, "model"));
    *out = vown.release();
    return CCLQR_OK;
}

// ---- a stationary gain's cost-to-go by doubling (policy_doubling.hip): lqr.jl:169-170 with the one gain of LQR{T,Inf} (lqr.jl:40-43)
// what both entry points refuse about the evaluation's own arguments, before anything is allocated or launched
static int doubling_check(int nprob, int N, double tol, int max_levels, int n_weights, const cclqr_riccati_opts* opts, const char* of) {
    if (N < 0) return fail(CCLQR_EINVAL, "N = " + std::to_string(N) + ": a horizon of N >= 1 knots, or 0 = to convergence");
    if (N == 0 && (max_levels < 1 || max_levels > 60)) return fail(CCLQR_EINVAL, "max_levels = " + std::to_string(max_levels) + ": 1 .. 60 (2^max_levels steps)");
    if (!(tol >= 0.0)) return fail(CCLQR_EINVAL, "tol is negative or not a number");
    TRY(check_fp64_path(opts, "policy evaluation", ""));
    return check_n_weights(n_weights, nprob, of);
}
// the host results of run_doubling and run_covariance
struct DblOut { std::vector<int> lv, rs, st; std::vector<double> dn, gn; };
// what the two runs share before their launch, inside the caller's WsScope: the sizes, the models and gains, the two workspaces (work2_doubles: the launch's own
// count, from the sizes set here) and the device diagnostics of a DblArgs; Q, R and P_out are the caller's to set
static int doubling_args(DblArgs& a, int nprob, int mx, int mu, int ml, int N, double tol, int max_levels, const AnaDev& d, int path,
                         size_t (*work2_doubles)(const RicArgs&), const char* what) {
    double *dwork = nullptr, *dwork2 = nullptr, *ddn = nullptr, *dgn = nullptr;
    int *dlv = nullptr, *drs = nullptr, *dst = nullptr, *dstop = nullptr;
    const size_t np = (size_t)nprob;
    RicArgs& r = a.r;
    ric_sizes(r, nprob, mx, mu, ml, N, 0, tol, path);
    HIPTRY(what, ws_get((void**)&dwork, ric_total_work_doubles(r) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dwork2, work2_doubles(r) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&ddn, 2 * np * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dgn, 2 * np * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dstop, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dlv, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&drs, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dst, np * sizeof(int)));
    r.stop = dstop; r.A = d.m.A; r.Bu = d.m.Bu; r.Bl = d.m.Bl; r.G = d.m.G; r.kbreak = nullptr; r.status = dst; r.work = dwork; r.P_out = d.P;
    a.k = d.k; a.max_levels = max_levels; a.work2 = dwork2; a.levels = dlv; a.reason = drs; a.dnorm = ddn; a.gnorm = dgn;
    return CCLQR_OK;
}
// ... and after it: the device is waited for and the launch's diagnostics come onto the host (gnorm: the second pair of norms, RdbArgs' anorm).  Callers:
// run_doubling, run_covariance, cclqr_riccati_doubling
static int doubling_read_back(size_t np, const int* levels, const int* reason, const int* status, const double* dnorm, const double* gnorm, DblOut& o, const char* what) {
    HIPTRY(what, hipDeviceSynchronize());
    TRY(download(o.lv, levels, np, what));
    TRY(download(o.rs, reason, np, what));
    TRY(download(o.st, status, np, what));
    TRY(download(o.dn, dnorm, 2 * np, what));
    return download(o.gn, gnorm, 2 * np, what);
}
// shared tail of the two entry points, as run_policy is: the evaluation on device-resident models and gains, inside the caller's WsScope
static int run_doubling(int nprob, int mx, int mu, int ml, int N, double tol, int max_levels, const AnaDev& d, int n_weights, const double* Q, const double* R, int path,
                        DblOut& o) {
    static const char* const what = "policy evaluation by doubling";
    DblArgs a;
    WeightsIn w;
    TRY(doubling_args(a, nprob, mx, mu, ml, N, tol, max_levels, d, path, dbl_work_doubles, what));
    TRY(upload_weights(mx, mu, n_weights, Q, R, w, what));
    ric_weights(a.r, w);
    HIPTRY(what, launch_policy_doubling(a, nullptr));
    return doubling_read_back((size_t)nprob, a.levels, a.reason, a.r.status, a.dnorm, a.gnorm, o, what);
}
// the diagnostics of a DblOut into the caller's arrays (each may be null), up to the problem the call is refused for.  Callers: the five doubling entry points
static int doubling_report(const DblOut& o, int nprob, int32_t* levels, int32_t* reason, double* dnorm, double* gnorm, const char* of) {
    for (int p = 0; p < nprob; p++) {
        if (levels) levels[p] = o.lv[p];
        if (reason) reason[p] = o.rs[p];
        put_pair(dnorm, o.dn, p);
        put_pair(gnorm, o.gn, p);
        if (o.st[p] != 0) return singular_in(of, p);
    }
    return CCLQR_OK;
}

extern "C" int cclqr_policy_value_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                           int32_t n_gains, const double* K, int32_t n_weights, const double* Q, const double* R, int32_t N, double tol,
                                           int32_t max_levels, double* P, int32_t* levels, int32_t* reason, double* dnorm, double* gnorm, const cclqr_riccati_opts* opts) {
    static const char* const what = "policy evaluation by doubling";
    if (!A || !Q || !P || (mu > 0 && (!Bu || !R || !K)) || (ml > 0 && (!Bl || !G))) return fail(CCLQR_EINVAL, "null argument");
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_gains(n_gains, nprob, false, "problem"));
    TRY(doubling_check(nprob, N, tol, max_levels, n_weights, opts, "problem"));
    WsScope scope;
    AnaDev d;
    TRY(raw_upload(what, nprob, mx, mu, ml, 1, A, Bu, Bl, G, n_gains, 1, true, K, d));
    DblOut o;
    TRY(run_doubling(nprob, mx, mu, ml, N, tol, max_levels, d, n_weights, Q, R, opts ? opts->path : 0, o));
    HIPTRY(what, hipMemcpy(P, d.P, (size_t)nprob * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    return doubling_report(o, nprob, levels, reason, dnorm, gnorm, "problem");
}

extern "C" int cclqr_value_create_policy_doubling(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, const double* zd, int32_t mu,
                                                  const int32_t* ctrl_joint, const double* Fd, const cclqr_ctrl* c, int32_t n_weights, const double* Q, const double* R,
                                                  int32_t N, double tol, int32_t max_levels, int32_t* levels, int32_t* reason, double* dnorm, double* gnorm,
                                                  cclqr_value** out) {
    if (!m || !zd || !c || !Q || !out || (mu > 0 && (!ctrl_joint || !R))) return fail(CCLQR_EINVAL, "null argument");
    int cj[CCLQR_MAXL];
    int64_t tables = 1;
    TRY(policy_ctrl_check(m, plants, first_plant, n_models, mu, ctrl_joint, c, "policy evaluation", n_models < 1 || mu < 1 || mu > m->nb, true, cj, &tables));
    if (c->host.nK != 1)
        return fail(CCLQR_EINVAL, "the controller's tables hold " + std::to_string(c->host.nK) + " gain rows: doubling evaluates ONE stationary gain (a finite-horizon table is what cclqr_value_create_policy steps through)");
    TRY(doubling_check(n_models, N, tol, max_levels, n_weights, nullptr, "model"));
    ValueOwner vown(value_new(m, n_models));
    WsScope scope;
    AnaDev d;
    TRY(policy_models_and_gains(m, plants, first_plant, n_models, zd, Fd, mu, ctrl_joint, c, tables, vown.p, d, "policy evaluation by doubling"));
    DblOut o;
    TRY(run_doubling(n_models, 12 * m->nb, mu, 5 * m->nb, N, tol, max_levels, d, n_weights, Q, R, 0, o));
    TRY(doubling_report(o, n_models, levels, reason, dnorm, gnorm, "model"));
    *out = vown.release();
    return CCLQR_OK;
}

// ---- closed-loop state covariance under input noise by doubling (covariance_doubling.hip): Σ⁺ = Abar Σ Abar' + D Wu D' with the one gain of LQR{T,Inf}
// (lqr.jl:40-43, 169), the noise law of trackingLQR_triple_cartpole.jl:98
// what both entry points refuse about the noise and the moments, after doubling_check and before anything is allocated or launched
static int covariance_check(int nprob, int mu, int N, int n_noise, const double* Wu, const double* Sigma0, const double* Q, const double* R, const double* cost,
                            const char* of) {
    TRY(check_n_noise(n_noise, nprob, "Wu / Sigma0 are", of));
    if (!Wu && !Sigma0) return fail(CCLQR_EINVAL, "Wu and Sigma0 are both null: there is no covariance to propagate");
    if (Wu && mu == 0) return fail(CCLQR_EINVAL, "Wu is given with mu = 0: there is no input for the noise to enter through");
    if (cost && (!Q || (mu > 0 && !R))) return fail(CCLQR_EINVAL, "cost is asked for without Q / R");
    if (N == 0 && Sigma0) return fail(CCLQR_EINVAL, "N = 0 with Sigma0: a steady state does not depend on the start (pass Sigma0 = NULL)");
    return CCLQR_OK;
}
// the host moments of run_covariance; each is filled only if asked for
struct CovOut { std::vector<double> cost, zstd, ustd; };
// shared tail of the two entry points, run_doubling's shape: the covariance on device-resident models and gains, inside the caller's WsScope; d.P receives Σ.  Wu,
// Sigma0, Q, R: HOST, as the entry points take them
static int run_covariance(int nprob, int mx, int mu, int ml, int N, double tol, int max_levels, const AnaDev& d, int n_weights, const double* Q, const double* R,
                          int n_noise, const double* Wu, const double* Sigma0, int path, bool want_cost, bool want_zstd, bool want_ustd, DblOut& o, CovOut& m) {
    static const char* const what = "covariance by doubling";
    const size_t np = (size_t)nprob;
    CovArgs c{};
    TRY(doubling_args(c.d, nprob, mx, mu, ml, N, tol, max_levels, d, path, cov_work_doubles, what));
    if (want_cost) {
        TRY(upload_weights(mx, mu, n_weights, Q, R, c.w, what));
        HIPTRY(what, ws_get((void**)&c.cost, 2 * np * sizeof(double)));
    }
    TRY(upload_noise(mx, mu, n_noise, Wu, Sigma0, c.n, what));
    if (want_zstd) HIPTRY(what, ws_get((void**)&c.zstd, np * mx * sizeof(double)));
    if (want_ustd) HIPTRY(what, ws_get((void**)&c.ustd, (np * mu + 1) * sizeof(double)));
    HIPTRY(what, launch_covariance_doubling(c, nullptr));
    TRY(doubling_read_back(np, c.d.levels, c.d.reason, c.d.r.status, c.d.dnorm, c.d.gnorm, o, what));
    if (want_cost) TRY(download(m.cost, c.cost, 2 * np, what));
    if (want_zstd) TRY(download(m.zstd, c.zstd, np * mx, what));
    if (want_ustd && mu > 0) TRY(download(m.ustd, c.ustd, np * mu, what));
    return CCLQR_OK;
}
// the moments of run_covariance into the caller's arrays (each may be null), for the problems before the one the call is refused for (doubling_report names it)
static void covariance_report(const DblOut& o, const CovOut& m, int nprob, int mx, int mu, double* cost, double* zstd, double* ustd) {
    for (int p = 0; p < nprob && o.st[p] == 0; p++) {
        put_pair(cost, m.cost, p);
        if (zstd) memcpy(zstd + (size_t)p * mx, m.zstd.data() + (size_t)p * mx, (size_t)mx * sizeof(double));
        if (ustd && mu > 0) memcpy(ustd + (size_t)p * mu, m.ustd.data() + (size_t)p * mu, (size_t)mu * sizeof(double));
    }
}

extern "C" int cclqr_covariance_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                         int32_t n_gains, const double* K, int32_t n_weights, const double* Q, const double* R, int32_t n_noise, const double* Wu,
                                         const double* Sigma0, int32_t N, double tol, int32_t max_levels, double* Sigma, double* cost, double* zstd, double* ustd,
                                         int32_t* levels, int32_t* reason, double* dnorm, double* gnorm, const cclqr_riccati_opts* opts) {
    static const char* const what = "covariance by doubling";
    if (!A || !Sigma || (mu > 0 && (!Bu || !K)) || (ml > 0 && (!Bl || !G))) return fail(CCLQR_EINVAL, "null argument");
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_gains(n_gains, nprob, false, "problem"));
    TRY(doubling_check(nprob, N, tol, max_levels, n_weights, opts, "problem"));
    TRY(covariance_check(nprob, mu, N, n_noise, Wu, Sigma0, Q, R, cost, "problem"));
    WsScope scope;
    AnaDev d;
    TRY(raw_upload(what, nprob, mx, mu, ml, 1, A, Bu, Bl, G, n_gains, 1, true, K, d));
    DblOut o;
    CovOut mo;
    TRY(run_covariance(nprob, mx, mu, ml, N, tol, max_levels, d, n_weights, Q, R, n_noise, Wu, Sigma0, opts ? opts->path : 0, cost != nullptr, zstd != nullptr,
                       ustd != nullptr, o, mo));
    HIPTRY(what, hipMemcpy(Sigma, d.P, (size_t)nprob * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    covariance_report(o, mo, nprob, mx, mu, cost, zstd, ustd);
    return doubling_report(o, nprob, levels, reason, dnorm, gnorm, "problem");
}

extern "C" int cclqr_value_create_covariance_doubling(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, const double* zd, int32_t mu,
                                                      const int32_t* ctrl_joint, const double* Fd, const cclqr_ctrl* c, int32_t n_weights, const double* Q, const double* R,
                                                      int32_t n_noise, const double* Wu, const double* Sigma0, int32_t N, double tol, int32_t max_levels, double* cost,
                                                      double* zstd, double* ustd, int32_t* levels, int32_t* reason, double* dnorm, double* gnorm, cclqr_value** out) {
    if (!m || !zd || !c || !out || (mu > 0 && !ctrl_joint)) return fail(CCLQR_EINVAL, "null argument");
    int cj[CCLQR_MAXL];
    int64_t tables = 1;
    TRY(policy_ctrl_check(m, plants, first_plant, n_models, mu, ctrl_joint, c, "policy evaluation", n_models < 1 || mu < 1 || mu > m->nb, true, cj, &tables));
    if (c->host.nK != 1)
        return fail(CCLQR_EINVAL, "the controller's tables hold " + std::to_string(c->host.nK) + " gain rows: the covariance by doubling is that of ONE stationary gain");
    TRY(doubling_check(n_models, N, tol, max_levels, n_weights, nullptr, "model"));
    TRY(covariance_check(n_models, mu, N, n_noise, Wu, Sigma0, Q, R, cost, "model"));
    const int mx = 12 * m->nb;
    ValueOwner vown(value_new(m, n_models));
    WsScope scope;
    AnaDev d;
    TRY(policy_models_and_gains(m, plants, first_plant, n_models, zd, Fd, mu, ctrl_joint, c, tables, vown.p, d, "covariance by doubling"));
    DblOut o;
    CovOut mo;
    TRY(run_covariance(n_models, mx, mu, 5 * m->nb, N, tol, max_levels, d, n_weights, Q, R, n_noise, Wu, Sigma0, 0, cost != nullptr, zstd != nullptr, ustd != nullptr, o, mo));
    covariance_report(o, mo, n_models, mx, mu, cost, zstd, ustd);
    TRY(doubling_report(o, n_models, levels, reason, dnorm, gnorm, "model"));
    *out = vown.release();
    return CCLQR_OK;
}

// ---- the two knot-by-knot analyses of a tracked run, one family: the state covariance (covariance_tracking.hip, Σ_{j+1} = Abar_j Σ_j Abar_j' + D_j Wu D_j') and its
// adjoint, the cost-to-go (policy_tracking.hip, P_j = Q + K_j' R K_j + Abar_j' P_{j+1} Abar_j), each with the gain row and the model of knot j (lqr_tracking.jl:63-65,
// 88-89, 107-108) and the noise law of trackingLQR_triple_cartpole.jl:98.  What the two do alike is done once, here, on the fields their records share (the Riccati
// record, the gain table, the noise, status and knot); each keeps short functions for its own outputs below
// what both refuse first about their counts, in this order.  Callers: tracking_cov_check, tracking_pol_check
static int tracking_counts_check(int nprob, int mu, int N, int nlin, int n_gains, int nK, const char* of) {
    if (N > 1 && nlin != 1 && nlin != N - 1)
        return fail(CCLQR_EINVAL, "nlin = " + std::to_string(nlin) + ": one time-invariant model (1) or one per knot 0 .. N-2 (" + std::to_string(N - 1) + ")");
    TRY(check_n_gains(n_gains, nprob, true, of));
    if (N > 1 && mu > 0 && nK != 1 && nK != N - 1)
        return fail(CCLQR_EINVAL, "nK = " + std::to_string(nK) + ": a gain table holds one row (a stationary gain) or N - 1 = " + std::to_string(N - 1) + " rows, one per knot 0 .. N-2");
    return CCLQR_OK;
}
// ... and last about the launch; what = the analysis' name.  Callers: tracking_cov_check, tracking_pol_check
static int tracking_launch_check(int nprob, const cclqr_riccati_opts* opts, const char* what) {
    if (nprob > 65535) return fail(CCLQR_EINVAL, "nprob = " + std::to_string(nprob) + ": at most 65535 problems per call (they are the y extent of the launch grids)");
    return check_fp64_path(opts, what, "the ");
}
// what a tracking call brings back to the host: the per-knot records (moments / prices), the totals, and of every problem its status and the knot it names
struct TrackOut { std::vector<double> rec, total; std::vector<int> st, knot; };
// the shared part of a setup, inside the caller's WsScope: the sizes of a launch of `chunk` problems, the noise (HOST, as the entries take it), the workspace of one
// launch, status and knot of ALL nprob problems.  Callers: ctk_setup, ptk_setup
static int tracking_setup(RicArgs& r, NoiseIn& n, int nprob, int chunk, int mx, int mu, int ml, int N, int nlin, int n_noise, const double* Wu, const double* Sigma0, int path,
                          const char* what) {
    const size_t np = (size_t)nprob;
    double* dwork = nullptr;
    int *dst = nullptr, *dkn = nullptr;
    ric_sizes(r, chunk, mx, mu, ml, N, (N > 1 && nlin > 1) ? 1 : 0, 0.0, path);
    TRY(upload_noise(mx, mu, n_noise, Wu, Sigma0, n, what));
    HIPTRY(what, ws_get((void**)&dwork, ric_total_work_doubles(r) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dst, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dkn, np * sizeof(int)));
    r.work = dwork; r.status = dst; r.kbreak = dkn;
    return CCLQR_OK;
}
// the shared part of a chunk's launch record, from the call's (problem 0 onwards) to that of the problems c0 .. c0 + nc - 1: their models (nlin per problem) lie at md,
// their gains in `tables` (the tables of ALL problems).  Callers: ctk_launch_chunk, ptk_launch_chunk
static void tracking_chunk(RicArgs& r, GainTable& k, NoiseIn& n, size_t c0, size_t nc, const RicModels& md, const GainTable& tables) {
    r.nprob = (int)nc; r.A = md.A; r.Bu = md.Bu; r.Bl = md.Bl; r.G = md.G;
    r.status += c0; r.kbreak += c0;
    k = tables; k.Kin += (long long)c0 * k.k_stride;
    if (n.Wu) n.Wu += (long long)c0 * n.wu_stride;
    if (n.Sigma0) n.Sigma0 += (long long)c0 * n.s0_stride;
}
// status and knot of every problem onto the host.  Callers: ctk_read_back, ptk_read_back
static int tracking_read_back(const RicArgs& r, int nprob, TrackOut& o, const char* what) {
    TRY(download(o.st, r.status, (size_t)nprob, what));
    return download(o.knot, r.kbreak, (size_t)nprob, what);
}
// the body the two raw entries share around their own setup, launch and report.  First what they refuse about sizes and pointers ...
static int tracking_raw_check(int nprob, int mx, int mu, int ml, int N, const double* A, const double* Bu, const double* Bl, const double* G, const double* K) {
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0 || N < 1) return fail(CCLQR_EINVAL, "bad sizes");
    if (N > 1 && (!A || (mu > 0 && (!Bu || !K)) || (ml > 0 && (!Bl || !G)))) return fail(CCLQR_EINVAL, "null argument");
    return CCLQR_OK;
}
// ... then raw_upload for a horizon of N knots (N = 1: no model and no gain is read) and, if asked for, the [nprob][N][mx][mx] matrices of every knot ...
static int tracking_raw_upload(const char* what, int nprob, int mx, int mu, int ml, int nlin, const double* A, const double* Bu, const double* Bl, const double* G, int n_gains,
                               int nK, const double* K, int N, bool want_all, AnaDev& d, double** dAll) {
    TRY(raw_upload(what, nprob, mx, mu, ml, N > 1 ? nlin : 0, A, Bu, Bl, G, n_gains, nK, N > 1, K, d));
    if (want_all) HIPTRY(what, ws_get((void**)dAll, (size_t)nprob * mx * mx * N * sizeof(double)));
    return CCLQR_OK;
}
// ... and after the read-back the matrices of the problems before the first one the call is refused for: the arrays are filled up to it
static int tracking_raw_matrices(const TrackOut& o, int nprob, int mx, int N, double* out, const double* dP, double* out_all, const double* dAll, const char* what) {
    int bad = nprob;
    for (int p = nprob - 1; p >= 0; p--) if (o.st[p] != 0) bad = p;
    if (out && bad > 0) HIPTRY(what, hipMemcpy(out, dP, (size_t)bad * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    if (out_all && bad > 0) HIPTRY(what, hipMemcpy(out_all, dAll, (size_t)bad * N * mx * mx * sizeof(double), hipMemcpyDeviceToHost));
    return CCLQR_OK;
}

// ---- the tracking covariance's own: what the entry refuses about its counts and its noise, before anything is allocated or launched
static int tracking_cov_check(int nprob, int mu, int N, int nlin, int n_gains, int nK, int n_weights, int n_noise, const double* Wu, const double* Sigma0, const double* Q,
                              const double* R, bool want_cost, const cclqr_riccati_opts* opts, const char* of) {
    TRY(tracking_counts_check(nprob, mu, N, nlin, n_gains, nK, of));
    if (want_cost) TRY(check_n_weights(n_weights, nprob, of));
    TRY(check_n_noise(n_noise, nprob, "Wu / Sigma0 are", of));
    if (!Wu && !Sigma0) return fail(CCLQR_EINVAL, "Wu and Sigma0 are both null: there is no covariance to propagate");
    if (Wu && mu == 0) return fail(CCLQR_EINVAL, "Wu is given with mu = 0: there is no input for the noise to enter through");
    if (want_cost && (!Q || (mu > 0 && !R))) return fail(CCLQR_EINVAL, "cost / total are asked for without Q / R");
    return tracking_launch_check(nprob, opts, "tracking covariance");
}
// fills c, inside the caller's WsScope, with the launch arguments of problem 0 onwards: tracking_setup, and the weights, records and totals of ALL nprob problems.
// Q, R: HOST (Q = null: no cost is asked for)
static int ctk_setup(int nprob, int chunk, int mx, int mu, int ml, int N, int nlin, int n_weights, const double* Q, const double* R, int n_noise, const double* Wu,
                     const double* Sigma0, int path, hipStream_t stream, CtkArgs& c) {
    static const char* const what = "tracking covariance";
    const size_t np = (size_t)nprob, mm = (size_t)mx * mx, uu = (size_t)mu * mu;
    c = CtkArgs{};
    if (Q) {
        TRY(upload_weights(mx, mu, n_weights, Q, R, c.w, what));
    } else {      // no cost asked for: the kernels form it against zero weights, written on the stream the kernels run on
        double *dQ = nullptr, *dR = nullptr;
        HIPTRY(what, ws_get((void**)&dQ, mm * sizeof(double)));
        HIPTRY(what, ws_get((void**)&dR, (uu + 1) * sizeof(double)));
        HIPTRY(what, hipMemsetAsync(dQ, 0, mm * sizeof(double), stream));
        HIPTRY(what, hipMemsetAsync(dR, 0, (uu + 1) * sizeof(double), stream));
        c.w.Q = dQ; c.w.R = dR;
    }
    TRY(tracking_setup(c.r, c.n, nprob, chunk, mx, mu, ml, N, nlin, n_noise, Wu, Sigma0, path, what));
    HIPTRY(what, ws_get((void**)&c.mom, np * N * (size_t)ctk_record(mx, mu) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&c.total, 2 * np * sizeof(double)));
    return CCLQR_OK;
}
// the recursion for the problems c0 .. c0 + nc - 1 on `stream` (tracking_chunk); dSigma [nprob][mx][mx] and dSigma_all [nprob][N][mx][mx] (or null) are the whole call's
static hipError_t ctk_launch_chunk(const CtkArgs& d, size_t c0, size_t nc, const RicModels& md, const GainTable& tables, double* dSigma, double* dSigma_all, hipStream_t stream) {
    CtkArgs c = d;
    const size_t mm = (size_t)c.r.mx * c.r.mx, N = (size_t)c.r.N, rec = (size_t)ctk_record(c.r.mx, c.r.mu);
    tracking_chunk(c.r, c.k, c.n, c0, nc, md, tables);
    c.w.Q += (long long)c0 * c.w.q_stride; c.w.R += (long long)c0 * c.w.r_stride;
    c.mom += c0 * N * rec; c.total += 2 * c0;
    c.Sigma = dSigma + c0 * mm;
    c.Sigma_all = dSigma_all ? dSigma_all + c0 * N * mm : nullptr;
    return launch_covariance_tracking(c, stream);
}
static int ctk_read_back(const CtkArgs& d, int nprob, TrackOut& o) {
    static const char* const what = "tracking covariance";
    const size_t np = (size_t)nprob;
    TRY(download(o.rec, d.mom, np * (size_t)d.r.N * (size_t)ctk_record(d.r.mx, d.r.mu), what));
    TRY(download(o.total, d.total, 2 * np, what));
    return tracking_read_back(d.r, nprob, o, what);
}
// the per-knot records into the caller's arrays (each may be null), for the problems before the one the call is refused for, which it names with its knot
static int tracking_cov_report(const TrackOut& o, int nprob, int mx, int mu, int N, double* cost, double* zstd, double* ustd, double* total, const char* of) {
    const size_t rec = (size_t)ctk_record(mx, mu);
    for (int p = 0; p < nprob; p++) {
        if (o.st[p] != 0) return singular_in(of, p, &o.knot[p]);
        for (int j = 0; j < N; j++) {
            const double* m = o.rec.data() + ((size_t)p * N + j) * rec;
            const size_t k = (size_t)p * N + j;
            if (cost) { cost[2 * k] = m[0]; cost[2 * k + 1] = m[1]; }
            if (zstd) memcpy(zstd + k * mx, m + 2, (size_t)mx * sizeof(double));
            if (ustd && mu > 0) memcpy(ustd + k * mu, m + 2 + mx, (size_t)mu * sizeof(double));
        }
        put_pair(total, o.total, p);
    }
    return CCLQR_OK;
}

extern "C" int cclqr_covariance_tracking(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, int32_t nlin, const double* A, const double* Bu, const double* Bl, const double* G,
                                         int32_t n_gains, int32_t nK, const double* K, int32_t n_weights, const double* Q, const double* R, int32_t n_noise, const double* Wu,
                                         const double* Sigma0, int32_t N, double* Sigma, double* Sigma_all, double* cost, double* zstd, double* ustd, double* total,
                                         const cclqr_riccati_opts* opts) {
    static const char* const what = "tracking covariance";
    TRY(tracking_raw_check(nprob, mx, mu, ml, N, A, Bu, Bl, G, K));
    const bool want_cost = cost || total;
    TRY(tracking_cov_check(nprob, mu, N, nlin, n_gains, nK, n_weights, n_noise, Wu, Sigma0, Q, R, want_cost, opts, "problem"));
    WsScope scope;
    AnaDev d;
    double* dAll = nullptr;
    TRY(tracking_raw_upload(what, nprob, mx, mu, ml, nlin, A, Bu, Bl, G, n_gains, nK, K, N, Sigma_all != nullptr, d, &dAll));
    TrackOut o;
    CtkArgs dev;
    TRY(ctk_setup(nprob, nprob, mx, mu, ml, N, nlin, n_weights, want_cost ? Q : nullptr, R, n_noise, Wu, Sigma0, opts ? opts->path : 0, nullptr, dev));
    HIPTRY(what, ctk_launch_chunk(dev, 0, (size_t)nprob, d.m, d.k, d.P, dAll, nullptr));
    HIPTRY(what, hipDeviceSynchronize());
    TRY(ctk_read_back(dev, nprob, o));
    TRY(tracking_raw_matrices(o, nprob, mx, N, Sigma, d.P, Sigma_all, dAll, what));
    return tracking_cov_report(o, nprob, mx, mu, N, cost, zstd, ustd, total, "problem");
}

// A knot-by-knot recursion for a CONTROLLER on a mechanism's plants, the ONE host sequence of the tracking analyses (cclqr_value_create_covariance_tracking,
// cclqr_value_create_policy_tracking): linearsystem at the knots 0 .. N-2 of trajectory k on plant first_plant + k (lqr_tracking.jl:88), the controller's gain rows
// gathered on the device, the problems in chunks within the workspace budget.  What an analysis brings of its own:
//   check(nlin, tables, nK)                        its refusals about counts, weights and noise, before anything is allocated or launched
//   plan(mx, ml, ric_per, ric_fixed, &per, &fixed) the bytes one problem adds to a chunk and the bytes the call holds once (tracking_cov_ / tracking_pol_problem_bytes)
//   setup(chunk, mx, ml, nlin, stream)             its launch arguments, inside this sequence's WsScope
//   launch(c0, nc, models, tables, P_dev, stream)  the recursion for the problems c0 .. c0 + nc - 1 on the chunk's models
//   report()                                       its read-back into the caller's arrays, after every knot has converged
template <class Check, class Plan, class Setup, class Launch, class Report>
static int tracking_value_on_plants(const char* what, const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, int32_t N, const double* zd,
                                    const double* Fd, int32_t on_device, int32_t mu, const int32_t* ctrl_joint, const cclqr_ctrl* c, int64_t workspace_bytes, void* stream,
                                    cclqr_value** out, Check check, Plan plan, Setup setup, Launch launch, Report report) {
    if (!m || !zd || !c || !out || (mu > 0 && !ctrl_joint)) return fail(CCLQR_EINVAL, "null argument");
    LinArgs la;
    memset(&la, 0, sizeof(la));
    int64_t tables = 1;
    TRY(policy_ctrl_check(m, plants, first_plant, n_models, mu, ctrl_joint, c, std::string("the ") + what, n_models < 1 || N < 1 || mu < 1 || mu > m->nb, false, la.cj, &tables));
    const CtrlDev& H = c->host;
    if (N > 1 && H.nK != 1 && H.nK != N - 1)
        return fail(CCLQR_EINVAL, "the controller's tables hold " + std::to_string(H.nK) + " gain rows: one (a stationary gain) or N - 1 = " + std::to_string(N - 1) + ", one per knot 0 .. N-2");
    const int nb = m->nb, mx = 12 * nb, ml = 5 * nb, nlin = N > 1 ? N - 1 : 1;
    TRY(check(nlin, (int)tables, H.nK));
    // the chunks the workspace budget allows, before anything is allocated
    RicArgs r1;
    ric_sizes(r1, 1, mx, mu, ml, N, nlin > 1 ? 1 : 0, 0.0, 0);
    RicArgs r2 = r1;
    r2.nprob = 2;
    const long long ric_per = (long long)(ric_total_work_doubles(r2) - ric_total_work_doubles(r1)), ric_fixed = (long long)ric_total_work_doubles(r1) - ric_per;
    long long per_bytes = 0, fixed_bytes = 0;
    plan(mx, ml, ric_per, ric_fixed, &per_bytes, &fixed_bytes);
    const long long budget = workspace_bytes > 0 ? (long long)workspace_bytes : CCLQR_TRACKING_WORKSPACE_BYTES;
    const long long per_chunk = tracking_chunk_problems(n_models, per_bytes, fixed_bytes, budget);
    if (per_chunk < 1)
        return fail(CCLQR_EINVAL, "workspace_bytes = " + std::to_string(budget) + " does not hold one problem: N = " + std::to_string(N) + " knots of this mechanism need " +
                                  std::to_string(fixed_bytes + per_bytes) + " bytes");
    const size_t np = (size_t)n_models, pc = (size_t)per_chunk, nk = (size_t)N - 1, nz = 13 * (size_t)nb, smx = (size_t)mx, sml = (size_t)ml, smu = (size_t)mu;
    hipStream_t st_ = (hipStream_t)stream;
    ValueOwner vown(value_new(m, n_models));
    HIPTRY(what, value_alloc(vown.p));
    struct StreamWait { hipStream_t s; ~StreamWait() { (void)hipStreamSynchronize(s); } };      // nothing of the call may still run on the blocks the scope below frees
    WsScope scope;
    StreamWait wait{st_};
    // the trajectories: a device array is read where it lies (the linearisation permutes as it loads), a host array is copied
    const double *dzd = zd, *dFd = Fd;
    if (!on_device && nk > 0) {
        double *uz = nullptr, *uf = nullptr;
        HIPTRY(what, ws_get((void**)&uz, np * N * nz * sizeof(double)));
        HIPTRY(what, hipMemcpy(uz, zd, np * N * nz * sizeof(double), hipMemcpyHostToDevice));
        dzd = uz;
        if (Fd) {
            HIPTRY(what, ws_get((void**)&uf, np * N * smu * sizeof(double)));
            HIPTRY(what, hipMemcpy(uf, Fd, np * N * smu * sizeof(double), hipMemcpyHostToDevice));
            dFd = uf;
        }
    }
    GainTable gains;
    TRY(gather_gains(m, c, mu, tables, st_, gains, what));
    RicModels md = {};
    int* dlst = nullptr;
    const size_t nkk = nk > 0 ? nk : 1;
    HIPTRY(what, ws_get((void**)&md.A, pc * nkk * smx * smx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&md.Bu, pc * nkk * smx * smu * sizeof(double)));
    HIPTRY(what, ws_get((void**)&md.Bl, pc * nkk * smx * sml * sizeof(double)));
    HIPTRY(what, ws_get((void**)&md.G, pc * nkk * sml * smx * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dlst, (np * nkk + 1) * sizeof(int)));
    TRY(setup((int)pc, mx, ml, nlin, st_));
    la.M = m->dev; la.mu = mu;
    la.plants = plants ? plants->dev : nullptr;
    la.knots_per_plant = (int)nk; la.rows_per_plant = N;
    la.A = md.A; la.Bu = md.Bu; la.Bl = md.Bl; la.G = md.G;
    for (size_t c0 = 0; c0 < np; c0 += pc) {
        const size_t nc = np - c0 < pc ? np - c0 : pc;
        if (nk > 0) {      // linearsystem at the knots 0 .. N-2 of the chunk's trajectories (lqr_tracking.jl:88), one launch; N = 1 reads no model
            la.nk = (int)(nc * nk);
            la.zd = dzd + c0 * (size_t)N * nz;
            la.Fd = dFd ? dFd + c0 * (size_t)N * smu : nullptr;
            la.plant_off = plants ? first_plant - plants->first_index + (long long)c0 : 0;
            la.status = dlst + c0 * nk;
            HIPTRY(what, launch_linearize(la, m->shape, st_));
        }
        HIPTRY(what, launch(c0, nc, md, gains, vown.p->P_dev, st_));
    }
    HIPTRY(what, hipStreamSynchronize(st_));
    long long bad = -1;
    if (nk > 0) HIPTRY(what, knots_converged(dlst, np * nk, &bad));
    if (bad >= 0)
        return fail(CCLQR_ENOCONV, "Newton did not converge at the setpoint of knot " + std::to_string((size_t)bad % nk) + " of table " + std::to_string((size_t)bad / nk));
    TRY(report());
    *out = vown.release();
    return CCLQR_OK;
}

extern "C" int cclqr_value_create_covariance_tracking(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, int32_t N, const double* zd,
                                                      const double* Fd, int32_t on_device, int32_t mu, const int32_t* ctrl_joint, const cclqr_ctrl* c, int32_t n_weights,
                                                      const double* Q, const double* R, int32_t n_noise, const double* Wu, const double* Sigma0, int64_t workspace_bytes,
                                                      double* cost, double* zstd, double* ustd, double* total, void* stream, cclqr_value** out) {
    const bool want_cost = cost || total;
    CtkArgs dev;
    return tracking_value_on_plants(
        "tracking covariance", m, plants, first_plant, n_models, N, zd, Fd, on_device, mu, ctrl_joint, c, workspace_bytes, stream, out,
        [&](int nlin, int tables, int nK) { return tracking_cov_check(n_models, mu, N, nlin, tables, nK, n_weights, n_noise, Wu, Sigma0, Q, R, want_cost, nullptr, "model"); },
        [&](int mx, int ml, long long ric_per, long long ric_fixed, long long* per, long long* fixed) {
            *per = tracking_cov_problem_bytes(mx, mu, ml, N, ric_per);
            *fixed = tracking_cov_fixed_bytes(mx, mu, ric_fixed, want_cost ? n_weights : 1, n_noise);
        },
        [&](int chunk, int mx, int ml, int nlin, hipStream_t st) {
            return ctk_setup(n_models, chunk, mx, mu, ml, N, nlin, n_weights, want_cost ? Q : nullptr, R, n_noise, Wu, Sigma0, 0, st, dev);
        },
        [&](size_t c0, size_t nc, const RicModels& md, const GainTable& gains, double* P_dev, hipStream_t st) {
            return ctk_launch_chunk(dev, c0, nc, md, gains, P_dev, nullptr, st);
        },
        [&]() {
            TrackOut o;
            TRY(ctk_read_back(dev, n_models, o));
            return tracking_cov_report(o, n_models, dev.r.mx, mu, N, cost, zstd, ustd, total, "table");
        });
}

// ---- the tracking policy value's own: what the entry refuses about its counts and its noise, before anything is allocated or launched: tracking_cov_check's list, and
// a price without a noise
static int tracking_pol_check(int nprob, int mu, int N, int nlin, int n_gains, int nK, int n_weights, int n_noise, const double* Wu, const double* Q, const double* R,
                              const double* price, const double* noise_total, int knot, const cclqr_riccati_opts* opts, const char* of) {
    TRY(tracking_counts_check(nprob, mu, N, nlin, n_gains, nK, of));
    TRY(check_n_weights(n_weights, nprob, of));
    TRY(check_n_noise(n_noise, nprob, "Wu is", of));
    if (Wu && mu == 0) return fail(CCLQR_EINVAL, "Wu is given with mu = 0: there is no input for the noise to enter through");
    if (!Wu && (price || noise_total)) return fail(CCLQR_EINVAL, "price / noise_total are asked for without Wu: there is no noise to price");
    if (!Q || (mu > 0 && !R)) return fail(CCLQR_EINVAL, "the cost-to-go needs Q / R");
    if (knot < 0 || knot > N - 1) return fail(CCLQR_EINVAL, "knot = " + std::to_string(knot) + ": the cost-to-go is that of a knot in 0 .. N-1 = " + std::to_string(N - 1));
    return tracking_launch_check(nprob, opts, "tracking policy value");
}
// fills c, inside the caller's WsScope, with the launch arguments of problem 0 onwards: tracking_setup, and the weights, prices and totals of ALL nprob problems.
// Q, R: HOST, as the entries take them
static int ptk_setup(int nprob, int chunk, int mx, int mu, int ml, int N, int nlin, int knot, int n_weights, const double* Q, const double* R, int n_noise, const double* Wu,
                     int path, PtkArgs& c) {
    static const char* const what = "tracking policy value";
    const size_t np = (size_t)nprob;
    c = PtkArgs{};
    WeightsIn w;
    TRY(upload_weights(mx, mu, n_weights, Q, R, w, what));
    ric_weights(c.r, w);
    TRY(tracking_setup(c.r, c.n, nprob, chunk, mx, mu, ml, N, nlin, n_noise, Wu, nullptr, path, what));
    if (Wu) {
        HIPTRY(what, ws_get((void**)&c.price, np * N * sizeof(double)));
        HIPTRY(what, ws_get((void**)&c.total, np * sizeof(double)));
    }
    c.knot = knot;
    return CCLQR_OK;
}
// the recursion for the problems c0 .. c0 + nc - 1 on `stream` (tracking_chunk); dP [nprob][mx][mx] (or null) and dP_all [nprob][N][mx][mx] (or null) are the whole call's
static hipError_t ptk_launch_chunk(const PtkArgs& d, size_t c0, size_t nc, const RicModels& md, const GainTable& tables, double* dP, double* dP_all, hipStream_t stream) {
    PtkArgs c = d;
    const size_t mm = (size_t)c.r.mx * c.r.mx, N = (size_t)c.r.N;
    tracking_chunk(c.r, c.k, c.n, c0, nc, md, tables);
    c.r.Q += (long long)c0 * c.r.q_stride; c.r.R += (long long)c0 * c.r.r_stride;
    if (c.n.Wu) { c.price += c0 * N; c.total += c0; }
    c.P = dP ? dP + c0 * mm : nullptr;
    c.P_all = dP_all ? dP_all + c0 * N * mm : nullptr;
    return launch_policy_tracking(c, stream);
}
static int ptk_read_back(const PtkArgs& d, int nprob, TrackOut& o) {
    static const char* const what = "tracking policy value";
    const size_t np = (size_t)nprob;
    if (d.price) {
        TRY(download(o.rec, d.price, np * (size_t)d.r.N, what));
        TRY(download(o.total, d.total, np, what));
    }
    return tracking_read_back(d.r, nprob, o, what);
}
// the prices into the caller's arrays (each may be null), for the problems before the one the call is refused for, which it names with its knot
static int tracking_pol_report(const TrackOut& o, int nprob, int N, double* price, double* noise_total, const char* of) {
    for (int p = 0; p < nprob; p++) {
        if (o.st[p] != 0) return singular_in(of, p, &o.knot[p]);
        if (price) memcpy(price + (size_t)p * N, o.rec.data() + (size_t)p * N, (size_t)N * sizeof(double));
        if (noise_total) noise_total[p] = o.total[(size_t)p];
    }
    return CCLQR_OK;
}

extern "C" int cclqr_policy_value_tracking(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, int32_t nlin, const double* A, const double* Bu, const double* Bl, const double* G,
                                           int32_t n_gains, int32_t nK, const double* K, int32_t n_weights, const double* Q, const double* R, int32_t n_noise, const double* Wu,
                                           int32_t N, double* P, double* P_all, double* price, double* noise_total, const cclqr_riccati_opts* opts) {
    static const char* const what = "tracking policy value";
    TRY(tracking_raw_check(nprob, mx, mu, ml, N, A, Bu, Bl, G, K));
    TRY(tracking_pol_check(nprob, mu, N, nlin, n_gains, nK, n_weights, n_noise, Wu, Q, R, price, noise_total, 0, opts, "problem"));
    WsScope scope;
    AnaDev d;
    double* dAll = nullptr;
    TRY(tracking_raw_upload(what, nprob, mx, mu, ml, nlin, A, Bu, Bl, G, n_gains, nK, K, N, P_all != nullptr, d, &dAll));
    TrackOut o;
    PtkArgs dev;
    TRY(ptk_setup(nprob, nprob, mx, mu, ml, N, nlin, 0, n_weights, Q, R, n_noise, Wu, opts ? opts->path : 0, dev));
    HIPTRY(what, ptk_launch_chunk(dev, 0, (size_t)nprob, d.m, d.k, d.P, dAll, nullptr));
    HIPTRY(what, hipDeviceSynchronize());
    TRY(ptk_read_back(dev, nprob, o));
    TRY(tracking_raw_matrices(o, nprob, mx, N, P, d.P, P_all, dAll, what));
    return tracking_pol_report(o, nprob, N, price, noise_total, "problem");
}

// the same recursion for a CONTROLLER on a mechanism's plants, down to `knot`: tracking_value_on_plants with the policy's plan (tracking_pol_problem_bytes)
extern "C" int cclqr_value_create_policy_tracking(const cclqr_mech* m, const cclqr_plants* plants, int64_t first_plant, int32_t n_models, int32_t N, const double* zd,
                                                  const double* Fd, int32_t on_device, int32_t mu, const int32_t* ctrl_joint, const cclqr_ctrl* c, int32_t n_weights,
                                                  const double* Q, const double* R, int32_t n_noise, const double* Wu, int32_t knot, int64_t workspace_bytes, double* price,
                                                  double* noise_total, void* stream, cclqr_value** out) {
    PtkArgs dev;
    return tracking_value_on_plants(
        "tracking policy value", m, plants, first_plant, n_models, N, zd, Fd, on_device, mu, ctrl_joint, c, workspace_bytes, stream, out,
        [&](int nlin, int tables, int nK) { return tracking_pol_check(n_models, mu, N, nlin, tables, nK, n_weights, n_noise, Wu, Q, R, price, noise_total, knot, nullptr, "model"); },
        [&](int mx, int ml, long long ric_per, long long ric_fixed, long long* per, long long* fixed) {
            *per = tracking_pol_problem_bytes(mx, mu, ml, N, ric_per);
            *fixed = tracking_pol_fixed_bytes(mx, mu, ric_fixed, n_weights, Wu ? n_noise : 0);
        },
        [&](int chunk, int mx, int ml, int nlin, hipStream_t) { return ptk_setup(n_models, chunk, mx, mu, ml, N, nlin, knot, n_weights, Q, R, n_noise, Wu, 0, dev); },
        [&](size_t c0, size_t nc, const RicModels& md, const GainTable& gains, double* P_dev, hipStream_t st) {
            return ptk_launch_chunk(dev, c0, nc, md, gains, P_dev, nullptr, st);
        },
        [&]() {
            TrackOut o;
            TRY(ptk_read_back(dev, n_models, o));
            return tracking_pol_report(o, n_models, N, price, noise_total, "table");
        });
}

// ---- the Riccati map itself by doubling (riccati_doubling.hip): Ku[1] and the last Pkp1 of lqr.jl:141-184 after N - 1 steps, or at convergence (lqr.jl:25-27, 39-43)
extern "C" int cclqr_riccati_doubling(int32_t nprob, int32_t mx, int32_t mu, int32_t ml, const double* A, const double* Bu, const double* Bl, const double* G,
                                      int32_t n_weights, const double* Q, const double* R, int32_t N, double tol, int32_t max_levels, double* K, double* P,
                                      int32_t* levels, int32_t* reason, double* dnorm, double* anorm, const cclqr_riccati_opts* opts) {
    static const char* const what = "riccati doubling";
    if (!A || !Q || (mu > 0 && (!Bu || !R || !K)) || (ml > 0 && (!Bl || !G))) return fail(CCLQR_EINVAL, "null argument");
    if (nprob < 1 || mx < 1 || mu < 0 || ml < 0) return fail(CCLQR_EINVAL, "bad sizes");
    TRY(check_n_weights(n_weights, nprob, "problem"));
    TRY(riccati_doubling_check(N, tol, max_levels, opts, mx, mu, n_weights, Q, R));
    WsScope scope;
    RicModels d = {};
    TRY(upload_models((size_t)nprob, mx, mu, ml, A, Bu, Bl, G, d));
    const size_t np = (size_t)nprob, nK = np * mu * mx, nP = np * mx * mx;
    double *dK = nullptr, *dP = nullptr, *dwork = nullptr, *dwork2 = nullptr, *ddn = nullptr, *dan = nullptr;
    int *dlv = nullptr, *drs = nullptr, *dst = nullptr, *dstop = nullptr;
    RdbArgs a;
    RicArgs& r = a.r;
    WeightsIn w;
    ric_sizes(r, nprob, mx, mu, ml, N, 0, tol, 0, 1);
    TRY(upload_weights(mx, mu, n_weights, Q, R, w, what));
    ric_weights(r, w);
    HIPTRY(what, ws_get((void**)&dK, (nK + 1) * sizeof(double)));
    if (P) HIPTRY(what, ws_get((void**)&dP, nP * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dwork, ric_total_work_doubles(r) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dwork2, rdb_work_doubles(nprob, mx) * sizeof(double)));
    HIPTRY(what, ws_get((void**)&ddn, 2 * np * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dan, 2 * np * sizeof(double)));
    HIPTRY(what, ws_get((void**)&dstop, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dlv, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&drs, np * sizeof(int)));
    HIPTRY(what, ws_get((void**)&dst, np * sizeof(int)));
    HIPTRY(what, hipMemset(dK, 0, (nK + 1) * sizeof(double)));
    r.stop = dstop; r.A = d.A; r.Bu = d.Bu; r.Bl = d.Bl; r.G = d.G; r.K = dK; r.kbreak = nullptr; r.status = dst; r.work = dwork; r.P_out = dP;
    a.max_levels = max_levels; a.work2 = dwork2; a.levels = dlv; a.reason = drs; a.dnorm = ddn; a.anorm = dan;
    HIPTRY(what, launch_riccati_doubling(a, nullptr));
    DblOut o;
    TRY(doubling_read_back(np, dlv, drs, dst, ddn, dan, o, what));
    if (nK) HIPTRY(what, hipMemcpy(K, dK, nK * sizeof(double), hipMemcpyDeviceToHost));
    if (P) HIPTRY(what, hipMemcpy(P, dP, nP * sizeof(double), hipMemcpyDeviceToHost));
    return doubling_report(o, nprob, levels, reason, dnorm, anorm, "problem");
}

