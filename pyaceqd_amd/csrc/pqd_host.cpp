// pqd_host.cpp — C-ABI implementation of libpqd (include/pqd.h): validation, Liouvillian /
// superoperator construction, MTO scheduling, trajectory grouping, device buffers, launches.
// No arithmetic of the propagation itself happens on the host: the free propagators, the PT
// sweep, traces and the map-chain sweeps all run in the HIP kernels (free_prop.hip, pt_sweep.hip,
// mapchain.hip). Host code only assembles constant N^2 x N^2 generators from N x N operators.
#include "../../include/pqd.h"
#include "pqd_common.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <memory>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

using cd = std::complex<double>;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) return fail(PQD_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                 \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc((void**)&p, count * sizeof(T));
    }
    hipError_t upload(const T* src, size_t count, hipStream_t s) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || count == 0) return e;
        return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

const cd* C(const pqd_c128* p) { return reinterpret_cast<const cd*>(p); }

int pad_chi(int chi) {
    if (chi <= 16) return 16;
    if (chi <= 32) return 32;
    if (chi <= 64) return 64;
    if (chi <= 128) return 128;
    if (chi <= 256) return 256;  // multi-trajectory split groups only (pt_msplit.hip, slice rows streamed)
    return -1;
}

// ---- superoperators in the row-major vec convention: vec(A rho B) = (A (x) B^T) vec(rho)
void kron_left(int N, const cd* A, cd* S, cd f) {  // S += f * (A (x) I)
    const int N2 = N * N;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < N; ++k) S[(size_t)(i * N + j) * N2 + (k * N + j)] += f * A[i * N + k];
}
void kron_right(int N, const cd* B, cd* S, cd f) {  // S += f * (I (x) B^T): rho -> rho B
    const int N2 = N * N;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            for (int l = 0; l < N; ++l) S[(size_t)(i * N + j) * N2 + (i * N + l)] += f * B[l * N + j];
}
void commutator(int N, const cd* H, double hbar, cd* S) {  // S += -i/hbar [H, .]
    const cd f(0.0, -1.0 / hbar);
    kron_left(N, H, S, f);
    kron_right(N, H, S, -f);
}
void dissipator(int N, const cd* Lk, double g, cd* S) {  // S += g (L . L^dag - 1/2 {L^dag L, .})
    const int N2 = N * N;
    std::vector<cd> LdL(N * N);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            cd s = 0;
            for (int k = 0; k < N; ++k) s += std::conj(Lk[k * N + i]) * Lk[k * N + j];
            LdL[i * N + j] = s;
        }
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            for (int k = 0; k < N; ++k)
                for (int l = 0; l < N; ++l)
                    S[(size_t)(i * N + j) * N2 + (k * N + l)] += g * Lk[i * N + k] * std::conj(Lk[j * N + l]);
    kron_left(N, LdL.data(), S, cd(-0.5 * g));
    kron_right(N, LdL.data(), S, cd(-0.5 * g));
}
void matmul_sq(int n, const cd* A, const cd* B, cd* Cm) {
    std::vector<cd> t((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) {
            const cd a = A[(size_t)i * n + k];
            for (int j = 0; j < n; ++j) t[(size_t)i * n + j] += a * B[(size_t)k * n + j];
        }
    std::copy(t.begin(), t.end(), Cm);
}

// max_dim: 6 wherever N^2 x N^2 superoperators are built; HB_NMAX for a plan without PT (lind_hilbert.hip)
int check_system(const pqd_system* sys, int max_dim = 6) {
    if (!sys) return fail(PQD_ERR_ARG, "system is NULL");
    if (sys->dim < 2 || sys->dim > max_dim)
        return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [2, %d]", sys->dim, max_dim);
    if (!sys->H0) return fail(PQD_ERR_ARG, "H0 is NULL");
    if (!(sys->hbar > 0)) return fail(PQD_ERR_ARG, "hbar must be > 0");
    if (sys->n_lind < 0 || (sys->n_lind > 0 && (!sys->lind_ops || !sys->lind_rates)))
        return fail(PQD_ERR_ARG, "bad Lindblad arguments");
    if (sys->n_chan < 0 || sys->n_chan > 4) return fail(PQD_ERR_UNSUPPORTED, "n_chan %d not in [0, 4]", sys->n_chan);
    if (sys->n_chan > 0 && (!sys->chan_ops || !sys->chan_samples || sys->n_samples < 1 || !(sys->sample_dt > 0)))
        return fail(PQD_ERR_ARG, "bad pulse-channel arguments");
    return PQD_OK;
}

int check_grid(const pqd_grid* g) {
    if (!g) return fail(PQD_ERR_ARG, "grid is NULL");
    if (g->n_steps < 0) return fail(PQD_ERR_ARG, "n_steps < 0");
    if (!(g->dt > 0)) return fail(PQD_ERR_ARG, "dt must be > 0");
    if (g->n_sub < 1 || g->n_sub > 64) return fail(PQD_ERR_ARG, "n_sub %d not in [1, 64]", g->n_sub);
    return PQD_OK;
}

struct Generators {
    std::vector<cd> L0, S, T, samples;
};

void build_generators(const pqd_system* sys, Generators& G) {
    const int N = sys->dim, N2 = N * N;
    const size_t m2 = (size_t)N2 * N2;
    G.L0.assign(m2, 0.0);
    commutator(N, C(sys->H0), sys->hbar, G.L0.data());
    for (int q = 0; q < sys->n_lind; ++q)
        dissipator(N, C(sys->lind_ops) + (size_t)q * N * N, sys->lind_rates[q], G.L0.data());
    const int nc = sys->n_chan;
    G.S.assign(std::max<size_t>(1, nc * m2), 0.0);
    G.T.assign(std::max<size_t>(1, nc * m2), 0.0);
    for (int p = 0; p < nc; ++p) {
        const cd* X = C(sys->chan_ops) + (size_t)p * N * N;
        std::vector<cd> Xd(N * N);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) Xd[i * N + j] = std::conj(X[j * N + i]);
        commutator(N, X, sys->hbar, G.S.data() + p * m2);
        commutator(N, Xd.data(), sys->hbar, G.T.data() + p * m2);
    }
    if (nc > 0)
        G.samples.assign(C(sys->chan_samples), C(sys->chan_samples) + (size_t)nc * sys->n_samples);
    else
        G.samples.assign(1, 0.0);
}

}  // namespace

// =================================================================================================
struct pqd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // map-chain sweeps: one device arena reused across calls (grown on demand), so a call allocates nothing
    DevBuf<char> mc_arena;
    double dressed_ms = -1.0;  // kernel duration of the last pqd_dressed_states call (pqd_dressed_timing)
    double dynmap_ms = -1.0;   // duration of the map instance of the last pqd_dynmap_wide call (pqd_dynmap_timing)
    double tlmap_ms = -1.0;    // kernel duration of the last pqd_tl_dynmap_pseudo call (pqd_tl_dynmap_timing)
    int tlmap_sweeps = -1;     // its largest Jacobi sweep count (either kernel)
    double mcw_ms = -1.0;      // kernel duration of the last wide map-chain call (pqd_mc_wide_timing)
    int mcw_launches = 0;      // its kernel launches
};

namespace {
int Q_of(const std::vector<int>& pos, int n_tau) {
    int q = 0;
    for (int v : pos) q = std::max(q, v + n_tau);
    return q;
}

// write one byte per 4 KiB page of a host output buffer (its contents are overwritten afterwards), on up to 8
// threads for buffers of several MB
void touch_pages(void* buf, size_t bytes) {
    if (bytes < ((size_t)1 << 20)) return;
    char* b = static_cast<char*>(buf);
    const int nth = (int)std::min<size_t>(8, bytes >> 22) + 1;
    const size_t chunk = ((bytes / nth) + 4095) & ~(size_t)4095;
    auto work = [=](int k) {
        volatile char* q = b;
        for (size_t o = (size_t)k * chunk; o < std::min(bytes, (size_t)(k + 1) * chunk); o += 4096) q[o] = 0;
    };
    std::vector<std::thread> th;
    int k_started = 1;
    try {
        for (; k_started < nth; ++k_started) th.emplace_back(work, k_started);
    } catch (...) {  // no thread could be started: touch the remaining chunks here (no exception crosses the C-ABI)
    }
    for (int k = k_started; k < nth; ++k) work(k);
    work(0);
    for (auto& t : th) t.join();
}

// 64-bit FNV-1a over a host array's bytes, chained through h (the table hashes of pqd_plan_describe)
template <class T>
uint64_t fnv1a(const std::vector<T>& v, uint64_t h = 14695981039346656037ull) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
}  // namespace

struct pqd_pt {
    pqd_ctx* ctx = nullptr;
    int dim = 0, chi = 0, CHI = 0, D = 0, n_slices = 0;
    DevBuf<double2> Q, closure, closure0, bond0;
    DevBuf<double> Qsum;      // Re + Im of every slice element (the 3M operand of the TLS quad kernel; N2 = 4 only)
    DevBuf<int> gmap;
    std::vector<int> gmap_h;  // host copy: the plan derives its PT row units from it
    bool wide = false;        // pqd_pt_create_wide: slices as given (CHI = chi), for lind_hilbert_pt.hip only
};

struct pqd_plan {
    pqd_ctx* ctx = nullptr;
    int N2 = 0, CHI = 1, BT = 4, n_traj = 0, n_blocks = 0, n_steps = 0, n_sys = 1;
    bool nopt = true;
    bool split = false;  // small batch: one trajectory over N2 workgroups (pt_split.hip)
    bool quad = false;   // two-level system: register-resident quads (pt_quad.hip), blocks of BT = 4
    int qpw = 2;         // quads per workgroup (PQD_QPW)
    int qcg = 4;         // 4-column groups per wave (PQD_QCG; auto: 2 when the quads do not fill the CUs)
    int split_chunk = 0; // split groups: trajectories per launch when the batch exceeds the device (0: one launch)
    // split groups carrying several trajectories each (pt_msplit.hip): composite MTO operators, groups, exchange
    bool msplit = false;
    MsplitParams mq{};
    int n_cev = 0;
    DevBuf<int> ms_gtraj, ms_gend, cev_start;
    DevBuf<int4> cev;
    DevBuf<double2> Fev, Wev, msX;
    DevBuf<unsigned> ms_cnt;
    DevBuf<double2> Xs;
    DevBuf<unsigned> cnt, err;
    DevBuf<double2> L0, S, T, samples, M, Midle, F, W, rho0, ovec, sop, out;
    DevBuf<double2> Fidle, Widle;  // idle fused operators per system (pulse windows)
    DevBuf<int2> win;              // per-system pulse windows (free_prop.hip free_win_kernel), PQD_WIN=0: none
    int win_mode = 0;              // PQD_WIN: 1 auto (windows when they leave out >= 10% of the half steps), 2 always
    DevBuf<FreePropSys> systab;
    FuseParams fu{};
    DevBuf<int> sched, blk_traj, blk_end, blk_sys, blk_act, blk_src, traj_sys, wbeg, wend, ev_start;
    DevBuf<int> blk_fast;         // per block: first step of the lean instance's fast region (block_fast_steps)
    bool lean_ro = false;         // some block of a lean plan has fast steps (pqd_plan_sweep_readout)
    DevBuf<int> blk_stage;        // per block: the one system whose column operands the fast region stages, or -1
    int n_stage = 0;              // blocks of a lean plan that stage (pqd_plan_sweep_stage)
    std::vector<int> h_unit0;     // per wave: the slice of its first PT row unit (< 0: the wave has none)
    // Liouville rows the main batched sweep contracts with the PT (live_row_mask; all 1 where the plan skips none:
    // PQD_LIVE_ROWS=0, another path, no PT) and whether synchronize verifies the operators' zero blocks (PQD_LIVE_ROWS=2)
    std::vector<uint8_t> live;
    bool live_check = false;
    int64_t traj_steps = 0;       // executed trajectory-steps per execute (shared trunks counted once)
    int branch = 1;               // shared-trunk activation in the batched sweep (PQD_BRANCH)
    // trunk pre-pass (pqd_host.cpp plan_trunks): one MTO-free trajectory per system writes the checkpoints the
    // main sweep's slots start from
    int n_trunk = 0, tk_blocks = 0, tk_BT = 4;
    int tk_chunk = 0;  // split trunks per launch when they do not all fit the device at once (0: one launch)
    bool tk_split = false;
    SweepParams tk{};
    DevBuf<double2> ck, tk_out, tk_Xs;
    DevBuf<int> tk_ckmap, tk_wbeg, tk_wend, tk_evstart, tk_tsys, tk_blk_traj, tk_blk_end, tk_blk_sys, tk_blk_act,
        tk_blk_src;
    DevBuf<long long> tk_woff;
    DevBuf<int4> tk_units;
    DevBuf<unsigned> tk_cnt, tk_err;
    DevBuf<long long> woff;
    DevBuf<int4> ev, units;
    FreePropParams fp{};
    SweepParams sp{};
    // Hilbert-space path (lind_hilbert.hip): N x N operators per system, jump operators as nonzero lists by rows; the
    // plan's M, F, W, blocks, trunks and superoperators stay empty
    bool hilbert = false;
    HilbertParams hp{};
    // the same with a wide PT (lind_hilbert_pt.hip): hp plus the bond workspace and the PT units
    bool hilbert_pt = false;
    HilbertPtParams hq{};
    DevBuf<double2> hq_X;
    DevBuf<int> hq_unit_g, hq_unit_el;
    DevBuf<HilbertSys> hb_systab;
    DevBuf<double2> hb_K0, hb_Xs, hb_Xt, hb_val, hb_valg;
    DevBuf<int> hb_row, hb_col;
    int64_t out_len = 0;
    int n_out = 0;
    double t_start = 0.0, dt = 0.0;
    std::vector<long long> toff;  // ACE-table offsets per trajectory ((1 + n_out) rows of its window), + total
    DevBuf<long long> toff_d;
    DevBuf<double2> table;
    DevBuf<unsigned> flags;       // bit 0: non-finite output (PQD_ERR_NUMERIC)
    int split_fallbacks = 0;      // split launches that timed out and were re-run on the batched kernel
    // pqd_plan_describe: the device's CU count and FNV-1a hashes of the block arrays, the PT row-unit list and the
    // multi-trajectory group tables as uploaded (0: the plan has none)
    int n_cu = 0;
    uint64_t h_blocks = 0, h_units = 0, h_groups = 0;
    // hipEvent triplets (start, free propagators done, sweep done) of the last RING executes, created once
    static constexpr int RING = 64;
    hipEvent_t ring[3 * RING] = {};
    bool ring_ready = false;
    int ev_head = 0, ev_count = 0;  // next slot; executes recorded since the last timing reset (<= RING kept)
    int32_t execs = 0;
    ~pqd_plan() {
        if (ring_ready)
            for (auto& e : ring) (void)hipEventDestroy(e);
    }
};


// upload the generators of n_sys systems into concatenated device buffers + a device table
static int upload_systems(int n_sys, const pqd_system* systems, hipStream_t s, DevBuf<double2>& L0,
                          DevBuf<double2>& S, DevBuf<double2>& T, DevBuf<double2>& smp, DevBuf<FreePropSys>& tab) {
    const int N = systems[0].dim, N2 = N * N;
    const size_t m2 = (size_t)N2 * N2;
    std::vector<Generators> G(n_sys);
    size_t nS = 0, nT = 0, nsmp = 0;
    for (int k = 0; k < n_sys; ++k) {
        build_generators(&systems[k], G[k]);
        nS += G[k].S.size(); nT += G[k].T.size(); nsmp += G[k].samples.size();
    }
    std::vector<cd> l0((size_t)n_sys * m2), sv, tv, sm;
    sv.reserve(nS); tv.reserve(nT); sm.reserve(nsmp);
    std::vector<size_t> oS, oT, oM;
    for (int k = 0; k < n_sys; ++k) {
        std::copy(G[k].L0.begin(), G[k].L0.end(), l0.begin() + k * m2);
        oS.push_back(sv.size()); sv.insert(sv.end(), G[k].S.begin(), G[k].S.end());
        oT.push_back(tv.size()); tv.insert(tv.end(), G[k].T.begin(), G[k].T.end());
        oM.push_back(sm.size()); sm.insert(sm.end(), G[k].samples.begin(), G[k].samples.end());
    }
    HIPCHK(L0.upload(reinterpret_cast<double2*>(l0.data()), l0.size(), s));
    HIPCHK(S.upload(reinterpret_cast<double2*>(sv.data()), sv.size(), s));
    HIPCHK(T.upload(reinterpret_cast<double2*>(tv.data()), tv.size(), s));
    HIPCHK(smp.upload(reinterpret_cast<double2*>(sm.data()), sm.size(), s));
    std::vector<FreePropSys> t(n_sys);
    for (int k = 0; k < n_sys; ++k) {
        const pqd_system& y = systems[k];
        t[k].L0 = L0.p + k * m2;
        t[k].S = S.p + oS[k];
        t[k].T = T.p + oT[k];
        t[k].samples = smp.p + oM[k];
        t[k].n_chan = y.n_chan;
        t[k].n_samples = std::max(1, y.n_samples);
        t[k].s_t0 = y.sample_t0;
        t[k].s_dt = y.n_chan > 0 ? y.sample_dt : 1.0;
    }
    HIPCHK(tab.upload(t.data(), t.size(), s));
    return PQD_OK;
}

extern "C" {

int32_t pqd_version(void) { return 1; }
const char* pqd_last_error(void) { return g_err.c_str(); }
int pqd_hip_versions(int32_t* build, int32_t* runtime) {
    if (!build || !runtime) return fail(PQD_ERR_ARG, "NULL argument");
    *build = HIP_VERSION;
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) return fail(PQD_ERR_HIP, "hipRuntimeGetVersion failed");
    *runtime = v;
    return PQD_OK;
}

int pqd_ctx_create(int32_t device, pqd_ctx** out) {
    if (!out) return fail(PQD_ERR_ARG, "out is NULL");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(PQD_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PQD_ERR_UNSUPPORTED, "libpqd is built for gfx950 (MI355X); device is %s", prop.gcnArchName);
    auto* c = new pqd_ctx;
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(PQD_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    *out = c;
    return PQD_OK;
}

void pqd_ctx_destroy(pqd_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int pqd_ctx_synchronize(pqd_ctx* ctx) {
    if (!ctx) return fail(PQD_ERR_ARG, "ctx is NULL");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PQD_OK;
}

int pqd_pt_create(pqd_ctx* ctx, int32_t dim, const pqd_pt_desc* d, pqd_pt** out) {
    if (!ctx || !d || !out) return fail(PQD_ERR_ARG, "NULL argument");
    if (dim < 2 || dim > 6) return fail(PQD_ERR_UNSUPPORTED, "dim %d", dim);
    const int N2 = dim * dim;
    const int CHI = pad_chi(d->chi);
    if (d->chi < 1 || CHI < 0) return fail(PQD_ERR_UNSUPPORTED, "chi %d not in [1, 256]", d->chi);
    if (d->D < 1 || d->n_slices < 1) return fail(PQD_ERR_ARG, "D and n_slices must be >= 1");
    if (!d->Q || !d->closure || !d->closure0 || !d->bond0 || !d->gmap) return fail(PQD_ERR_ARG, "NULL PT array");
    for (int a = 0; a < N2; ++a)
        if (d->gmap[a] < 0 || d->gmap[a] >= d->D) return fail(PQD_ERR_ARG, "gmap[%d]=%d out of [0,%d)", a, d->gmap[a], d->D);
    HIPCHK(hipSetDevice(ctx->device));
    const int chi = d->chi;
    const size_t qn = (size_t)d->n_slices * d->D * CHI * CHI;
    std::vector<double2> Q(qn, make_double2(0, 0)), cl((size_t)d->n_slices * CHI, make_double2(0, 0));
    std::vector<double2> c0(CHI, make_double2(0, 0)), b0(CHI, make_double2(0, 0));
    const double2* src = reinterpret_cast<const double2*>(d->Q);
    for (size_t s = 0; s < (size_t)d->n_slices * d->D; ++s)
        for (int r = 0; r < chi; ++r)
            std::memcpy(&Q[(s * CHI + r) * CHI], &src[(s * chi + r) * chi], sizeof(double2) * chi);
    for (int s = 0; s < d->n_slices; ++s)
        std::memcpy(&cl[(size_t)s * CHI], reinterpret_cast<const double2*>(d->closure) + (size_t)s * chi,
                    sizeof(double2) * chi);
    std::memcpy(c0.data(), d->closure0, sizeof(double2) * chi);
    std::memcpy(b0.data(), d->bond0, sizeof(double2) * chi);
    auto* pt = new pqd_pt;
    pt->ctx = ctx; pt->dim = dim; pt->chi = chi; pt->CHI = CHI; pt->D = d->D; pt->n_slices = d->n_slices;
    pt->gmap_h.assign(d->gmap, d->gmap + N2);
    hipError_t e = pt->Q.upload(Q.data(), qn, ctx->stream);
    if (e == hipSuccess && N2 == 4) {
        std::vector<double> qs(qn);
        for (size_t k = 0; k < qn; ++k) qs[k] = Q[k].x + Q[k].y;
        e = pt->Qsum.upload(qs.data(), qn, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // qs goes out of scope
    }
    if (e == hipSuccess) e = pt->closure.upload(cl.data(), cl.size(), ctx->stream);
    if (e == hipSuccess) e = pt->closure0.upload(c0.data(), CHI, ctx->stream);
    if (e == hipSuccess) e = pt->bond0.upload(b0.data(), CHI, ctx->stream);
    if (e == hipSuccess) e = pt->gmap.upload(d->gmap, N2, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        delete pt;
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "PT upload: %s", hipGetErrorString(e));
    }
    *out = pt;
    return PQD_OK;
}

int pqd_pt_create_wide(pqd_ctx* ctx, int32_t dim, const pqd_pt_desc* d, pqd_pt** out) {
    if (!ctx || !d || !out) return fail(PQD_ERR_ARG, "NULL argument");
    if (dim < 2 || dim > HB_NMAX) return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [2, %d]", dim, HB_NMAX);
    const int N2 = dim * dim;
    if (d->chi < 1 || d->chi > 256) return fail(PQD_ERR_UNSUPPORTED, "chi %d not in [1, 256]", d->chi);
    if (d->D < 1 || d->n_slices < 1) return fail(PQD_ERR_ARG, "D and n_slices must be >= 1");
    if (!d->Q || !d->closure || !d->closure0 || !d->bond0 || !d->gmap) return fail(PQD_ERR_ARG, "NULL PT array");
    for (int a = 0; a < N2; ++a)
        if (d->gmap[a] < 0 || d->gmap[a] >= d->D) return fail(PQD_ERR_ARG, "gmap[%d]=%d out of [0,%d)", a, d->gmap[a], d->D);
    HIPCHK(hipSetDevice(ctx->device));
    const int chi = d->chi;
    auto pt = std::make_unique<pqd_pt>();
    pt->ctx = ctx; pt->dim = dim; pt->chi = chi; pt->CHI = chi; pt->D = d->D; pt->n_slices = d->n_slices;
    pt->wide = true;
    pt->gmap_h.assign(d->gmap, d->gmap + N2);
    hipStream_t s = ctx->stream;
    hipError_t e = pt->Q.upload(reinterpret_cast<const double2*>(d->Q), (size_t)d->n_slices * d->D * chi * chi, s);
    if (e == hipSuccess) e = pt->closure.upload(reinterpret_cast<const double2*>(d->closure), (size_t)d->n_slices * chi, s);
    if (e == hipSuccess) e = pt->closure0.upload(reinterpret_cast<const double2*>(d->closure0), chi, s);
    if (e == hipSuccess) e = pt->bond0.upload(reinterpret_cast<const double2*>(d->bond0), chi, s);
    if (e == hipSuccess) e = pt->gmap.upload(d->gmap, N2, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the uploads read the caller's arrays
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "PT upload: %s", hipGetErrorString(e));
    *out = pt.release();
    return PQD_OK;
}

void pqd_pt_destroy(pqd_pt* pt) { delete pt; }

// Every PQD_* switch that plan creation and pqd_free_propagators read (A/B only: the defaults are the measured-best
// paths; INTEGRATION.md "Runtime switches", in that order). read_plan_env() is the only getenv of the plan code. It
// runs once per pqd_plan_create_multi / pqd_free_propagators call and its result is never kept across calls: tests
// flip switches between plans of one process. Each field keeps the form its reader always parsed: the raw integer,
// "not 0", "exactly 1", or "set at all" (an extra value or flag for unset). The switches read in several places
// (PQD_SPLIT, PQD_MSPLIT, PQD_FUSE, PQD_SPLIT_XCD, PQD_TRUNK, PQD_QUAD, PQD_WIN) gave every reader the same value, so
// each has one field.
struct PlanEnv {
    int split, msplit, ms_tb, ms_ptm, fp4, fpm, pt_mode, cmul3, trpre, bt, colbig, trunk, quad, qpw, qcg, qprio, win,
        rowpair, ablate, hbpt_g, live_rows, live_part, live_col;
    bool ms_l2, split_ow, split_gran, split_xcd, sweep_lean, lean_ro, lean_stage, pt_mode_set, fuse, branch, idle, unitbal, split_l2, hilbert;
    unsigned split_spin;
};

static PlanEnv read_plan_env() {
    auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    PlanEnv v;
    v.split = num("PQD_SPLIT", 1);              // single-trajectory split groups: 0 off, 1 auto, 2 whenever they fit
    v.msplit = num("PQD_MSPLIT", 1);            // multi-trajectory split groups: 0 off, 1 auto, 2 whenever supported
    v.ms_tb = num("PQD_MS_TB", 0);              // at least this many trajectories per group (unset: as few as fit)
    v.ms_ptm = set("PQD_MS_PTM") ? num("PQD_MS_PTM", 0) != 0 : -1;  // their PT rows on the VALU (0) / matrix cores (1); -1 unset
    v.ms_l2 = num("PQD_MS_L2", 1) != 0;         // exchange lines kept in L2 on the XCD-grouped grid (0: sc1 stores)
    v.split_gran = num("PQD_SPLIT_GRAN", 0) == 1;  // 1: data-tagged granule exchange instead of the arrival counter
    v.split_ow = !v.split_gran && num("PQD_SPLIT_OW", 1) != 0;  // output workgroup per split group (counter form only)
    v.split_xcd = num("PQD_SPLIT_XCD", 1) != 0;  // each group's workgroups on one XCD (0: the plain grid)
    v.fp4 = num("PQD_FP4", 1) != 0;             // N2 = 4 free propagators, 16 matrices per workgroup (0: general kernel)
    v.fpm = num("PQD_FPM", 1);                  // N2 = 25, 36 free propagators on the matrix cores (raw value; 0: LDS)
    v.sweep_lean = num("PQD_SWEEP_LEAN", 1) != 0;  // the lean sweep instance where the plan allows it (sweep_lean_ok)
    v.lean_ro = num("PQD_LEAN_RO", 1) != 0;      // lean instance: outputs read inside the fused column phase (0: closure pass)
    v.lean_stage = num("PQD_LEAN_STAGE", 1) != 0;  // its fast region: next step's F, closure, W staged in LDS (0: loaded in place)
    v.pt_mode_set = set("PQD_PT_MODE");
    v.pt_mode = num("PQD_PT_MODE", 0);          // PT-row variant (raw value; unset: 5 at BT = 4, else 4)
    v.cmul3 = num("PQD_CMUL3", 1);              // 3M column products (raw value)
    v.fuse = num("PQD_FUSE", 1) != 0;           // fused half steps F(n), W(n)
    v.trpre = num("PQD_TRPRE", 1);              // prefetched trace rows (raw value; needs fused half steps)
    v.bt = set("PQD_BT") ? (num("PQD_BT", 0) >= 8 ? 8 : 4) : 0;  // trajectories per workgroup, 4 or 8 (0: unset, auto)
    v.colbig = num("PQD_COLBIG", 1);            // N2 > 16 column phases in one piece (raw value; 0: tile by tile)
    v.branch = num("PQD_BRANCH", 1) != 0;       // shared trunks inside lock-step workgroups
    v.trunk = num("PQD_TRUNK", -1);             // trunk pre-pass: -1 auto (by estimated time), 1 always, 0 never
    v.quad = num("PQD_QUAD", 1);                // two-level quads: 0 off, 1 auto, 2 also at chi = 64
    v.qpw = set("PQD_QPW") ? std::max(1, num("PQD_QPW", 1)) : 0;  // quads per workgroup (0: unset, by chi)
    v.qcg = !set("PQD_QCG") ? 0 : num("PQD_QCG", 4) == 2 ? 2 : num("PQD_QCG", 4) == 1 ? 1 : 4;  // 4-column groups per wave: 2, 4, 1 (chi = 32 only); 0: unset
    v.qprio = num("PQD_QPRIO", 2) & 3;          // quad wave priorities (2: raised outside the PT contraction)
    v.idle = num("PQD_IDLE", 1) != 0;           // idle half steps copy one operator (0: compute every half step)
    v.win = num("PQD_WIN", 1);                  // pulse windows: 0 never, 1 when they leave out a tenth, 2 always
    v.unitbal = num("PQD_UNITBAL", 1) != 0;     // PT row units split to balance the waves (0: whole units)
    v.live_rows = num("PQD_LIVE_ROWS", 1);      // PT rows that stay exactly zero get no unit (0: all rows; 2: and verify M, F)
    v.live_part = num("PQD_LIVE_PART", 1) != 0;  // ... and the lean instance deals the live rows in quarters (0: whole rows)
    v.live_col = num("PQD_LIVE_COL", 1) != 0;    // ... and applies F(n) in their compact index, 3 k-steps (0: all 4)
    v.rowpair = set("PQD_ROWPAIR") ? num("PQD_ROWPAIR", 1) != 0 : -1;  // 0: one PT row per unit; -1 unset
    v.ablate = num("PQD_ABLATE", 0);            // kernel phase ablation and stamps (raw value; measurements only)
    const char* spin = getenv("PQD_SPLIT_SPIN");
    v.split_spin = spin ? (unsigned)strtoul(spin, nullptr, 10) : (1u << 22);  // polls before a split wait times out (~0.1 s)
    v.split_l2 = num("PQD_SPLIT_L2", 1) != 0;   // split exchange lines kept in L2 (0: sc1 stores)
    v.hilbert = num("PQD_HILBERT", 0) == 1;     // 1: no-PT plans of dim <= 6 run the Hilbert-space kernel too (dim > 6 always)
    v.hbpt_g = num("PQD_HBPT_G", 0);            // wide PT: at most this many bond slices in flight (raw value; <= 0: no cap)
    return v;
}

int pqd_free_propagators(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, pqd_c128* M_out) {
    if (!ctx || !M_out) return fail(PQD_ERR_ARG, "NULL argument");
    int rc = check_system(sys);
    if (rc) return rc;
    if ((rc = check_grid(grid))) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const int N2 = sys->dim * sys->dim;
    DevBuf<double2> L0, S, T, smp, M, Mi;
    DevBuf<FreePropSys> tab;
    hipStream_t s = ctx->stream;
    if ((rc = upload_systems(1, sys, s, L0, S, T, smp, tab))) return rc;
    const size_t nM = (size_t)2 * grid->n_steps * N2 * N2;
    HIPCHK(M.alloc(nM));
    FreePropParams fp{};
    fp.systems = tab.p; fp.n_sys = 1;
    fp.ta = grid->ta; fp.dt = grid->dt; fp.n_steps = grid->n_steps; fp.n_sub = grid->n_sub; fp.M = M.p;
    const PlanEnv env = read_plan_env();
    fp.packed4 = env.fp4;
    fp.mfma = env.fpm;
    if (env.idle) {
        HIPCHK(Mi.alloc((size_t)N2 * N2));
        fp.Midle = Mi.p;
    }
    HIPCHK(launch_free_prop(N2, fp, s));
    if (nM) HIPCHK(hipMemcpyAsync(M_out, M.p, nM * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PQD_OK;
}

// Dressed states: H0, the channel operators and the samples of every system go up as they are (no generators: the
// kernel diagonalises H itself), one kernel solves every (system, output time), the requested outputs come back.
// The two entry points differ in the dim range, the kernel's launcher and the sweep limit their messages name.
typedef hipError_t (*dressed_launcher)(int, const DressedParams&, hipStream_t);
static int dressed_states_impl(const char* who, int lo, int hi, dressed_launcher launch, int max_sweeps, pqd_ctx* ctx,
                               int32_t n_sys, const pqd_system* systems, const pqd_grid* grid, const pqd_c128* rho,
                               double* evals, pqd_c128* evecs, double* occ) {
    if (!evals && !evecs && !occ) return fail(PQD_ERR_ARG, "no output requested (evals, evecs and occ are all NULL)");
    if (occ && !rho) return fail(PQD_ERR_ARG, "occ needs rho");
    if (n_sys < 1 || !systems) return fail(PQD_ERR_ARG, "need at least one system");
    for (int k = 0; k < n_sys; ++k) {  // check_system without the Lindblad terms and hbar, which H(t) does not hold
        const pqd_system& y = systems[k];
        if (y.dim < lo || y.dim > hi) return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [%d, %d]", y.dim, lo, hi);
        if (!y.H0) return fail(PQD_ERR_ARG, "H0 is NULL");
        if (y.n_chan < 0 || y.n_chan > 4) return fail(PQD_ERR_UNSUPPORTED, "n_chan %d not in [0, 4]", y.n_chan);
        if (y.n_chan > 0 && (!y.chan_ops || !y.chan_samples || y.n_samples < 1 || !(y.sample_dt > 0)))
            return fail(PQD_ERR_ARG, "bad pulse-channel arguments");
        if (systems[k].dim != systems[0].dim)
            return fail(PQD_ERR_UNSUPPORTED, "systems of unequal dim (%d and %d)", systems[0].dim, systems[k].dim);
    }
    if (!grid) return fail(PQD_ERR_ARG, "grid is NULL");
    if (grid->n_steps < 0) return fail(PQD_ERR_ARG, "n_steps < 0");
    if (!(grid->dt > 0)) return fail(PQD_ERR_ARG, "dt must be > 0");
    if (!ctx) return fail(PQD_ERR_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N = systems[0].dim;
    const size_t nn = (size_t)N * N, n_prob = (size_t)n_sys * ((size_t)grid->n_steps + 1);

    std::vector<cd> h0(n_sys * nn), xs, sm;
    std::vector<size_t> oX(n_sys), oM(n_sys);
    for (int k = 0; k < n_sys; ++k) {
        const pqd_system& y = systems[k];
        std::copy(C(y.H0), C(y.H0) + nn, h0.begin() + k * nn);
        oX[k] = xs.size();
        oM[k] = sm.size();
        if (y.n_chan > 0) {
            xs.insert(xs.end(), C(y.chan_ops), C(y.chan_ops) + (size_t)y.n_chan * nn);
            sm.insert(sm.end(), C(y.chan_samples), C(y.chan_samples) + (size_t)y.n_chan * y.n_samples);
        }
    }
    if (xs.empty()) xs.assign(1, 0.0);
    if (sm.empty()) sm.assign(1, 0.0);
    DevBuf<double2> dH0, dX, dS, dRho, dVec;
    DevBuf<double> dVal, dOcc;
    DevBuf<DressedSys> tab;
    DevBuf<unsigned> flags;
    HIPCHK(dH0.upload(reinterpret_cast<double2*>(h0.data()), h0.size(), s));
    HIPCHK(dX.upload(reinterpret_cast<double2*>(xs.data()), xs.size(), s));
    HIPCHK(dS.upload(reinterpret_cast<double2*>(sm.data()), sm.size(), s));
    std::vector<DressedSys> t(n_sys);
    for (int k = 0; k < n_sys; ++k) {
        const pqd_system& y = systems[k];
        t[k].H0 = dH0.p + k * nn;
        t[k].X = dX.p + oX[k];
        t[k].samples = dS.p + oM[k];
        t[k].n_chan = y.n_chan;
        t[k].n_samples = std::max(1, y.n_samples);
        t[k].s_t0 = y.sample_t0;
        t[k].s_dt = y.n_chan > 0 ? y.sample_dt : 1.0;
    }
    HIPCHK(tab.upload(t.data(), t.size(), s));
    if (occ) HIPCHK(dRho.upload(reinterpret_cast<const double2*>(rho), n_prob * nn, s));
    if (evals) HIPCHK(dVal.alloc(n_prob * N));
    if (evecs) HIPCHK(dVec.alloc(n_prob * nn));
    if (occ) HIPCHK(dOcc.alloc(n_prob * N));
    HIPCHK(flags.alloc(1));
    HIPCHK(hipMemsetAsync(flags.p, 0, sizeof(unsigned), s));

    DressedParams dp{};
    dp.systems = tab.p; dp.n_sys = n_sys; dp.n_steps = grid->n_steps;
    dp.ta = grid->ta; dp.dt = grid->dt;
    dp.rho = dRho.p; dp.evals = dVal.p; dp.evecs = dVec.p; dp.occ = dOcc.p; dp.flags = flags.p;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0));
    hipError_t he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, s);
    if (he == hipSuccess) he = launch(N, dp, s);
    if (he == hipSuccess) he = hipEventRecord(e1, s);
    unsigned hf = 0;
    if (he == hipSuccess && evals)
        he = hipMemcpyAsync(evals, dVal.p, n_prob * N * sizeof(double), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && evecs)
        he = hipMemcpyAsync(evecs, dVec.p, n_prob * nn * sizeof(double2), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && occ)
        he = hipMemcpyAsync(occ, dOcc.p, n_prob * N * sizeof(double), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipMemcpyAsync(&hf, flags.p, sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    float ms = -1.0f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (he != hipSuccess) return fail(PQD_ERR_HIP, "%s: %s", who, hipGetErrorString(he));
    ctx->dressed_ms = ms;
    if (hf & 1u) return fail(PQD_ERR_NUMERIC, "%s: H(t) holds a non-finite entry", who);
    if (hf & 2u)
        return fail(PQD_ERR_NUMERIC, "%s: a problem did not converge in %d Jacobi sweeps", who, max_sweeps);
    return PQD_OK;
}

int pqd_dressed_states(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const pqd_grid* grid,
                       const pqd_c128* rho, double* evals, pqd_c128* evecs, double* occ) {
    return dressed_states_impl("pqd_dressed_states", 2, 6, launch_dressed, 30, ctx, n_sys, systems, grid, rho, evals,
                               evecs, occ);
}

// The cavity and sensor models (dim 7..24): the same call on the LDS-resident round-robin solver (dressed_wide.hip)
int pqd_dressed_states_wide(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const pqd_grid* grid,
                            const pqd_c128* rho, double* evals, pqd_c128* evecs, double* occ) {
    return dressed_states_impl("pqd_dressed_states_wide", 7, 24, launch_dressed_wide, 40, ctx, n_sys, systems, grid,
                               rho, evals, evecs, occ);
}

int pqd_dressed_timing(pqd_ctx* ctx, double* ms_kernel) {
    if (!ctx || !ms_kernel) return fail(PQD_ERR_ARG, "NULL argument");
    if (ctx->dressed_ms < 0) return fail(PQD_ERR_ARG, "no pqd_dressed_states call on this context yet");
    *ms_kernel = ctx->dressed_ms;
    return PQD_OK;
}

// PT rows per wave for the 3M sweep. Rows whose coupling-eigenvalue pair maps to the same slice (dictionary
// PTs, e.g. 16 biexciton rows over 9 slices) are contracted together in units of up to rmax rows, so one L2
// read of a slice feeds all of them. Units (cost = rows) go to the least-loaded wave, largest first. A unit is
// (slice, row 0, row 1 or -1, row 2 | row 3 << 16 or -1, a missing row 3 being 0x7FFF); each wave's list ends
// with slice -1. live: rows with 0 stay exactly zero (live_row_mask) and get no unit: the kernels leave them
// untouched, whole row blocks and dormant slots included (NULL: every row; with every row live the list is the same).
// row_cap > 0: at most that many rows per wave, the others returned in `left` (lean_part_units deals them in parts)
static std::vector<int4> pt_row_units(const std::vector<int>& gmap, int NW, int rmax, bool balance,
                                      const std::vector<uint8_t>* live = nullptr, int row_cap = 0,
                                      std::vector<int>* left = nullptr) {
    const int N2 = (int)gmap.size();
    std::vector<int4> units;
    std::vector<int> done(N2, 0);
    int n_live = N2;
    if (live)
        for (int a = 0; a < N2; ++a)
            if (!(*live)[a]) { done[a] = 1; --n_live; }
    for (int a = 0; a < N2; ++a) {
        if (done[a]) continue;
        int rows[4] = {-1, -1, -1, -1}, cnt = 0;
        for (int c = a; c < N2 && cnt < rmax; ++c)
            if (!done[c] && gmap[c] == gmap[a]) { done[c] = 1; rows[cnt++] = c; }
        const int w = cnt > 2 ? (rows[2] | ((cnt > 3 ? rows[3] : 0x7FFF) << 16)) : -1;
        units.push_back(make_int4(gmap[a], rows[0], rows[1], w));
    }
    auto cost = [](const int4& e) { return e.z < 0 ? 1 : e.w < 0 ? 2 : (e.w >> 16) == 0x7FFF ? 3 : 4; };
    std::stable_sort(units.begin(), units.end(), [&](const int4& x, const int4& y) { return cost(x) > cost(y); });
    std::vector<std::vector<int4>> per(NW);
    std::vector<int> load(NW, 0);
    // the PT phase lasts as long as the most-loaded wave: aim at T = ceil(rows / waves) rows per wave. Whole units go
    // to the least-loaded wave they fit (largest first); a unit that fits nowhere is split into its rows,
    // which then fill the waves' remaining capacity, rows of one slice kept together per wave (a split slice is read
    // once more from L2 per extra wave). Six-level dictionary PT (9 slices x 4 rows, 8 waves): max 5 rows per wave
    // instead of 8 (one wave held two 4-row units). Least-loaded first, so the two waves of a SIMD (w, w + NW / 2)
    // also stay balanced: their MFMAs share its matrix pipe
    int T = (n_live + NW - 1) / NW;
    if (!balance) T = 1 << 20;  // PQD_UNITBAL=0 (A/B): whole units, least loaded
    if (row_cap > 0) T = row_cap;
    std::vector<int> pending;  // rows of split units, slice-ordered
    for (const int4& e : units) {
        int w = -1;
        for (int k = 0; k < NW; ++k)
            if (load[k] + cost(e) <= T && (w < 0 || load[k] < load[w])) w = k;
        if (w >= 0) {
            per[w].push_back(e);
            load[w] += cost(e);
            continue;
        }
        const int rows[4] = {e.y, e.z, e.w >= 0 ? (e.w & 0xFFFF) : -1, e.w >= 0 ? (e.w >> 16) : -1};
        for (int r : rows)
            if (r >= 0 && r != 0x7FFF) pending.push_back(r);
    }
    for (size_t i = 0; i < pending.size();) {
        int w = 0;  // the least-loaded wave takes as many rows of this slice as fit (at most rmax)
        for (int k = 1; k < NW; ++k)
            if (load[k] < load[w]) w = k;
        if (row_cap > 0 && load[w] >= row_cap) {  // every wave is full: the rest goes back to the caller
            left->assign(pending.begin() + i, pending.end());
            break;
        }
        const int room = std::max(1, std::min(rmax, T - load[w]));
        int rows[4] = {-1, -1, -1, -1}, cnt = 0;
        const int g = gmap[pending[i]];
        while (i < pending.size() && cnt < room && gmap[pending[i]] == g) rows[cnt++] = pending[i++];
        const int wv = cnt > 2 ? (rows[2] | ((cnt > 3 ? rows[3] : 0x7FFF) << 16)) : -1;
        per[w].push_back(make_int4(g, rows[0], rows[1], wv));
        load[w] += cnt;
    }
    size_t umax = 1;
    for (auto& v : per) umax = std::max(umax, v.size() + 1);
    std::vector<int4> out((size_t)NW * umax, make_int4(-1, 0, -1, -1));
    for (int w = 0; w < NW; ++w)
        for (size_t k = 0; k < per[w].size(); ++k) out[(size_t)w * umax + k] = per[w][k];
    return out;
}

// The lean instance's list for a plan some of whose rows stay zero (pt_sweep.hip LeanPt::run_parts). Whole rows balance
// the waves only in steps of a row: 10 live rows over 8 waves leave two SIMDs with three rows and two with two, and the
// PT phase lasts as long as the fullest. So the rows are dealt in quarters (one of a slice's NG = 4 column groups of 16
// columns): every wave aims at Tq = ceil(4 live / NW) quarters, takes one whole row first, and the rows left over are cut
// into partial units of ng = 1 or 2 column groups, one per wave, in wave order (waves 0 .. NW/2 - 1 are one per SIMD, so
// the two waves of a SIMD, w and w + NW/2, stay level). 10 rows: a whole row and a quarter on every wave, 1.25 rows on
// the critical path instead of 2. A wave's list is [partial,] whole, end: the partial unit first, because its columns
// are written behind a barrier the whole unit then hides. Empty where whole rows do as well (live <= NW or two whole
// rows per wave) or where the rest does not fit one partial unit of at most two groups per wave (live 13, 14): the
// caller keeps the whole-row list of the live rows.
static std::vector<int4> lean_part_units(const std::vector<int>& gmap, int NW, const std::vector<uint8_t>& live) {
    constexpr int NG = 4;
    int n_live = 0;
    for (uint8_t v : live) n_live += v != 0;
    const int Tq = (NG * n_live + NW - 1) / NW;
    if (n_live <= NW || Tq / NG != 1) return {};
    std::vector<int> left;
    const std::vector<int4> whole = pt_row_units(gmap, NW, 1, true, &live, 1, &left);
    const size_t wmax = whole.size() / NW;
    for (int w = 0; w < NW; ++w)
        if (whole[w * wmax].x < 0 || whole[w * wmax].z >= 0 || (wmax > 1 && whole[w * wmax + 1].x >= 0)) return {};
    const int quarters = NG * (int)left.size(), ng = quarters > NW ? 2 : 1;
    if (left.empty() || quarters > NW * ng || ng > Tq - NG) return {};
    std::vector<int4> out((size_t)NW * 3, make_int4(-1, 0, -1, -1));
    for (int w = 0; w < NW; ++w) {
        const int q = w * ng;  // this wave's first quarter of the rows left
        size_t k = (size_t)w * 3;
        if (q < quarters) out[k++] = make_int4(gmap[left[q / NG]], left[q / NG], -1, (q % NG) | (ng << 4));
        out[k] = whole[w * wmax];
    }
    return out;
}

// The compact row index of the lean instance's column phase (pt_sweep.hip LeanCol): rho lists the live
// rows in increasing order, then the rows that stay zero in increasing order, and the product F(n) S needs
// KC = ceil(n_live / 4) k-steps of four compact rows. Increasing order is what keeps the states bit-identical: every
// live row receives its live products in the order the uncompacted product adds them.
static int live_col_map(const std::vector<uint8_t>& live, std::vector<uint8_t>& rho) {
    rho.clear();
    for (size_t a = 0; a < live.size(); ++a)
        if (live[a]) rho.push_back((uint8_t)a);
    const int n_live = (int)rho.size();
    for (size_t a = 0; a < live.size(); ++a)
        if (!live[a]) rho.push_back((uint8_t)a);
    return (n_live + 3) / 4;
}

// Shared trunks inside a lock-step block (the reference re-propagates 0 -> t1 in every trajectory of a two-time
// sweep: correlations.py:155-169, pol_entanglement/G2.py:486-497). j[t] = the last step at whose top (before its
// outputs) trajectory t still holds the MTO-free state: its first MTO's step if that MTO applies after the output,
// one less if it applies before. Slots are ordered by j; slot k becomes active at
// act[k] = min(j_k, out_begin_k, j_m) by copying the (state, fused flag) of an earlier slot m of the same system that
// is already active then (act[m] < act[k]) and still MTO-free (j_m >= act[k]); before that it is dormant (no column
// phases, its PT rows skipped where a whole row block is dormant). Outputs before act[k] are never needed
// (act[k] <= out_begin_k), so every trajectory's outputs are those of its own full run.
static void branch_slots(int BT, const int* members, const std::vector<int>& jv, const int32_t* out_begin,
                         const std::vector<int>& tsys, bool enable, int* act, int* src) {
    for (int k = 0; k < BT; ++k) {
        const int t = members[k];
        src[k] = -1;
        if (t < 0) { act[k] = INT_MAX; continue; }
        act[k] = 0;
        if (!enable) continue;
        const int a = std::min(jv[t], out_begin[t]);
        int best = 0, bm = -1;
        for (int m = 0; m < k; ++m) {
            const int tm = members[m];
            if (tm < 0 || tsys[tm] != tsys[t]) continue;
            const int cand = std::min(a, jv[tm]);
            if (act[m] < cand && cand > best) { best = cand; bm = m; }
        }
        if (bm >= 0) { act[k] = best; src[k] = bm; }
    }
}

// What plan creation asks of the device: the CU count and the workgroups per CU the runtime reports for the two split
// kernels. The queries are function pointers, so each is made only where its path is considered (PQD_SPLIT=0 asks
// nothing) and a host-only test can drive choose_path with numbers of its own.
struct DeviceCaps {
    int n_cu;
    int (*split_blocks_per_cu)(int N2, int CHI), (*msplit_blocks_per_cu)(int N2, int CHI);
};

// Single-trajectory split groups the device holds at once. The spin hand-off needs every workgroup of a launch
// resident, by the occupancy the runtime reports for the split kernel. A batch just above `fit` runs as consecutive
// co-resident launches, up to 4 at N2 >= 25 and 2 below, where they still beat one batched pass (a group step is
// 3.6x / 2.4x faster than a batched block's; C5: 8 six-level trunks = 288 workgroups -> 7 + 1).
struct SplitCap {
    int slots, fit, launches;  // workgroups and groups resident at once; launches in a row that still pay
    bool takes(int N2, int CHI, int n, int max_launches, bool ow) const {  // n groups in at most max_launches launches
        return fit >= 1 && split_supported(N2, CHI, std::min(n, fit), slots, ow) && n <= max_launches * fit;
    }
};
static SplitCap split_capacity(int N2, int CHI, bool ow, const DeviceCaps& caps) {
    const int bpc = caps.split_blocks_per_cu(N2, CHI), slots = caps.n_cu * bpc;
    return {slots, bpc >= 1 ? slots / split_group_size(N2, ow) : 0, N2 >= 25 ? 4 : 2};
}

// Trunk pre-pass of a plan: one MTO-free trajectory per system that has checkpoints, propagated from step 0 to
// its last checkpoint step, writing the augmented state at the top of every checkpoint step (ck_steps[y], indices
// ck_base[y] + k). It runs before the main sweep on split groups when those fit (N2 >= 9, as in auto mode), else
// as batched workgroups of four; the batched layout is always built (fallback after a split timeout).
static int plan_trunks(pqd_plan* P, const std::vector<std::vector<int>>& ck_steps, const std::vector<int>& ck_base,
                       int n_ck, const pqd_pt* pt, const PlanEnv& env, const DeviceCaps& caps, hipStream_t s) {
    const int ns = P->n_steps, CHI = P->CHI, N2 = P->N2, n_out = P->n_out, n_sys = P->n_sys;
    std::vector<int> wb, we, ts, map;
    std::vector<long long> wo;
    for (int y = 0; y < n_sys; ++y) {
        if (ck_steps[y].empty()) continue;
        const int t = (int)ts.size(), L = ck_steps[y].back();
        ts.push_back(y);
        wb.push_back(L);
        we.push_back(L);
        wo.push_back((long long)t * n_out);
        map.resize((size_t)(t + 1) * (ns + 1), -1);
        for (size_t k = 0; k < ck_steps[y].size(); ++k) map[(size_t)t * (ns + 1) + ck_steps[y][k]] = ck_base[y] + (int)k;
        P->traj_steps += L + 1;
    }
    const int nt = (int)ts.size();
    P->n_trunk = nt;
    if (!nt) return PQD_OK;
    std::vector<int> evs0(nt + 1, 0);
    HIPCHK(P->ck.alloc((size_t)n_ck * N2 * CHI));
    HIPCHK(P->tk_out.alloc((size_t)nt * n_out));
    HIPCHK(P->tk_ckmap.upload(map.data(), map.size(), s));
    HIPCHK(P->tk_wbeg.upload(wb.data(), nt, s));
    HIPCHK(P->tk_wend.upload(we.data(), nt, s));
    HIPCHK(P->tk_woff.upload(wo.data(), nt, s));
    HIPCHK(P->tk_tsys.upload(ts.data(), nt, s));
    HIPCHK(P->tk_evstart.upload(evs0.data(), evs0.size(), s));
    // batched layout: four trunks per workgroup
    const int BT = 4;
    std::vector<int> bt, be, bs, ba, bsrc;
    for (int t = 0; t < nt; t += BT) {
        int end = 0;
        for (int q = 0; q < BT; ++q) {
            const int u = t + q < nt ? t + q : -1;
            bt.push_back(u);
            ba.push_back(u >= 0 ? 0 : INT_MAX);
            bsrc.push_back(-1);
            if (u >= 0) end = std::max(end, we[u]);
        }
        be.push_back(end);
        bs.push_back(ts[t]);
    }
    P->tk_BT = BT;
    P->tk_blocks = (int)be.size();
    HIPCHK(P->tk_blk_traj.upload(bt.data(), bt.size(), s));
    HIPCHK(P->tk_blk_end.upload(be.data(), be.size(), s));
    HIPCHK(P->tk_blk_sys.upload(bs.data(), bs.size(), s));
    HIPCHK(P->tk_blk_act.upload(ba.data(), ba.size(), s));
    HIPCHK(P->tk_blk_src.upload(bsrc.data(), bsrc.size(), s));
    {
        const int nw = BT * sweep_wpt(N2, BT, CHI);
        std::vector<int4> u = pt_row_units(pt->gmap_h, nw, sweep_rmax(N2, BT, CHI), env.unitbal);
        HIPCHK(P->tk_units.upload(u.data(), u.size(), s));
    }
    // more trunks than the device holds as co-resident groups: consecutive launches of as many as fit
    const SplitCap cap = split_capacity(N2, CHI, env.split_ow, caps);
    P->tk_chunk = cap.fit >= 1 && nt > cap.fit ? cap.fit : 0;
    P->tk_split = env.split != 0 && N2 >= 9 && cap.takes(N2, CHI, nt, cap.launches, env.split_ow);
    HIPCHK(P->tk_Xs.alloc((size_t)nt * 4 * N2 * CHI));  // split exchange: 2 slots of granules (pt_split.hip)
    HIPCHK(P->tk_cnt.alloc((size_t)nt * 64));  // split arrival flags: two 128-B lines per group
    HIPCHK(P->tk_err.alloc(4));
    return PQD_OK;
}

// The lean instance of the batched sweep (pt_sweep.hip LEAN) is compiled for one configuration, the headline one:
// N2 = 16, chi = 64, BT = 8, 3M unit-list PT rows with at most two units per wave (umax counts the list's end
// marker too), 3M columns, fused half steps, traces one lane per (trajectory, output, row), no ablation. Every other
// plan runs the general instance. PQD_SWEEP_LEAN=0 forces the general instance (A/B, tests).
static bool sweep_lean_ok(const pqd_plan* P, const SweepParams& sp, const PlanEnv& env) {
    return env.sweep_lean && P->N2 == 16 && P->CHI == 64 && P->BT == 8 && sp.pt_mode == 4 && sp.cmul3 == 1 && sp.fuse == 1 &&
           sp.trpre == 1 && sp.ablate == 0 && sp.units && sp.umax >= 2 && sp.umax <= 3 &&
           P->BT * sp.n_out * P->N2 <= 512;
}

// the trunk pre-pass launch parameters: the main sweep's, with the trunk trajectories and checkpoint map
static void finalize_trunks(pqd_plan* P) {
    P->sp.ck = P->ck.p;
    P->sp.ck_map = nullptr;
    if (!P->n_trunk) return;
    SweepParams& k = P->tk;
    k = P->sp;
    k.blk_traj = P->tk_blk_traj.p; k.blk_end = P->tk_blk_end.p; k.blk_sys = P->tk_blk_sys.p;
    k.blk_act = P->tk_blk_act.p; k.blk_src = P->tk_blk_src.p;
    k.traj_sys = P->tk_tsys.p; k.wbeg = P->tk_wbeg.p; k.wend = P->tk_wend.p; k.woff = P->tk_woff.p;
    k.ev_start = P->tk_evstart.p; k.out = P->tk_out.p;
    k.ck_map = P->tk_ckmap.p; k.ck_stride = P->n_steps + 1;
    k.lean = 0;
    k.lean_parts = 0;
    k.lean_colk = 4;
    k.lean_rho = 0;
    k.blk_fast = nullptr;
    k.blk_stage = nullptr;
    const int nw = P->tk_BT * sweep_wpt(P->N2, P->tk_BT, P->CHI);
    k.units = (P->sp.units ? P->tk_units.p : nullptr);
    k.umax = (int)(P->tk_units.n / nw);
}

// the main batched sweep of a plan: quads (N2 = 4) or BT-trajectory workgroups
static hipError_t launch_main(pqd_plan* P, hipStream_t s) {
    if (P->quad) return launch_quad(P->CHI, P->n_blocks, P->qpw, P->qcg, P->sp, s);
    return launch_sweep(P->N2, P->CHI, P->BT, P->n_blocks, P->sp, s);
}

static hipError_t launch_trunks(pqd_plan* P, hipStream_t s) {
    if (!P->n_trunk) return hipSuccess;
    if (P->tk_split)
        return launch_split(P->N2, P->CHI, P->n_trunk, P->tk, P->tk_Xs.p, P->tk_cnt.p, P->tk_err.p, s, P->tk_chunk);
    return launch_sweep(P->N2, P->CHI, P->tk_BT, P->tk_blocks, P->tk, s);
}

// ---- plan creation, stage by stage, in the order pqd_plan_create_multi calls them; values pass as arguments and results
// the arguments of pqd_plan_create_multi; sch: the slice of every step (sched, or the PT's own order)
static int check_plan_args(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                           const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                           int32_t n_out, const pqd_c128* out_ops, const pqd_traj* tr, int64_t out_len,
                           pqd_plan** out, std::vector<int32_t>& sch) {
    if (!ctx || !rho0 || !tr || !out || !systems) return fail(PQD_ERR_ARG, "NULL argument");
    if (n_sys < 1) return fail(PQD_ERR_ARG, "n_sys must be >= 1");
    if (n_sys > 1 && !traj_sys) return fail(PQD_ERR_ARG, "traj_sys is NULL with n_sys > 1");
    int rc = 0;
    for (int k = 0; k < n_sys; ++k) {
        if ((rc = check_system(&systems[k], pt && !pt->wide ? 6 : HB_NMAX))) return rc;
        if (systems[k].dim != systems[0].dim) return fail(PQD_ERR_ARG, "system %d: dim %d != %d", k, systems[k].dim, systems[0].dim);
        if (systems[k].dim > 6 && systems[k].n_lind > HB_LMAX)  // dim > 6 runs in Hilbert space only (lind_hilbert.hip)
            return fail(PQD_ERR_UNSUPPORTED, "system %d: n_lind %d not in [0, %d] at dim %d > 6", k, systems[k].n_lind,
                        HB_LMAX, systems[k].dim);
        if (pt && pt->wide && systems[k].n_lind > HB_LMAX)  // a wide PT runs in Hilbert space at every dim
            return fail(PQD_ERR_UNSUPPORTED, "system %d: n_lind %d not in [0, %d] with a wide PT", k, systems[k].n_lind,
                        HB_LMAX);
    }
    const pqd_system* sys = systems;
    for (int t = 0; t < tr->n_traj; ++t)
        if (traj_sys && (traj_sys[t] < 0 || traj_sys[t] >= n_sys)) return fail(PQD_ERR_ARG, "traj_sys[%d]=%d out of [0,%d)", t, traj_sys[t], n_sys);
    if ((rc = check_grid(grid))) return rc;
    const int N = sys->dim, N2 = N * N;
    const int ns = grid->n_steps;
    if (n_out < 1 || n_out > 256 || !out_ops) return fail(PQD_ERR_ARG, "n_out %d not in [1, 256]", n_out);
    if (tr->n_traj < 0 || (tr->n_traj > 0 && (!tr->out_begin || !tr->out_end || !tr->out_offset)))
        return fail(PQD_ERR_ARG, "bad trajectory arrays");
    if (pt) {
        if (pt->ctx != ctx) return fail(PQD_ERR_ARG, "PT belongs to another context");
        if (pt->dim != N) return fail(PQD_ERR_ARG, "PT dim %d != system dim %d", pt->dim, N);
        if (!pt->wide && !sweep_supported(N2, pt->CHI) && !(pt->CHI == 256 && msplit_supported(N2, pt->CHI, n_out)))
            return fail(PQD_ERR_UNSUPPORTED, "N2=%d CHI=%d (chi 256: N2 4, 9 or 16 and at most 8 outputs)", N2, pt->CHI);
    }
    for (int t = 0; t < tr->n_traj; ++t) {
        const int b = tr->out_begin[t], e = tr->out_end[t];
        if (b < 0 || e < b || e > ns)
            return fail(PQD_ERR_ARG, "trajectory %d window [%d, %d] outside [0, %d]", t, b, e, ns);
        const int64_t hi = tr->out_offset[t] + (int64_t)(e - b + 1) * n_out;
        if (tr->out_offset[t] < 0 || hi > out_len)
            return fail(PQD_ERR_ARG, "trajectory %d output [%lld, %lld) exceeds out_len %lld", t,
                        (long long)tr->out_offset[t], (long long)hi, (long long)out_len);
    }
    if (tr->n_mto < 0 || (tr->n_mto > 0 && (!tr->mto_traj || !tr->mto_step || !tr->mto_before || !tr->mto_kind || !tr->mto_ops)))
        return fail(PQD_ERR_ARG, "bad MTO arrays");
    for (int q = 0; q < tr->n_mto; ++q) {
        if (tr->mto_traj[q] < 0 || tr->mto_traj[q] >= tr->n_traj) return fail(PQD_ERR_ARG, "MTO %d: bad trajectory", q);
        if (tr->mto_step[q] < 0 || tr->mto_step[q] > ns) return fail(PQD_ERR_ARG, "MTO %d: step %d outside [0, %d]", q, tr->mto_step[q], ns);
        if (tr->mto_kind[q] < 0 || tr->mto_kind[q] > 2) return fail(PQD_ERR_ARG, "MTO %d: kind %d", q, tr->mto_kind[q]);
    }
    sch.assign(std::max(1, ns), 0);
    if (pt) {
        for (int n = 0; n < ns; ++n) {
            const int s = sched ? sched[n] : std::min(n, pt->n_slices - 1);
            if (s < 0 || s >= pt->n_slices) return fail(PQD_ERR_ARG, "sched[%d]=%d out of [0,%d)", n, s, pt->n_slices);
            sch[n] = s;
        }
    }
    return PQD_OK;
}

// MTO events: per trajectory (events ev_start[t] .. ev_start[t + 1]), stable-sorted by (step, phase), same-slot ops
// composed: evs = (step, 1 after the output / 0 before, superoperator index, 0). Every MTO kind is
// rho -> L rho R ("": A rho A^dag, _left: A rho, _right: rho A), so a slot's ops compose as N x N products
// (L = L_k ... L_1, R = R_1 ... R_k) and its superoperator is L (x) R^T; identical (L, R) pairs share one
// superoperator (a two-time sweep applies the same operators at every t1).
struct MtoEvents {
    std::vector<int> ev_start;
    std::vector<int4> evs;
    std::vector<cd> sops;
};
static MtoEvents compose_mtos(int N, const pqd_traj* tr) {
    const int N2 = N * N;
    const size_t m2 = (size_t)N2 * N2, nn = (size_t)N * N;
    std::vector<std::vector<int>> per(tr->n_traj);
    for (int q = 0; q < tr->n_mto; ++q) per[tr->mto_traj[q]].push_back(q);
    MtoEvents E;
    auto &ev_start = E.ev_start; auto &evs = E.evs; auto &sops = E.sops;
    ev_start.assign(tr->n_traj + 1, 0);
    std::unordered_map<std::string, int> sop_index;
    std::vector<cd> Lm(nn), Rm(nn), Lq(nn), Rq(nn), key_buf(2 * nn);
    auto eye = [&](std::vector<cd>& M) { std::fill(M.begin(), M.end(), cd(0)); for (int i = 0; i < N; ++i) M[(size_t)i * N + i] = 1.0; };
    for (int t = 0; t < tr->n_traj; ++t) {
        auto& v = per[t];
        auto key = [&](int q) { return 2 * tr->mto_step[q] + (tr->mto_before[q] ? 0 : 1); };
        std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return key(a) < key(b); });
        ev_start[t] = (int)evs.size();
        size_t i = 0;
        while (i < v.size()) {
            const int k0 = key(v[i]);
            eye(Lm);
            eye(Rm);
            for (; i < v.size() && key(v[i]) == k0; ++i) {
                const int q = v[i];
                const cd* A = C(tr->mto_ops) + (size_t)q * nn;
                const int kind = tr->mto_kind[q];
                if (kind == 2) eye(Lq); else std::copy(A, A + nn, Lq.begin());
                if (kind == 1) eye(Rq);
                else if (kind == 2) std::copy(A, A + nn, Rq.begin());
                else
                    for (int r = 0; r < N; ++r)
                        for (int c = 0; c < N; ++c) Rq[(size_t)r * N + c] = std::conj(A[(size_t)c * N + r]);
                matmul_sq(N, Lq.data(), Lm.data(), Lm.data());  // L <- L_q L
                matmul_sq(N, Rm.data(), Rq.data(), Rm.data());  // R <- R R_q
            }
            std::copy(Lm.begin(), Lm.end(), key_buf.begin());
            std::copy(Rm.begin(), Rm.end(), key_buf.begin() + nn);
            std::string kb(reinterpret_cast<const char*>(key_buf.data()), key_buf.size() * sizeof(cd));
            auto it = sop_index.find(kb);
            int idx;
            if (it != sop_index.end()) {
                idx = it->second;
            } else {
                idx = (int)(sops.size() / m2);
                sop_index.emplace(std::move(kb), idx);
                sops.resize(sops.size() + m2);
                cd* S = sops.data() + (size_t)idx * m2;
                for (int a = 0; a < N; ++a)
                    for (int j = 0; j < N; ++j)
                        for (int k = 0; k < N; ++k)
                            for (int l = 0; l < N; ++l)
                                S[(size_t)(a * N + j) * N2 + (k * N + l)] = Lm[(size_t)a * N + k] * Rm[(size_t)l * N + j];
            }
            evs.push_back(make_int4(k0 >> 1, k0 & 1, idx, 0));
        }
    }
    ev_start[tr->n_traj] = (int)evs.size();
    if (evs.empty()) evs.push_back(make_int4(-1, -1, 0, 0));
    if (sops.empty()) sops.assign(m2, 0.0);
    return E;
}

// Liouville rows that can ever be nonzero in a plan (pqd_live_rows): the closure of the initial state's
// nonzero entries under the edges b -> a of every operator the sweep applies to the system index: L0 of every system,
// S_p and T_p of every channel with a nonzero sample anywhere in its sample array, and every MTO superoperator, each
// judged by exact != 0 on the values as they are uploaded. No edge leads from a live row into a dead one, so the
// [dead row, live column] block of the generator is zero at every time, and with it that block of every sum and
// product of such matrices: the Taylor / squaring exponentials, F = M_a M_b and the idle operators (with 3M products
// too: each of the three real products has an exact-zero factor). The PT contraction is diagonal in the row index.
// A dead row therefore holds exact zeros at every step of every trajectory, and its PT contraction is skipped.
static std::vector<uint8_t> live_row_mask(int n_sys, const pqd_system* systems, const cd* rho0, const MtoEvents& E) {
    const int N = systems[0].dim, N2 = N * N;
    const size_t m2 = (size_t)N2 * N2;
    std::vector<uint8_t> edge(m2, 0);
    auto add = [&](const cd* Mx) {
        for (size_t k = 0; k < m2; ++k)
            if (Mx[k] != cd(0.0)) edge[k] = 1;
    };
    for (int k = 0; k < n_sys; ++k) {
        Generators G;
        build_generators(&systems[k], G);
        add(G.L0.data());
        for (int p = 0; p < systems[k].n_chan; ++p) {
            bool driven = false;
            for (int q = 0; q < systems[k].n_samples && !driven; ++q)
                driven = G.samples[(size_t)p * systems[k].n_samples + q] != cd(0.0);
            if (!driven) continue;
            add(G.S.data() + p * m2);
            add(G.T.data() + p * m2);
        }
    }
    for (size_t k = 0; k + m2 <= E.sops.size(); k += m2) add(E.sops.data() + k);
    std::vector<uint8_t> live(N2, 0);
    std::vector<int> todo;
    for (int a = 0; a < N2; ++a)
        if (rho0[a] != cd(0.0)) { live[a] = 1; todo.push_back(a); }
    while (!todo.empty()) {
        const int b = todo.back();
        todo.pop_back();
        for (int a = 0; a < N2; ++a)
            if (edge[(size_t)a * N2 + b] && !live[a]) { live[a] = 1; todo.push_back(a); }
    }
    return live;
}

// the plan's inputs on the device: generators for the free propagators (one table entry per system), MTO events,
// output operators (ovec[k][i*N+j] = O_k[j][i], <O> = Tr(O rho)), initial state, windows
static int upload_inputs(pqd_plan* P, const pqd_system* systems, const std::vector<int>& tsys, MtoEvents& E,
                         const pqd_c128* rho0, const pqd_c128* out_ops, const pqd_traj* tr, hipStream_t s) {
    const int N = systems->dim, N2 = P->N2, n_out = P->n_out, n_w = std::max(1, P->n_traj);
    int rc = upload_systems(P->n_sys, systems, s, P->L0, P->S, P->T, P->samples, P->systab);
    if (rc) return rc;
    HIPCHK(P->M.alloc(std::max<size_t>(1, (size_t)P->n_sys * 2 * P->n_steps * N2 * N2)));
    HIPCHK(P->traj_sys.upload(tsys.data(), tsys.size(), s));
    HIPCHK(P->ev.upload(E.evs.data(), E.evs.size(), s));
    HIPCHK(P->ev_start.upload(E.ev_start.data(), E.ev_start.size(), s));
    HIPCHK(P->sop.upload(reinterpret_cast<double2*>(E.sops.data()), E.sops.size(), s));
    std::vector<cd> ov((size_t)n_out * N2);
    for (int k = 0; k < n_out; ++k)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) ov[(size_t)k * N2 + i * N + j] = C(out_ops)[(size_t)k * N2 + j * N + i];
    HIPCHK(P->ovec.upload(reinterpret_cast<double2*>(ov.data()), ov.size(), s));
    HIPCHK(P->rho0.upload(reinterpret_cast<const double2*>(rho0), N2, s));
    HIPCHK(P->wbeg.upload(tr->out_begin, n_w, s));
    HIPCHK(P->wend.upload(tr->out_end, n_w, s));
    HIPCHK(P->woff.upload(reinterpret_cast<const long long*>(tr->out_offset), n_w, s));
    return PQD_OK;
}

// Block order of the trajectories and j[t], the last step whose top still sees the MTO-free state (branch_slots):
// grouped by system (a workgroup whose trajectories share one system reads one set of free propagators), longest
// first inside a system so lock-step blocks end together, then by branch step (neighbouring slots share the longest
// trunk)
struct TrajOrder {
    std::vector<int> order, jv;
};
static TrajOrder order_trajectories(const pqd_traj* tr, const std::vector<int>& tsys, const MtoEvents& E) {
    TrajOrder o;
    o.order.resize(tr->n_traj);
    for (int t = 0; t < tr->n_traj; ++t) o.order[t] = t;
    o.jv.assign(std::max(1, tr->n_traj), 0);
    for (int t = 0; t < tr->n_traj; ++t) {
        if (E.ev_start[t] == E.ev_start[t + 1]) { o.jv[t] = tr->out_end[t]; continue; }
        const int4 e = E.evs[E.ev_start[t]];
        o.jv[t] = e.y == 1 ? e.x : e.x - 1;
    }
    std::stable_sort(o.order.begin(), o.order.end(), [&](int a, int b) {
        if (tsys[a] != tsys[b]) return tsys[a] < tsys[b];
        if (tr->out_end[a] != tr->out_end[b]) return tr->out_end[a] > tr->out_end[b];
        return o.jv[a] < o.jv[b];
    });
    return o;
}
// The kernel a plan runs and its grid (choose_path)
struct PlanShape {
    int N2, CHI, n_steps, n_out, n_sys;
    bool pt;  // the plan has a process tensor
};
struct PathChoice {
    bool split = false;    // small batch: one trajectory over N2 workgroups (pt_split.hip)
    int split_chunk = 0;   // ... trajectories per launch when the batch exceeds the device (0: one launch)
    int BT = 4;            // trajectories per lock-step workgroup
    bool quad = false;     // two-level system: register-resident quads (pt_quad.hip), blocks of BT = 4
    int qpw = 2, qcg = 4;  // ... quads per workgroup, 4-column groups per wave
    bool msplit = false;   // split groups of ms_TB trajectories each (pt_msplit.hip)
    int ms_TB = 0, ms_groups = 0, ms_xcd = 0;  // ... groups, groups per XCD slot (0: the plain grid)
};

// Path selection: single-trajectory split groups, else quads (N2 = 4), else multi-trajectory split groups, else the
// batched sweep; a plan without PT takes none of them. Reads its arguments only: no plan, no HIP call beyond the
// occupancy queries of `caps`. Fails for a chi = 256 batch the multi-trajectory groups cannot take.
static int choose_path(const PlanShape& sh, const pqd_traj* tr, const std::vector<int>& tsys, const TrajOrder& to,
                       const MtoEvents& E, const PlanEnv& env, const DeviceCaps& caps, PathChoice& pc) {
    const int N2 = sh.N2, CHI = sh.CHI, n_traj = tr->n_traj, n_cu = caps.n_cu;
    const bool fuse_on = sh.pt && sh.n_steps > 0 && env.fuse;
    // latency path: a batch whose trajectories fit one group of N2 workgroups each on the device runs
    // each trajectory over N2 workgroups (pt_split.hip). Measured: 2.3-3.6x faster per step
    // at N2 = 16 and 36; at N2 = 4 the batched kernel's single workgroup is as fast, so auto mode skips it.
    // PQD_SPLIT: 0 off, 1 auto, 2 whenever the device holds the groups.
    if (sh.pt && env.split != 0) {
        const SplitCap cap = split_capacity(N2, CHI, env.split_ow, caps);
        // one launch only where multi-trajectory groups can take the batch (one launch of those beats consecutive
        // launches). ms_can is a guess from PQD_MSPLIT, msplit_supported and PQD_FUSE alone: the decision below may
        // still refuse the batch, which then runs batched
        const bool ms_can = env.msplit != 0 && msplit_supported(N2, CHI, sh.n_out) && env.fuse;
        // PQD_MSPLIT=2: multi-trajectory split groups in place of these (A/B, tests)
        pc.split = env.msplit != 2 && cap.takes(N2, CHI, n_traj, ms_can ? 1 : cap.launches, env.split_ow) &&
                   (env.split == 2 || N2 >= 9);
        pc.split_chunk = pc.split && n_traj > cap.fit ? cap.fit : 0;
    }
    // trajectories per workgroup: 8 (half the PT-slice L2 traffic per trajectory) when the LDS allows it
    // and the batch still fills every CU, else 4
    pc.BT = (sweep_max_bt(N2) >= 8 && n_traj >= 8 * n_cu) ? 8 : 4;
    if (env.bt) pc.BT = std::min(env.bt, sweep_max_bt(N2));
    if (CHI > 64) pc.BT = 4;  // chi = 128: only four augmented states fit the LDS
    // two-level system: the register-resident quad kernel (pt_quad.hip) unless split groups were forced or
    // PQD_QUAD=0 (A/B); its blocks are quads.
    // chi = 64 quads only on request (PQD_QUAD=2): their slices do not fit the registers yet and the batched
    // kernel is faster (C2 shape at chi = 64: 19.9 ms batched, 41.9 ms quads; profiles/r03/q64.log)
    pc.quad = sh.pt && !pc.split && quad_supported(N2, CHI) && env.quad != 0 && (CHI != 64 || env.quad == 2);
    // chi = 32: one quad per workgroup, so the two 8-column-strip workgroups sharing a CU barrier independently
    // (C2: 19.8 -> 18.4 ms per launch with the strips below, profiles/r02/quad/envab_qpw_qcg.log). Set whether or not
    // the plan runs quads
    if (CHI == 32) pc.qpw = 1;
    if (env.qpw) pc.qpw = env.qpw;
    if (pc.quad) {
        pc.BT = 4;
        // strips of 8 columns (twice the waves, two per SIMD) overlap one wave's round trips with the
        // other's MFMAs: with no more quads than CUs (C2 single run 17.2 -> 13.1 ms), and at chi = 32 with one quad per
        // workgroup on a full device too (C2 scan 18.9 -> 18.4 ms); chi = 16 full devices keep the 16-column strips.
        // qpw is then set to the quads per workgroup launch_quad instantiates for (CHI, qcg), so that the trunk
        // estimate and PQD_QPW mean what the kernel runs
        const int nbq = (n_traj + pc.BT - 1) / pc.BT;  // blocks (build_blocks)
        pc.qcg = (nbq <= n_cu || (CHI == 32 && pc.qpw == 1)) ? 2 : 4;
        if (env.qcg) pc.qcg = (env.qcg == 1 && CHI != 32) ? 4 : env.qcg;
        pc.qpw = quad_qpw(CHI, pc.qpw, pc.qcg);
    }
    // batches the single-trajectory split groups do not take: split groups of TB trajectories each (pt_msplit.hip),
    // G = N2 / 2 workgroups per group (N2 = 9: 9), up to 32 / G groups per XCD (their hand-offs in one L2). PQD_MSPLIT: 0 off, 1 auto,
    // 2 whenever supported; PQD_MS_TB forces the trajectories per group
    int mode = env.msplit;
    // PQD_SPLIT=0 (batched kernel only) and a forced trunk pre-pass (PQD_TRUNK=1) keep the batched path
    if (env.split == 0) mode = 0;
    if (env.trunk == 1 && mode == 1) mode = 0;
    if (sh.pt && CHI == 256) mode = 2;  // no other path holds chi = 256
    const int bpc = (sh.pt && !pc.split && mode != 0 && fuse_on && n_traj >= 1 && msplit_supported(N2, CHI, sh.n_out))
                        ? caps.msplit_blocks_per_cu(N2, CHI) : 0;
    if (bpc >= 1) {
        const int G = msplit_group_size(N2, CHI);
        const int resident = n_cu * bpc / G;          // groups the device holds at once
        const int gps = 32 / G;                        // groups per XCD slot (32 CUs per XCD on MI355X)
        // PQD_SPLIT_XCD=0: the plain grid (groups may span XCDs, sc1 exchange), as many groups as are resident
        bool xgrid = env.split_xcd;
        // where the XCD slots hold fewer groups than the device (G > 16: one group of 18 per 32 CUs at N2 = 36)
        // and that leaves more than 8 trajectories per group, the plain grid's extra groups pay for its cross-XCD
        // exchange (six-level, 128 trajectories: 11.6 against 14.6 us per grid step; equal at 64, slower below,
        // profiles/r06/msx2/)
        if (xgrid && gps >= 1 && 8 * gps < resident) {
            const int tbx = (n_traj + 8 * gps - 1) / (8 * gps), tbp = (n_traj + resident - 1) / resident;
            if (tbx > 8 && tbp < tbx) xgrid = false;
        }
        const int max_groups = std::min(resident, (xgrid && gps >= 1) ? 8 * gps : resident);
        const int TB = std::max((n_traj + max_groups - 1) / std::max(1, max_groups), env.ms_tb);
        const int n_groups = (n_traj + TB - 1) / TB;
        // auto: while a group's per-step work stays below the batched kernel's per-step time
        // (DESIGN.md §4.10); the single-trajectory groups keep the batches they fit
        // and while shared trunks would save little: the batched sweep starts each slot at its branch step (a
        // G2_reuse grid saves about half of its steps there), a split group runs every trajectory from step 0
        // (a system's trunk itself is propagated once: what sharing saves is the activations beyond its longest)
        int64_t shared = 0, total = 0;
        std::vector<int> amax(sh.n_sys, 0);
        for (int t = 0; t < n_traj; ++t) {
            const int a = std::max(0, std::min(to.jv[t], tr->out_begin[t]));
            shared += a;
            amax[tsys[t]] = std::max(amax[tsys[t]], a);
            total += tr->out_end[t] + 1;
        }
        for (int y = 0; y < sh.n_sys; ++y) shared -= amax[y];
        // (measured, profiles/r06/bfly/c4ntraj.log, µs per grid step vs the batched kernel: 32 trajectories TB = 1
        // 2.8 vs 13.5; 256 TB = 8 6.0 vs 11.8; 384 TB = 12 8.3 vs 11.5; 512 TB = 16 9.8 vs 11.1)
        const bool want = mode == 2 || (TB <= 16 && 4 * shared <= total);
        // a group's composite MTO steps are held in LDS (pt_msplit.hip s_cev): at most msplit_cev_max() per group
        int max_cev = 0;
        for (int k0 = 0; k0 < n_traj; k0 += TB) {
            int c = 0;
            for (int k = k0; k < std::min(n_traj, k0 + TB); ++k) {
                const int t = to.order[k];
                for (int i = E.ev_start[t]; i < E.ev_start[t + 1]; ++i)
                    if (i == E.ev_start[t] || E.evs[i].x != E.evs[i - 1].x) ++c;
            }
            max_cev = std::max(max_cev, c);
        }
        if (want && TB <= msplit_tbmax(N2, CHI) && n_groups <= resident && max_cev <= msplit_cev_max()) {
            pc.msplit = true;
            pc.ms_TB = TB;
            pc.ms_groups = n_groups;
            pc.ms_xcd = (xgrid && gps >= 1 && n_groups <= 8 * gps) ? (n_groups + 7) / 8 : 0;
            if (!env.split_xcd) pc.ms_xcd = 0;
        }
    }
    if (sh.pt && CHI == 256 && !pc.msplit)
        return fail(PQD_ERR_UNSUPPORTED, "chi 256 runs on multi-trajectory split groups only: %d trajectories at N2=%d do "
                    "not fit one launch of them (at most 8 per group), or the plan has no fused steps (PQD_FUSE=0)",
                    n_traj, N2);
    return PQD_OK;
}

// Lock-step blocks of BT slots, filled in block order. Blocks may straddle systems (each wave indexes its own
// system's propagators), so a scan with one trajectory per system still fills every slot of a workgroup. bt: the
// slots' trajectories (-1 empty), be / bs: a block's last step and first system, ba / bsrc: branch_slots
struct Blocks {
    std::vector<int> bt, be, bs, ba, bsrc;
};
static Blocks build_blocks(int BT, const TrajOrder& to, const std::vector<int>& tsys, const pqd_traj* tr,
                           bool branch_on) {
    Blocks B;
    for (size_t k = 0; k < to.order.size();) {
        const int sy = tsys[to.order[k]];
        int filled = 0, end = 0;
        const size_t b0 = B.bt.size();
        while (k < to.order.size() && filled < BT) {
            B.bt.push_back(to.order[k]);
            end = std::max(end, tr->out_end[to.order[k]]);
            ++k; ++filled;
        }
        for (; filled < BT; ++filled) B.bt.push_back(-1);
        // slots by branch step (empty ones last): the trunk passes from slot to slot
        std::stable_sort(B.bt.begin() + b0, B.bt.end(), [&](int a, int b) {
            if (a < 0 || b < 0) return a >= 0 && b < 0;
            return to.jv[a] < to.jv[b];
        });
        B.ba.resize(B.bt.size());
        B.bsrc.resize(B.bt.size());
        branch_slots(BT, B.bt.data() + b0, to.jv, tr->out_begin, tsys, branch_on, B.ba.data() + b0, B.bsrc.data() + b0);
        B.be.push_back(end);
        B.bs.push_back(sy);
    }
    return B;
}

// Trunk pre-pass instead of in-workgroup chains: every slot starts at its own branch step from a checkpoint
// of its system's MTO-free trunk, which one trajectory per system propagates first. Chosen (PQD_TRUNK=-1,
// auto) when the estimated critical path — trunk latency + the longest block from its first activation — is
// shorter than the longest block from step 0; PQD_TRUNK=1 forces it, 0 disables it. Needs shared trunks (`enable`:
// a batched or quad plan with PQD_BRANCH on) and fused half steps (checkpoints hold the state with M_b(n-1) deferred).
struct TrunkChoice {
    bool use_trunk = false;
    std::vector<std::vector<int>> ck_steps;  // per system: checkpoint steps (as met; apply_trunks sorts them)
    std::vector<int> ca;                     // per slot: activation with a checkpoint (0 = fresh)
};
static TrunkChoice choose_trunks(const PlanShape& sh, const PathChoice& pc, const Blocks& B, const TrajOrder& to,
                                 const std::vector<int>& tsys, const pqd_traj* tr, bool enable, int trunk_mode,
                                 int n_cu) {
    TrunkChoice tc;
    tc.ca.assign(B.bt.size(), 0);
    tc.ck_steps.resize(sh.n_sys);
    if (!enable || trunk_mode == 0 || sh.n_steps <= 0) return tc;
    const int BT = pc.BT, N2 = sh.N2;
    // estimated main-sweep time in steps of one block: the longest block (critical path) or, with more blocks than
    // the device holds at once, the total block-steps over the resident blocks, whichever is larger. Without the
    // pre-pass a block spans [0, end] (its chain's first slot carries the trunk from step 0, dormant slots cost a
    // lock-step block the same), with it [first activation, end]
    int64_t crit_no = 0, crit_tk = 0, max_ck = 0, sum_no = 0, sum_tk = 0;
    const int nbk = (int)B.be.size();
    for (int b = 0; b < nbk; ++b) {
        int start = INT_MAX;
        for (int q = 0; q < BT; ++q) {
            const int t = B.bt[(size_t)b * BT + q];
            if (t < 0) continue;
            const int a = std::max(0, std::min(to.jv[t], tr->out_begin[t]));
            tc.ca[(size_t)b * BT + q] = a;
            start = std::min(start, a);
            if (a >= 1) { tc.ck_steps[tsys[t]].push_back(a); max_ck = std::max<int64_t>(max_ck, a); }
        }
        crit_no = std::max<int64_t>(crit_no, B.be[b]);
        sum_no += B.be[b];
        if (start != INT_MAX) {
            crit_tk = std::max<int64_t>(crit_tk, B.be[b] - start);
            sum_tk += B.be[b] - start;
        }
    }
    // blocks resident at once: quads (one workgroup of qpw quads per CU) or BT-workgroups as the LDS allows
    int64_t conc = n_cu;
    if (pc.quad) {
        conc = (int64_t)n_cu * (sh.CHI == 32 ? 2 : pc.qpw);  // chi = 32: two quads per CU either way
    } else {
        const int64_t lds = ((int64_t)BT * (N2 * (sh.CHI + 1) + 4) + (int64_t)BT * N2) * 16;
        conc = (int64_t)n_cu * std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / std::max<int64_t>(1, lds)));
    }
    const double t_no = std::max((double)crit_no, (double)sum_no / (double)conc);
    const double t_tk = std::max((double)crit_tk, (double)sum_tk / (double)conc);
    // trunk step latency relative to a lock-step main-sweep step: split groups (N2 >= 9) ~0.5, one batched
    // workgroup ~0.7
    const double r = N2 >= 9 ? 0.5 : 0.7;
    tc.use_trunk = max_ck > 0 && (trunk_mode == 1 || t_tk + r * (double)max_ck < 0.995 * t_no);
    return tc;
}

// the chosen trunk pre-pass: number the checkpoints, point every slot with an activation at its checkpoint (blk_src =
// -2 - index) and lay the trunks out (plan_trunks)
static int apply_trunks(pqd_plan* P, TrunkChoice& tc, Blocks& B, const std::vector<int>& tsys, const pqd_pt* pt,
                        const PlanEnv& env, const DeviceCaps& caps, hipStream_t s) {
    std::vector<int> ck_base(P->n_sys, 0);
    int n_ck = 0;
    for (int y = 0; y < P->n_sys; ++y) {
        auto& v = tc.ck_steps[y];
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        ck_base[y] = n_ck;
        n_ck += (int)v.size();
    }
    for (size_t i = 0; i < B.bt.size(); ++i) {
        const int t = B.bt[i];
        if (t < 0) continue;
        const int a = tc.ca[i];
        if (a >= 1) {
            const auto& v = tc.ck_steps[tsys[t]];
            const int idx = ck_base[tsys[t]] + (int)(std::lower_bound(v.begin(), v.end(), a) - v.begin());
            B.ba[i] = a;
            B.bsrc[i] = -2 - idx;
        } else {
            B.ba[i] = 0;
            B.bsrc[i] = -1;
        }
    }
    return plan_trunks(P, tc.ck_steps, ck_base, n_ck, pt, env, caps, s);
}

// the blocks on the device (a plan without trajectories gets one empty block), their hash, and the trajectory-steps
// of the main sweep (after the trunks' own, which plan_trunks counted); then the slice schedule and the output buffer.
// Device buffers are allocated in the order plan creation always did: the sweep's time moves by up to 0.4% with where
// its buffers lie (profiles/r08/plan_stages/), so the stages change nothing about their placement
static int upload_blocks(pqd_plan* P, Blocks& B, const pqd_traj* tr, const std::vector<int32_t>& sch, hipStream_t s) {
    for (size_t i = 0; i < B.bt.size(); ++i)
        if (B.bt[i] >= 0) P->traj_steps += tr->out_end[B.bt[i]] - B.ba[i] + 1;
    P->n_blocks = (int)B.be.size();
    if (B.bt.empty()) { B.bt.assign(P->BT, -1); B.be.assign(1, 0); B.bs.assign(1, 0); B.ba.assign(P->BT, INT_MAX); B.bsrc.assign(P->BT, -1); }
    HIPCHK(P->blk_traj.upload(B.bt.data(), B.bt.size(), s));
    HIPCHK(P->blk_end.upload(B.be.data(), B.be.size(), s));
    HIPCHK(P->blk_sys.upload(B.bs.data(), B.bs.size(), s));
    HIPCHK(P->blk_act.upload(B.ba.data(), B.ba.size(), s));
    HIPCHK(P->blk_src.upload(B.bsrc.data(), B.bsrc.size(), s));
    P->h_blocks = fnv1a(B.bsrc, fnv1a(B.ba, fnv1a(B.bs, fnv1a(B.be, fnv1a(B.bt)))));
    HIPCHK(P->sched.upload(sch.data(), sch.size(), s));
    HIPCHK(P->out.alloc(std::max<int64_t>(1, P->out_len)));
    HIPCHK(hipMemsetAsync(P->out.p, 0, std::max<int64_t>(1, P->out_len) * sizeof(double2), s));
    return PQD_OK;
}

// Per block, the first step of the lean instance's fast region (pt_sweep.hip LeanCol): from it on every occupied slot
// enters each step fused, has no MTO event at that step or later, and was activated at an earlier step. A slot enters
// step n fused when it was active at n - 1 and has no event at n (events are sorted by step per trajectory), so the step
// is 1 + the largest activation or event step of the block's slots; INT_MAX where that leaves no fast step (the region
// ends before the block's last PT step, n_end - 1: every fast step loads PT operands for its successor) or the block is
// empty
static std::vector<int> block_fast_steps(int BT, const Blocks& B, const MtoEvents& E) {
    std::vector<int> bf(B.be.size(), INT_MAX);
    for (size_t b = 0; b < B.be.size(); ++b) {
        int64_t f = 1;
        bool any = false;
        for (int q = 0; q < BT; ++q) {
            const int t = B.bt[b * BT + q];
            if (t < 0) continue;
            any = true;
            f = std::max<int64_t>(f, (int64_t)B.ba[b * BT + q] + 1);
            if (E.ev_start[t + 1] > E.ev_start[t]) f = std::max<int64_t>(f, (int64_t)E.evs[E.ev_start[t + 1] - 1].x + 1);
        }
        if (any && f < (int64_t)B.be[b] - 1) bf[b] = (int)f;
    }
    return bf;
}

// Per block, the system whose column operands F(n + 1), W(n + 1) the fast region stages in LDS during the PT phase of
// step n (pt_sweep.hip LeanStage): the one system of all its occupied slots, or -1 where the block has no fast region
// or its slots mix systems (one staging area holds one system's operands; such a block loads them in place as before)
static std::vector<int> block_stage_systems(int BT, const Blocks& B, const std::vector<int>& tsys,
                                            const std::vector<int>& blk_fast) {
    std::vector<int> bs(B.be.size(), -1);
    for (size_t b = 0; b < B.be.size(); ++b) {
        if (blk_fast[b] == INT_MAX) continue;
        int y = -1;
        bool one = true;
        for (int q = 0; q < BT; ++q) {
            const int t = B.bt[b * BT + q];
            if (t < 0) continue;
            if (y < 0) y = tsys[t];
            one = one && tsys[t] == y;
        }
        if (one) bs[b] = y;
    }
    return bs;
}

// the free-propagator build of a plan: idle operators and pulse windows. After the trunks: windows need n_trunk == 0
static int setup_free_props(pqd_plan* P, const pqd_grid* grid, const PlanEnv& env, hipStream_t s) {
    const int n_sys = P->n_sys, ns = P->n_steps;
    const size_t m2 = (size_t)P->N2 * P->N2;
    P->fp.systems = P->systab.p; P->fp.n_sys = n_sys;
    if (env.idle) {  // PQD_IDLE=0: compute every half step (A/B)
        HIPCHK(P->Midle.alloc((size_t)n_sys * m2));
        P->fp.Midle = P->Midle.p;
        // pulse windows: half steps outside a system's [first, last] non-idle half step are neither stored nor
        // re-read (kernels take Midle / Fidle / Widle there). PQD_WIN=0 stores every half step, 2 always uses the
        // windows, 1 (default) uses them when they leave out at least a tenth of the half steps
        // Windows only where every kernel of the plan reads through them: the quad and no-PT kernels without a
        // trunk pre-pass (the batched sweep reads every half step as stored; the split path may fall back to it).
        const bool win_ok = (P->nopt || P->quad) && P->n_trunk == 0;
        if (win_ok && env.win != 0) {
            HIPCHK(P->win.alloc((size_t)n_sys));
            P->fp.win = P->win.p;
            P->win_mode = env.win;
        }
    }
    P->fp.ta = grid->ta; P->fp.dt = grid->dt; P->fp.n_steps = ns; P->fp.n_sub = grid->n_sub; P->fp.M = P->M.p;
    if (P->win.p && P->win_mode == 1 && ns > 0) {
        HIPCHK(launch_free_win(P->fp, s));
        std::vector<int2> wh(n_sys);
        HIPCHK(hipMemcpyAsync(wh.data(), P->win.p, sizeof(int2) * n_sys, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int64_t stored = 0;
        for (const int2& w : wh) stored += w.y >= w.x ? (int64_t)(w.y - w.x + 1) : 0;
        if (10 * stored > 9 * (int64_t)n_sys * 2 * ns) {  // windows leave out < 10%: store every half step
            P->win.release();
            P->fp.win = nullptr;
        }
    }
    P->fp.packed4 = env.fp4;
    P->fp.mfma = env.fpm;
    return PQD_OK;
}

// the launch parameters of the main sweep: the plan's buffers, the kernel variants, the PT row units, the fused
// half steps, and whether the plan runs the lean instance
static int fill_sweep_params(pqd_plan* P, const pqd_pt* pt, const PlanEnv& env, const std::vector<int>& blk_fast,
                             const std::vector<int>& blk_stage, hipStream_t s) {
    const int n_sys = P->n_sys, ns = P->n_steps, N2 = P->N2, n_out = P->n_out;
    const size_t m2 = (size_t)N2 * N2;
    SweepParams& sp = P->sp;
    sp.M = P->M.p;
    if (pt) {
        sp.Q = pt->Q.p; sp.Qsum = pt->Qsum.p; sp.D = pt->D; sp.closure = pt->closure.p; sp.closure0 = pt->closure0.p;
        sp.bond0 = pt->bond0.p; sp.gmap = pt->gmap.p;
    }
    sp.sched = P->sched.p; sp.rho0 = P->rho0.p; sp.n_out = n_out; sp.ovec = P->ovec.p;
    sp.blk_traj = P->blk_traj.p; sp.blk_end = P->blk_end.p; sp.blk_sys = P->blk_sys.p;
    sp.blk_act = P->blk_act.p; sp.blk_src = P->blk_src.p;
    sp.traj_sys = P->traj_sys.p; sp.m_stride = (long long)2 * ns * m2; sp.wbeg = P->wbeg.p; sp.wend = P->wend.p;
    sp.ablate = env.ablate;
    // exchange form: counter (default; with the XCD-grouped grid C3 runs 5.02 us per step against 5.33 for the granules,
    // profiles/r04/split/xcd/) or data-tagged granules (PQD_SPLIT_GRAN=1)
    sp.split_gran = env.split_gran ? 1 : 0;
    sp.split_ow = env.split_ow ? 1 : 0;  // the output workgroup (pt_split.hip OWG): the flag split_capacity sized groups with
    sp.split_xcd = env.split_xcd ? 1 : 0;
    sp.split_l2 = env.split_l2 ? 1 : 0;
    // polls of a split group's counter before the wait counts as a timeout (~0.1 s); PQD_SPLIT_SPIN overrides
    // it (tests provoke the batched fallback with 0)
    sp.spin_limit = env.split_spin;
    HIPCHK(P->flags.alloc(4));
    HIPCHK(hipMemsetAsync(P->flags.p, 0, 4 * sizeof(unsigned), s));
    sp.flags = P->flags.p;
    // PT rows: 3M on the matrix cores; at BT = 4 (N2 > 16, chi = 128) with two k-steps of the slice in flight
    // (six-level scan c5: 84.7 -> 79.5 ms per launch, profiles/r03/exp_c/c5_ptmode.log)
    sp.pt_mode = env.pt_mode_set ? env.pt_mode : (P->BT == 4 ? 5 : 4);
    sp.cmul3 = env.cmul3;
    sp.trpre = env.trpre;
    sp.colbig = env.colbig;
    if (pt && (sp.pt_mode == 4 || sp.pt_mode == 5)) {
        const int nw = P->BT * sweep_wpt(P->N2, P->BT, P->CHI);
        int rmax = sweep_rmax(P->N2, P->BT, P->CHI);
        if (env.rowpair >= 0) rmax = std::max(1, std::min(rmax, env.rowpair ? rmax : 1));
        // rows that stay exactly zero get no unit (P->live: all 1 unless the main path is this sweep and PQD_LIVE_ROWS
        // is on). The lean instance balances what is left below row granularity (lean_part_units; PQD_LIVE_PART=0: whole
        // rows only); whether the plan will run it is asked with the fields fill_sweep_params sets further down
        bool dead = false;
        for (uint8_t v : P->live) dead = dead || !v;
        std::vector<int4> u = pt_row_units(pt->gmap_h, nw, rmax, env.unitbal, dead ? &P->live : nullptr);
        if (dead && env.live_part && env.unitbal && env.rowpair < 0) {
            SweepParams t = sp;
            t.fuse = (!P->nopt && ns > 0 && env.fuse) ? 1 : 0;
            t.trpre = t.fuse ? env.trpre : 0;
            t.units = u.data();  // (only asked whether a list exists)
            t.umax = 3;
            if (sweep_lean_ok(P, t, env)) {
                std::vector<int4> pu = lean_part_units(pt->gmap_h, nw, P->live);
                if (!pu.empty()) {
                    u.swap(pu);
                    sp.lean_parts = 1;
                }
            }
        }
        HIPCHK(P->units.upload(u.data(), u.size(), s));
        P->h_units = fnv1a(u);
        sp.units = P->units.p;
        sp.umax = (int)(u.size() / nw);
        for (int w = 0; w < nw; ++w) P->h_unit0.push_back(u[(size_t)w * sp.umax].x);
    }
    sp.fuse = (!P->nopt && ns > 0 && env.fuse) ? 1 : 0;
    if (!sp.fuse) sp.trpre = 0;  // the prefetched rows are W(n), which exists only with fused half steps
    if (sp.fuse) {
        HIPCHK(P->F.alloc((size_t)n_sys * ns * m2));
        HIPCHK(P->W.alloc((size_t)n_sys * (ns + 1) * n_out * N2));
        P->fu = FuseParams{P->M.p, P->F.p, P->W.p, P->ovec.p, n_sys, ns, n_out};
        P->fu.mfma = P->fp.mfma;
        if (P->win.p) {
            HIPCHK(P->Fidle.alloc((size_t)n_sys * m2));
            HIPCHK(P->Widle.alloc((size_t)n_sys * n_out * N2));
            P->fu.win = P->win.p; P->fu.Midle = P->Midle.p; P->fu.Fidle = P->Fidle.p; P->fu.Widle = P->Widle.p;
        }
        sp.f_stride = (long long)ns * m2;
        sp.w_stride = (long long)(ns + 1) * n_out * N2;
    }
    sp.F = P->F.p; sp.W = P->W.p;
    sp.win = P->win.p; sp.Midle = P->Midle.p; sp.Fidle = P->Fidle.p; sp.Widle = P->Widle.p;
    sp.woff = P->woff.p; sp.ev_start = P->ev_start.p; sp.ev = P->ev.p; sp.sop = P->sop.p; sp.out = P->out.p;
    sp.n_steps = ns;
    sp.n_blk = P->n_blocks;
    // quad kernel: waves raise their priority outside the PT contraction, so a wave on its serial chain (column
    // operator, exchange, relayout) issues ahead of the other quad's MFMA stream on the same SIMD (C2: 17.5 -> 16.1 ms;
    // a static bias between the grid halves gains nothing; profiles/r03/quad_prio.log)
    sp.qprio = env.qprio;
    sp.lean = sweep_lean_ok(P, sp, env) ? 1 : 0;
    if (sp.lean_parts && !sp.lean)  // partial units are read by the lean instance alone (asked above with these fields)
        return fail(PQD_ERR_UNSUPPORTED, "internal: a unit list with partial units outside the lean instance");
    // the lean instance's column phase in the compact index of the live rows: 3 k-steps instead of 4 where 9 to 12 rows
    // are live. lean_part_units returns a list for exactly these counts (Tq = 5 or 6 quarters per wave; 13 and 14 do not
    // fit one partial unit per wave), and the compacted code exists in the instance for partial units only, so any other
    // plan keeps all four k-steps (PQD_LIVE_COL=0: every plan)
    sp.lean_colk = 4;
    sp.lean_rho = 0;
    if (sp.lean && sp.lean_parts && env.live_col && P->live.size() == 16) {
        std::vector<uint8_t> rho;
        int n_live = 0;
        for (uint8_t v : P->live) n_live += v != 0;
        if (n_live >= 9 && n_live <= 12 && live_col_map(P->live, rho) == 3) {
            sp.lean_colk = 3;
            for (int c = 0; c < 16; ++c) sp.lean_rho |= (unsigned long long)(rho[c] & 15) << (4 * c);
        }
    }
    // the lean instance's readout inside the fused column phase (PQD_LEAN_RO=0: the closure pass on every step). The
    // table is the plan's last allocation, so the buffers before it lie where they did
    if (sp.lean && env.lean_ro) {
        HIPCHK(P->blk_fast.upload(blk_fast.data(), blk_fast.size(), s));
        sp.blk_fast = P->blk_fast.p;
        for (int f : blk_fast) P->lean_ro = P->lean_ro || f != INT_MAX;
        // the fast region's operands staged a step ahead (PQD_LEAN_STAGE=0: every block loads them in place); allocated
        // behind blk_fast for the same reason. A wave issues its piece in the first k-step of its first PT unit, so the
        // six waves with a piece need units (16 rows over 8 waves: they have, unless the row-unit switches leave fewer)
        bool units_ok = P->h_unit0.size() >= 6;
        for (int w = 0; units_ok && w < 6; ++w) units_ok = P->h_unit0[w] >= 0;
        if (env.lean_stage && units_ok) {
            HIPCHK(P->blk_stage.upload(blk_stage.data(), blk_stage.size(), s));
            sp.blk_stage = P->blk_stage.p;
            for (int y : blk_stage) P->n_stage += y >= 0;
        }
    }
    return PQD_OK;
}

// the tables and buffers of a plan on multi-trajectory split groups: the groups (consecutive trajectories of the
// block order, ms_TB per group), the composite MTO events, the exchange and the launch parameters
static int build_msplit_tables(pqd_plan* P, const PathChoice& pc, const std::vector<int>& order, const pqd_traj* tr,
                               const std::vector<int>& tsys, const MtoEvents& E, const PlanEnv& env, hipStream_t s) {
    const int ms_TB = pc.ms_TB, ms_groups = pc.ms_groups, ms_xcd = pc.ms_xcd, N2 = P->N2, n_out = P->n_out;
    const size_t m2 = (size_t)N2 * N2;
    std::vector<int> gt((size_t)ms_groups * ms_TB, -1), ge(ms_groups, 0);
    for (int k = 0; k < tr->n_traj; ++k) {
        const int gi = k / ms_TB, t = order[k];
        gt[(size_t)gi * ms_TB + k % ms_TB] = t;
        ge[gi] = std::max(ge[gi], tr->out_end[t]);
    }
    // composite MTO events: one per (trajectory, step) with MTOs, the before / after superoperators of that step
    std::vector<int4> ce;
    std::vector<int> cs(tr->n_traj + 1, 0);
    for (int t = 0; t < tr->n_traj; ++t) {
        cs[t] = (int)ce.size();
        for (int i = E.ev_start[t]; i < E.ev_start[t + 1]; ++i) {
            const int4 v = E.evs[i];
            if (ce.size() > (size_t)cs[t] && ce.back().x == v.x) {
                if (v.y == 0) ce.back().y = v.z; else ce.back().z = v.z;
            } else {
                ce.push_back(make_int4(v.x, v.y == 0 ? v.z : -1, v.y == 0 ? -1 : v.z, tsys[t]));
            }
        }
    }
    cs[tr->n_traj] = (int)ce.size();
    P->n_cev = (int)ce.size();
    if (ce.empty()) ce.push_back(make_int4(INT_MAX, -1, -1, 0));
    HIPCHK(P->ms_gtraj.upload(gt.data(), gt.size(), s));
    HIPCHK(P->ms_gend.upload(ge.data(), ge.size(), s));
    HIPCHK(P->cev.upload(ce.data(), ce.size(), s));
    P->h_groups = fnv1a(ce, fnv1a(ge, fnv1a(gt)));
    HIPCHK(P->cev_start.upload(cs.data(), cs.size(), s));
    HIPCHK(P->Fev.alloc((size_t)std::max(1, P->n_cev) * m2));
    HIPCHK(P->Wev.alloc((size_t)std::max(1, P->n_cev) * n_out * N2));
    HIPCHK(P->msX.alloc((size_t)ms_groups * ms_TB * 2 * N2 * P->CHI));
    HIPCHK(P->ms_cnt.alloc((size_t)ms_groups * 64));
    HIPCHK(P->err.alloc(4));
    // L2-kept exchange lines on the XCD-grouped grid (PQD_MS_L2=0: sc1 stores, as on the plain grid)
    const int l2keep = ms_xcd > 0 && env.ms_l2;
    // PT contraction on the matrix cores from 3 trajectories per group (a row block of 4 rows per MFMA; below
    // that the VALU path's per-trajectory work is smaller); PQD_MS_PTM=0/1 forces the VALU / matrix-core path
    const int ptm = env.ms_ptm >= 0 ? env.ms_ptm : (ms_TB >= 3 && P->CHI <= 64);
    P->mq = MsplitParams{P->ms_gtraj.p, P->ms_gend.p, P->cev_start.p, P->cev.p, P->Fev.p, P->Wev.p,
                         ms_TB, ms_groups, ms_xcd, l2keep, ptm};
    return PQD_OK;
}

// A plan on the Hilbert-space path (lind_hilbert.hip): per system K0 = -(i/hbar) H0 - 1/2 sum_k gamma_k A_k^dag A_k,
// the channel operators scaled by -i/hbar, the jump operators' nonzeros by rows and the Frobenius norms of the kernel's
// step bound; MTOs as the N x N operators they are, in array order inside a (trajectory, step, phase) slot. No
// superoperator, block, trunk or free propagator is built. Refuses a system whose bound needs more than HB_SMAX
// Taylor factors per sub-step (a non-finite bound passes: the run then ends in PQD_ERR_NUMERIC).
static int setup_hilbert(pqd_plan* P, const pqd_system* systems, const std::vector<int>& tsys, const pqd_grid* grid,
                         const pqd_c128* rho0, const pqd_c128* out_ops, const pqd_traj* tr, hipStream_t s) {
    const int N = systems->dim, NN = N * N, n_sys = P->n_sys, n_out = P->n_out, n_w = std::max(1, P->n_traj);
    const double w = 0.5 * grid->dt / grid->n_sub;
    std::vector<cd> k0((size_t)n_sys * NN), xs, xt, sm, val, valg;
    std::vector<int> row, col;
    std::vector<HilbertSys> tab(n_sys);
    std::vector<size_t> oX(n_sys), oM(n_sys), oR(n_sys), oV(n_sys);
    auto fro = [&](const cd* A) { double q = 0; for (int e = 0; e < NN; ++e) q += std::norm(A[e]); return std::sqrt(q); };
    int nl_max = 0;
    size_t csr_max = 0;
    for (int k = 0; k < n_sys; ++k) {
        const pqd_system& y = systems[k];
        HilbertSys& h = tab[k];
        const cd mih(0.0, -1.0 / y.hbar);
        cd* K0 = k0.data() + (size_t)k * NN;
        for (int e = 0; e < NN; ++e) K0[e] = mih * C(y.H0)[e];
        h.n_lind = y.n_lind;
        h.nD = 0.0;
        oR[k] = row.size();
        oV[k] = val.size();
        for (int q = 0; q < y.n_lind; ++q) {
            const cd* A = C(y.lind_ops) + (size_t)q * NN;
            const double g = y.lind_rates[q];
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    cd a = 0;
                    for (int m = 0; m < N; ++m) a += std::conj(A[m * N + i]) * A[m * N + j];
                    K0[i * N + j] -= 0.5 * g * a;
                }
            const double nA = fro(A);
            h.nD += std::fabs(g) * nA * nA;
            for (int i = 0; i < N; ++i) {
                row.push_back((int)(val.size() - oV[k]));
                for (int j = 0; j < N; ++j)
                    if (A[i * N + j] != cd(0.0)) {
                        col.push_back(j);
                        val.push_back(A[i * N + j]);
                        valg.push_back(g * std::conj(A[i * N + j]));
                    }
            }
            row.push_back((int)(val.size() - oV[k]));
        }
        h.nnz = (int)(val.size() - oV[k]);
        h.nK0 = fro(K0);
        h.n_chan = y.n_chan;
        h.n_samples = std::max(1, y.n_samples);
        h.s_t0 = y.sample_t0;
        h.s_dt = y.n_chan > 0 ? y.sample_dt : 1.0;
        oX[k] = xs.size();
        oM[k] = sm.size();
        double bound = h.nK0;
        for (int p = 0; p < y.n_chan; ++p) {
            const cd* X = C(y.chan_ops) + (size_t)p * NN;
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    xs.push_back(mih * X[i * N + j]);
                    xt.push_back(mih * std::conj(X[j * N + i]));
                }
            h.nX[p] = fro(xs.data() + xs.size() - NN) + fro(xt.data() + xt.size() - NN);
            const cd* f = C(y.chan_samples) + (size_t)p * y.n_samples;
            double fmax = 0.0;
            for (int q = 0; q < y.n_samples; ++q) fmax = std::max(fmax, std::abs(f[q]));  // a NaN sample is skipped here
            bound += fmax * h.nX[p];
            sm.insert(sm.end(), f, f + y.n_samples);
        }
        const double theta = w * (2.0 * bound + h.nD);
        if (std::isfinite(theta) && theta > (double)HB_SMAX)
            return fail(PQD_ERR_UNSUPPORTED, "system %d: the norm bound of L w is %.3g, above %d Taylor factors per "
                        "sub-step (lower dt or raise n_sub)", k, theta, HB_SMAX);
        nl_max = std::max(nl_max, y.n_lind);
        csr_max = std::max(csr_max, hilbert_csr_bytes(N, y.n_lind, h.nnz));
    }
    if (xs.empty()) { xs.assign(1, 0.0); xt.assign(1, 0.0); }
    if (sm.empty()) sm.assign(1, 0.0);
    if (val.empty()) { val.assign(1, 0.0); valg.assign(1, 0.0); col.assign(1, 0); }
    if (row.empty()) row.assign(1, 0);
    HIPCHK(P->hb_K0.upload(reinterpret_cast<double2*>(k0.data()), k0.size(), s));
    HIPCHK(P->hb_Xs.upload(reinterpret_cast<double2*>(xs.data()), xs.size(), s));
    HIPCHK(P->hb_Xt.upload(reinterpret_cast<double2*>(xt.data()), xt.size(), s));
    HIPCHK(P->samples.upload(reinterpret_cast<double2*>(sm.data()), sm.size(), s));
    HIPCHK(P->hb_val.upload(reinterpret_cast<double2*>(val.data()), val.size(), s));
    HIPCHK(P->hb_valg.upload(reinterpret_cast<double2*>(valg.data()), valg.size(), s));
    HIPCHK(P->hb_col.upload(col.data(), col.size(), s));
    HIPCHK(P->hb_row.upload(row.data(), row.size(), s));
    for (int k = 0; k < n_sys; ++k) {
        tab[k].K0 = P->hb_K0.p + (size_t)k * NN;
        tab[k].Xs = P->hb_Xs.p + oX[k];
        tab[k].Xt = P->hb_Xt.p + oX[k];
        tab[k].samples = P->samples.p + oM[k];
        tab[k].rowptr = P->hb_row.p + oR[k];
        tab[k].col = P->hb_col.p + oV[k];
        tab[k].val = P->hb_val.p + oV[k];
        tab[k].valg = P->hb_valg.p + oV[k];
    }
    HIPCHK(P->hb_systab.upload(tab.data(), tab.size(), s));
    HIPCHK(P->traj_sys.upload(tsys.data(), tsys.size(), s));

    // MTO events per trajectory, stable-sorted by (step, phase): (step, 1 after the output / 0 before, operator, kind)
    std::vector<std::vector<int>> per(tr->n_traj);
    for (int q = 0; q < tr->n_mto; ++q) per[tr->mto_traj[q]].push_back(q);
    std::vector<int> ev_start(tr->n_traj + 1, 0);
    std::vector<int4> evs;
    for (int t = 0; t < tr->n_traj; ++t) {
        auto& v = per[t];
        auto key = [&](int q) { return 2 * tr->mto_step[q] + (tr->mto_before[q] ? 0 : 1); };
        std::stable_sort(v.begin(), v.end(), [&](int a, int b) { return key(a) < key(b); });
        ev_start[t] = (int)evs.size();
        for (int q : v) evs.push_back(make_int4(key(q) >> 1, key(q) & 1, q, tr->mto_kind[q]));
        P->traj_steps += tr->out_end[t] + 1;
    }
    ev_start[tr->n_traj] = (int)evs.size();
    if (evs.empty()) evs.push_back(make_int4(-1, -1, 0, 0));
    HIPCHK(P->ev.upload(evs.data(), evs.size(), s));
    HIPCHK(P->ev_start.upload(ev_start.data(), ev_start.size(), s));
    if (tr->n_mto > 0)
        HIPCHK(P->sop.upload(reinterpret_cast<const double2*>(tr->mto_ops), (size_t)tr->n_mto * NN, s));
    std::vector<cd> ov((size_t)n_out * NN);
    for (int k = 0; k < n_out; ++k)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) ov[(size_t)k * NN + i * N + j] = C(out_ops)[(size_t)k * NN + j * N + i];
    HIPCHK(P->ovec.upload(reinterpret_cast<double2*>(ov.data()), ov.size(), s));
    HIPCHK(P->rho0.upload(reinterpret_cast<const double2*>(rho0), NN, s));
    HIPCHK(P->wbeg.upload(tr->out_begin, n_w, s));
    HIPCHK(P->wend.upload(tr->out_end, n_w, s));
    HIPCHK(P->woff.upload(reinterpret_cast<const long long*>(tr->out_offset), n_w, s));
    HIPCHK(P->out.alloc(std::max<int64_t>(1, P->out_len)));
    HIPCHK(hipMemsetAsync(P->out.p, 0, std::max<int64_t>(1, P->out_len) * sizeof(double2), s));
    HIPCHK(P->flags.alloc(4));
    HIPCHK(hipMemsetAsync(P->flags.p, 0, 4 * sizeof(unsigned), s));

    HilbertParams& hp = P->hp;
    hp.systems = P->hb_systab.p; hp.traj_sys = P->traj_sys.p;
    hp.N = N; hp.n_sub = grid->n_sub; hp.n_out = n_out; hp.nl_max = nl_max;
    hp.ta = grid->ta; hp.dt = grid->dt;
    hp.rho0 = P->rho0.p; hp.ovec = P->ovec.p; hp.wbeg = P->wbeg.p; hp.wend = P->wend.p; hp.woff = P->woff.p;
    hp.ev_start = P->ev_start.p; hp.ev = P->ev.p; hp.mto = P->sop.p; hp.out = P->out.p;
    hp.csr_lds = csr_max <= (size_t)HB_CSR_LDS ? (int)csr_max : 0;
    P->BT = 1;
    P->n_blocks = P->n_traj;
    HIPCHK(hipStreamSynchronize(s));  // the uploads read host vectors of this frame
    return PQD_OK;
}

// slices of the bond in flight in a free half step of lind_hilbert_pt.hip: as many as the thread bound (N^2 rounded up
// to whole waves per slice), the LDS beside the nonzero lists (K and Kd once, R, T, Tn and nl_max B_k per slice) and chi
// allow, then the fewest that keep the number of passes over the bond (no idle groups in the last pass); cap > 0
// bounds it (PQD_HBPT_G). Speed only: a slice's arithmetic does not depend on it
static int hilbert_pt_groups(int N, int nl_max, int chi, int csr_lds, int cap) {
    const int nt1 = (N * N + 63) / 64 * 64;
    int G = std::min(HBPT_NT_MAX / nt1, chi);
    while (G > 1 && hbpt_mat_elems(N, nl_max, G) * sizeof(double2) + csr_lds > (size_t)HBPT_LDS_MAX) --G;
    if (cap > 0) G = std::min(G, cap);
    G = std::max(G, 1);
    const int passes = (chi + G - 1) / G;
    return (chi + passes - 1) / passes;
}

// The PT side of a plan on the Hilbert-space path with a wide PT: the schedule, the bond workspace, the elements
// ordered by dictionary entry in units of HBPT_EB, G and the LDS tile (lind_hilbert_pt.hip)
static int setup_hilbert_pt(pqd_plan* P, const pqd_pt* pt, const std::vector<int32_t>& sch, const PlanEnv& env,
                            hipStream_t s) {
    const int N = P->hp.N, NN = N * N, chi = pt->chi;
    std::vector<int> ug, uel;
    for (int g = 0; g < pt->D; ++g) {
        int fill = HBPT_EB;
        for (int a = 0; a < NN; ++a) {
            if (pt->gmap_h[a] != g) continue;
            if (fill == HBPT_EB) {
                ug.push_back(g);
                uel.insert(uel.end(), HBPT_EB, -1);
                fill = 0;
            }
            uel[uel.size() - HBPT_EB + fill++] = a;
        }
    }
    const int n_units = (int)ug.size();
    HilbertPtParams& hq = P->hq;
    hq.h = P->hp;
    hq.chi = chi; hq.D = pt->D;
    hq.G = hilbert_pt_groups(N, P->hp.nl_max, chi, P->hp.csr_lds, env.hbpt_g);
    // the tile: the units that fit the LDS the matrices take anyway (one unit where that is more: chi = 256 is 33 KB)
    const size_t cap_elems = ((size_t)HBPT_LDS_MAX - P->hp.csr_lds) / sizeof(double2);
    const size_t mat = hbpt_mat_elems(N, P->hp.nl_max, hq.G), unit = hbpt_unit_elems(chi);
    size_t ut = std::max<size_t>(1, mat / unit);
    ut = std::min<size_t>({ut, cap_elems / unit, (size_t)n_units});
    if (ut < 1) return fail(PQD_ERR_UNSUPPORTED, "chi %d: a PT unit does not fit the LDS beside the nonzero lists", chi);
    hq.ut = (int)ut;
    hq.lds_elems = (int)std::max(mat, ut * unit);
    hq.n_units = n_units;
    HIPCHK(P->sched.upload(sch.data(), sch.size(), s));
    HIPCHK(P->hq_unit_g.upload(ug.data(), ug.size(), s));
    HIPCHK(P->hq_unit_el.upload(uel.data(), uel.size(), s));
    const size_t xn = std::max<size_t>(1, (size_t)P->n_traj * chi * NN);
    if (hipError_t e = P->hq_X.alloc(xn); e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "bond workspace of %zu bytes: %s",
                    xn * sizeof(double2), hipGetErrorString(e));
    hq.Q = pt->Q.p; hq.closure = pt->closure.p; hq.closure0 = pt->closure0.p; hq.bond0 = pt->bond0.p;
    hq.sched = P->sched.p; hq.X = P->hq_X.p; hq.unit_g = P->hq_unit_g.p; hq.unit_el = P->hq_unit_el.p;
    HIPCHK(hipStreamSynchronize(s));  // the uploads read host vectors of this frame
    return PQD_OK;
}

int pqd_plan_create_multi(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                          const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                          int32_t n_out, const pqd_c128* out_ops, const pqd_traj* tr, int64_t out_len,
                          pqd_plan** out) {
    std::vector<int32_t> sch;
    int rc = check_plan_args(ctx, n_sys, systems, traj_sys, grid, pt, sched, rho0, n_out, out_ops, tr, out_len, out, sch);
    if (rc) return rc;
    const PlanEnv env = read_plan_env();
    const int N = systems->dim, N2 = N * N, ns = grid->n_steps, n_traj = tr->n_traj;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    auto* P = new pqd_plan;
    std::unique_ptr<pqd_plan> guard(P);
    P->ctx = ctx; P->N2 = N2; P->n_traj = n_traj; P->n_steps = ns; P->out_len = out_len;
    P->n_out = n_out; P->t_start = grid->ta; P->dt = grid->dt;
    P->toff.assign(n_traj + 1, 0);
    for (int t = 0; t < n_traj; ++t)
        P->toff[t + 1] = P->toff[t] + (long long)(1 + n_out) * (tr->out_end[t] - tr->out_begin[t] + 1);
    P->nopt = (pt == nullptr);
    P->CHI = pt ? pt->CHI : 1;
    P->n_sys = n_sys;
    DeviceCaps caps{256, split_blocks_per_cu, msplit_blocks_per_cu};
    if (hipDeviceProp_t prop; hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) caps.n_cu = prop.multiProcessorCount;
    P->n_cu = caps.n_cu;

    std::vector<int> tsys(std::max(1, n_traj), 0);
    for (int t = 0; t < n_traj; ++t) tsys[t] = traj_sys ? traj_sys[t] : 0;
    // without a PT, dim > 6 runs in Hilbert space (nothing else holds it); PQD_HILBERT=1 sends dim <= 6 there too,
    // where the systems keep to the kernel's limit of jump operators
    bool hb_fits = !pt;
    for (int k = 0; k < n_sys; ++k) hb_fits = hb_fits && systems[k].n_lind <= HB_LMAX;
    if (!pt && (N > 6 || (env.hilbert && hb_fits))) {
        P->hilbert = true;
        if ((rc = setup_hilbert(P, systems, tsys, grid, rho0, out_ops, tr, s))) return rc;
        *out = guard.release();
        return PQD_OK;
    }
    if (pt && pt->wide) {  // the same inputs, then the bond workspace and the PT units (lind_hilbert_pt.hip)
        P->hilbert = true;
        P->hilbert_pt = true;
        if ((rc = setup_hilbert(P, systems, tsys, grid, rho0, out_ops, tr, s))) return rc;
        if ((rc = setup_hilbert_pt(P, pt, sch, env, s))) return rc;
        *out = guard.release();
        return PQD_OK;
    }
    MtoEvents E = compose_mtos(N, tr);
    if ((rc = upload_inputs(P, systems, tsys, E, rho0, out_ops, tr, s))) return rc;

    // decisions: block order, path, blocks, trunk pre-pass
    const TrajOrder to = order_trajectories(tr, tsys, E);
    const PlanShape sh{N2, P->CHI, ns, n_out, n_sys, pt != nullptr};
    PathChoice pc;
    if ((rc = choose_path(sh, tr, tsys, to, E, env, caps, pc))) return rc;
    P->split = pc.split; P->split_chunk = pc.split_chunk; P->BT = pc.BT; P->quad = pc.quad; P->qpw = pc.qpw;
    P->qcg = pc.qcg; P->msplit = pc.msplit; P->branch = env.branch ? 1 : 0;
    const bool branch_on = env.branch && pt && !pc.split && !pc.msplit, fuse_on = pt && ns > 0 && env.fuse;
    Blocks B = build_blocks(pc.BT, to, tsys, tr, branch_on);
    TrunkChoice tc = choose_trunks(sh, pc, B, to, tsys, tr, branch_on && fuse_on, env.trunk, caps.n_cu);
    if (tc.use_trunk && (rc = apply_trunks(P, tc, B, tsys, pt, env, caps, s))) return rc;
    if ((rc = upload_blocks(P, B, tr, sch, s))) return rc;
    const std::vector<int> blk_fast = block_fast_steps(pc.BT, B, E);
    // rows that stay exactly zero: only the batched sweep's unit list leaves them out. Every other path and the trunk
    // pre-pass contract all rows, and so does this sweep under PQD_LIVE_ROWS=0
    P->live.assign(N2, 1);
    if (pt && env.live_rows != 0 && !pc.split && !pc.msplit && !pc.quad) {
        P->live = live_row_mask(n_sys, systems, C(rho0), E);
        P->live_check = env.live_rows == 2;
    }

    // launch parameters
    if ((rc = setup_free_props(P, grid, env, s))) return rc;
    if ((rc = fill_sweep_params(P, pt, env, blk_fast, block_stage_systems(pc.BT, B, tsys, blk_fast), s))) return rc;
    finalize_trunks(P);
    if (pc.split) {
        HIPCHK(P->Xs.alloc((size_t)n_traj * 4 * N2 * P->CHI));  // split exchange: 2 slots of granules
        HIPCHK(P->cnt.alloc((size_t)n_traj * 64));  // split arrival flags: two 128-B lines per group
        HIPCHK(P->err.alloc(4));
    }
    if (pc.msplit && (rc = build_msplit_tables(P, pc, to.order, tr, tsys, E, env, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    *out = guard.release();
    return PQD_OK;
}

int pqd_plan_create(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, const pqd_pt* pt,
                    const int32_t* sched, const pqd_c128* rho0, int32_t n_out, const pqd_c128* out_ops,
                    const pqd_traj* tr, int64_t out_len, pqd_plan** out) {
    return pqd_plan_create_multi(ctx, 1, sys, nullptr, grid, pt, sched, rho0, n_out, out_ops, tr, out_len, out);
}

int pqd_plan_execute(pqd_plan* P, int32_t rebuild_free) {
    if (!P) return fail(PQD_ERR_ARG, "plan is NULL");
    HIPCHK(hipSetDevice(P->ctx->device));
    hipStream_t s = P->ctx->stream;
    if (!P->ring_ready) {
        for (auto& e : P->ring) HIPCHK(hipEventCreate(&e));
        P->ring_ready = true;
    }
    hipEvent_t* e = P->ring + 3 * P->ev_head;
    HIPCHK(hipEventRecord(e[0], s));
    if (P->hilbert) {  // one kernel, no free propagators to rebuild
        HIPCHK(hipEventRecord(e[1], s));
        if (P->hilbert_pt)
            HIPCHK(launch_hilbert_pt(P->n_traj, P->hq, s));
        else
            HIPCHK(launch_hilbert(P->n_traj, P->hp, s));
        HIPCHK(hipEventRecord(e[2], s));
        P->ev_head = (P->ev_head + 1) % pqd_plan::RING;
        P->ev_count++;
        P->execs++;
        return PQD_OK;
    }
    if (rebuild_free && P->n_steps > 0) {
        HIPCHK(launch_free_prop(P->N2, P->fp, s));
        if (P->sp.fuse) HIPCHK(launch_fuse_steps(P->N2, P->fu, s));
        if (P->msplit) HIPCHK(launch_evcomp(P->N2, P->sp, P->mq, P->n_cev, P->n_steps, s));
    }
    HIPCHK(hipEventRecord(e[1], s));
    HIPCHK(launch_trunks(P, s));
    if (P->nopt)
        HIPCHK(launch_sweep_nopt(P->N2, P->n_traj, P->sp, s));
    else if (P->split)
        HIPCHK(launch_split(P->N2, P->CHI, P->n_traj, P->sp, P->Xs.p, P->cnt.p, P->err.p, s, P->split_chunk));
    else if (P->msplit)
        HIPCHK(launch_msplit(P->N2, P->CHI, P->sp, P->mq, P->msX.p, P->ms_cnt.p, P->err.p, s));
    else
        HIPCHK(launch_main(P, s));
    HIPCHK(hipEventRecord(e[2], s));
    P->ev_head = (P->ev_head + 1) % pqd_plan::RING;
    P->ev_count++;
    P->execs++;
    return PQD_OK;
}

void* pqd_plan_output_device(pqd_plan* P) { return P ? (void*)P->out.p : nullptr; }

// Wait for the plan's last execute and check it. A split launch whose groups could not all be resident (the device
// is shared with other work, so a peer workgroup never arrived) ends with its error word set: the plan then re-runs
// the same step range on the batched kernel, which needs no co-residency, and stays on it. A non-finite output
// value raises PQD_ERR_NUMERIC.
int pqd_plan_synchronize(pqd_plan* P) {
    if (!P) return fail(PQD_ERR_ARG, "plan is NULL");
    HIPCHK(hipSetDevice(P->ctx->device));
    hipStream_t s = P->ctx->stream;
    HIPCHK(hipMemsetAsync(P->flags.p, 0, sizeof(unsigned), s));
    if (P->n_trunk && P->tk_split) {
        unsigned err = 0;
        HIPCHK(hipMemcpyAsync(&err, P->tk_err.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (err) {  // the checkpoints are incomplete: redo the trunks on batched workgroups, then the main sweep
            P->tk_split = false;
            P->split_fallbacks++;
            HIPCHK(hipMemsetAsync(P->tk_err.p, 0, sizeof(unsigned), s));
            HIPCHK(launch_trunks(P, s));
            HIPCHK(launch_main(P, s));
        }
    }
    if (P->split || P->msplit) {
        unsigned err[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(err, P->err.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (err[0] && err[1] && P->msplit && P->mq.l2keep) {
            // a group's workgroups were not all on one XCD (pt_msplit.hip l2keep): again with sc1 exchange stores,
            // which need no placement, and stay there
            P->mq.l2keep = 0;
            P->split_fallbacks++;
            HIPCHK(launch_msplit(P->N2, P->CHI, P->sp, P->mq, P->msX.p, P->ms_cnt.p, P->err.p, s));
            HIPCHK(hipMemcpyAsync(err, P->err.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (err[0] && P->msplit && P->CHI > 128)
            return fail(PQD_ERR_HIP, "multi-trajectory split groups timed out at chi %d (no batched fallback holds that "
                        "bond); the device is shared or the groups could not all be resident", P->CHI);
        if (err[0]) {
            P->split = false;
            P->msplit = false;
            P->split_fallbacks++;
            HIPCHK(hipMemsetAsync(P->err.p, 0, sizeof(unsigned), s));
            HIPCHK(launch_main(P, s));
        }
    }
    unsigned flags = 0;
    HIPCHK(launch_check_finite(P->out.p, P->out_len, P->flags.p, s));
    if (P->live_check && P->n_steps > 0) {
        // PQD_LIVE_ROWS=2: every stored operator is exactly zero from a live column into a dead row (flags bit 1)
        uint64_t mask = 0;
        for (int a = 0; a < P->N2; ++a) mask |= (uint64_t)(P->live[a] != 0) << a;
        const int64_t nM = (int64_t)P->n_sys * 2 * P->n_steps, m2 = (int64_t)P->N2 * P->N2;
        HIPCHK(launch_check_dead_block(P->M.p, nM, P->N2, mask, P->flags.p, s));
        for (int y = 0; P->sp.fuse && y < P->n_sys; ++y)  // F(m) exists for 1 <= m < n_steps (FuseParams): F(0) is never written
            HIPCHK(launch_check_dead_block(P->F.p + ((int64_t)y * P->n_steps + 1) * m2, P->n_steps - 1, P->N2, mask,
                                           P->flags.p, s));
        HIPCHK(launch_check_dead_block(P->Midle.p, P->Midle.p ? P->n_sys : 0, P->N2, mask, P->flags.p, s));
        HIPCHK(launch_check_dead_block(P->Fidle.p, P->Fidle.p ? P->n_sys : 0, P->N2, mask, P->flags.p, s));
    }
    HIPCHK(hipMemcpyAsync(&flags, P->flags.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags & 2u)
        return fail(PQD_ERR_NUMERIC, "PQD_LIVE_ROWS=2: a free propagator couples a live column into a row taken for zero");
    if (flags & 1u) return fail(PQD_ERR_NUMERIC, "non-finite value (NaN/Inf) in the propagated outputs");
    return PQD_OK;
}

int pqd_plan_download(pqd_plan* P, pqd_c128* out, int64_t out_len) {
    if (!P || !out) return fail(PQD_ERR_ARG, "NULL argument");
    if (out_len < P->out_len) return fail(PQD_ERR_ARG, "out_len %lld < plan out_len %lld", (long long)out_len, (long long)P->out_len);
    int rc = pqd_plan_synchronize(P);
    if (rc && rc != PQD_ERR_NUMERIC) return rc;
    if (P->out_len > 0) {
        HIPCHK(hipMemcpyAsync(out, P->out.p, P->out_len * sizeof(double2), hipMemcpyDeviceToHost, P->ctx->stream));
        HIPCHK(hipStreamSynchronize(P->ctx->stream));
    }
    return rc;  // PQD_ERR_NUMERIC still hands the values over (they show where the run went bad)
}

int pqd_plan_table_len(const pqd_plan* P, int64_t* table_len) {
    if (!P || !table_len) return fail(PQD_ERR_ARG, "NULL argument");
    *table_len = P->toff.empty() ? 0 : P->toff.back();
    return PQD_OK;
}

int pqd_plan_download_table(pqd_plan* P, pqd_c128* table, int64_t table_len) {
    if (!P || !table) return fail(PQD_ERR_ARG, "NULL argument");
    const long long need = P->toff.empty() ? 0 : P->toff.back();
    if (table_len < need) return fail(PQD_ERR_ARG, "table_len %lld < %lld", (long long)table_len, need);
    int rc = pqd_plan_synchronize(P);
    if (rc && rc != PQD_ERR_NUMERIC) return rc;
    if (need > 0) {
        hipStream_t s = P->ctx->stream;
        if (!P->toff_d.p) HIPCHK(P->toff_d.upload(P->toff.data(), P->toff.size(), s));
        if (!P->table.p) HIPCHK(P->table.alloc((size_t)need));
        HIPCHK(launch_table(P->out.p, P->woff.p, P->wbeg.p, P->wend.p, P->toff_d.p, P->n_traj, P->n_out, P->t_start,
                            P->dt, P->table.p, s));
        HIPCHK(hipMemcpyAsync(table, P->table.p, (size_t)need * sizeof(double2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return rc;
}

int pqd_plan_trapz(pqd_plan* P, int32_t n_pairs, const int32_t* k_head, const int32_t* k_tail, double dx,
                   pqd_c128* res) {
    if (!P || (n_pairs > 0 && (!k_head || !k_tail || !res))) return fail(PQD_ERR_ARG, "NULL argument");
    if (n_pairs < 0) return fail(PQD_ERR_ARG, "n_pairs %d < 0", n_pairs);
    for (int q = 0; q < n_pairs; ++q)
        if (k_head[q] < 0 || k_head[q] >= P->n_out || k_tail[q] < 0 || k_tail[q] >= P->n_out)
            return fail(PQD_ERR_ARG, "pair %d: output (%d, %d) not in [0, %d)", q, k_head[q], k_tail[q], P->n_out);
    int rc = pqd_plan_synchronize(P);
    if (rc && rc != PQD_ERR_NUMERIC) return rc;
    const size_t n = (size_t)P->n_traj * n_pairs;
    if (n == 0) return rc;
    hipStream_t s = P->ctx->stream;
    DevBuf<int> kd;
    DevBuf<double2> rd;
    std::vector<int> k(2 * (size_t)n_pairs);
    for (int q = 0; q < n_pairs; ++q) { k[q] = k_head[q]; k[n_pairs + q] = k_tail[q]; }
    HIPCHK(kd.upload(k.data(), k.size(), s));
    HIPCHK(rd.alloc(n));
    HIPCHK(launch_trapz(P->out.p, P->woff.p, P->wbeg.p, P->wend.p, P->n_traj, P->n_out, n_pairs, kd.p, kd.p + n_pairs,
                        dx, rd.p, s));
    HIPCHK(hipMemcpyAsync(res, rd.p, n * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return rc;
}

// the flat output length the trajectories' offsets and windows need
static int64_t traj_out_len(const pqd_traj* tr, int32_t n_out) {
    int64_t n = 0;
    for (int t = 0; t < tr->n_traj; ++t)
        n = std::max<int64_t>(n, tr->out_offset[t] + (int64_t)(tr->out_end[t] - tr->out_begin[t] + 1) * n_out);
    return n;
}

int pqd_propagate_trapz(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* tr, int32_t n_pairs,
                        const int32_t* k_head, const int32_t* k_tail, double dx, pqd_c128* res) {
    if (!tr) return fail(PQD_ERR_ARG, "NULL argument");
    const int64_t out_len = traj_out_len(tr, n_out);
    pqd_plan* P = nullptr;
    int rc = pqd_plan_create_multi(ctx, n_sys, systems, traj_sys, grid, pt, sched, rho0, n_out, out_ops, tr,
                                   std::max<int64_t>(1, out_len), &P);
    if (rc) return rc;
    rc = pqd_plan_execute(P, 1);
    if (!rc) rc = pqd_plan_trapz(P, n_pairs, k_head, k_tail, dx, res);
    pqd_plan_destroy(P);
    return rc;
}

int pqd_plan_copy_output(pqd_plan* P, void* dst, int64_t out_len) {
    if (!P || !dst) return fail(PQD_ERR_ARG, "NULL argument");
    if (out_len < P->out_len) return fail(PQD_ERR_ARG, "out_len %lld < plan out_len %lld", (long long)out_len, (long long)P->out_len);
    int rc = pqd_plan_synchronize(P);
    if (rc && rc != PQD_ERR_NUMERIC) return rc;
    if (P->out_len > 0) {
        HIPCHK(hipMemcpyAsync(dst, P->out.p, P->out_len * sizeof(double2), hipMemcpyDefault, P->ctx->stream));
        HIPCHK(hipStreamSynchronize(P->ctx->stream));
    }
    return rc;
}

int pqd_plan_windows(const pqd_plan* P, int32_t* on) {
    if (!P || !on) return fail(PQD_ERR_ARG, "NULL argument");
    *on = P->win.p ? 1 : 0;
    return PQD_OK;
}

int pqd_plan_sweep_lean(const pqd_plan* P, int32_t* on) {
    if (!P || !on) return fail(PQD_ERR_ARG, "NULL argument");
    *on = (P->sp.lean && !P->nopt && !P->split && !P->msplit && !P->quad) ? 1 : 0;
    return PQD_OK;
}

int pqd_plan_sweep_readout(const pqd_plan* P, int32_t* on) {
    if (!P || !on) return fail(PQD_ERR_ARG, "NULL argument");
    *on = (P->sp.lean && P->lean_ro && !P->nopt && !P->split && !P->msplit && !P->quad) ? 1 : 0;
    return PQD_OK;
}

int pqd_plan_sweep_colk(const pqd_plan* P, int32_t* colk) {
    if (!P || !colk) return fail(PQD_ERR_ARG, "NULL argument");
    *colk = (P->sp.lean && P->lean_ro && !P->nopt && !P->split && !P->msplit && !P->quad) ? P->sp.lean_colk : 4;
    return PQD_OK;
}

int pqd_live_col_map(const uint8_t* live, int32_t len, uint8_t* rho, int32_t* kc) {
    if (!live || !rho || !kc) return fail(PQD_ERR_ARG, "NULL argument");
    if (len < 1 || len > 256) return fail(PQD_ERR_ARG, "pqd_live_col_map: len %d outside 1 .. 256", len);
    std::vector<uint8_t> r;
    *kc = live_col_map(std::vector<uint8_t>(live, live + len), r);
    std::copy(r.begin(), r.end(), rho);
    return PQD_OK;
}

int pqd_plan_sweep_stage(const pqd_plan* P, int32_t* n_blocks) {
    if (!P || !n_blocks) return fail(PQD_ERR_ARG, "NULL argument");
    *n_blocks = (P->sp.lean && P->lean_ro && !P->nopt && !P->split && !P->msplit && !P->quad) ? P->n_stage : 0;
    return PQD_OK;
}

static int plan_path(const pqd_plan* P) {
    return P->hilbert_pt ? PQD_PATH_HILBERT_PT : P->hilbert ? PQD_PATH_HILBERT : P->nopt ? PQD_PATH_NOPT : P->split ? PQD_PATH_SPLIT : P->msplit ? PQD_PATH_MSPLIT
         : P->quad ? PQD_PATH_QUAD : PQD_PATH_BATCHED;
}

int pqd_plan_describe(const pqd_plan* P, char* buf, int32_t len) {
    if (!P || !buf || len < 1) return fail(PQD_ERR_ARG, "NULL argument");
    const SweepParams& sp = P->sp;
    const MsplitParams& mq = P->mq;
    const int n = snprintf(
        buf, (size_t)len,
        "n_cu=%d path=%d BT=%d n_blocks=%d traj_steps=%lld split_chunk=%d quad=%d qpw=%d qcg=%d ms_TB=%d ms_groups=%d "
        "ms_xcd=%d ms_l2keep=%d ms_ptm=%d n_cev=%d branch=%d n_trunk=%d tk_split=%d tk_chunk=%d tk_blocks=%d idle=%d "
        "win=%d win_mode=%d fuse=%d pt_mode=%d cmul3=%d trpre=%d colbig=%d umax=%d tk_umax=%d lean=%d split_gran=%d "
        "split_ow=%d split_xcd=%d split_l2=%d spin_limit=%u qprio=%d ablate=%d fp4=%d fpm=%d blocks=%016llx "
        "units=%016llx groups=%016llx",
        P->n_cu, plan_path(P), P->BT, P->n_blocks, (long long)P->traj_steps, P->split_chunk, P->quad ? 1 : 0, P->qpw,
        P->qcg, mq.TB, mq.n_groups, mq.xcd, mq.l2keep, mq.ptm, P->n_cev, P->branch, P->n_trunk, P->tk_split ? 1 : 0,
        P->tk_chunk, P->tk_blocks, P->fp.Midle ? 1 : 0, P->win.p ? 1 : 0, P->win_mode, sp.fuse, sp.pt_mode, sp.cmul3,
        sp.trpre, sp.colbig, sp.umax, P->n_trunk ? P->tk.umax : 0, sp.lean, sp.split_gran, sp.split_ow, sp.split_xcd,
        sp.split_l2, sp.spin_limit, sp.qprio, sp.ablate, P->fp.packed4, P->fp.mfma, (unsigned long long)P->h_blocks,
        (unsigned long long)P->h_units, (unsigned long long)P->h_groups);
    if (n < 0 || n >= len) return fail(PQD_ERR_ARG, "pqd_plan_describe: the line needs %d bytes, len is %d", n + 1, len);
    // a plan that leaves rows out says so (bit a of live: row a is contracted); with every row live the line is as it was
    uint64_t mask = 0;
    bool dead = false;
    for (size_t a = 0; a < P->live.size(); ++a) { mask |= (uint64_t)(P->live[a] != 0) << a; dead = dead || !P->live[a]; }
    if (dead) {
        int32_t colk = 4;
        (void)pqd_plan_sweep_colk(P, &colk);
        const int m = snprintf(buf + n, (size_t)(len - n), colk == 3 ? " live=%llx parts=%d colk=3" : " live=%llx parts=%d",
                               (unsigned long long)mask, sp.lean_parts);
        if (m < 0 || m >= len - n)
            return fail(PQD_ERR_ARG, "pqd_plan_describe: the line needs %d bytes, len is %d", n + m + 1, len);
    }
    return PQD_OK;
}

int pqd_plan_live_rows(const pqd_plan* P, uint8_t* live, int32_t len) {
    if (!P || !live) return fail(PQD_ERR_ARG, "NULL argument");
    const int n = P->hilbert ? P->hp.N * P->hp.N : P->N2;
    if (len != n) return fail(PQD_ERR_ARG, "pqd_plan_live_rows: len %d, the plan has %d rows", len, n);
    for (int a = 0; a < n; ++a) live[a] = (size_t)a < P->live.size() ? P->live[a] : 1;
    return PQD_OK;
}

int pqd_live_rows(int32_t n_sys, const pqd_system* systems, const pqd_c128* rho0, const pqd_traj* tr, uint8_t* live) {
    if (!systems || !rho0 || !live) return fail(PQD_ERR_ARG, "NULL argument");
    if (n_sys < 1) return fail(PQD_ERR_ARG, "n_sys must be >= 1");
    for (int k = 0; k < n_sys; ++k) {
        if (int rc = check_system(&systems[k])) return rc;
        if (systems[k].dim != systems[0].dim)
            return fail(PQD_ERR_ARG, "system %d: dim %d != %d", k, systems[k].dim, systems[0].dim);
    }
    const int N = systems[0].dim;
    pqd_traj none{};
    if (!tr) tr = &none;
    if (tr->n_traj < 0 || tr->n_mto < 0 ||
        (tr->n_mto > 0 && (!tr->mto_traj || !tr->mto_step || !tr->mto_before || !tr->mto_kind || !tr->mto_ops)))
        return fail(PQD_ERR_ARG, "bad MTO arrays");
    for (int q = 0; q < tr->n_mto; ++q) {
        if (tr->mto_traj[q] < 0 || tr->mto_traj[q] >= tr->n_traj) return fail(PQD_ERR_ARG, "MTO %d: bad trajectory", q);
        if (tr->mto_kind[q] < 0 || tr->mto_kind[q] > 2) return fail(PQD_ERR_ARG, "MTO %d: kind %d", q, tr->mto_kind[q]);
    }
    const MtoEvents E = compose_mtos(N, tr);
    const std::vector<uint8_t> m = live_row_mask(n_sys, systems, C(rho0), E);
    std::copy(m.begin(), m.end(), live);
    return PQD_OK;
}

int pqd_plan_info(const pqd_plan* P, int32_t* path, int32_t* bt, int32_t* split_fallbacks, int64_t* traj_steps) {
    if (!P) return fail(PQD_ERR_ARG, "plan is NULL");
    if (traj_steps) *traj_steps = P->traj_steps;
    if (path) *path = plan_path(P);
    if (bt) *bt = P->msplit ? P->mq.TB : P->BT;
    if (split_fallbacks) *split_fallbacks = P->split_fallbacks;
    return PQD_OK;
}

int pqd_plan_timing(pqd_plan* P, double* ms_free, double* ms_sweep, int32_t* n, int32_t reset) {
    if (!P) return fail(PQD_ERR_ARG, "plan is NULL");
    HIPCHK(hipSetDevice(P->ctx->device));
    double f = 0, w = 0;
    const int k = std::min(P->ev_count, pqd_plan::RING);  // the most recent k executes
    for (int i = 0; i < k; ++i) {
        const int slot = ((P->ev_head - 1 - i) % pqd_plan::RING + pqd_plan::RING) % pqd_plan::RING;
        hipEvent_t* e = P->ring + 3 * slot;
        float a = 0, b = 0;
        HIPCHK(hipEventSynchronize(e[2]));
        HIPCHK(hipEventElapsedTime(&a, e[0], e[1]));
        HIPCHK(hipEventElapsedTime(&b, e[1], e[2]));
        f += a; w += b;
    }
    if (P->hilbert) f = 0.0;  // no free-propagator build on this path (the two events are back to back)
    if (ms_free) *ms_free = k ? f / k : 0.0;
    if (ms_sweep) *ms_sweep = k ? w / k : 0.0;
    if (n) *n = k;
    if (reset) P->ev_count = 0;
    return PQD_OK;
}

void pqd_plan_destroy(pqd_plan* P) {
    if (!P) return;
    (void)hipSetDevice(P->ctx->device);
    (void)hipStreamSynchronize(P->ctx->stream);
    delete P;
}

int pqd_propagate(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, const pqd_pt* pt,
                  const int32_t* sched, const pqd_c128* rho0, int32_t n_out, const pqd_c128* out_ops,
                  const pqd_traj* tr, pqd_c128* out, int64_t out_len) {
    return pqd_propagate_multi(ctx, 1, sys, nullptr, grid, pt, sched, rho0, n_out, out_ops, tr, out, out_len);
}

int pqd_propagate_multi(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* tr, pqd_c128* out,
                        int64_t out_len) {
    pqd_plan* P = nullptr;
    int rc = pqd_plan_create_multi(ctx, n_sys, systems, traj_sys, grid, pt, sched, rho0, n_out, out_ops, tr, out_len, &P);
    if (rc) return rc;
    rc = pqd_plan_execute(P, 1);
    if (!rc) rc = pqd_plan_download(P, out, out_len);
    pqd_plan_destroy(P);
    return rc;
}

int pqd_propagate_table(pqd_ctx* ctx, int32_t n_sys, const pqd_system* systems, const int32_t* traj_sys,
                        const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched, const pqd_c128* rho0,
                        int32_t n_out, const pqd_c128* out_ops, const pqd_traj* tr, pqd_c128* table,
                        int64_t table_len) {
    if (!tr) return fail(PQD_ERR_ARG, "NULL argument");
    const int64_t out_len = traj_out_len(tr, n_out);
    pqd_plan* P = nullptr;
    int rc = pqd_plan_create_multi(ctx, n_sys, systems, traj_sys, grid, pt, sched, rho0, n_out, out_ops, tr,
                                   std::max<int64_t>(1, out_len), &P);
    if (rc) return rc;
    rc = pqd_plan_execute(P, 1);
    if (!rc) rc = pqd_plan_download_table(P, table, table_len);
    pqd_plan_destroy(P);
    return rc;
}

// Dynamical maps on the Hilbert-space path: n_maps * N^2 trajectories of one system in one launch of a map instance
// (lind_hilbert.hip, lind_hilbert_pt.hip), trajectory m N^2 + beta from the basis element beta at ta[m], every one
// with the caller's MTOs; then the assembly into dm[m][n][alpha][beta] on the device (pqd_util.hip), the finite check
// and one download. The system tables, the events and (with a PT) the units, G and the tile are those a plan of one
// trajectory with these MTOs gets (setup_hilbert, setup_hilbert_pt); only the bond workspace is sized for all.
int pqd_dynmap_wide(pqd_ctx* ctx, const pqd_system* sys, const pqd_grid* grid, const pqd_pt* pt, const int32_t* sched,
                    int32_t n_maps, const double* ta, int32_t n_mto, const int32_t* mto_step,
                    const int32_t* mto_before, const int32_t* mto_kind, const pqd_c128* mto_ops, pqd_c128* dm,
                    int64_t dm_len) {
    if (!ctx) return fail(PQD_ERR_ARG, "ctx is NULL");
    int rc = check_system(sys, HB_NMAX);
    if (rc) return rc;
    if ((rc = check_grid(grid))) return rc;
    const int N = sys->dim, NN = N * N, ns = grid->n_steps;
    if (sys->n_lind > HB_LMAX)
        return fail(PQD_ERR_UNSUPPORTED, "n_lind %d not in [0, %d] on the Hilbert-space path", sys->n_lind, HB_LMAX);
    if (n_maps < 1) return fail(PQD_ERR_ARG, "n_maps %d must be >= 1", n_maps);
    if (ns < 1) return fail(PQD_ERR_ARG, "n_steps %d must be >= 1", ns);
    const int64_t n_traj = (int64_t)n_maps * NN;
    if (n_traj > INT_MAX)
        return fail(PQD_ERR_UNSUPPORTED, "n_maps %d x dim^2 %d = %lld workgroups exceed the grid limit %d", n_maps, NN,
                    (long long)n_traj, INT_MAX);
    const int64_t need = (int64_t)n_maps * ns * NN * NN;
    if (dm_len != need)
        return fail(PQD_ERR_ARG, "dm_len %lld != n_maps * n_steps * dim^4 = %lld", (long long)dm_len, (long long)need);
    if (!dm) return fail(PQD_ERR_ARG, "dm is NULL");
    if (n_mto < 0 || (n_mto > 0 && (!mto_step || !mto_before || !mto_kind || !mto_ops)))
        return fail(PQD_ERR_ARG, "bad MTO arrays");
    for (int q = 0; q < n_mto; ++q) {
        if (mto_step[q] < 0 || mto_step[q] > ns) return fail(PQD_ERR_ARG, "MTO %d: step %d outside [0, %d]", q, mto_step[q], ns);
        if (mto_kind[q] < 0 || mto_kind[q] > 2) return fail(PQD_ERR_ARG, "MTO %d: kind %d", q, mto_kind[q]);
    }
    std::vector<int32_t> sch(ns, 0);
    if (pt) {
        if (pt->ctx != ctx) return fail(PQD_ERR_ARG, "PT belongs to another context");
        if (!pt->wide) return fail(PQD_ERR_ARG, "the PT handle is not one of pqd_pt_create_wide");
        if (pt->dim != N) return fail(PQD_ERR_ARG, "PT dim %d != system dim %d", pt->dim, N);
        for (int n = 0; n < ns; ++n) {
            const int v = sched ? sched[n] : std::min(n, pt->n_slices - 1);
            if (v < 0 || v >= pt->n_slices) return fail(PQD_ERR_ARG, "sched[%d]=%d out of [0,%d)", n, v, pt->n_slices);
            sch[n] = v;
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const PlanEnv env = read_plan_env();

    // the plan of one template trajectory: system table, norm-bound refusal, events in the order of a step
    pqd_plan P;
    P.ctx = ctx; P.N2 = NN; P.n_traj = 1; P.n_steps = ns; P.n_sys = 1; P.n_out = 0; P.out_len = 0;
    const int32_t w0 = 0, w1 = ns;
    const int64_t o0 = 0;
    const std::vector<int32_t> mtraj(std::max(1, (int)n_mto), 0);
    const pqd_traj tr{1, &w0, &w1, &o0, n_mto, mtraj.data(), mto_step, mto_before, mto_kind, mto_ops};
    const std::vector<int> tsys(1, 0);
    const std::vector<cd> zero(NN, 0.0);  // rho0 of the template: the map instances start from basis elements
    if ((rc = setup_hilbert(&P, sys, tsys, grid, reinterpret_cast<const pqd_c128*>(zero.data()), nullptr, &tr, s))) return rc;
    P.n_traj = (int)n_traj;  // sizes the bond workspace
    if (pt && (rc = setup_hilbert_pt(&P, pt, sch, env, s))) return rc;

    std::vector<double> tav(n_maps);
    for (int m = 0; m < n_maps; ++m) tav[m] = ta ? ta[m] : grid->ta;
    DevBuf<double> ta_d;
    DevBuf<double2> stage, dmd;
    HIPCHK(ta_d.upload(tav.data(), tav.size(), s));
    hipError_t e = stage.alloc((size_t)need);
    if (e == hipSuccess) e = dmd.alloc((size_t)need);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "map buffers of 2 x %lld bytes: %s",
                    (long long)need * (long long)sizeof(double2), hipGetErrorString(e));
    HilbertParams& hp = pt ? P.hq.h : P.hp;
    hp.map_ta = ta_d.p; hp.map_steps = ns; hp.map_nev = n_mto; hp.out = stage.p;

    hipEvent_t ev[2];
    HIPCHK(hipEventCreate(&ev[0]));
    if (hipError_t e1 = hipEventCreate(&ev[1]); e1 != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        return fail(PQD_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e1));
    }
    auto run = [&]() -> int {
        HIPCHK(hipEventRecord(ev[0], s));
        if (pt) HIPCHK(launch_hilbert_pt_map((int)n_traj, P.hq, s));
        else HIPCHK(launch_hilbert_map((int)n_traj, P.hp, s));
        HIPCHK(hipEventRecord(ev[1], s));
        HIPCHK(launch_map_assemble(stage.p, dmd.p, NN, n_maps, ns, s));
        unsigned flags = 0;
        HIPCHK(launch_check_finite(dmd.p, need, P.flags.p, s));
        HIPCHK(hipMemcpyAsync(&flags, P.flags.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        touch_pages(dm, (size_t)need * sizeof(double2));
        HIPCHK(hipMemcpyAsync(dm, dmd.p, (size_t)need * sizeof(double2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->dynmap_ms = ms;
        // the values are handed over all the same (they show where the run went bad)
        if (flags & 1u) return fail(PQD_ERR_NUMERIC, "non-finite value (NaN/Inf) in the dynamical maps");
        return PQD_OK;
    };
    rc = run();
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return rc;
}

int pqd_dynmap_timing(pqd_ctx* ctx, double* ms_kernel) {
    if (!ctx || !ms_kernel) return fail(PQD_ERR_ARG, "NULL argument");
    if (ctx->dynmap_ms < 0) return fail(PQD_ERR_ARG, "no pqd_dynmap_wide call has completed on this context");
    *ms_kernel = ctx->dynmap_ms;
    return PQD_OK;
}

int pqd_fail_msg(int code, const char* msg) { return fail(code, "%s", msg); }

// =================================================================================================
// map-chain sweeps
// =================================================================================================
// dims of the map-chain, propagate_tau and four-time entry points: one trajectory's Liouville vector fits a wave
static bool check_dim_2_6(int dim) { return dim >= 2 && dim <= 6; }
// pqd_calc_onetime_parallel and pqd_propagate_tau: above dim 6 on the sweep by position (mapchain_wide.hip)
static bool check_dim_2_24(int dim) { return dim >= 2 && dim <= HB_NMAX; }

// The PQD_MC_* switches (in that order), read once per call: tests flip them between calls.
struct McEnv { bool blocked, pipe, timing, wide; int L; };
static McEnv read_mc_env() {
    auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    McEnv v;
    v.blocked = num("PQD_MC_BLOCKED", 1) != 0;  // modes 0 and 1 on the blocked sweep (0: map by map)
    v.L = num("PQD_MC_L", INT_MIN);             // its block length (raw value; INT_MIN: unset, sqrt(n_tau))
    v.pipe = num("PQD_MC_PIPE", 1) != 0;        // map-by-map tau sweep with the register pipeline (0: mc_tau_kernel)
    v.timing = getenv("PQD_MC_TIMING") != nullptr;  // host-side phase times of the call on stderr
    v.wide = num("PQD_MC_WIDE", 0) != 0;        // dim 2..6: calc_onetime_parallel and propagate_tau on mapchain_wide.hip
    return v;
}

struct McIn {  // the host arrays of one map-chain call (nA, nB, nT maps in dmA, dmB, dmT)
    const pqd_c128 *dmA, *dmB, *dmT, *dm_s, *rho_init, *opA, *opB, *opC;
    size_t nA, nB, nT;
    const double *time, *time_sparse;
};

// the trunk ends pos[i] = j_i - 1 with the Fortran's own comparisons (propagate_tau.f90:144-151); never decreasing
static std::vector<int> trunk_positions(const MapChainParams& p, const McIn& in) {
    std::vector<int> pos(p.n_t);
    for (int i = 0, j = 1; i < p.n_t; ++i) {
        while (j <= p.n_tfull && in.time[j - 1] < in.time_sparse[i]) ++j;
        pos[i] = j - 1;
    }
    return pos;
}

// mode 0 above dim 6, and below under PQD_MC_WIDE=1: the sweep by position of mapchain_wide.hip
static bool mc_wide(const MapChainParams& p, const McEnv& env) { return p.mode == 0 && (p.dim > 6 || env.wide); }

// Blocked sweep (mapchain.hip) or map by map: sets `blocked`, and for the blocked sweep pos, p.q_s, p.L, p.Q, p.n_blk
static int choose_blocked(MapChainParams& p, const McEnv& env, const McIn& in, bool& blocked, std::vector<int>& pos) {
    blocked = (p.mode == 0 || p.mode == 1) && env.blocked && n2_listed(p.N2) && !mc_wide(p, env);
    if (p.mode == 0 || blocked) pos = trunk_positions(p, in);
    // mode 0 reads dm_tl(:, :, j_i - 1 + n_tau) at its last tau step, on either set of kernels
    if (p.mode == 0 && (size_t)Q_of(pos, p.n_tau) > in.nA)
        return fail(PQD_ERR_ARG, "the sweep would read map %d of %zu (time_sparse beyond time, or n_tau too long "
                    "for dm_tl)", Q_of(pos, p.n_tau), in.nA);
    if (blocked && p.mode == 1) {
        // a trunk that ends past the first period (j > n_tb) never wraps in the tau loop (:270-287: jj resets only at
        // n_tb + 1) and applies dm_s at every tau step: it starts at q_s, where a constant dm_s region begins (map_at)
        int qp = 0, any_s = 0;
        for (int i = 0; i < p.n_t; ++i) {
            if (pos[i] + 1 <= p.n_tb) qp = std::max(qp, pos[i] + p.n_tau);
            else any_s = 1;
        }
        p.q_s = any_s ? qp : INT_MAX;
        for (int i = 0; i < p.n_t; ++i)
            if (pos[i] + 1 > p.n_tb) pos[i] = p.q_s;
        // precondition of that region: with n_map > n_tb a trunk ending at n_tb < j <= n_map walks dm_block(j ..
        // n_map) before dm_s (:270-281), which map_at does not represent; such calls run on the map-by-map kernels
        if (any_s && p.n_map > p.n_tb) blocked = false;
    }
    if (blocked) {
        const int L = env.L != INT_MIN ? env.L : (int)std::lround(std::sqrt((double)std::max(1, p.n_tau)));
        p.L = std::max(8, std::min(256, L));
        p.Q = std::max(Q_of(pos, p.n_tau), 1);
        p.n_blk = (p.Q + p.L - 1) / p.L;
    }
    return PQD_OK;
}

// the caller's result array is typically fresh (f2py-style: np.zeros, pages not yet mapped): its pages are faulted
// in on a few host threads while the maps upload and the kernels run, so the copy back runs at the link rate (a
// 41 MB copy into fresh pages: 1.7 ms, into mapped ones 0.73 ms; scripts/ubench_h2d.py). Without a thread the
// copy back is only slower: nothing is thrown.
struct PageToucher {
    std::thread t;
    PageToucher(void* buf, size_t bytes) { try { t = std::thread(touch_pages, buf, bytes); } catch (...) {} }
    ~PageToucher() { if (t.joinable()) t.join(); }
};

// PQD_MC_TIMING: host-side phase times of the call on stderr (diagnostics)
static void print_mc_timing(const std::chrono::steady_clock::time_point (&t)[5]) {
    auto ms = [&](int a, int b) { return std::chrono::duration<double, std::milli>(t[b] - t[a]).count(); };
    fprintf(stderr, "pqd mapchain: upload+launch %.3f ms, page touch left %.3f ms, kernels left %.3f ms, download %.3f ms\n",
            ms(0, 1), ms(1, 2), ms(2, 3), ms(3, 4));
}

// ---- the sweep by position (mapchain_wide.hip) ----
// What the host loop does at position q = 0 .. Q (Q = max_i p_i + n_tau): first the spawns of the trajectories
// [spawn_lo, spawn_hi) whose trunk ends at q, then (q < Q) one step over the live trajectories [live_lo, live_hi), those
// with p_i <= q < p_i + n_tau, and over the trunk column while q < max_i p_i. pos never decreases, so both are ranges.
struct McwPos { int live_lo, live_hi, trunk, spawn_lo, spawn_hi; };
static std::vector<McwPos> mc_wide_schedule(const std::vector<int>& pos, int n_tau) {
    const int n_t = (int)pos.size(), Q = Q_of(pos, n_tau), p_max = pos.empty() ? 0 : pos.back();
    std::vector<McwPos> sch((size_t)Q + 1);
    int lo = 0, hi = 0;
    for (int q = 0; q <= Q; ++q) {
        const int started = hi;
        while (hi < n_t && pos[hi] <= q) ++hi;
        while (lo < hi && q - pos[lo] >= n_tau) ++lo;
        sch[q] = {lo, hi, q < p_max ? 1 : 0, started, hi};
    }
    return sch;
}

// The periodic sweep (calc_onetime_parallel_block, propagate_tau.f90:189-295) by position. Two map cursors: the straight
// one, dm_block(:, :, q + 1) while q < n_map and dm_s after, is followed by the trunk and by the trajectories whose
// trunk ends at p_i >= n_tb (their j never meets the wrap test j == n_tb + 1, :285); the ring one, the same rule at
// q mod n_tb, by the trajectories with p_i < n_tb. pos never decreases, so the ring trajectories are [0, n_ring) and
// the live range of mc_wide_schedule splits at n_ring into one range per cursor. Map index n_map stands for dm_s.
struct McwBlockPos { int ring_lo, ring_hi, ring_map, str_lo, str_hi, trunk, str_map, spawn_lo, spawn_hi; };
static std::vector<McwBlockPos> mc_wide_block_schedule(const std::vector<int>& pos, int n_tb, int n_tau, int n_map) {
    const std::vector<McwPos> one = mc_wide_schedule(pos, n_tau);
    const int n_ring = (int)(std::lower_bound(pos.begin(), pos.end(), n_tb) - pos.begin());
    std::vector<McwBlockPos> sch(one.size());
    for (size_t q = 0; q < one.size(); ++q) {
        const McwPos& r = one[q];
        sch[q] = {std::min(r.live_lo, n_ring), std::min(r.live_hi, n_ring), std::min((int)(q % (size_t)n_tb), n_map),
                  std::max(r.live_lo, n_ring), std::max(r.live_hi, n_ring), r.trunk,
                  (int)std::min(q, (size_t)n_map), r.spawn_lo, r.spawn_hi};
    }
    return sch;
}

// the two events of a timed stretch of the stream
struct EventPair {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~EventPair() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create() {
        hipError_t e = hipEventCreate(&ev[0]);
        return e != hipSuccess ? e : hipEventCreate(&ev[1]);
    }
};

// the context's arena with room for `bytes`; PQD_ERR_NOMEM naming them when it cannot grow
static int mc_arena_reserve(pqd_ctx* ctx, size_t bytes, hipStream_t s) {
    if (ctx->mc_arena.n >= bytes + 256) return PQD_OK;
    HIPCHK(hipStreamSynchronize(s));
    const size_t want = bytes + std::min(bytes / 4, (size_t)64 << 20) + 256;
    const hipError_t e = ctx->mc_arena.alloc(want);
    if (e == hipSuccess) return PQD_OK;
    ctx->mc_arena.release();
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "map-chain arena of %zu bytes: %s", want,
                hipGetErrorString(e));
}

// The driver of both sweeps by position: uploads the n_up maps of `maps` that the schedule reads and then `last` (dm_s;
// NULL in mode 0) as map n_up, then per position at most one spawn launch and one step launch. A map index of the
// schedule below n_up is that map, any other is `last`. The device footprint is n_up + 1 maps, two state buffers and
// the result: it does not grow with the number of positions.
static int mapchain_wide_run(pqd_ctx* ctx, const MapChainParams& p, const McIn& in, const std::vector<int>& pos,
                             const std::vector<McwBlockPos>& sch, const pqd_c128* maps, size_t n_up,
                             const pqd_c128* last, const McEnv& env, pqd_c128* result) {
    hipStream_t s = ctx->stream;
    const size_t n = p.N2, m2 = n * n, n_t = p.n_t, nres = n_t * ((size_t)p.n_tau + 1);
    const int Q = (int)sch.size() - 1;
    const size_t n_dev = n_up + (last ? 1 : 0);
    const size_t ncol = (n_t + 1 + 15) / 16 * 16;  // the trajectories, the trunk state in column n_t, padding
    // w[r] of Tr(opB R) over the column-major view of R: r = b + a dim gets opB(a, b) (mapchain.hip trace_weight)
    std::vector<cd> w(n);
    for (size_t r = 0; r < n; ++r) w[r] = C(in.opB)[r / p.dim + (r % p.dim) * (size_t)p.dim];
    struct { double2 *E, *U, *w, *opA, *opB, *opC, *X[2], *res; int* pos; } d{};
    auto carve = [&](Carve& c) {
        d.E = c.take<double2>(n_dev * m2); d.U = c.take<double2>(n_dev * n); d.w = c.take<double2>(n);
        d.opA = c.take<double2>(n); d.opB = c.take<double2>(n); d.opC = c.take<double2>(n);
        d.X[0] = c.take<double2>(ncol * n); d.X[1] = c.take<double2>(ncol * n);
        d.res = c.take<double2>(nres); d.pos = c.take<int>(n_t);
    };
    Carve sz, cv;
    carve(sz);
    if (int rc = mc_arena_reserve(ctx, sz.off, s)) return rc;
    cv.base = ctx->mc_arena.p;
    carve(cv);
    EventPair ev;
    HIPCHK(ev.create());
    auto now = [] { return std::chrono::steady_clock::now(); };
    const decltype(now()) t0 = now();
    PageToucher toucher((void*)result, nres * sizeof(double2));
    const size_t vb = n * sizeof(double2);
    const struct { void* dst; const void* src; size_t bytes; } ups[] = {
        {d.E, maps, n_up * m2 * sizeof(double2)}, {d.E + n_up * m2, last, last ? m2 * sizeof(double2) : 0},
        {d.w, w.data(), vb}, {d.opA, in.opA, vb}, {d.opB, in.opB, vb},
        {d.opC, in.opC, vb}, {d.X[0] + n_t * n, in.rho_init, vb}, {d.pos, pos.data(), n_t * sizeof(int)}};
    for (const auto& u : ups)
        if (u.bytes) HIPCHK(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, s));
    int launches = 0;
    HIPCHK(hipEventRecord(ev.ev[0], s));
    if (p.n_tau > 0 && n_dev > 0) {
        HIPCHK(launch_mcw_weights(d.E, d.w, d.U, (int)n, (int)n_dev, s));
        ++launches;
    }
    for (int q = 0; q <= Q; ++q) {
        const McwBlockPos& r = sch[q];
        double2 *Xr = d.X[q & 1], *Xw = d.X[(q + 1) & 1];
        if (r.spawn_hi > r.spawn_lo) {
            HIPCHK(launch_mcw_spawn({d.opA, d.opB, d.opC, Xr, d.res, p.dim, (int)n, p.n_t, r.spawn_lo},
                                    r.spawn_hi - r.spawn_lo, s));
            ++launches;
        }
        auto family = [&](int lo, int hi, int trunk, int map) {
            const size_t k = std::min((size_t)map, n_up);
            McwStep st{};
            st.E = d.E + k * m2; st.u = p.n_tau > 0 ? d.U + k * n : nullptr;
            st.X = Xr; st.Y = Xw; st.pos = d.pos; st.result = d.res;
            st.n = (int)n; st.q = q; st.n_tau = p.n_tau; st.n_t = p.n_t;
            st.c0 = lo; st.c1 = hi; st.trunk = trunk;
            return st;
        };
        const bool ring = r.ring_hi > r.ring_lo, str = r.str_hi > r.str_lo || r.trunk;
        if (q == Q || !(ring || str)) continue;
        // one product when only one cursor has a live column or both name the same map (mcw_live leaves out the
        // columns of the merged range that are not in flight), else the two families in one launch
        if (ring && str && r.ring_map != r.str_map)
            HIPCHK(launch_mcw_step2(family(r.ring_lo, r.ring_hi, 0, r.ring_map),
                                    family(r.str_lo, r.str_hi, r.trunk, r.str_map), s));
        else
            HIPCHK(launch_mcw_step(family(ring ? r.ring_lo : r.str_lo, str ? r.str_hi : r.ring_hi, r.trunk,
                                          str ? r.str_map : r.ring_map), s));
        ++launches;
    }
    HIPCHK(hipEventRecord(ev.ev[1], s));
    const auto t1 = now();
    if (toucher.t.joinable()) toucher.t.join();
    const auto t2 = now();
    if (env.timing) HIPCHK(hipStreamSynchronize(s));
    const auto t3 = now();
    HIPCHK(hipMemcpyAsync(result, d.res, nres * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (env.timing) print_mc_timing({t0, t1, t2, t3, now()});
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
    ctx->mcw_ms = ms;
    ctx->mcw_launches = launches;
    return PQD_OK;
}

// mode 0 (checked by mapchain_run, pos from choose_blocked) on that driver: one cursor, map q at position q, every
// trajectory and the trunk in the straight family; the Q maps the sweep reads are uploaded
static int mapchain_wide_mode0(pqd_ctx* ctx, const MapChainParams& p, const McIn& in, const std::vector<int>& pos,
                               const McEnv& env, pqd_c128* result) {
    const std::vector<McwPos> one = mc_wide_schedule(pos, p.n_tau);
    std::vector<McwBlockPos> sch(one.size());
    for (size_t q = 0; q < one.size(); ++q)
        sch[q] = {0, 0, 0, one[q].live_lo, one[q].live_hi, one[q].trunk, (int)q, one[q].spawn_lo, one[q].spawn_hi};
    return mapchain_wide_run(ctx, p, in, pos, sch, in.dmA, (size_t)Q_of(pos, p.n_tau), nullptr, env, result);
}

static int mapchain_run(pqd_ctx* ctx, MapChainParams& p, const McIn& in, pqd_c128* result) {
    if (!ctx || !in.rho_init || !in.opA || !in.opB || !in.opC || !in.time || !in.time_sparse || !result || !in.dmA)
        return fail(PQD_ERR_ARG, "NULL argument");
    if (p.mode == 0 ? !check_dim_2_24(p.dim) : !check_dim_2_6(p.dim))
        return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [2, %d]", p.dim, p.mode == 0 ? HB_NMAX : 6);
    if (p.n_t < 1 || p.n_tfull < 1 || p.n_tau < 0) return fail(PQD_ERR_ARG, "bad sizes");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    p.N2 = p.dim * p.dim;
    const size_t nres = (size_t)p.n_t * (p.n_tau + 1);
    const McEnv env = read_mc_env();
    bool blocked;
    std::vector<int> pos;
    if (int rc = choose_blocked(p, env, in, blocked, pos)) return rc;
    if (mc_wide(p, env)) return mapchain_wide_mode0(ctx, p, in, pos, env, result);
    // every device buffer of the call carved from the context's arena
    const size_t N2 = p.N2, m2 = N2 * N2;
    auto carve = [&](Carve& c) {
        p.dmA = c.take<double2>(in.nA * m2);
        p.dmB = in.dmB ? c.take<double2>(in.nB * m2) : nullptr;
        p.dmT = in.dmT ? c.take<double2>(in.nT * m2) : nullptr;
        p.dm_s = in.dm_s ? c.take<double2>(m2) : nullptr;
        p.rho_init = c.take<double2>(N2); p.opA = c.take<double2>(N2); p.opB = c.take<double2>(N2); p.opC = c.take<double2>(N2);
        p.time = c.take<double>(p.n_tfull); p.time_sparse = c.take<double>(p.n_t);
        p.rho_buf = c.take<double2>(p.n_t * N2); p.j_arr = c.take<int>(p.n_t); p.result = c.take<double2>(nres);
        if (!blocked) return;
        p.pos = c.take<int>(p.n_t); p.U = c.take<double2>(p.Q * N2); p.Rend = c.take<double2>(p.n_blk * m2);
        p.P = c.take<double2>((p.n_blk + 1) * N2); p.X = c.take<double2>((size_t)p.n_blk * p.n_t * N2);
    };
    Carve sz, cv;
    carve(sz);
    if (ctx->mc_arena.n < sz.off + 256) {
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(ctx->mc_arena.alloc(sz.off + sz.off / 4 + 256));
    }
    cv.base = ctx->mc_arena.p;
    carve(cv);
    auto now = [] { return std::chrono::steady_clock::now(); };
    const decltype(now()) t0 = now();
    PageToucher toucher((void*)result, nres * sizeof(double2));
    const size_t vb = N2 * sizeof(double2), mb = vb * N2;  // the inputs; pos (the blocked sweep's trunk ends) last
    const struct { const void *dst, *src; size_t bytes; } ups[] = {
        {p.dmA, in.dmA, in.nA * mb}, {p.dmB, in.dmB, in.nB * mb}, {p.dmT, in.dmT, in.nT * mb}, {p.dm_s, in.dm_s, mb},
        {p.rho_init, in.rho_init, vb}, {p.opA, in.opA, vb}, {p.opB, in.opB, vb}, {p.opC, in.opC, vb},
        {p.time, in.time, p.n_tfull * sizeof(double)}, {p.time_sparse, in.time_sparse, p.n_t * sizeof(double)},
        {p.pos, blocked ? pos.data() : nullptr, p.n_t * sizeof(int)}};
    for (const auto& u : ups)
        if (u.src && u.bytes) HIPCHK(hipMemcpyAsync(const_cast<void*>(u.dst), u.src, u.bytes, hipMemcpyHostToDevice, s));
    if (blocked) {
        // every result element is written by the blocked kernels; n_chain from the last, largest trunk end (mode 0)
        HIPCHK(launch_mapchain_blocked(p, p.mode == 0 ? pos.back() / p.L : 0, s));
    } else {
        HIPCHK(hipMemsetAsync(p.result, 0, nres * sizeof(double2), s));
        HIPCHK(launch_mapchain(p, env.pipe, s));
    }
    const auto t1 = now();
    if (toucher.t.joinable()) toucher.t.join();
    const auto t2 = now();
    if (env.timing) HIPCHK(hipStreamSynchronize(s));
    const auto t3 = now();
    HIPCHK(hipMemcpyAsync(result, p.result, nres * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (env.timing) print_mc_timing({t0, t1, t2, t3, now()});
    return PQD_OK;
}

int pqd_calc_onetime_parallel(pqd_ctx* ctx, const pqd_c128* dm_tl, const pqd_c128* rho_init, int32_t n_tau,
                              int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                              const pqd_c128* opB, const pqd_c128* opC, const double* time,
                              const double* time_sparse, pqd_c128* result) {
    MapChainParams p{};
    p.mode = 0; p.dim = dim; p.n_t = n_t; p.n_tfull = n_tfull; p.n_tau = n_tau;
    // the tau loop reads maps up to index j_max - 1 + n_tau <= n_tfull - 1 (Fortran bounds)
    return mapchain_run(ctx, p, {dm_tl, nullptr, nullptr, nullptr, rho_init, opA, opB, opC,
                                 (size_t)std::max(1, n_tfull - 1), 0, 0, time, time_sparse}, result);
}

int pqd_calc_onetime_parallel_block(pqd_ctx* ctx, const pqd_c128* dm_block, const pqd_c128* dm_s,
                                    const pqd_c128* rho_init, int32_t n_tb, int32_t nx_tau, int32_t n_map,
                                    int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                                    const pqd_c128* opB, const pqd_c128* opC, const double* time,
                                    const double* time_sparse, pqd_c128* result) {
    if (!dm_s) return fail(PQD_ERR_ARG, "dm_s is NULL");
    if (n_map < 1 || n_tb < 1 || nx_tau < 0) return fail(PQD_ERR_ARG, "bad block sizes");
    MapChainParams p{};
    p.mode = 1; p.dim = dim; p.n_t = n_t; p.n_tfull = n_tfull; p.n_tau = n_tb * nx_tau;
    p.n_map = n_map; p.n_tb = n_tb; p.nx_tau = nx_tau;
    return mapchain_run(ctx, p, {dm_block, nullptr, nullptr, dm_s, rho_init, opA, opB, opC, (size_t)n_map, 0, 0, time,
                                 time_sparse}, result);
}

int pqd_calc_twotime_phonon_block(pqd_ctx* ctx, const pqd_c128* dm_taucs2, const pqd_c128* dm_sep1,
                                  const pqd_c128* dm_sep2, const pqd_c128* dm_s, const pqd_c128* rho_init,
                                  int32_t n_tb, int32_t nx_tau, int32_t n_map, int32_t n_t, int32_t n_tfull,
                                  int32_t n_tauc, int32_t dim, const pqd_c128* opA, const pqd_c128* opB,
                                  const pqd_c128* opC, const double* time, const double* time_sparse,
                                  pqd_c128* result) {
    if (n_map < 1 || n_tb < 1 || nx_tau < 0 || n_tauc < 0) return fail(PQD_ERR_ARG, "bad block sizes");
    // n_tauc = 0: the loop over the per-trajectory maps is empty (:466), dm_taucs2 has no element and is not read
    if ((n_tauc > 0 && !dm_taucs2) || !dm_sep2 || !dm_s) return fail(PQD_ERR_ARG, "NULL map argument");
    if (n_tauc > n_t) return fail(PQD_ERR_ARG, "n_tauc %d > n_t %d (reads past rho_buffer in the reference)", n_tauc, n_t);
    MapChainParams p{};
    p.mode = 2; p.dim = dim; p.n_t = n_t; p.n_tfull = n_tfull; p.n_tau = n_tb * nx_tau;
    p.n_map = n_map; p.n_tb = n_tb; p.nx_tau = nx_tau; p.n_tauc = n_tauc;
    return mapchain_run(ctx, p, {dm_sep1, dm_sep2, n_tauc > 0 ? dm_taucs2 : nullptr, dm_s, rho_init, opA, opB, opC,
                                 (size_t)n_map, (size_t)n_map, (size_t)n_tauc * n_map, time, time_sparse}, result);
}

// pqd_propagate_tau above dim 6 (and below under PQD_MC_WIDE=1): the step kernel of the sweep by position with one
// column, X = out[:, k] and Y = out[:, k + 1] in place; only the n_tau maps the sweep reads are uploaded
static int propagate_tau_wide(pqd_ctx* ctx, const pqd_c128* dm_tl, const pqd_c128* rho_init, int n_tau, int N2,
                              int j_start, pqd_c128* rho_out) {
    hipStream_t s = ctx->stream;
    const size_t n = N2, m2 = n * n, nout = n * ((size_t)n_tau + 1);
    DevBuf<double2> A, o;
    hipError_t e = A.upload(reinterpret_cast<const double2*>(dm_tl) + (size_t)j_start * m2, (size_t)n_tau * m2, s);
    if (e == hipSuccess) e = o.alloc(nout);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "maps and states of %zu bytes: %s",
                    ((size_t)n_tau * m2 + nout) * sizeof(double2), hipGetErrorString(e));
    HIPCHK(hipMemcpyAsync(o.p, rho_init, n * sizeof(double2), hipMemcpyHostToDevice, s));
    EventPair ev;
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev.ev[0], s));
    for (int k = 0; k < n_tau; ++k) {
        McwStep st{};
        st.E = A.p + (size_t)k * m2; st.X = o.p + (size_t)k * n; st.Y = o.p + (size_t)(k + 1) * n;
        st.n = N2; st.q = k; st.n_tau = n_tau; st.c0 = 0; st.c1 = 1;
        HIPCHK(launch_mcw_step(st, s));
    }
    HIPCHK(hipEventRecord(ev.ev[1], s));
    HIPCHK(hipMemcpyAsync(rho_out, o.p, nout * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
    ctx->mcw_ms = ms;
    ctx->mcw_launches = n_tau;
    return PQD_OK;
}

int pqd_propagate_tau(pqd_ctx* ctx, const pqd_c128* dm_tl, int32_t n_maps, const pqd_c128* rho_init,
                      int32_t n_tau, int32_t dim, int32_t j_start, pqd_c128* rho_out) {
    if (!ctx || !dm_tl || !rho_init || !rho_out) return fail(PQD_ERR_ARG, "NULL argument");
    if (!check_dim_2_24(dim)) return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [2, %d]", dim, HB_NMAX);
    if (n_tau < 0 || j_start < 0 || j_start + n_tau > n_maps)
        return fail(PQD_ERR_ARG, "maps j_start+1..j_start+n_tau = %d..%d outside 1..%d", j_start + 1, j_start + n_tau, n_maps);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N2 = dim * dim;
    if (dim > 6 || read_mc_env().wide) return propagate_tau_wide(ctx, dm_tl, rho_init, n_tau, N2, j_start, rho_out);
    DevBuf<double2> A, r0, o;
    HIPCHK(A.upload(reinterpret_cast<const double2*>(dm_tl), (size_t)n_maps * N2 * N2, s));
    HIPCHK(r0.upload(reinterpret_cast<const double2*>(rho_init), N2, s));
    HIPCHK(o.alloc((size_t)N2 * (n_tau + 1)));
    HIPCHK(launch_propagate_tau(N2, A.p, r0.p, n_tau, j_start, o.p, s));
    HIPCHK(hipMemcpyAsync(rho_out, o.p, (size_t)N2 * (n_tau + 1) * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PQD_OK;
}

int pqd_mc_wide_schedule(const double* time, int32_t n_tfull, const double* time_sparse, int32_t n_t, int32_t n_tau,
                         int32_t* pos, int32_t* n_rows, int32_t* sched, int32_t sched_rows) {
    if (!time || !time_sparse || !n_rows) return fail(PQD_ERR_ARG, "NULL argument");
    if (n_t < 1 || n_tfull < 1 || n_tau < 0) return fail(PQD_ERR_ARG, "bad sizes");
    MapChainParams p{};
    p.n_t = n_t; p.n_tfull = n_tfull; p.n_tau = n_tau;
    McIn in{};
    in.time = time; in.time_sparse = time_sparse;
    const std::vector<int> ps = trunk_positions(p, in);
    if ((long long)ps.back() + n_tau >= INT_MAX) return fail(PQD_ERR_ARG, "positions do not fit an int");
    if (pos) std::copy(ps.begin(), ps.end(), pos);
    const std::vector<McwPos> sch = mc_wide_schedule(ps, n_tau);
    *n_rows = (int32_t)sch.size();
    if (!sched) return PQD_OK;
    if ((size_t)std::max(sched_rows, 0) < sch.size())
        return fail(PQD_ERR_ARG, "sched holds %d rows, the schedule has %zu", sched_rows, sch.size());
    for (size_t q = 0; q < sch.size(); ++q) {
        const int32_t row[5] = {sch[q].live_lo, sch[q].live_hi, sch[q].trunk, sch[q].spawn_lo, sch[q].spawn_hi};
        std::copy(row, row + 5, sched + 5 * q);
    }
    return PQD_OK;
}

int pqd_mc_wide_timing(pqd_ctx* ctx, double* ms_kernel, int32_t* launches) {
    if (!ctx || !ms_kernel || !launches) return fail(PQD_ERR_ARG, "NULL argument");
    if (ctx->mcw_ms < 0) return fail(PQD_ERR_ARG, "no wide map-chain call has completed on this context");
    *ms_kernel = ctx->mcw_ms;
    *launches = ctx->mcw_launches;
    return PQD_OK;
}

// the checks of the block arguments that pqd_calc_onetime_parallel_block_wide and pqd_mc_wide_block_schedule share,
// then the trunk ends and the schedule
static int block_schedule(const double* time, int n_tfull, const double* time_sparse, int n_t, int n_tb, int nx_tau,
                          int n_map, std::vector<int>& pos, std::vector<McwBlockPos>& sch) {
    if (n_map < 1 || n_tb < 1 || nx_tau < 0) return fail(PQD_ERR_ARG, "bad block sizes");
    if (n_t < 1 || n_tfull < 1) return fail(PQD_ERR_ARG, "bad sizes");
    MapChainParams p{};
    p.n_t = n_t; p.n_tfull = n_tfull;
    McIn in{};
    in.time = time; in.time_sparse = time_sparse;
    pos = trunk_positions(p, in);
    if ((long long)pos.back() + (long long)n_tb * nx_tau >= INT_MAX)
        return fail(PQD_ERR_ARG, "positions do not fit an int");
    sch = mc_wide_block_schedule(pos, n_tb, n_tb * nx_tau, n_map);
    return PQD_OK;
}

int pqd_mc_wide_block_schedule(const double* time, int32_t n_tfull, const double* time_sparse, int32_t n_t,
                               int32_t n_tb, int32_t nx_tau, int32_t n_map, int32_t* pos, int32_t* n_rows,
                               int32_t* sched, int32_t sched_rows) {
    if (!time || !time_sparse || !n_rows) return fail(PQD_ERR_ARG, "NULL argument");
    std::vector<int> ps;
    std::vector<McwBlockPos> sch;
    if (int rc = block_schedule(time, n_tfull, time_sparse, n_t, n_tb, nx_tau, n_map, ps, sch)) return rc;
    if (pos) std::copy(ps.begin(), ps.end(), pos);
    *n_rows = (int32_t)sch.size();
    if (!sched) return PQD_OK;
    if ((size_t)std::max(sched_rows, 0) < sch.size())
        return fail(PQD_ERR_ARG, "sched holds %d rows, the schedule has %zu", sched_rows, sch.size());
    for (size_t q = 0; q < sch.size(); ++q) {
        const McwBlockPos& r = sch[q];
        const int32_t row[9] = {r.ring_lo, r.ring_hi, r.ring_map, r.str_lo, r.str_hi, r.trunk, r.str_map, r.spawn_lo,
                                r.spawn_hi};
        std::copy(row, row + 9, sched + 9 * q);
    }
    return PQD_OK;
}

int pqd_calc_onetime_parallel_block_wide(pqd_ctx* ctx, const pqd_c128* dm_block, const pqd_c128* dm_s,
                                         const pqd_c128* rho_init, int32_t n_tb, int32_t nx_tau, int32_t n_map,
                                         int32_t n_t, int32_t n_tfull, int32_t dim, const pqd_c128* opA,
                                         const pqd_c128* opB, const pqd_c128* opC, const double* time,
                                         const double* time_sparse, pqd_c128* result) {
    if (!dm_s) return fail(PQD_ERR_ARG, "dm_s is NULL");
    if (n_map < 1 || n_tb < 1 || nx_tau < 0) return fail(PQD_ERR_ARG, "bad block sizes");
    if (!ctx || !rho_init || !opA || !opB || !opC || !time || !time_sparse || !result || !dm_block)
        return fail(PQD_ERR_ARG, "NULL argument");
    if (!check_dim_2_24(dim)) return fail(PQD_ERR_UNSUPPORTED, "dim %d not in [2, %d]", dim, HB_NMAX);
    std::vector<int> pos;
    std::vector<McwBlockPos> sch;
    if (int rc = block_schedule(time, n_tfull, time_sparse, n_t, n_tb, nx_tau, n_map, pos, sch)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    MapChainParams p{};
    p.mode = 1; p.dim = dim; p.N2 = dim * dim; p.n_t = n_t; p.n_tfull = n_tfull; p.n_tau = n_tb * nx_tau;
    p.n_map = n_map; p.n_tb = n_tb; p.nx_tau = nx_tau;
    // the block maps the steps read: a prefix of dm_block, up to the highest index a step with a live column names
    int n_up = 0;
    for (size_t q = 0; q + 1 < sch.size(); ++q) {
        const McwBlockPos& r = sch[q];
        if (r.ring_hi > r.ring_lo && r.ring_map < n_map) n_up = std::max(n_up, r.ring_map + 1);
        if ((r.str_hi > r.str_lo || r.trunk) && r.str_map < n_map) n_up = std::max(n_up, r.str_map + 1);
    }
    const McIn in{dm_block, nullptr, nullptr, dm_s, rho_init, opA, opB, opC, (size_t)n_map, 0, 0, time, time_sparse};
    return mapchain_wide_run(ctx, p, in, pos, sch, dm_block, (size_t)n_up, dm_s, read_mc_env(), result);
}

int pqd_map_tail(pqd_ctx* ctx, const pqd_c128* M, int32_t N2, const pqd_c128* X, int32_t n_x, const pqd_c128* w,
                 int32_t n_steps, pqd_c128* out) {
    if (!ctx || !M || !X || !w || !out) return fail(PQD_ERR_ARG, "NULL argument");
    if (!n2_listed(N2)) return fail(PQD_ERR_UNSUPPORTED, "N2 %d", N2);
    if (n_x < 0 || n_steps < 0) return fail(PQD_ERR_ARG, "n_x %d n_steps %d", n_x, n_steps);
    if (n_x == 0 || n_steps == 0) return PQD_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<double2> dM, dX, dw, o;
    HIPCHK(dM.upload(reinterpret_cast<const double2*>(M), (size_t)N2 * N2, s));
    HIPCHK(dX.upload(reinterpret_cast<const double2*>(X), (size_t)n_x * N2, s));
    HIPCHK(dw.upload(reinterpret_cast<const double2*>(w), N2, s));
    HIPCHK(o.alloc((size_t)n_x * n_steps));
    HIPCHK(launch_map_tail(N2, dM.p, dX.p, n_x, dw.p, n_steps, o.p, s));
    HIPCHK(hipMemcpyAsync(out, o.p, (size_t)n_x * n_steps * sizeof(double2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PQD_OK;
}

// propagate_tb's step counts (timebin_tl.f90:59-62, as prop_tb in mapchain.hip takes them): the steps left to the binary
// powers after the explicit maps, or -1 for a segment that indexes the explicit maps below 1 or whose counts do not
// fit an int
static long long tb_remainder(double ts, double te, double dt, int n_dm) {
    const double qs = (double)llround(ts * 1000000.0) / 1000000.0 / dt;
    const double qe = (double)llround(te * 1000000.0) / 1000000.0 / dt;
    if (!(std::fabs(qs) < 1e9) || !(std::fabs(qe) < 1e9)) return -1;
    const int n_start = (int)qs, n_stop = (int)qe;
    int n_steps = n_stop - n_start;
    const int steps_dm = std::min(n_dm - n_start, n_steps);
    if (steps_dm > 0) {
        if (n_start < 0) return -1;
        n_steps -= steps_dm;
    }
    return std::max(n_steps, 0);
}

static int four_time_common(pqd_ctx* ctx, FourTimeParams& p, const pqd_c128* dm_1, const pqd_c128* dm_2,
                            const pqd_c128* rho_init, const double* t1, const pqd_c128* precalc, const pqd_c128* ops,
                            int n_ops, pqd_c128* result, bool dyn, int row_lo = 0, int row_hi = INT_MAX) {
    if (!ctx || !dm_1 || !dm_2 || !rho_init || !t1 || !precalc || !result || (!dyn && !ops))
        return fail(PQD_ERR_ARG, "NULL argument");
    if (!check_dim_2_6(p.dim)) return fail(PQD_ERR_UNSUPPORTED, "dim %d", p.dim);
    if (p.n_t < 1 || p.n_map < 1 || p.n_precalc < 1 || !(p.dt > 0)) return fail(PQD_ERR_ARG, "bad sizes");
    {
        // every segment the call propagates over: fast_propagate (timebin_tl.f90:36-46) reads dm_tl_precalc(:, :, bit + 1)
        // for every set bit of the remainder, past the array when the remainder reaches 2^n_precalc; the kernels
        // stop at n_precalc, so such a call is refused rather than answered with steps dropped
        const long long lim = p.n_precalc < 31 ? (1LL << p.n_precalc) : (1LL << 31);
        auto bad = [&](double ts, double te) {
            const long long r = tb_remainder(ts, te, p.dt, p.n_map);
            if (r >= 0 && r < lim) return 0;
            if (r < 0)
                return fail(PQD_ERR_ARG, "segment (%g, %g) starts before the first map or is too long for dt %g", ts, te,
                            p.dt);
            return fail(PQD_ERR_ARG, "segment (%g, %g) leaves %lld steps after the %d explicit maps: needs precalc "
                        "map %d of %d", ts, te, r, p.n_map, 64 - __builtin_clzll((unsigned long long)r), p.n_precalc);
        };
        int rc = 0;
        if (dyn) {
            for (int i = 0; i + 1 < p.n_t && !rc; ++i) rc = bad(t1[i], t1[i + 1]);
        } else {
            const bool to_tb = p.variant != 0 || !p.early_only;  // (t2, tb) is not reached under early_only
            for (int i = 0; i < p.n_t && !rc; ++i) {
                rc = bad(0.0, t1[i]);
                if (!rc && to_tb) rc = bad(t1[i], p.tb);
                for (int j = i; j < p.n_t && !rc; ++j) rc = bad(t1[i], t1[j]);
            }
        }
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int N2 = p.dim * p.dim;
    p.N2 = N2;
    const size_t m2 = (size_t)N2 * N2;
    DevBuf<double2> d1, d2, pc, r0, op, res;
    DevBuf<double> tt;
    DevBuf<int2> pr;
    HIPCHK(d1.upload(reinterpret_cast<const double2*>(dm_1), p.n_map * m2, s));
    HIPCHK(d2.upload(reinterpret_cast<const double2*>(dm_2), p.n_map * m2, s));
    HIPCHK(pc.upload(reinterpret_cast<const double2*>(precalc), p.n_precalc * m2, s));
    HIPCHK(r0.upload(reinterpret_cast<const double2*>(rho_init), N2, s));
    HIPCHK(tt.upload(t1, p.n_t, s));
    if (!dyn) HIPCHK(op.upload(reinterpret_cast<const double2*>(ops), (size_t)n_ops * N2, s));
    p.dm1 = d1.p; p.dm2 = d2.p; p.precalc = pc.p; p.rho_init = r0.p; p.t1 = tt.p; p.ops = op.p;
    if (dyn) {
        const size_t n = (size_t)N2 * (2 * p.n_t - 1);
        HIPCHK(res.alloc(n));
        HIPCHK(launch_dynamics_t1(p, res.p, s));
        HIPCHK(hipMemcpyAsync(result, res.p, n * sizeof(double2), hipMemcpyDeviceToHost, s));
    } else {
        std::vector<int2> pairs;
        pairs.reserve((size_t)p.n_t * (p.n_t + 1) / 2);
        for (int i = std::max(0, row_lo); i < std::min(p.n_t, row_hi); ++i)
            for (int j = 0; j <= p.n_t - 1 - i; ++j) pairs.push_back(make_int2(i, j));
        HIPCHK(pr.upload(pairs.data(), pairs.size(), s));
        p.pairs = pr.p; p.n_pairs = (int)pairs.size();
        const size_t nres = (size_t)p.n_t * p.n_t;
        HIPCHK(res.alloc(nres + (size_t)p.n_t * N2));  // + prologue scratch
        HIPCHK(hipMemsetAsync(res.p, 0, nres * sizeof(double2), s));
        p.result = res.p;
        HIPCHK(launch_four_time(p, s));
        HIPCHK(hipMemcpyAsync(result, res.p, nres * sizeof(double2), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return PQD_OK;
}

static FourTimeParams ft_params(int dim, int n_t, int n_map, int n_precalc, double dt, double tb, int variant = 0,
                                int early_only = 0, int late_t1_only = 0) {
    FourTimeParams p{};
    p.dim = dim; p.n_t = n_t; p.n_map = n_map; p.n_precalc = n_precalc; p.dt = dt; p.tb = tb;
    p.variant = variant; p.early_only = early_only; p.late_t1_only = late_t1_only;
    return p;
}

int pqd_four_time_8op_rows(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                           const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                           int32_t dim, const pqd_c128* ops8, int32_t early_only, int32_t late_t1_only, double tb,
                           int32_t n_precalc, int32_t row_lo, int32_t row_hi, pqd_c128* result) {
    if (row_lo < 0 || row_hi < row_lo || row_hi > n_t) return fail(PQD_ERR_ARG, "rows [%d, %d) outside [0, %d)", row_lo, row_hi, n_t);
    FourTimeParams p = ft_params(dim, n_t, n_map, n_precalc, dt, tb, 0, early_only, late_t1_only);
    return four_time_common(ctx, p, dm_1, dm_2, rho_init, t1, precalc, ops8, 8, result, false, row_lo, row_hi);
}

int pqd_four_time_8op(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                      const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                      int32_t dim, const pqd_c128* ops8, int32_t early_only, int32_t late_t1_only, double tb,
                      int32_t n_precalc, pqd_c128* result) {
    FourTimeParams p = ft_params(dim, n_t, n_map, n_precalc, dt, tb, 0, early_only, late_t1_only);
    return four_time_common(ctx, p, dm_1, dm_2, rho_init, t1, precalc, ops8, 8, result, false, 0, n_t);
}

int pqd_four_time(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                  const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map, int32_t dim,
                  const pqd_c128* ops4, double tb, int32_t n_precalc, pqd_c128* result) {
    FourTimeParams p = ft_params(dim, n_t, n_map, n_precalc, dt, tb, 1);
    return four_time_common(ctx, p, dm_1, dm_2, rho_init, t1, precalc, ops4, 4, result, false);
}

int pqd_dynamics_t1(pqd_ctx* ctx, const pqd_c128* dm_1, const pqd_c128* dm_2, const pqd_c128* rho_init,
                    const double* t1, const pqd_c128* precalc, int32_t n_t, double dt, int32_t n_map,
                    int32_t dim, double tb, int32_t n_precalc, pqd_c128* result) {
    FourTimeParams p = ft_params(dim, n_t, n_map, n_precalc, dt, tb);
    return four_time_common(ctx, p, dm_1, dm_2, rho_init, t1, precalc, nullptr, 0, result, true);
}

int pqd_tl_dynmap_pseudo(pqd_ctx* ctx, const pqd_c128* dm, int32_t n_maps, int32_t n, double rcond,
                         pqd_c128* out) {
    if (!ctx || !dm || !out) return fail(PQD_ERR_ARG, "NULL argument");
    if (n < 1 || n > tl_dynmap_wide_nmax())
        return fail(PQD_ERR_UNSUPPORTED, "map size %d (max %d)", n, tl_dynmap_wide_nmax());
    if (n_maps < 0) return fail(PQD_ERR_ARG, "n_maps %d", n_maps);
    if (!(rcond >= 0.0)) return fail(PQD_ERR_ARG, "rcond %g", rcond);
    if (n_maps == 0) return PQD_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool wide = n > tl_dynmap_nmax();   // tlmap_wide.hip; up to tl_dynmap_nmax() the single-wave kernel as before
    const size_t m2 = (size_t)n * n;
    const size_t total = (size_t)n_maps * m2;
    int grid = 0;
    size_t ws_elems = 0;
    if (wide) {
        int n_cu = 256;
        if (hipDeviceProp_t prop; hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) n_cu = prop.multiProcessorCount;
        HIPCHK(tl_dynmap_wide_plan(n, n_maps, n_cu, &grid, &ws_elems));
    }
    DevBuf<double2> d, o, ws;
    DevBuf<unsigned> aux;   // [0] the flags, [1] the largest sweep count
    auto nomem = [&](hipError_t e, const char* what, size_t elems) {
        return fail(e == hipErrorOutOfMemory ? PQD_ERR_NOMEM : PQD_ERR_HIP, "%s of %zu bytes: %s", what,
                    elems * sizeof(double2), hipGetErrorString(e));
    };
    if (hipError_t e = d.alloc(total); e != hipSuccess) return nomem(e, "input maps", total);
    if (hipError_t e = o.alloc(total); e != hipSuccess) return nomem(e, "output maps", total);
    if (wide) {
        if (hipError_t e = ws.alloc(ws_elems); e != hipSuccess) return nomem(e, "Jacobi workspace", ws_elems);
    }
    HIPCHK(aux.alloc(2));
    HIPCHK(hipMemsetAsync(aux.p, 0, 2 * sizeof(unsigned), s));
    HIPCHK(hipMemcpyAsync(d.p, dm, total * sizeof(double2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(o.p, d.p, m2 * sizeof(double2), hipMemcpyDeviceToDevice, s));  // out[0] = dm[0]

    hipEvent_t ev[2];
    HIPCHK(hipEventCreate(&ev[0]));
    if (hipError_t e1 = hipEventCreate(&ev[1]); e1 != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        return fail(PQD_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e1));
    }
    auto run = [&]() -> int {
        unsigned res[2] = {0u, 0u};
        HIPCHK(hipEventRecord(ev[0], s));
        if (wide)
            HIPCHK(launch_tl_dynmap_wide(d.p, n_maps, n, rcond, o.p, ws.p, grid, aux.p,
                                         reinterpret_cast<int*>(aux.p + 1), s));
        else
            HIPCHK(launch_tl_dynmap(d.p, n_maps, n, rcond, o.p, aux.p, s));
        HIPCHK(hipEventRecord(ev[1], s));
        HIPCHK(hipMemcpyAsync(res, aux.p, sizeof res, hipMemcpyDeviceToHost, s));
        touch_pages(out, total * sizeof(double2));
        HIPCHK(hipMemcpyAsync(out, o.p, total * sizeof(double2), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ctx->tlmap_ms = ms;
        ctx->tlmap_sweeps = (int)res[1];
        // the maps are handed over all the same (they show where the run went bad)
        if (res[0] & 1u) return fail(PQD_ERR_NUMERIC, "non-finite value (NaN/Inf) in the singular values of a map");
        if (res[0] & 2u)
            return fail(PQD_ERR_NUMERIC, "the Jacobi SVD of a map was still rotating after %d sweeps", (int)res[1]);
        return PQD_OK;
    };
    const int rc = run();
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return rc;
}

int pqd_tl_dynmap_timing(pqd_ctx* ctx, double* ms_kernel) {
    if (!ctx || !ms_kernel) return fail(PQD_ERR_ARG, "NULL argument");
    if (ctx->tlmap_ms < 0) return fail(PQD_ERR_ARG, "no pqd_tl_dynmap_pseudo call has completed on this context");
    *ms_kernel = ctx->tlmap_ms;
    return PQD_OK;
}

int pqd_tl_dynmap_sweeps(pqd_ctx* ctx, int32_t* max_sweeps) {
    if (!ctx || !max_sweeps) return fail(PQD_ERR_ARG, "NULL argument");
    if (ctx->tlmap_ms < 0) return fail(PQD_ERR_ARG, "no pqd_tl_dynmap_pseudo call has completed on this context");
    *max_sweeps = ctx->tlmap_sweeps;
    return PQD_OK;
}

}  // extern "C"
