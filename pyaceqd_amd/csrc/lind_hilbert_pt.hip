// lind_hilbert_pt.hip — propagation with a process tensor in Hilbert space (PQD_PATH_HILBERT_PT), for the cavity and
// sensor models at dim 7..24 (and any dim >= 2 a wide PT handle is given for): one workgroup per trajectory, no
// N^2 x N^2 superoperator, no communication between workgroups.
//
// Semantics: DESIGN.md §2 with a PT. Per step: MTOs before -> outputs through the closure (closure0 at step 0, else
// closure[sched[n-1]]) -> MTOs after -> half step a -> PT slice sched[n] -> half step b. The state rho (x) bond is
// X[d][i N + j], chi slices of N x N (slice-major), in the plan's workspace (n_traj chi N^2 16 B; a trajectory's part
// stays in L2); it starts as rho0 (x) bond0. A workgroup owns its trajectory's part: it alone reads and writes it, its
// waves hand values over through __syncthreads().
//
// Free half step: the n_sub exponential-midpoint factors of lind_hilbert.hip, with its midpoints, channel samples,
// norm bound, s and deg (restated here). K(t), K(t)^dag, s and deg depend on the system
// and the time only: they are built once per sub-step and shared by all slices. The slices are independent: G of them
// are in flight at a time, each group of threads with its own R, T, Tn and B_k in LDS (thread lt of a group owns
// element lt of its slice's matrices, the groups are whole waves). A group loads its slice from the workspace, takes it
// through all s factors of deg Taylor terms, and stores it back. The arithmetic of a slice is that of one
// lind_hilbert.hip trajectory: it does not depend on G, on the group it ran in or on the batch. Every barrier is
// reached by every thread of the workgroup (s, deg, the slice count and the events are uniform).
//
// PT phase: X'[alpha][d'] = sum_d X[alpha][d] Q[s][gmap[alpha]][d][d']. The elements are ordered by dictionary entry on
// the host and cut into units of up to HBPT_EB elements of one entry. A tile of units is loaded with all chi bond
// values of its elements into the LDS the matrices used (element-major, odd row stride), then one thread per (unit,
// d') runs d = 0 .. chi - 1 in order with one accumulator per element of the unit: a fetched element of Q (global
// memory, lanes over d': whole rows) serves the unit's HBPT_EB elements. Results go straight back to the workspace: an
// element's new bond vector depends on its own old one only, and the old ones of the tile are in LDS. The slice
// stream per trajectory-step is chi^2 16 B times the number of units (sum over the entries of ceil(elements / HBPT_EB)).
//
// Outputs: rho_red[e] = sum_d c[d] X[d][e], d ascending, one thread per element, into LDS; then the per-wave sums and
// the butterfly of lind_hilbert_kernel. MTOs: the N x N operators with their kind applied to every slice, in array order
// per (trajectory, step, phase) slot.
//
// LDS (dynamic, 16-byte elements): K, Kd, then per group R, T, Tn, B_0 .. B_{nl_max-1}; the PT tile and rho_red overlay
// them (K and Kd are rebuilt by every sub-step, R is reloaded by every slice); then the nonzero lists. The host picks
// G and the tile (pqd_host.cpp setup_hilbert_pt): at N = 24 with 8 jump operators only G = 1 fits.
#include "pqd_common.h"

namespace {

static_assert(hbpt_mat_elems(HB_NMAX, HB_LMAX, 1) * sizeof(double2) + HB_CSR_LDS <= HBPT_LDS_MAX, "LDS budget at G = 1");
static_assert(HBPT_NT_MAX % 64 == 0 && HBPT_NT_MAX >= (HB_NMAX * HB_NMAX + 63) / 64 * 64, "one group fits a workgroup");

enum { HP_LEFT, HP_RIGHT, HP_RIGHT_DAG };
// element (i, j) of A src (LEFT), src A (RIGHT) or src A^dag (RIGHT_DAG); A dense in global memory, src in LDS
template <int MODE>
__device__ __forceinline__ double2 hp_dense(const double2* __restrict__ A, const double2* src, int N, int i, int j) {
    double2 acc = c_zero();
#pragma unroll 4
    for (int m = 0; m < N; ++m) {
        if constexpr (MODE == HP_LEFT) c_fma(acc, A[i * N + m], src[m * N + j]);
        else if constexpr (MODE == HP_RIGHT) c_fma(acc, src[i * N + m], A[m * N + j]);
        else c_fma(acc, src[i * N + m], c_conj(A[j * N + m]));
    }
    return acc;
}

// MAP: the map instance (HilbertParams, map mode): rho0 is a basis element, the start time the map's own, and the closed
// reduced state is stored after every step in place of the output sums.
template <bool CSR_LDS, bool MAP>
__global__ __launch_bounds__(HBPT_NT_MAX) void lind_hilbert_pt_kernel(HilbertPtParams q) {
    extern __shared__ __attribute__((aligned(16))) char hp_smem[];
    const HilbertParams& p = q.h;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int t = blockIdx.x;
    const int N = p.N, NN = N * N;
    const int chi = q.chi, G = q.G;
    const int nt1 = nt / G;  // threads of a group: N^2 rounded up to whole waves
    const HilbertSys sy = p.systems[MAP ? 0 : p.traj_sys[t]];
    const int nl = sy.n_lind < HB_LMAX ? sy.n_lind : HB_LMAX;
    const int nc = sy.n_chan < 4 ? sy.n_chan : 4;
    const int gi = tid / nt1, lt = tid - gi * nt1;
    // the thread's element of its group's slice; threads past the matrix take part in barriers, copies and sums only
    const bool own = lt < NN;
    const int e = own ? lt : 0;
    const int i = e / N, j = e - i * N;

    double2* W = reinterpret_cast<double2*>(hp_smem);  // the work area, lds_elems elements
    double2* K = W;
    double2* Kd = K + NN;
    double2* R = Kd + NN + (size_t)gi * (3 + p.nl_max) * NN;
    double2* T = R + NN;
    double2* Tn = T + NN;
    double2* B = Tn + NN;  // nl_max matrices
    const double2* nzv = sy.val;
    const double2* nzg = sy.valg;
    const int* nzc = sy.col;
    const int* nzr = sy.rowptr;
    if constexpr (CSR_LDS) {
        double2* lv = W + q.lds_elems;
        double2* lg = lv + sy.nnz;
        int* lc = reinterpret_cast<int*>(lg + sy.nnz);
        int* lr = lc + sy.nnz;
        for (int z = tid; z < sy.nnz; z += nt) { lv[z] = sy.val[z]; lg[z] = sy.valg[z]; lc[z] = sy.col[z]; }
        for (int z = tid; z < nl * (N + 1); z += nt) lr[z] = sy.rowptr[z];
        nzv = lv; nzg = lg; nzc = lc; nzr = lr;
    }
    double2* X = q.X + (size_t)t * chi * NN;
    // initial state rho0 (x) bond0
    for (int z = tid; z < chi * NN; z += nt) {
        const int d = z / NN;
        if constexpr (MAP) X[z] = z - d * NN == t % NN ? q.bond0[d] : c_zero();
        else X[z] = c_mul(p.rho0[z - d * NN], q.bond0[d]);
    }
    __syncthreads();
    int ib[HB_LMAX], ie[HB_LMAX], jb[HB_LMAX], je[HB_LMAX];
#pragma unroll
    for (int k = 0; k < HB_LMAX; ++k) {
        ib[k] = ie[k] = jb[k] = je[k] = 0;
        if (k < nl) {
            const int* rp = nzr + k * (N + 1);
            ib[k] = rp[i]; ie[k] = rp[i + 1]; jb[k] = rp[j]; je[k] = rp[j + 1];
        }
    }

    const int wb = MAP ? 0 : p.wbeg[t], we = MAP ? p.map_steps : p.wend[t];
    const long long wo = MAP ? (long long)t * p.map_steps * NN : p.woff[t];
    int ev_cur = MAP ? 0 : p.ev_start[t];
    const int ev_lim = MAP ? p.map_nev : p.ev_start[t + 1];
    const double ta = MAP ? p.map_ta[t / NN] : p.ta;
    const int nsub = p.n_sub > 0 ? p.n_sub : 1;
    const double w = 0.5 * p.dt / nsub;
    const int lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    const int cs = chi | 1;  // row stride of a PT tile

    // every MTO of the trajectory at (step, phase), in array order, on every slice: R <- A R A^dag (0), A R (1), R A (2)
    auto apply_mtos = [&](int step, int after) {
        while (ev_cur < ev_lim) {
            const int4 ev = p.ev[ev_cur];
            if (ev.x != step || ev.y != after) break;
            const double2* A = p.mto + (size_t)ev.z * NN;
            for (int d0 = 0; d0 < chi; d0 += G) {
                const bool act = own && d0 + gi < chi;
                double2* Xd = X + (size_t)(act ? d0 + gi : 0) * NN;
                if (act) R[e] = Xd[e];
                __syncthreads();
                double2 v = c_zero();
                if (act) v = ev.w == 2 ? hp_dense<HP_RIGHT>(A, R, N, i, j) : hp_dense<HP_LEFT>(A, R, N, i, j);
                if (ev.w == 0) {  // (A R) A^dag through T
                    if (act) T[e] = v;
                    __syncthreads();
                    if (act) v = hp_dense<HP_RIGHT_DAG>(A, T, N, i, j);
                }
                if (act) Xd[e] = v;
                __syncthreads();  // every read of R (and of T) is done; the slice is back in the workspace
            }
            ++ev_cur;
        }
    };

    apply_mtos(0, 0);
    for (int n = 0;; ++n) {
        if constexpr (MAP) {
            if (n >= 1) {
                // rho_red = sum_d c[d] X[d], d ascending, straight to the map's staging buffer
                const double2* cl = q.closure + (size_t)q.sched[n - 1] * chi;
                __syncthreads();  // half step b left the slices in the workspace, each stored by its own group
                for (int a = tid; a < NN; a += nt) {
                    double2 r = c_zero();
                    for (int d = 0; d < chi; ++d) c_fma(r, cl[d], X[(size_t)d * NN + a]);
                    p.out[wo + (long long)(n - 1) * NN + a] = r;
                }
                __syncthreads();  // the workspace is read above and written below
            }
        } else if (wb <= n && n <= we) {
            // rho_red = sum_d c[d] X[d], d ascending, into LDS (over K: the next sub-step rebuilds it)
            const double2* cl = n == 0 ? q.closure0 : q.closure + (size_t)q.sched[n - 1] * chi;
            __syncthreads();  // half step b left the slices in the workspace, each stored by its own group
            for (int a = tid; a < NN; a += nt) {
                double2 r = c_zero();
                for (int d = 0; d < chi; ++d) c_fma(r, cl[d], X[(size_t)d * NN + a]);
                W[a] = r;
            }
            __syncthreads();
            // wave v sums outputs v, v + n_waves, ...: lanes over the elements, then a butterfly (the same order in
            // every run and for every G)
            for (int k = wave; k < p.n_out; k += n_waves) {
                const double2* ov = p.ovec + (size_t)k * NN;
                double2 s = c_zero();
                for (int a = lane; a < NN; a += 64) c_fma(s, ov[a], W[a]);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) s = c_add(s, c_shfl_xor(s, m));
                if (lane == 0) p.out[wo + (long long)(n - wb) * p.n_out + k] = s;
            }
            __syncthreads();  // W is read above and written below
        }
        if (n >= we) break;
        apply_mtos(n, 1);
        for (int h = 0; h < 2; ++h) {
            for (int js = 0; js < nsub; ++js) {
                const double tm = ta + n * p.dt + h * 0.5 * p.dt + (js + 0.5) * w;
                double2 f[4];
                double nk = sy.nK0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f[c] = c_zero();
                    if (c < nc) {
                        f[c] = sample_ch(sy, c, tm);
                        nk += hypot(f[c].x, f[c].y) * sy.nX[c];
                    }
                }
                // K(t) and its adjoint, once for all slices
                if (tid < NN) {
                    const int ki = tid / N, kj = tid - ki * N;
                    double2 v = sy.K0[tid];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        if (c < nc) {
                            c_fma(v, f[c], sy.Xs[(size_t)c * NN + tid]);
                            c_fma(v, c_conj(f[c]), sy.Xt[(size_t)c * NN + tid]);
                        }
                    }
                    K[tid] = v;
                    Kd[kj * N + ki] = c_conj(v);
                }
                // factors and degree from the norm bound (lind_hilbert.hip): uniform, independent of the state
                const double theta = w * (2.0 * nk + sy.nD);
                int s = 1, deg = HB_DEGMAX;
                if (theta <= (double)HB_SMAX) {  // false for NaN
                    s = theta > 1.0 ? (int)ceil(theta) : 1;
                    if (s > HB_SMAX) s = HB_SMAX;
                    const double x = theta / s;
                    double rem = 0.5 * x * x;
                    deg = 1;
                    while (deg < HB_DEGMAX && rem * (deg + 2.0) / (deg + 2.0 - x) >= 0x1p-56) {
                        ++deg;
                        rem *= x / (deg + 1);
                    }
                } else if (theta > (double)HB_SMAX && theta < INFINITY) {
                    s = HB_SMAX;  // refused at plan creation; kept finite here all the same
                }
                const double cw = w / s;
                __syncthreads();  // K, Kd complete
                for (int d0 = 0; d0 < chi; d0 += G) {
                    const bool act = own && d0 + gi < chi;
                    double2* Xd = X + (size_t)(act ? d0 + gi : 0) * NN;
                    if (act) R[e] = Xd[e];
                    for (int rep = 0; rep < s; ++rep) {
                        if (act) T[e] = R[e];
                        __syncthreads();
                        for (int m = 1; m <= deg; ++m) {
                            if (nl > 0) {
                                if (act) {
#pragma unroll
                                    for (int k = 0; k < HB_LMAX; ++k) {
                                        if (k < nl) {
                                            double2 acc = c_zero();
                                            for (int z = ib[k]; z < ie[k]; ++z) c_fma(acc, nzv[z], T[nzc[z] * N + j]);
                                            B[(size_t)k * NN + e] = acc;
                                        }
                                    }
                                }
                                __syncthreads();
                            }
                            if (act) {
                                double2 acc = c_zero();
#pragma unroll 6
                                for (int mm = 0; mm < N; ++mm) {
                                    c_fma(acc, K[i * N + mm], T[mm * N + j]);
                                    c_fma(acc, T[i * N + mm], Kd[mm * N + j]);
                                }
#pragma unroll
                                for (int k = 0; k < HB_LMAX; ++k) {
                                    if (k < nl) {
                                        const double2* Bk = B + (size_t)k * NN + i * N;
                                        for (int z = jb[k]; z < je[k]; ++z) c_fma(acc, Bk[nzc[z]], nzg[z]);
                                    }
                                }
                                const double2 v = c_scale(acc, cw / m);
                                Tn[e] = v;
                                R[e] = c_add(R[e], v);
                            }
                            __syncthreads();
                            double2* sw = T; T = Tn; Tn = sw;
                        }
                    }
                    if (act) Xd[e] = R[e];
                }
            }
            if (h == 0) {
                // PT slice sched[n], tile by tile; the tiles overlay the matrices
                __syncthreads();  // the slices are back in the workspace, K and the matrices are free
                const double2* Qs = q.Q + (size_t)q.sched[n] * q.D * chi * chi;
                for (int u0 = 0; u0 < q.n_units; u0 += q.ut) {
                    const int nu = q.n_units - u0 < q.ut ? q.n_units - u0 : q.ut;
                    const int nel = nu * HBPT_EB;
                    for (int z = tid; z < nel * chi; z += nt) {
                        const int d = z / nel, sl = z - d * nel;
                        const int el = q.unit_el[(size_t)u0 * HBPT_EB + sl];
                        W[(size_t)sl * cs + d] = el >= 0 ? X[(size_t)d * NN + el] : c_zero();
                    }
                    __syncthreads();
                    for (int z = tid; z < nu * chi; z += nt) {
                        const int u = z / chi, dp = z - u * chi;
                        const double2* qp = Qs + (size_t)q.unit_g[u0 + u] * chi * chi + dp;
                        const double2* xs = W + (size_t)u * HBPT_EB * cs;
                        double2 acc[HBPT_EB];
#pragma unroll
                        for (int b = 0; b < HBPT_EB; ++b) acc[b] = c_zero();
                        for (int d = 0; d < chi; ++d) {
                            const double2 qv = qp[(size_t)d * chi];
#pragma unroll
                            for (int b = 0; b < HBPT_EB; ++b) c_fma(acc[b], xs[b * cs + d], qv);
                        }
#pragma unroll
                        for (int b = 0; b < HBPT_EB; ++b) {
                            const int el = q.unit_el[(size_t)(u0 + u) * HBPT_EB + b];
                            if (el >= 0) X[(size_t)dp * NN + el] = acc[b];
                        }
                    }
                    __syncthreads();  // the tile is read above and overwritten below; the new values are stored
                }
            }
        }
        apply_mtos(n + 1, 0);
    }
}

template <bool CSR_LDS, bool MAP>
hipError_t hp_launch(int n_traj, const HilbertPtParams& q, int nt, size_t lds, hipStream_t s) {
    static size_t attr[32] = {};  // per device: the dynamic LDS the device's copy of the kernel is allowed so far
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev >= 32 || lds > attr[dev]) {
        hipError_t e = hipFuncSetAttribute((const void*)lind_hilbert_pt_kernel<CSR_LDS, MAP>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev < 32) attr[dev] = lds;
    }
    hipLaunchKernelGGL((lind_hilbert_pt_kernel<CSR_LDS, MAP>), dim3(n_traj), dim3(nt), lds, s, q);
    return hipGetLastError();
}

template <bool MAP>
hipError_t hp_checked_launch(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    const HilbertParams& p = q.h;
    if (p.N < 2 || p.N > HB_NMAX || p.nl_max < 0 || p.nl_max > HB_LMAX || p.csr_lds < 0 || p.csr_lds > HB_CSR_LDS)
        return hipErrorInvalidValue;
    const int nt1 = (p.N * p.N + 63) / 64 * 64;
    if (q.chi < 1 || q.G < 1 || q.G > q.chi || q.G * nt1 > HBPT_NT_MAX || q.ut < 1 || q.n_units < 1 || !q.X)
        return hipErrorInvalidValue;
    // the work area holds the matrices of G groups and a PT tile; with the nonzero lists it fits the CU
    if ((size_t)q.lds_elems < hbpt_mat_elems(p.N, p.nl_max, q.G) ||
        (size_t)q.lds_elems < (size_t)q.ut * hbpt_unit_elems(q.chi))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)q.lds_elems * sizeof(double2) + p.csr_lds;
    if (lds > (size_t)HBPT_LDS_MAX) return hipErrorInvalidValue;
    if (p.csr_lds) return hp_launch<true, MAP>(n_traj, q, q.G * nt1, lds, s);
    return hp_launch<false, MAP>(n_traj, q, q.G * nt1, lds, s);
}

}  // namespace

hipError_t launch_hilbert_pt(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    return hp_checked_launch<false>(n_traj, q, s);
}

hipError_t launch_hilbert_pt_map(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    const HilbertParams& p = q.h;
    if (n_traj > 0 && (p.N < 2 || n_traj % (p.N * p.N) || !p.map_ta || p.map_steps < 1 || p.map_nev < 0 || !p.out))
        return hipErrorInvalidValue;
    return hp_checked_launch<true>(n_traj, q, s);
}
