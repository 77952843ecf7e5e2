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
// Free half step: the n_sub exponential-midpoint factors of lind_hilbert.hip, by the same code (lind_hilbert_step.h).
// K(t), K(t)^dag, s and deg depend on the system and the time only: they are built once per sub-step and shared by all
// slices. The slices are independent: G of them are in flight at a time, each group of threads with its own R, T, Tn
// and B_k in LDS (thread lt of a group owns element lt of its slice's matrices, the groups are whole waves). A group
// loads its slice from the workspace, takes it through all s factors of deg Taylor terms (hb_factors), and stores it
// back. The arithmetic of a slice is that of one lind_hilbert.hip trajectory: it does not depend on G, on the group it
// ran in or on the batch. Every barrier is reached by every thread of the workgroup (s, deg, the slice count and the
// events are uniform).
//
// PT phase: X'[alpha][d'] = sum_d X[alpha][d] Q[s][gmap[alpha]][d][d']. The elements are ordered by dictionary entry on
// the host and cut into units of up to HBPT_EB elements of one entry. A tile of units is loaded with all chi bond
// values of its elements into the LDS the matrices used (element-major, odd row stride), then one thread per (unit,
// d') runs d = 0 .. chi - 1 in order with one accumulator per element of the unit: a fetched element of Q (global
// memory, lanes over d': whole rows) serves the unit's HBPT_EB elements. Results go straight back to the workspace: an
// element's new bond vector depends on its own old one only, and the old ones of the tile are in LDS. The slice
// stream per trajectory-step is chi^2 16 B times the number of units (sum over the entries of ceil(elements / HBPT_EB)).
//
// Outputs: rho_red[e] = sum_d c[d] X[d][e], d ascending, one thread per element, into LDS; then the output sums of
// lind_hilbert_kernel (hb_readout). MTOs: the N x N operators with their kind applied to every slice (hb_mto), in array
// order per (trajectory, step, phase) slot.
//
// LDS (dynamic, 16-byte elements): K, Kd, then per group R, T, Tn, B_0 .. B_{nl_max-1}; the PT tile and rho_red overlay
// them (K and Kd are rebuilt by every sub-step, R is reloaded by every slice); then the nonzero lists. The host picks
// G and the tile (pqd_host.cpp setup_hilbert_pt): at N = 24 with 8 jump operators only G = 1 fits.
#include "lind_hilbert_step.h"

namespace {

static_assert(hbpt_mat_elems(HB_NMAX, HB_LMAX, 1) * sizeof(double2) + HB_CSR_LDS <= HBPT_LDS_MAX, "LDS budget at G = 1");
static_assert(HBPT_NT_MAX % 64 == 0 && HBPT_NT_MAX >= hb_threads(HB_NMAX), "one group fits a workgroup");

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
    const HbLists nz = hb_lists<CSR_LDS>(sy, nl, N, W + q.lds_elems, tid, nt);
    double2* X = q.X + (size_t)t * chi * NN;
    // initial state rho0 (x) bond0
    for (int z = tid; z < chi * NN; z += nt) {
        const int d = z / NN;
        if constexpr (MAP) X[z] = z - d * NN == t % NN ? q.bond0[d] : c_zero();
        else X[z] = c_mul(p.rho0[z - d * NN], q.bond0[d]);
    }
    __syncthreads();
    HbRows rows;
    hb_rows(rows, nz.rowptr, nl, N, i, j);
    HbTraj tr = hb_traj<MAP>(p, t, NN);
    const int cs = chi | 1;  // row stride of a PT tile

    // every MTO of the trajectory at (step, phase), in array order, on every slice: R <- A R A^dag (0), A R (1), R A (2)
    auto apply_mtos = [&](int step, int after) {
        while (tr.ev_cur < tr.ev_lim) {
            const int4 ev = p.ev[tr.ev_cur];
            if (ev.x != step || ev.y != after) break;
            for (int d0 = 0; d0 < chi; d0 += G) {
                const bool act = own && d0 + gi < chi;
                double2* Xd = X + (size_t)(act ? d0 + gi : 0) * NN;
                if (act) R[e] = Xd[e];
                __syncthreads();
                const double2 v = hb_mto(p.mto + (size_t)ev.z * NN, ev.w, act, R, T, e, N, i, j);
                if (act) Xd[e] = v;
                __syncthreads();  // every read of R (and of T) is done; the slice is back in the workspace
            }
            ++tr.ev_cur;
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
                    p.out[tr.wo + (long long)(n - 1) * NN + a] = r;
                }
                __syncthreads();  // the workspace is read above and written below
            }
        } else if (tr.wb <= n && n <= tr.we) {
            // rho_red = sum_d c[d] X[d], d ascending, into LDS (over K: the next sub-step rebuilds it)
            const double2* cl = n == 0 ? q.closure0 : q.closure + (size_t)q.sched[n - 1] * chi;
            __syncthreads();  // half step b left the slices in the workspace, each stored by its own group
            for (int a = tid; a < NN; a += nt) {
                double2 r = c_zero();
                for (int d = 0; d < chi; ++d) c_fma(r, cl[d], X[(size_t)d * NN + a]);
                W[a] = r;
            }
            __syncthreads();
            hb_readout(p, W, NN, tid, nt, p.out + tr.wo + (long long)(n - tr.wb) * p.n_out);  // the same sums for every G
            __syncthreads();  // W is read above and written below
        }
        if (n >= tr.we) break;
        apply_mtos(n, 1);
        for (int h = 0; h < 2; ++h) {
            for (int js = 0; js < tr.nsub; ++js) {
                const double tm = tr.ta + n * p.dt + h * 0.5 * p.dt + (js + 0.5) * tr.w;
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
                // K(t) and its adjoint, s and deg: once for all slices
                if (tid < NN) {
                    const int ki = tid / N, kj = tid - ki * N;
                    double2 v = sy.K0[tid];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {  // unrolled: f stays in registers
                        if (c < nc) {
                            c_fma(v, f[c], sy.Xs[(size_t)c * NN + tid]);
                            c_fma(v, c_conj(f[c]), sy.Xt[(size_t)c * NN + tid]);
                        }
                    }
                    K[tid] = v;
                    Kd[kj * N + ki] = c_conj(v);
                }
                const double theta = tr.w * (2.0 * nk + sy.nD);
                int s, deg;
                hb_factor_rule(theta, s, deg);
                __syncthreads();  // K, Kd complete
                for (int d0 = 0; d0 < chi; d0 += G) {
                    const bool act = own && d0 + gi < chi;
                    double2* Xd = X + (size_t)(act ? d0 + gi : 0) * NN;
                    if (act) R[e] = Xd[e];
                    hb_factors(act, e, i, j, N, nl, R, T, Tn, K, Kd, B, nz, rows, s, deg, tr.w / s);
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
hipError_t hp_launch(int n_traj, const HilbertPtParams& q, size_t lds, hipStream_t s) {
    hipError_t e = allow_dyn_lds<&lind_hilbert_pt_kernel<CSR_LDS, MAP>>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((lind_hilbert_pt_kernel<CSR_LDS, MAP>), dim3(n_traj), dim3(q.G * hb_threads(q.h.N)), lds, s, q);
    return hipGetLastError();
}

template <bool MAP>
hipError_t hp_checked_launch(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    const HilbertParams& p = q.h;
    if (!hb_params_ok(p) || (MAP && !hb_map_params_ok(p, n_traj))) return hipErrorInvalidValue;
    if (q.chi < 1 || q.G < 1 || q.G > q.chi || q.G * hb_threads(p.N) > HBPT_NT_MAX || q.ut < 1 || q.n_units < 1 || !q.X)
        return hipErrorInvalidValue;
    // the work area holds the matrices of G groups and a PT tile; with the nonzero lists it fits the CU
    if ((size_t)q.lds_elems < hbpt_mat_elems(p.N, p.nl_max, q.G) ||
        (size_t)q.lds_elems < (size_t)q.ut * hbpt_unit_elems(q.chi))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)q.lds_elems * sizeof(double2) + p.csr_lds;
    if (lds > (size_t)HBPT_LDS_MAX) return hipErrorInvalidValue;
    return p.csr_lds ? hp_launch<true, MAP>(n_traj, q, lds, s) : hp_launch<false, MAP>(n_traj, q, lds, s);
}

}  // namespace

hipError_t launch_hilbert_pt(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    return hp_checked_launch<false>(n_traj, q, s);
}

hipError_t launch_hilbert_pt_map(int n_traj, const HilbertPtParams& q, hipStream_t s) {
    return hp_checked_launch<true>(n_traj, q, s);
}
