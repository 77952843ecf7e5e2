// lind_hilbert.hip — Lindblad propagation without a process tensor in Hilbert space, for dim 7..24 (and dim <= 6
// under PQD_HILBERT=1): one workgroup per trajectory, rho as an N x N matrix in LDS, no N^2 x N^2 superoperator.
//
// Semantics: DESIGN.md §2 without a PT, exactly as sweep_nopt_kernel (pt_sweep.hip) runs it from stored free
// propagators: per step MTOs before -> outputs -> MTOs after -> half step a -> half step b; a half step is n_sub
// exponential-midpoint factors exp(L(t_mid) w), w = dt / (2 n_sub), at the midpoints free_prop.hip uses, with its
// channel sampling (sample_ch, pqd_common.h). The factor itself (s and deg from the norm bound, the Taylor terms from
// the jump operators' nonzero lists), the output sums and the value of an MTO are lind_hilbert_step.h, shared with
// lind_hilbert_pt.hip. Here: the LDS map of one trajectory, the loop over its steps and the build of K(t) (written
// out in both kernels: DESIGN.md §4.12).
//
// The workgroup has one thread per element of rho, rounded up to whole waves (N = 18: 6 waves, N = 24: 9); thread
// e = i N + j owns element (i, j) of every matrix.
//
// LDS (dynamic, 16-byte elements): R (rho, and the running sum), T, Tn (Taylor terms), K(t), Kd = K(t)^dag,
// B_0 .. B_{nl-1} (hb_mat_elems); then the nonzero lists. At N = 24 with 8 jump operators: 13 * 9216 B + 32 KiB =
// 149 KiB.
//
// Map instances (template parameter MAP, launch_hilbert_map): n_maps * N^2 trajectories of one system,
// trajectory m N^2 + beta from the basis element beta at the map's own start time, the state itself stored after every
// step in place of the output sums. A dynamical map is these columns (map_assemble_kernel, pqd_util.hip). The
// instances with MAP = false are the kernel as it was.
#include "lind_hilbert_step.h"

namespace {

constexpr int HB_NT_MAX = (HB_NMAX * HB_NMAX + 63) / 64 * 64;  // threads of the largest workgroup (576)
constexpr size_t HB_LDS_MAX = hb_mat_elems(HB_NMAX, HB_LMAX) * sizeof(double2) + HB_CSR_LDS;
static_assert(HB_LDS_MAX <= 160 * 1024, "LDS budget");
static_assert(HB_NT_MAX <= 1024, "one thread per element");

// MAP: the map instance (HilbertParams, map mode): the trajectory starts from a basis element at its map's own time
// and stores its state after every step in place of the output sums. Everything else of a step is the same code.
template <bool CSR_LDS, bool MAP>
__global__ __launch_bounds__(HB_NT_MAX) void lind_hilbert_kernel(HilbertParams p) {
    extern __shared__ __attribute__((aligned(16))) char hb_smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int t = blockIdx.x;
    const int N = p.N, NN = N * N;
    const HilbertSys sy = p.systems[MAP ? 0 : p.traj_sys[t]];
    const int nl = sy.n_lind < HB_LMAX ? sy.n_lind : HB_LMAX;
    const int nc = sy.n_chan < 4 ? sy.n_chan : 4;
    // the thread's element; threads past the matrix (the last wave's tail) only take part in barriers, copies and
    // the output sums
    const bool own = tid < NN;
    const int e = own ? tid : 0;
    const int i = e / N, j = e - i * N;

    double2* R = reinterpret_cast<double2*>(hb_smem);
    double2* T = R + NN;
    double2* Tn = T + NN;
    double2* K = Tn + NN;
    double2* Kd = K + NN;
    double2* B = Kd + NN;  // nl_max matrices
    const HbLists nz = hb_lists<CSR_LDS>(sy, nl, N, B + (size_t)p.nl_max * NN, tid, nt);
    if constexpr (MAP) {
        if (own) R[e] = e == t % NN ? make_double2(1.0, 0.0) : c_zero();
    } else {
        if (own) R[e] = p.rho0[e];
    }
    __syncthreads();
    HbRows rows;
    hb_rows(rows, nz.rowptr, nl, N, i, j);
    HbTraj tr = hb_traj<MAP>(p, t, NN);

    // every MTO of the trajectory at (step, phase), in array order: R <- A R A^dag (kind 0), A R (1), R A (2)
    auto apply_mtos = [&](int step, int after) {
        while (tr.ev_cur < tr.ev_lim) {
            const int4 ev = p.ev[tr.ev_cur];
            if (ev.x != step || ev.y != after) break;
            const double2 v = hb_mto(p.mto + (size_t)ev.z * NN, ev.w, own, R, T, e, N, i, j);
            __syncthreads();  // every read of R (and of T) is done
            if (own) R[e] = v;
            __syncthreads();
            ++tr.ev_cur;
        }
    };

    apply_mtos(0, 0);
    for (int n = 0;; ++n) {
        if constexpr (MAP) {
            // the state itself, every thread its own element (which it wrote last): no barrier
            if (n >= 1 && own) p.out[tr.wo + (long long)(n - 1) * NN + e] = R[e];
        } else if (tr.wb <= n && n <= tr.we) {
            hb_readout(p, R, NN, tid, nt, p.out + tr.wo + (long long)(n - tr.wb) * p.n_out);
            __syncthreads();  // R is read above and written below
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
                // K(t) and its adjoint
                if (own) {
                    double2 v = sy.K0[e];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {  // unrolled: f stays in registers
                        if (c < nc) {
                            c_fma(v, f[c], sy.Xs[(size_t)c * NN + e]);
                            c_fma(v, c_conj(f[c]), sy.Xt[(size_t)c * NN + e]);
                        }
                    }
                    K[e] = v;
                    Kd[j * N + i] = c_conj(v);
                }
                const double theta = tr.w * (2.0 * nk + sy.nD);
                int s, deg;
                hb_factor_rule(theta, s, deg);
                __syncthreads();  // K, Kd complete
                hb_factors(own, e, i, j, N, nl, R, T, Tn, K, Kd, B, nz, rows, s, deg, tr.w / s);
            }
        }
        apply_mtos(n + 1, 0);
    }
}

template <bool CSR_LDS, bool MAP>
hipError_t hb_launch(int n_traj, const HilbertParams& p, hipStream_t s) {
    hipError_t e = allow_dyn_lds<&lind_hilbert_kernel<CSR_LDS, MAP>>(HB_LDS_MAX);
    if (e != hipSuccess) return e;
    const size_t lds = hb_mat_elems(p.N, p.nl_max) * sizeof(double2) + p.csr_lds;
    hipLaunchKernelGGL((lind_hilbert_kernel<CSR_LDS, MAP>), dim3(n_traj), dim3(hb_threads(p.N)), lds, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_hilbert(int n_traj, const HilbertParams& p, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    if (!hb_params_ok(p)) return hipErrorInvalidValue;
    return p.csr_lds ? hb_launch<true, false>(n_traj, p, s) : hb_launch<false, false>(n_traj, p, s);
}

hipError_t launch_hilbert_map(int n_traj, const HilbertParams& p, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    if (!hb_params_ok(p) || !hb_map_params_ok(p, n_traj)) return hipErrorInvalidValue;
    return p.csr_lds ? hb_launch<true, true>(n_traj, p, s) : hb_launch<false, true>(n_traj, p, s);
}
