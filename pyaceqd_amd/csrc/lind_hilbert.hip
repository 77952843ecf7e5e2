// lind_hilbert.hip — Lindblad propagation without a process tensor in Hilbert space, for dim 7..24 (and dim <= 6
// under PQD_HILBERT=1): one workgroup per trajectory, rho as an N x N matrix in LDS, no N^2 x N^2 superoperator.
//
// Semantics: DESIGN.md §2 without a PT, exactly as sweep_nopt_kernel (pt_sweep.hip) runs it from stored free
// propagators: per step MTOs before -> outputs -> MTOs after -> half step a -> half step b; a half step is n_sub
// exponential-midpoint factors exp(L(t_mid) w), w = dt / (2 n_sub), at the midpoints free_prop.hip uses, with its
// channel sampling (sample_ch, pqd_common.h).
//
// A factor is applied to rho, never built:
//   L(rho) = K rho + rho K^dag + sum_k gamma_k A_k rho A_k^dag,    K(t) = K0 + sum_p (f_p Xs_p + conj(f_p) Xt_p)
// (K0, Xs, Xt: HilbertSys; the Liouvillian of commutator / dissipator in pqd_host.cpp), as s scaled Taylor series
//   exp(L w) rho = (exp(L w / s))^s rho,    exp(L c) rho = sum_{m <= deg} c^m L^m rho / m!,  c = w / s.
// s and deg come from a bound of ||L w|| in the Frobenius norm of rho, ||K rho|| <= ||K||_F ||rho||_F and
// ||A rho A^dag|| <= ||A||_F^2 ||rho||_F:
//   theta = w (2 (||K0|| + sum_p |f_p(t_mid)| (||Xs_p|| + ||Xt_p||)) + sum_k |gamma_k| ||A_k||^2)
// s = ceil(theta) (at least 1, at most HB_SMAX), x = theta / s <= 1, deg = the smallest m <= HB_DEGMAX with
// x^(m+1) / (m+1)! (m+2) / (m+2-x) < 2^-56 (the remainder rule of free_prop.hip; x = 1 gives 18). Both depend on the
// system and the time only, never on rho, so every trajectory of a system runs the same arithmetic and its outputs are
// the same bits in any batch. A non-finite theta takes s = 1, deg = HB_DEGMAX: the kernel ends, the outputs are not
// finite, and pqd_plan_synchronize reports PQD_ERR_NUMERIC. Plan creation refuses a finite bound above HB_SMAX
// (pqd_host.cpp), so the cap on s is never what a finished run depended on.
//
// The workgroup has one thread per element of rho, rounded up to whole waves (N = 18: 6 waves, N = 24: 9); thread
// e = i N + j owns element (i, j) of every matrix. One Taylor term is two passes:
//   1. B_k = A_k T for every jump operator, from the operator's nonzeros by rows;
//   2. Tn = c/m (K T + T K^dag + sum_k B_k (gamma_k A_k^dag)), R += Tn   (gamma_k conj(A_k) by the rows of A_k: valg),
// with a barrier after each. Jump operators are held as nonzero lists (a reference model's has at most N entries; a
// dense one has N^2 and costs N times as much, with the same code); a thread keeps the bounds of its two rows of every
// list (row i for pass 1, row j for pass 2) in registers. The lists are read from LDS when every system's fit
// HB_CSR_LDS bytes, else from global memory.
//
// LDS (dynamic, 16-byte elements): R (rho, and the running sum), T, Tn (Taylor terms), K(t), Kd = K(t)^dag (so that both
// products read consecutive addresses across lanes), B_0 .. B_{nl-1}; then the nonzero lists. At N = 24 with 8 jump
// operators: 13 * 9216 B + 32 KiB = 149 KiB.
//
// Map instances (template parameter MAP, launch_hilbert_map): n_maps * N^2 trajectories of one system,
// trajectory m N^2 + beta from the basis element beta at the map's own start time, the state itself stored after every
// step in place of the output sums. A dynamical map is these columns (map_assemble_kernel, pqd_util.hip). The
// instances with MAP = false are the kernel as it was.
#include "pqd_common.h"

namespace {

constexpr int HB_NT_MAX = (HB_NMAX * HB_NMAX + 63) / 64 * 64;  // threads of the largest workgroup (576)
constexpr size_t HB_LDS_MAX = (size_t)(5 + HB_LMAX) * HB_NMAX * HB_NMAX * sizeof(double2) + HB_CSR_LDS;
static_assert(HB_LDS_MAX <= 160 * 1024, "LDS budget");
static_assert(HB_CSR_LDS % 16 == 0, "the nonzero lists start on a 16-byte boundary");
static_assert(HB_NT_MAX <= 1024, "one thread per element");

// LDS bytes of the nonzero lists of one system: values, gamma conj(values), then columns, then row offsets
__host__ __device__ inline size_t hb_csr_bytes(int N, int n_lind, int nnz) {
    return (size_t)nnz * 2 * sizeof(double2) + ((size_t)nnz + (size_t)n_lind * (N + 1)) * sizeof(int);
}

// element (i, j) of A src (LEFT), src A (RIGHT) or src A^dag (RIGHT_DAG); A dense in global memory, src in LDS
enum { HB_LEFT, HB_RIGHT, HB_RIGHT_DAG };
template <int MODE>
__device__ __forceinline__ double2 hb_dense(const double2* __restrict__ A, const double2* src, int N, int i, int j) {
    double2 acc = c_zero();
#pragma unroll 4
    for (int m = 0; m < N; ++m) {
        if constexpr (MODE == HB_LEFT) c_fma(acc, A[i * N + m], src[m * N + j]);
        else if constexpr (MODE == HB_RIGHT) c_fma(acc, src[i * N + m], A[m * N + j]);
        else c_fma(acc, src[i * N + m], c_conj(A[j * N + m]));
    }
    return acc;
}

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
    // nonzero lists: LDS copies (filled below) or the global arrays
    const double2* nzv = sy.val;
    const double2* nzg = sy.valg;
    const int* nzc = sy.col;
    const int* nzr = sy.rowptr;
    if constexpr (CSR_LDS) {
        double2* lv = B + (size_t)p.nl_max * NN;
        double2* lg = lv + sy.nnz;
        int* lc = reinterpret_cast<int*>(lg + sy.nnz);
        int* lr = lc + sy.nnz;
        for (int z = tid; z < sy.nnz; z += nt) { lv[z] = sy.val[z]; lg[z] = sy.valg[z]; lc[z] = sy.col[z]; }
        for (int z = tid; z < nl * (N + 1); z += nt) lr[z] = sy.rowptr[z];
        nzv = lv; nzg = lg; nzc = lc; nzr = lr;
    }
    if constexpr (MAP) {
        if (own) R[e] = e == t % NN ? make_double2(1.0, 0.0) : c_zero();
    } else {
        if (own) R[e] = p.rho0[e];
    }
    __syncthreads();
    // the thread's rows of every jump operator's list: row i (pass 1), row j (pass 2)
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

    // every MTO of the trajectory at (step, phase), in array order: R <- A R A^dag (kind 0), A R (1), R A (2)
    auto apply_mtos = [&](int step, int after) {
        while (ev_cur < ev_lim) {
            const int4 ev = p.ev[ev_cur];
            if (ev.x != step || ev.y != after) break;
            const double2* A = p.mto + (size_t)ev.z * NN;
            double2 v = c_zero();
            if (own) v = ev.w == 2 ? hb_dense<HB_RIGHT>(A, R, N, i, j) : hb_dense<HB_LEFT>(A, R, N, i, j);
            if (ev.w == 0) {  // (A R) A^dag through T
                if (own) T[e] = v;
                __syncthreads();
                if (own) v = hb_dense<HB_RIGHT_DAG>(A, T, N, i, j);
            }
            __syncthreads();  // every read of R (and of T) is done
            if (own) R[e] = v;
            __syncthreads();
            ++ev_cur;
        }
    };

    apply_mtos(0, 0);
    for (int n = 0;; ++n) {
        if constexpr (MAP) {
            // the state itself, every thread its own element (which it wrote last): no barrier
            if (n >= 1 && own) p.out[wo + (long long)(n - 1) * NN + e] = R[e];
        } else if (wb <= n && n <= we) {
            // wave v sums outputs v, v + n_waves, ...: lanes over the elements, then a butterfly (the same order in
            // every run)
            for (int k = wave; k < p.n_out; k += n_waves) {
                const double2* ov = p.ovec + (size_t)k * NN;
                double2 s = c_zero();
                for (int a = lane; a < NN; a += 64) c_fma(s, ov[a], R[a]);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) s = c_add(s, c_shfl_xor(s, m));
                if (lane == 0) p.out[wo + (long long)(n - wb) * p.n_out + k] = s;
            }
            __syncthreads();  // R is read above and written below
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
                // factors and degree from the norm bound (header): uniform over the workgroup, independent of rho
                const double theta = w * (2.0 * nk + sy.nD);
                int s = 1, deg = HB_DEGMAX;
                if (theta <= (double)HB_SMAX) {  // false for NaN
                    s = theta > 1.0 ? (int)ceil(theta) : 1;
                    if (s > HB_SMAX) s = HB_SMAX;
                    const double x = theta / s;
                    double rem = 0.5 * x * x;  // x^(deg+1) / (deg+1)! for deg = 1
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
                for (int rep = 0; rep < s; ++rep) {
                    if (own) T[e] = R[e];
                    __syncthreads();
                    for (int m = 1; m <= deg; ++m) {
                        if (nl > 0) {
                            if (own) {
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
                        if (own) {
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
            }
        }
        apply_mtos(n + 1, 0);
    }
}

template <bool CSR_LDS, bool MAP>
hipError_t hb_launch(int n_traj, const HilbertParams& p, size_t lds, hipStream_t s) {
    static unsigned attr = 0;  // per-device bitmask (the attribute belongs to the device's copy of the kernel)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev >= 32 || !(attr & (1u << dev))) {
        hipError_t e = hipFuncSetAttribute((const void*)lind_hilbert_kernel<CSR_LDS, MAP>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)HB_LDS_MAX);
        if (e != hipSuccess) return e;
        if (dev < 32) attr |= 1u << dev;
    }
    const int nt = (p.N * p.N + 63) / 64 * 64;  // one thread per element, whole waves
    hipLaunchKernelGGL((lind_hilbert_kernel<CSR_LDS, MAP>), dim3(n_traj), dim3(nt), lds, s, p);
    return hipGetLastError();
}

}  // namespace

size_t hilbert_csr_bytes(int N, int n_lind, int nnz) { return (hb_csr_bytes(N, n_lind, nnz) + 15) & ~(size_t)15; }

hipError_t launch_hilbert(int n_traj, const HilbertParams& p, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    if (p.N < 2 || p.N > HB_NMAX || p.nl_max < 0 || p.nl_max > HB_LMAX || p.csr_lds < 0 || p.csr_lds > HB_CSR_LDS)
        return hipErrorInvalidValue;
    const size_t mats = (size_t)(5 + p.nl_max) * p.N * p.N * sizeof(double2);
    if (p.csr_lds) return hb_launch<true, false>(n_traj, p, mats + p.csr_lds, s);
    return hb_launch<false, false>(n_traj, p, mats, s);
}

hipError_t launch_hilbert_map(int n_traj, const HilbertParams& p, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    if (p.N < 2 || p.N > HB_NMAX || p.nl_max < 0 || p.nl_max > HB_LMAX || p.csr_lds < 0 || p.csr_lds > HB_CSR_LDS)
        return hipErrorInvalidValue;
    if (n_traj % (p.N * p.N) || !p.map_ta || p.map_steps < 1 || p.map_nev < 0 || !p.out) return hipErrorInvalidValue;
    const size_t mats = (size_t)(5 + p.nl_max) * p.N * p.N * sizeof(double2);
    if (p.csr_lds) return hb_launch<true, true>(n_traj, p, mats + p.csr_lds, s);
    return hb_launch<false, true>(n_traj, p, mats, s);
}
