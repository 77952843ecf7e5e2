// mapchain_wide.hip — calc_onetime_parallel (two_time/propagate_tau.f90:110-187) and propagate_tau (:3-19) for the
// map sizes above mapchain.hip's one-wave layout: n = N^2 up to 576 (N = 7 .. 24; any n >= 1 runs, which is how the
// small sizes are checked against mapchain.hip under PQD_MC_WIDE=1).
//
// Every trajectory i walks the same map sequence E[q]: the trunk applies E[0 .. p_i - 1], the tau sweep
// E[p_i .. p_i + n_tau - 1] (p_i = j_i - 1, never decreasing in i). So the sweep goes by position, not by trajectory:
// at position q one product Y = E[q] X multiplies the n x n map into the block of all trajectories in flight at q (a
// contiguous range of i), with the trunk state as one more column (column n_t). One launch per position, plain
// launches on one stream: kernel boundaries are the only synchronisation between workgroups.
//   mcw_weights_kernel  u[q] = w^T E[q] for every position, once (w: the trace functional Tr(opB R), trace_weight's
//                       convention of mapchain.hip); the step takes u[q] as row n of the map, so the outputs
//                       G(i, k + 1) = (w^T E) x come out of the same product: (w^T E) x where the reference has w (E x),
//                       a difference of rounding only. No atomics: a result element is written by exactly one lane.
//   mcw_spawn_kernel    before the step of position q, for the trajectories with p_i == q: G(i, 1) = Tr(A (B (C rho)))
//                       and the tau start C rho A into column i (formulas and association of mapchain.hip's
//                       trunk_outputs).
//   mcw_step_kernel     Y[:, c] = E[q] X[:, c] for the live columns, complex FP64 on v_mfma_f64_16x16x4_f64.
//   mcw_step2_kernel    the same step for the periodic sweep (calc_onetime_parallel_block, propagate_tau.f90:189-295),
//                       where the trajectories follow one of two map cursors (pqd_host.cpp mc_wide_block_schedule): at a
//                       position where the cursors name different maps, the two products in one launch. u is then w^T E
//                       per uploaded map, not per position.
// X and Y are ping-pong buffers of n x (columns), each column contiguous. A column that is not live at q (not started,
// finished, padding) is loaded as zero and writes nothing, so whatever the buffers hold there never moves.
#include "pqd_common.h"
#include <algorithm>

namespace {

typedef double dbl4 __attribute__((ext_vector_type(4)));

constexpr int MCW_THREADS = 256;     // 4 waves: wave v owns rows 16 v .. 16 v + 15 of the workgroup's tile
constexpr int MCW_BM = 64;           // rows of a workgroup's tile
constexpr int MCW_BN = 32;           // columns (two MFMA tiles per wave: a map fragment serves both)
constexpr int MCW_BK = 16;           // k per staged chunk (four MFMA k steps)
constexpr int MCW_LDA = MCW_BM + 1;  // LDS row strides in double2
constexpr int MCW_LDB = MCW_BN + 1;
constexpr int MCW_NMAX = HB_NMAX * HB_NMAX;

__device__ __forceinline__ bool mcw_live(const McwStep& p, int c) {
    if (c >= p.c0 && c < p.c1) return !p.pos || (p.pos[c] <= p.q && p.q - p.pos[c] < p.n_tau);
    return p.trunk && c == p.n_t;
}

// Fragment maps of the f64 16x16x4 MFMA (as pt_sweep.hip col_apply_mfma): A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], C[i = (l >> 4) + 4 r][j = l & 15]. Complex product = 4 real ones into cr, ci.
// The map tile (64 rows x 16 k) and the X tile (16 k x 32 columns) of a chunk go through LDS: the X tile serves the
// four row tiles of the workgroup, a wave's map fragment its two column tiles. The next chunk's global loads are issued
// before the products of the current one. Rows >= n (+1 with u), k >= n and dead columns are zeros by guarded loads.
__device__ __forceinline__ void mcw_step(const McwStep& p, int by) {
    __shared__ double2 As[MCW_BK * MCW_LDA];
    __shared__ double2 Xs[MCW_BK * MCW_LDB];
    __shared__ int live[MCW_BN];
    __shared__ int any;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int n = p.n;
    const int r0 = blockIdx.x * MCW_BM, cb = (p.cb0 + by) * MCW_BN;
    if (tid == 0) any = 0;
    __syncthreads();
    if (tid < MCW_BN) {
        const int l = mcw_live(p, cb + tid) ? 1 : 0;
        live[tid] = l;
        if (l) any = 1;
    }
    __syncthreads();
    if (!any) return;  // the same in every thread

    const int a_rr = tid & 63, a_kk = tid >> 6;   // map tile: element (row a_rr, k a_kk + 4 u)
    const int x_kk = tid & 15, x_cc = tid >> 4;   // X tile: element (k x_kk, column x_cc + 16 u)
    const int a_r = r0 + a_rr;
    const bool x_live[2] = {live[x_cc] != 0, live[x_cc + 16] != 0};
    double2 av[4], xv[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + a_kk + 4 * u;
            double2 v = c_zero();
            if (k < n) {
                if (a_r < n) v = p.E[(size_t)k * n + a_r];
                else if (a_r == n && p.u) v = p.u[k];
            }
            av[u] = v;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = k0 + x_kk;
            xv[u] = (k < n && x_live[u]) ? p.X[(size_t)(cb + x_cc + 16 * u) * n + k] : c_zero();
        }
    };
    dbl4 cr[2], ci[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) { cr[t] = dbl4{0, 0, 0, 0}; ci[t] = dbl4{0, 0, 0, 0}; }
    fetch(0);
    for (int k0 = 0; k0 < n; k0 += MCW_BK) {
#pragma unroll
        for (int u = 0; u < 4; ++u) As[(a_kk + 4 * u) * MCW_LDA + a_rr] = av[u];
#pragma unroll
        for (int u = 0; u < 2; ++u) Xs[x_kk * MCW_LDB + x_cc + 16 * u] = xv[u];
        __syncthreads();
        if (k0 + MCW_BK < n) fetch(k0 + MCW_BK);
#pragma unroll
        for (int ks = 0; ks < MCW_BK / 4; ++ks) {
            const double2 a = As[(4 * ks + lk) * MCW_LDA + 16 * wave + li];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const double2 b = Xs[(4 * ks + lk) * MCW_LDB + 16 * t + li];
                cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, cr[t], 0, 0, 0);
                cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, cr[t], 0, 0, 0);
                ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, ci[t], 0, 0, 0);
                ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, ci[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int cc = 16 * t + li, c = cb + cc;
        if (!live[cc]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * wave + lk + 4 * r;
            const double2 v = make_double2(cr[t][r], ci[t][r]);
            if (row < n) p.Y[(size_t)c * n + row] = v;
            else if (row == n && p.u && p.pos && c < p.n_t)   // a live trajectory: p_i <= q < p_i + n_tau
                p.result[(size_t)c + (size_t)(p.q - p.pos[c] + 1) * p.n_t] = v;
        }
    }
}

__global__ __launch_bounds__(MCW_THREADS) void mcw_step_kernel(McwStep p) { mcw_step(p, blockIdx.y); }

// Two families at one position (the periodic sweep, calc_onetime_parallel_block): blockIdx.z picks the family, each
// with its own map, u row, column range and trunk flag over the same X, Y and result. A family's live columns lie
// inside its [c0, c1) (mcw_live), so a 32-column tile that straddles the border between the families is issued in
// both, and in each the other family's columns load zero and write nothing.
__global__ __launch_bounds__(MCW_THREADS) void mcw_step2_kernel(McwStep2 p) {
    const int z = blockIdx.z;
    if ((int)blockIdx.y >= (z ? p.ncb1 : p.ncb0)) return;  // the same in every thread
    if (z) mcw_step(p.f1, blockIdx.y);
    else mcw_step(p.f0, blockIdx.y);
}

// U[q][k] = sum_r w[r] E[q][r + k n]: one wave per map column, lanes over the rows, then a butterfly whose order is
// fixed (the same bits on every run)
__global__ __launch_bounds__(MCW_THREADS) void mcw_weights_kernel(const double2* __restrict__ E,
                                                                  const double2* __restrict__ w,
                                                                  double2* __restrict__ U, int n) {
    const int q = blockIdx.x, lane = threadIdx.x & 63;
    const int k = blockIdx.y * (MCW_THREADS / 64) + (threadIdx.x >> 6);
    if (k >= n) return;  // whole waves
    const double2* col = E + ((size_t)q * n + k) * n;
    double2 acc = c_zero();
    for (int r = lane; r < n; r += 64) c_fma(acc, w[r], col[r]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o, 64);
        acc.y += __shfl_xor(acc.y, o, 64);
    }
    if (lane == 0) U[(size_t)q * n + k] = acc;
}

// Z(e) for e = a + b dim: sum_k X(a, k) Y(k, b) (column-major dim x dim; mapchain.hip cm_mat)
__device__ __forceinline__ double2 mcw_mat(const double2* X, const double2* Y, int e, int dim) {
    const int a = e % dim, b = e / dim;
    double2 acc = c_zero();
    for (int k = 0; k < dim; ++k) c_fma(acc, X[a + k * dim], Y[k + b * dim]);
    return acc;
}

// one workgroup per starting trajectory, the n elements dealt in strided loops (propagate_tau.f90:154-163)
__global__ __launch_bounds__(MCW_THREADS) void mcw_spawn_kernel(McwSpawn p) {
    __shared__ double2 x[MCW_NMAX], t1[MCW_NMAX], t2[MCW_NMAX];
    const int tid = threadIdx.x, n = p.n, dim = p.dim;
    const int i = p.i0 + blockIdx.x;
    for (int e = tid; e < n; e += MCW_THREADS) x[e] = p.X[(size_t)p.n_t * n + e];
    __syncthreads();
    for (int e = tid; e < n; e += MCW_THREADS) t1[e] = mcw_mat(p.opC, x, e, dim);
    __syncthreads();
    for (int e = tid; e < n; e += MCW_THREADS) t2[e] = mcw_mat(p.opB, t1, e, dim);
    __syncthreads();
    for (int e = tid; e < n; e += MCW_THREADS) t1[e] = mcw_mat(p.opA, t2, e, dim);
    __syncthreads();
    if (tid == 0) {
        double2 s = c_zero();
        for (int l = 0; l < dim; ++l) s = c_add(s, t1[l + l * dim]);
        p.result[i] = s;
    }
    __syncthreads();
    for (int e = tid; e < n; e += MCW_THREADS) t1[e] = mcw_mat(p.opC, x, e, dim);
    __syncthreads();
    for (int e = tid; e < n; e += MCW_THREADS) p.X[(size_t)i * n + e] = mcw_mat(t1, p.opA, e, dim);
}

}  // namespace

hipError_t launch_mcw_weights(const double2* E, const double2* w, double2* U, int n, int Q, hipStream_t s) {
    if (n < 1 || n > MCW_NMAX || Q < 0) return hipErrorInvalidValue;
    if (Q == 0) return hipSuccess;
    const dim3 grid(Q, (n + MCW_THREADS / 64 - 1) / (MCW_THREADS / 64));
    hipLaunchKernelGGL(mcw_weights_kernel, grid, dim3(MCW_THREADS), 0, s, E, w, U, n);
    return hipGetLastError();
}

hipError_t launch_mcw_spawn(const McwSpawn& p, int count, hipStream_t s) {
    if (p.n < 1 || p.n > MCW_NMAX || p.dim * p.dim != p.n || count < 0 || p.i0 < 0 || p.i0 + count > p.n_t)
        return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(mcw_spawn_kernel, dim3(count), dim3(MCW_THREADS), 0, s, p);
    return hipGetLastError();
}

// the column blocks from the first live trajectory (or the trunk column) to the last live column: sets p.cb0 and
// returns their number (0: nothing live, -1: bad arguments); blocks in between without a live column return at once
static int mcw_blocks(McwStep& p) {
    const bool traj = p.c0 < p.c1;
    if (p.n < 1 || p.n > MCW_NMAX || p.c0 < 0 || (p.pos && p.c1 > p.n_t)) return -1;
    if (!traj && !p.trunk) return 0;
    const int first = traj ? p.c0 / MCW_BN : p.n_t / MCW_BN;
    const int last = p.trunk ? p.n_t / MCW_BN : (p.c1 - 1) / MCW_BN;
    p.cb0 = first;
    return last - first + 1;
}
static unsigned mcw_row_tiles(const McwStep& p) { return (unsigned)((p.n + (p.u ? 1 : 0) + MCW_BM - 1) / MCW_BM); }

hipError_t launch_mcw_step(const McwStep& p0, hipStream_t s) {
    McwStep p = p0;
    const int ncb = mcw_blocks(p);
    if (ncb < 0) return hipErrorInvalidValue;
    if (ncb == 0) return hipSuccess;
    hipLaunchKernelGGL(mcw_step_kernel, dim3(mcw_row_tiles(p), ncb), dim3(MCW_THREADS), 0, s, p);
    return hipGetLastError();
}

// one launch for the two families of a position; a family with nothing live leaves the launch to the other
hipError_t launch_mcw_step2(const McwStep& a, const McwStep& b, hipStream_t s) {
    McwStep2 p{a, b, 0, 0};
    p.ncb0 = mcw_blocks(p.f0);
    p.ncb1 = mcw_blocks(p.f1);
    if (p.ncb0 < 0 || p.ncb1 < 0 || a.n != b.n || !a.u != !b.u) return hipErrorInvalidValue;
    if (p.ncb0 == 0) return launch_mcw_step(b, s);
    if (p.ncb1 == 0) return launch_mcw_step(a, s);
    const dim3 grid(mcw_row_tiles(a), std::max(p.ncb0, p.ncb1), 2);
    hipLaunchKernelGGL(mcw_step2_kernel, grid, dim3(MCW_THREADS), 0, s, p);
    return hipGetLastError();
}
