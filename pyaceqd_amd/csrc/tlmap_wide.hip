// tlmap_wide.hip — time-local dynamical maps for the map sizes above tlmap.hip's single-wave kernel: 37 <= n <= 576
// (n = N^2 of the cavity and sensor models, N = 7 .. 24; any n in the range is taken, not only perfect squares).
//   out[0] = dm[0];  out[i] = dm[i] · pinv(dm[i-1], rcond)   for i = 1 .. n_maps-1
// The method is tlmap.hip's, a one-sided (Hestenes) Jacobi with the same rotations and the same kind of stop rule (a
// whole sweep without a pair |a_p^H a_q| > sqrt(n) eps |a_p| |a_q| (LAPACK zgesvj's threshold; n eps until the maps'
// consumer, mapchain_wide.hip, showed its 1.4e-14 at n = 64 in the correlations), where tlmap.hip has min(n, 4) eps;
// 40 sweeps at most),
// applied to the columns of A^H, that is to
// the ROWS of A = dm[i-1]: A^H·V = W with orthogonal columns w_j = s_j u_j, so A = V W^H,
//   pinv(A) = W diag(1/s_j^2) V^H  (s_j > rcond max s, else 0),   out[i] = (dm[i] W) diag(w) V^H;
// U is never formed, and no Gram matrix or normal equations enter (they would square the condition number and move the
// rcond cut). Why the rows: a dynamical map of a decaying system is graded by rows (the output components that have
// decayed are small rows, A = D·B with B well conditioned), while its columns, the images of the basis elements, all
// approach the stationary state: comparable norms, nearly parallel. Jacobi on columns that differ by scaling converges
// in about as many sweeps as a well-conditioned matrix; on the nearly parallel columns the count grows with the
// dynamic range (a 256 x 256 biexciton-cavity map with singular values down to 1e-25 max s, in a host restatement of
// this ordering: 21 sweeps on the rows, 38-39 on the columns; on the device the columns of that map were still
// rotating at the cap of 40).
//
// Shape: one workgroup of 256 threads per map, a persistent grid (workgroup g takes maps g + 1, g + 1 + grid, ...).
// W and V no longer fit the LDS: they live column-major in a per-workgroup slot of a device workspace (sized by the
// grid, not by n_maps), and the Jacobi is a block Jacobi. The columns are dealt into blocks of B; the block pairs
// (I, J > I) are taken row by row (one workgroup owns the map, so the order of the block pairs is free: block I stays
// in LDS while the blocks J stream through, which halves the workspace traffic of a tournament over block pairs). The
// n x 2B panels of W and of V sit in LDS, where the panel's column pairs are rotated with the scalar rotations of
// tlmap.hip in rounds of B disjoint pairs (rr_pair inside the panel):
//   * pairs (I, I + 1) with I even (every block appears in exactly one; a dummy block when the count is odd): all
//     (2B)(2B-1)/2 pairs of the panel, 2B-1 rounds: the pairs inside each block and the cross pairs;
//   * every other pair of blocks: only the B^2 cross pairs, B rounds of pairs (p_j, q_{(j + round) mod B}).
// So every column pair is visited exactly once per sweep. A pair belongs to a group of G = 256 / B consecutive lanes
// (half a wave or a wave): the lanes split the rows, reduce the three Gram entries with an xor butterfly (the same bits
// in every lane of the group, so every lane computes the same rotation: no LDS hand-over of c, s, phase) and rotate their
// rows of both panels. One barrier per round.
//   B = 8 (2B = 16, G = 32) for n <= 128, B = 4 (2B = 8, G = 64) above: both panels are n x 2B x 16 B, 66 KB at n = 128
//   and 148 KB at n = 576 of the CU's 160 KiB.
// Epilogue per map: s_j^2 = |w_j|^2 (one wave per column), the weights, then two tiled complex products through LDS
// (64 x 64 tile, 4 x 4 per thread, k in steps of 8): B = dm[i] W diag(w) into the slot's third n^2, out[i] = B V^H.
//
// Nothing is shared between workgroups, no floating-point atomics: a map's bits depend on its two input maps only.
// Every loop bound is data-independent (sweeps <= 40; a NaN compares false, rotates nothing and ends the sweep loop).
// flags: bit 0 a non-finite singular-value sum, bit 1 a map still rotating at the sweep cap.
#include "pqd_common.h"
#include <algorithm>
#include <cfloat>

namespace {

constexpr int TW_NMIN = 37;
constexpr int TW_NMAX = 576;
constexpr int TW_THREADS = 256;
constexpr int TW_MAX_SWEEPS = 40;
constexpr int TW_B8_NMAX = 128;   // blocks of 8 columns up to here, of 4 above
constexpr int TW_GT = 64;         // epilogue: output tile edge
constexpr int TW_GK = 8;          //           k step
constexpr int TW_GLD = TW_GT + 1;
constexpr size_t TW_GEMM_LDS = (size_t)2 * TW_GK * TW_GLD * sizeof(double2);

// round-robin tournament: m players (m even), player m-1 fixed; round k, slot j   (as tlmap.hip)
__device__ __forceinline__ void rr_pair(int m, int k, int j, int& p, int& q) {
    if (j == 0) { p = k; q = m - 1; return; }
    p = (k + j) % (m - 1);
    q = (k - j + (m - 1)) % (m - 1);
}

// sum over a group of G (32 or 64) consecutive lanes; every lane of the group ends with the same bits
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int w = G / 2; w >= 1; w >>= 1) v += __shfl_xor(v, w);
    return v;
}

struct TlWideParams {
    const double2* dm;
    double2* out;
    double2* ws;       // gridDim.x slots of 3 n^2: W, V (column-major), B (row-major)
    int n, n_maps;
    double rcond;
    unsigned* flags;
    int* sweeps;       // largest sweep count of the launch
};

// C[r][c] = sum_k A[r][k] Bop(k, c) (* scale[c]);  A and C row-major n x n.
// KFAST: Bop(k, c) = Bsrc[c n + k] (a column-major matrix);  else Bop(k, c) = conj(Bsrc[k n + c]) (its conjugate transpose)
template <bool KFAST>
__device__ void tw_gemm(const double2* __restrict__ A, const double2* __restrict__ Bsrc, double2* __restrict__ Cout,
                        const double* scale, int n, double2* As, double2* Bs, int tid) {
    const int tx = tid & 15, ty = tid >> 4;
    for (int r0 = 0; r0 < n; r0 += TW_GT)
        for (int c0 = 0; c0 < n; c0 += TW_GT) {
            double2 acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = c_zero();
            for (int k0 = 0; k0 < n; k0 += TW_GK) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int e = tid + TW_THREADS * u;
                    {
                        const int kk = e & (TW_GK - 1), rr = e / TW_GK;
                        const int r = r0 + rr, k = k0 + kk;
                        As[kk * TW_GLD + rr] = (r < n && k < n) ? A[(size_t)r * n + k] : c_zero();
                    }
                    if (KFAST) {
                        const int kk = e & (TW_GK - 1), cc = e / TW_GK;
                        const int c = c0 + cc, k = k0 + kk;
                        Bs[kk * TW_GLD + cc] = (c < n && k < n) ? Bsrc[(size_t)c * n + k] : c_zero();
                    } else {
                        const int cc = e & (TW_GT - 1), kk = e / TW_GT;
                        const int c = c0 + cc, k = k0 + kk;
                        Bs[kk * TW_GLD + cc] = (c < n && k < n) ? c_conj(Bsrc[(size_t)k * n + c]) : c_zero();
                    }
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < TW_GK; ++kk) {
                    double2 a[4], b[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = As[kk * TW_GLD + ty + 16 * i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = Bs[kk * TW_GLD + tx + 16 * j];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) c_fma(acc[i][j], a[i], b[j]);
                }
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = r0 + ty + 16 * i, c = c0 + tx + 16 * j;
                    if (r < n && c < n) Cout[(size_t)r * n + c] = scale ? c_scale(acc[i][j], scale[c]) : acc[i][j];
                }
        }
}

template <int B>
__global__ __launch_bounds__(TW_THREADS) void tl_dynmap_wide_kernel(TlWideParams p) {
    constexpr int G = TW_THREADS / B;   // lanes per column pair
    constexpr int C2 = 2 * B;           // panel columns
    static_assert(G == 32 || G == 64, "a pair's lanes are half a wave or a wave");
    extern __shared__ __attribute__((aligned(16))) double2 tw_lds[];
    __shared__ int rotated;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = tid / G, gl = tid % G;
    const int n = p.n, LD = n | 1;
    const size_t m2 = (size_t)n * n;
    double2* Wp = tw_lds;               // [C2][LD], a column contiguous
    double2* Vp = tw_lds + C2 * LD;
    double2* As = tw_lds;               // epilogue: the two operand tiles and the weights
    double2* Bs = tw_lds + TW_GK * TW_GLD;
    double* wsc = reinterpret_cast<double*>(tw_lds + 2 * TW_GK * TW_GLD);
    double2* __restrict__ W = p.ws + (size_t)blockIdx.x * 3 * m2;
    double2* __restrict__ V = W + m2;
    double2* __restrict__ Bm = V + m2;
    const int nb = (n + B - 1) / B;     // column blocks; the last may be short
    const double tol = 2.220446049250313e-16 * sqrt((double)n);

    for (int i = blockIdx.x + 1; i < p.n_maps; i += gridDim.x) {
        const double2* __restrict__ Ai = p.dm + (size_t)(i - 1) * m2;   // row-major dm[i-1] = column-major conj(A^H)
        const double2* __restrict__ Ei = p.dm + (size_t)i * m2;
        for (int e = tid; e < (int)m2; e += TW_THREADS) {
            const int r = e / n, c = e - r * n;
            W[e] = c_conj(Ai[e]);   // column c of A^H is row c of A: W[c n + r] = conj(A[c][r])
            V[e] = (r == c) ? make_double2(1.0, 0.0) : c_zero();
        }
        __syncthreads();

        // one half of the panel (B columns of W and of V) from or to the workspace: a wave per column, lanes over rows
        auto move_half = [&](int blk, int half, bool load) {
            for (int c = wave; c < B; c += TW_THREADS / 64) {
                const int gc = blk * B + c, pc = half * B + c;
                if (gc < n)
                    for (int r = lane; r < n; r += 64) {
                        if (load) {
                            Wp[pc * LD + r] = W[(size_t)gc * n + r];
                            Vp[pc * LD + r] = V[(size_t)gc * n + r];
                        } else {
                            W[(size_t)gc * n + r] = Wp[pc * LD + r];
                            V[(size_t)gc * n + r] = Vp[pc * LD + r];
                        }
                    }
            }
        };
        int sweeps = 0;
        bool conv = false;
        for (int sweep = 0; sweep < TW_MAX_SWEEPS; ++sweep) {
            if (tid == 0) rotated = 0;
            __syncthreads();
            // Row-cyclic over block pairs: block I stays in the panel's first half while the blocks J > I pass through
            // the second, so a pair of blocks costs one block's load and store, not two. The pairs inside the blocks
            // ride on the pairs (I, I + 1) with I even, which run the whole tournament of the 2B columns; an odd count
            // leaves the last block alone with the dummy block nb. Panel column c is global column I B + c (c < B) or
            // J B + c - B; columns >= n do not exist. Every element of W and V is always moved by the same thread
            // (B is a multiple of the wave count), so the barriers below order the LDS, not the workspace.
            for (int I = 0; I < nb; ++I) {
                if ((I & 1) && I == nb - 1) break;   // its inner pairs were rotated as block J of (I - 1, I)
                move_half(I, 0, true);
                const bool lone = I == nb - 1;
                for (int J = I + 1; J < (lone ? nb + 1 : nb); ++J) {
                    move_half(J, 1, true);
                    __syncthreads();
                    const bool full = !(I & 1) && J == I + 1;
                    const int nr = full ? C2 - 1 : B;
                    for (int rd = 0; rd < nr; ++rd) {
                        int pc, qc;
                        if (full) {
                            rr_pair(C2, rd, grp, pc, qc);
                            if (pc > qc) { const int t = pc; pc = qc; qc = t; }
                        } else {
                            pc = grp;
                            qc = B + (grp + rd) % B;
                        }
                        const int gp = pc < B ? I * B + pc : J * B + pc - B;
                        const int gq = qc < B ? I * B + qc : J * B + qc - B;
                        if (gp < n && gq < n) {   // uniform over the group's lanes
                            double2* wpc = Wp + pc * LD;
                            double2* wqc = Wp + qc * LD;
                            double al = 0.0, be = 0.0;
                            double2 g = c_zero();
                            for (int r = gl; r < n; r += G) {
                                const double2 x = wpc[r], y = wqc[r];
                                al = fma(x.x, x.x, fma(x.y, x.y, al));
                                be = fma(y.x, y.x, fma(y.y, y.y, be));
                                c_fma(g, c_conj(x), y);
                            }
                            al = group_sum<G>(al);
                            be = group_sum<G>(be);
                            g.x = group_sum<G>(g.x);
                            g.y = group_sum<G>(g.y);
                            const double ga = hypot(g.x, g.y);
                            if (ga > tol * sqrt(al) * sqrt(be) && ga > 0.0) {
                                const double zeta = (be - al) / (2.0 * ga);
                                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                                const double c = 1.0 / sqrt(1.0 + t * t);
                                const double s = c * t;
                                const double2 ph = make_double2(g.x / ga, -g.y / ga);  // e^{-i phi}, phi = arg(a_p^H a_q)
                                if (gl == 0) rotated = 1;
                                // a_p' = c a_p - s e^{-i phi} a_q ;  a_q' = s a_p + c e^{-i phi} a_q   (same on V)
                                double2* vpc = Vp + pc * LD;
                                double2* vqc = Vp + qc * LD;
                                for (int r = gl; r < n; r += G) {
                                    double2 x = wpc[r], y = c_mul(ph, wqc[r]);
                                    wpc[r] = c_sub(c_scale(x, c), c_scale(y, s));
                                    wqc[r] = c_add(c_scale(x, s), c_scale(y, c));
                                    x = vpc[r]; y = c_mul(ph, vqc[r]);
                                    vpc[r] = c_sub(c_scale(x, c), c_scale(y, s));
                                    vqc[r] = c_add(c_scale(x, s), c_scale(y, c));
                                }
                            }
                        }
                        __syncthreads();
                    }
                    move_half(J, 1, false);
                    __syncthreads();
                }
                move_half(I, 0, false);
                __syncthreads();
            }
            sweeps = sweep + 1;
            const int rot = rotated;   // the same in every thread: all stores lie before the last barrier
            __syncthreads();
            if (!rot) { conv = true; break; }
        }

        // s_j^2 = |w_j|^2, one wave per column
        for (int j = wave; j < n; j += TW_THREADS / 64) {
            double al = 0.0;
            for (int r = lane; r < n; r += 64) {
                const double2 x = W[(size_t)j * n + r];
                al = fma(x.x, x.x, fma(x.y, x.y, al));
            }
            al = group_sum<64>(al);
            if (lane == 0) wsc[j] = al;
        }
        __syncthreads();
        double smax2 = 0.0, ssum = 0.0;
        for (int j = 0; j < n; ++j) {
            smax2 = fmax(smax2, wsc[j]);
            ssum += wsc[j];
        }
        const double smax = sqrt(smax2);
        const bool finite = ssum <= DBL_MAX;   // false for Inf and NaN
        __syncthreads();
        // weights 1/s_j^2 above the cut-off (numpy: s > rcond * max(s))
        for (int j = tid; j < n; j += TW_THREADS) {
            const double s2 = wsc[j];
            wsc[j] = (sqrt(s2) > p.rcond * smax) ? 1.0 / s2 : 0.0;
        }
        if (tid == 0) {
            if (!finite) atomicOr(p.flags, 1u);
            else if (!conv) atomicOr(p.flags, 2u);
            atomicMax(p.sweeps, sweeps);
        }
        __syncthreads();
        tw_gemm<true>(Ei, W, Bm, wsc, n, As, Bs, tid);                          // B = dm[i] W diag(w)
        __syncthreads();
        tw_gemm<false>(Bm, V, p.out + (size_t)i * m2, nullptr, n, As, Bs, tid);  // out[i] = B V^H
        __syncthreads();
    }
}

size_t tw_lds_bytes(int n) {
    const int B = n <= TW_B8_NMAX ? 8 : 4;
    const size_t jac = (size_t)2 * (2 * B) * (n | 1) * sizeof(double2);
    const size_t epi = TW_GEMM_LDS + (size_t)n * sizeof(double);
    return std::max(jac, epi);
}
static_assert((size_t)2 * 8 * (TW_NMAX | 1) * sizeof(double2) + 64 <= 160 * 1024, "LDS budget");
static_assert((size_t)2 * 16 * (TW_B8_NMAX | 1) * sizeof(double2) + 64 <= 160 * 1024, "LDS budget");

template <int B>
hipError_t tw_prepare(size_t lds, int* per_cu) {
    hipError_t e0 = allow_dyn_lds<&tl_dynmap_wide_kernel<B>>(160 * 1024 - 64);
    if (e0 != hipSuccess) return e0;
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, tl_dynmap_wide_kernel<B>, TW_THREADS, lds);
    if (e != hipSuccess) return e;
    *per_cu = std::max(1, std::min(nb, 4));
    return hipSuccess;
}

}  // namespace

int tl_dynmap_wide_nmin() { return TW_NMIN; }
int tl_dynmap_wide_nmax() { return TW_NMAX; }

// the persistent grid for n_maps maps of size n on a device of n_cu compute units, and the workspace it needs
hipError_t tl_dynmap_wide_plan(int n, int n_maps, int n_cu, int* grid, size_t* ws_elems) {
    if (n < TW_NMIN || n > TW_NMAX) return hipErrorInvalidValue;
    const size_t lds = tw_lds_bytes(n);
    int per_cu = 1;
    hipError_t e = n <= TW_B8_NMAX ? tw_prepare<8>(lds, &per_cu) : tw_prepare<4>(lds, &per_cu);
    if (e != hipSuccess) return e;
    const long long want = std::max(1LL, (long long)n_maps - 1);
    *grid = (int)std::min<long long>(want, (long long)std::max(1, n_cu) * per_cu);
    *ws_elems = (size_t)*grid * 3 * (size_t)n * n;
    return hipSuccess;
}

hipError_t launch_tl_dynmap_wide(const double2* dm, int n_maps, int n, double rcond, double2* out, double2* ws,
                                 int grid, unsigned* flags, int* sweeps, hipStream_t s) {
    if (n < TW_NMIN || n > TW_NMAX || grid < 1) return hipErrorInvalidValue;
    if (n_maps <= 1) return hipSuccess;
    TlWideParams p{dm, out, ws, n, n_maps, rcond, flags, sweeps};
    const size_t lds = tw_lds_bytes(n);
    if (n <= TW_B8_NMAX)
        hipLaunchKernelGGL(tl_dynmap_wide_kernel<8>, dim3(grid), dim3(TW_THREADS), lds, s, p);
    else
        hipLaunchKernelGGL(tl_dynmap_wide_kernel<4>, dim3(grid), dim3(TW_THREADS), lds, s, p);
    return hipGetLastError();
}
