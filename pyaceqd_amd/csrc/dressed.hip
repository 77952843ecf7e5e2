// dressed.hip — dressed states: the eigenpairs of H(t_n) for every (system, output time), one launch.
//
// Replaces the reference's second binary `timedep_eigenstates` (general_system.py:297-304, absent offline) and the
// per-time eigenvector loops of general_dressed_states.py:62-70, 161-165. One problem per (system s, output time n):
//   1. H(t_n) = H0 + sum_p (f_p(t_n) X_p + conj(f_p(t_n)) X_p^dagger), f_p sampled as the free propagators sample it;
//   2. cyclic Jacobi on the complex Hermitian N x N matrix with V accumulated, until the off-diagonal Frobenius norm
//      is <= 4 eps ||H||_F (30 sweeps at most);
//   3. eigenvalues ascending (ties by column index), eigenvectors of unit norm with their first component above
//      1e-12 real and positive;
//   4. optionally occ[j] = Re sum_{i,k} v_j[i] conj(v_j[k]) R[i][k] (the reference's formula, taken literally).
//
// Layout: 8 lanes per matrix, 8 matrices per wave, 32 per workgroup. Lane c < N of a group holds column c of H and
// of V (4N doubles); lanes c >= N hold zero columns and only take part in the shuffles. A rotation (p, q) mixes the
// two columns across lanes p and q (one exchange), then every lane mixes its own rows p and q. Every register index
// is a compile-time constant (loops over template N, fully unrolled), so nothing goes to scratch. Results are staged
// in LDS in output order and written by the whole workgroup, consecutive lanes to consecutive elements.
#include "pqd_common.h"
#include <algorithm>
#include <cfloat>

namespace {

constexpr int DS_LPM = 8;                     // lanes per matrix
constexpr int DS_THREADS = 256;
constexpr int DS_PPB = DS_THREADS / DS_LPM;   // problems per workgroup
constexpr int DS_MAX_SWEEPS = 30;
constexpr long long DS_MAX_BLOCKS = 1LL << 22;  // the dispatch grid counts work-items in 32 bits: larger batches loop

__device__ __forceinline__ double2 c_shfl(double2 v, int src) {
    return make_double2(__shfl(v.x, src), __shfl(v.y, src));
}

// sum over the 8 lanes of a group, the same bits in every lane (each step adds the same pair)
__device__ __forceinline__ double group_sum(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

// one rotation (P, Q), P < Q, of the group's matrix: A <- J^dagger A J, V <- V J with
// J[P][P] = J[Q][Q] = c, J[P][Q] = s w, J[Q][P] = -s conj(w), w = A[P][Q] / |A[P][Q]|. `on` is uniform in the group.
template <int N, int P, int Q>
__device__ __forceinline__ void ds_rotate(double2 (&A)[N], double2 (&V)[N], int col, int base, bool on) {
    const double app = __shfl(A[P].x, base + P);
    const double aqq = __shfl(A[Q].x, base + Q);
    const double2 apq = c_shfl(A[P], base + Q);  // row P of column Q
    // the partner's columns (lanes other than P, Q read their own)
    const int src = base + (col == P ? Q : (col == Q ? P : col));
    double2 oA[N], oV[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        oA[r] = c_shfl(A[r], src);
        oV[r] = c_shfl(V[r], src);
    }
    const double b = hypot(apq.x, apq.y);
    if (!on || !(b > 0.0)) return;  // nothing to annihilate (also a NaN element: the problem is flagged elsewhere)
    const double2 w = make_double2(apq.x / b, apq.y / b);
    const double tau = (aqq - app) / (2.0 * b);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t);
    const double s = t * c;
    // columns: col_P' = c col_P - s conj(w) col_Q, col_Q' = s w col_P + c col_Q
    if (col == P || col == Q) {
        const double2 f = col == P ? make_double2(-s * w.x, s * w.y) : make_double2(s * w.x, s * w.y);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            double2 a = c_scale(A[r], c), v = c_scale(V[r], c);
            c_fma(a, f, oA[r]);
            c_fma(v, f, oV[r]);
            A[r] = a;
            V[r] = v;
        }
    }
    // rows: row_P' = c row_P - s w row_Q, row_Q' = s conj(w) row_P + c row_Q
    {
        const double2 xp = A[P], xq = A[Q];
        double2 np = c_scale(xp, c), nq = c_scale(xq, c);
        c_fma(np, make_double2(-s * w.x, -s * w.y), xq);
        c_fma(nq, make_double2(s * w.x, -s * w.y), xp);
        A[P] = np;
        A[Q] = nq;
    }
    // the annihilated pair is exactly zero, the diagonal exactly real
    if (col == P) { A[Q] = c_zero(); A[P].y = 0.0; }
    if (col == Q) { A[P] = c_zero(); A[Q].y = 0.0; }
}

template <int N, int P, int Q>
__device__ __forceinline__ void ds_sweep(double2 (&A)[N], double2 (&V)[N], int col, int base, bool on) {
    if constexpr (P < N - 1) {
        ds_rotate<N, P, Q>(A, V, col, base, on);
        if constexpr (Q + 1 < N) ds_sweep<N, P, Q + 1>(A, V, col, base, on);
        else ds_sweep<N, P + 1, P + 2>(A, V, col, base, on);
    }
}

template <int N>
__global__ __launch_bounds__(DS_THREADS) void dressed_kernel(DressedParams p) {
    __shared__ __attribute__((aligned(16))) double2 st_vec[DS_PPB * N * N];
    __shared__ double st_val[DS_PPB * N];
    __shared__ double st_occ[DS_PPB * N];

    const int tid = threadIdx.x;
    const int lane = tid & (PQD_WAVE - 1);
    const int col = lane & (DS_LPM - 1);      // column of H and V this lane holds
    const int base = lane - col;              // first lane of the group
    const int lp = tid / DS_LPM;              // problem within the workgroup
    const long long n_t = (long long)p.n_steps + 1;
    const long long total = (long long)p.n_sys * n_t;
    const long long n_blk = (total + DS_PPB - 1) / DS_PPB;

    for (long long blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
        const long long first = blk * DS_PPB;
        const long long prob = first + lp;
        const bool live = prob < total && col < N;

        // ---- 1. column `col` of H(t_n), made exactly Hermitian: (H[r][c] + conj(H[c][r])) / 2
        double2 A[N], V[N];
#pragma unroll
        for (int r = 0; r < N; ++r) {
            A[r] = c_zero();
            V[r] = make_double2(r == col ? 1.0 : 0.0, 0.0);
        }
        if (live) {
            const int si = (int)(prob / n_t);
            const int n = (int)(prob - (long long)si * n_t);
            const DressedSys sy = p.systems[si];
            const double t = p.ta + (double)n * p.dt;
#pragma unroll
            for (int r = 0; r < N; ++r) {
                const double2 a = sy.H0[r * N + col], b = sy.H0[col * N + r];
                A[r] = make_double2(a.x + b.x, a.y - b.y);
            }
            for (int ch = 0; ch < sy.n_chan; ++ch) {
                const double2 f = sample_ch(sy, ch, t);  // pqd_common.h: the free propagators' sampling
                const double2* X = sy.X + (size_t)ch * N * N;
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    // (f X + conj(f) X^dagger)[r][c] = f X[r][c] + conj(f X[c][r]); twice its Hermitian part
                    const double2 u = c_mul(f, X[r * N + col]), v = c_mul(f, X[col * N + r]);
                    A[r].x += 2.0 * (u.x + v.x);
                    A[r].y += 2.0 * (u.y - v.y);
                }
            }
#pragma unroll
            for (int r = 0; r < N; ++r) {
                A[r] = c_scale(A[r], 0.5);
                if (r == col) A[r].y = 0.0;
            }
        }

        // ---- 2. cyclic Jacobi
        double mine = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) mine += A[r].x * A[r].x + A[r].y * A[r].y;
        const double norm2 = group_sum(mine);
        const bool finite = norm2 <= DBL_MAX;   // false for Inf and NaN
        const double thr = 4.0 * DBL_EPSILON * sqrt(norm2);
        bool done = !finite;
        int sweeps = 0;
        for (;;) {
            double off = 0.0;
#pragma unroll
            for (int r = 0; r < N; ++r) off += r == col ? 0.0 : A[r].x * A[r].x + A[r].y * A[r].y;
            off = sqrt(group_sum(off));
            if (off <= thr) done = true;
            if (!__any(!done) || sweeps == DS_MAX_SWEEPS) break;
            ds_sweep<N, 0, 1>(A, V, col, base, !done);
            ++sweeps;
        }
        if (col == 0 && prob < total && (!finite || !done)) atomicOr(p.flags, finite ? 2u : 1u);

        // ---- 3. order, norm, phase
        double d = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) d = r == col ? A[r].x : d;
        int rank = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double dj = __shfl(d, base + j);
            rank += (dj < d || (dj == d && j < col)) ? 1 : 0;
        }
        double nv = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) nv += V[r].x * V[r].x + V[r].y * V[r].y;
        const double inv = nv > 0.0 ? 1.0 / sqrt(nv) : 0.0;
        bool found = false;
        double2 ph = make_double2(1.0, 0.0);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            V[r] = c_scale(V[r], inv);
            const double m = hypot(V[r].x, V[r].y);
            if (!found && m > 1e-12) {
                found = true;
                ph = make_double2(V[r].x / m, -V[r].y / m);
            }
        }
        found = false;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            const double m = hypot(V[r].x, V[r].y);
            const bool lead = !found && m > 1e-12;
            found = found || lead;
            const double2 z = c_mul(V[r], ph);
            V[r] = lead ? make_double2(m, 0.0) : z;
        }

        // ---- 4. occupations
        double oc = 0.0;
        if (live && p.occ) {
            const double2* R = p.rho + (size_t)prob * N * N;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double2 ti = c_zero();
#pragma unroll
                for (int k = 0; k < N; ++k) c_fma(ti, c_conj(V[k]), R[i * N + k]);
                oc += V[i].x * ti.x - V[i].y * ti.y;
            }
        }

        // ---- staged in output order, then written by consecutive lanes
        if (col < N) {
#pragma unroll
            for (int r = 0; r < N; ++r) st_vec[(lp * N + rank) * N + r] = V[r];
            st_val[lp * N + rank] = d;
            st_occ[lp * N + rank] = oc;
        }
        __syncthreads();
        const int n_here = (int)(total - first < DS_PPB ? total - first : DS_PPB);
        if (p.evecs)
            for (int e = tid; e < n_here * N * N; e += DS_THREADS) p.evecs[(size_t)first * N * N + e] = st_vec[e];
        if (p.evals)
            for (int e = tid; e < n_here * N; e += DS_THREADS) p.evals[(size_t)first * N + e] = st_val[e];
        if (p.occ)
            for (int e = tid; e < n_here * N; e += DS_THREADS) p.occ[(size_t)first * N + e] = st_occ[e];
        __syncthreads();
    }
}

template <int N>
hipError_t launch_dressed_n(const DressedParams& p, hipStream_t s) {
    const long long total = (long long)p.n_sys * ((long long)p.n_steps + 1);
    const long long n_blk = (total + DS_PPB - 1) / DS_PPB;
    if (n_blk <= 0) return hipSuccess;
    hipLaunchKernelGGL(dressed_kernel<N>, dim3((unsigned)std::min(n_blk, DS_MAX_BLOCKS)), dim3(DS_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dressed(int N, const DressedParams& p, hipStream_t s) {
    return dispatch_list<2, 3, 4, 5, 6>(N, [&](auto NN) { return launch_dressed_n<KV(NN)>(p, s); });
}
