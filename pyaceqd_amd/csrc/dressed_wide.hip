// dressed_wide.hip — dressed states of the cavity and sensor models: the eigenpairs of H(t_n) for 7 <= N <= 24.
//
// The same problem as dressed.hip (one per (system s, output time n): H(t_n) from H0, the channel operators and the
// samples; Jacobi with V accumulated; order, norm, phase; optionally the occupations), for the dimensions whose columns
// no longer fit a lane's registers (tls_photons_dressed_states, biexciton_photons[_extended]_dressed_states:
// tls.py:207-212, linear.py:105-109, 157-159; any model through general_dressed_states.py:26-44).
//
// Shape: one wave per problem, one problem per workgroup (64 threads), H and V in LDS, several elements per lane. A
// problem owns its workgroup, so its sweep loop is uniform over everything that shares a barrier, nothing depends on
// its neighbours in the batch, and a barrier is a wait for the wave's own LDS traffic, not a rendezvous.
//
// Ordering: parallel (round-robin) Jacobi. With m = N + (N & 1) and M = m - 1, round r = 0 .. M-1 holds the pairs
//   slot 0:            (r, M)                          (N even; for N odd index M = N does not exist: r sits out)
//   slot k = 1..m/2-1: ((r + k) mod M, (r - k) mod M)
// which are disjoint and cover every pair once per sweep. Per round, three phases with a barrier after each:
//   1. lane k computes the rotation of slot k from the pre-round matrix (w, tau, t, c, s);
//   2. columns of H and of V: item (row r, slot k) reads [r][p] and [r][q] and writes both (no item touches another's);
//   3. rows of H: item (slot k, column j) reads [p][j] and [q][j] and writes both; the items j = p and j = q set the
//      annihilated pair to exactly 0 and the two diagonal entries to exactly real.
// Stop: off-diagonal Frobenius norm <= 4 eps ||H||_F, checked before every sweep, 40 sweeps at most.
//
// LDS (N = 24: 24.5 KiB): H and V as [N][LD] double2 with LD odd (a column walk then spreads over all sixteen 16-byte
// slots of a bank row), the slots' rotations, N*N doubles of occupation partial sums, the diagonal. After the last
// sweep the H region becomes the output staging (eigenvectors in output order, contiguous) and the V region the
// problem's density matrix; every global store has consecutive lanes on consecutive elements.
#include "pqd_common.h"
#include <algorithm>
#include <cfloat>

namespace {

constexpr int DW_THREADS = PQD_WAVE;            // one wave, one problem
constexpr int DW_MAX_SWEEPS = 40;
constexpr long long DW_MAX_BLOCKS = 1LL << 16;  // 8 times the waves the chip holds; larger batches loop

// the same bits in every lane (each step adds the same pair)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int w = 1; w < PQD_WAVE; w <<= 1) v += __shfl_xor(v, w);
    return v;
}

// The kernel is a chain of dependent LDS round trips, so waves per CU pay: up to N = 20 the LDS leaves room for 9 or
// more workgroups per CU, and three waves per SIMD (168 VGPRs; N = 16..19 then spill 2-14 of them) beat two
// (39.5 -> 31.3 ms at N = 16, 63.8 -> 57.6 ms at N = 18). Above, the LDS holds 6-8 workgroups anyway.
template <int N>
__global__ __launch_bounds__(DW_THREADS, (N <= 20 ? 3 : 2)) void dressed_wide_kernel(DressedParams p) {
    constexpr int LD = N | 1;                   // odd row stride
    constexpr int M = N + (N & 1) - 1;          // rounds per sweep; the circle's fixed index
    constexpr int K0 = N & 1;                   // first live slot (slot 0 holds the missing index when N is odd)
    constexpr int NS = (N + (N & 1)) / 2;       // slots per round
    constexpr int NK = NS - K0;                 // live slots = N / 2
    __shared__ __attribute__((aligned(16))) double2 A[N * LD];
    __shared__ __attribute__((aligned(16))) double2 V[N * LD];
    __shared__ __attribute__((aligned(16))) double2 r_sw[NS];  // s w of the slot's rotation
    __shared__ double r_c[NS];
    __shared__ int r_p[NS], r_q[NS], r_on[NS];
    __shared__ double part[N * N];
    __shared__ double dg[N], st_val[N];

    const int lane = threadIdx.x;
    const long long n_t = (long long)p.n_steps + 1;
    const long long total = (long long)p.n_sys * n_t;

    for (long long prob = blockIdx.x; prob < total; prob += gridDim.x) {
        // ---- 1. H(t_n), made exactly Hermitian: (H[r][c] + conj(H[c][r])) / 2; V = 1
        {
            const int si = (int)(prob / n_t);
            const int n = (int)(prob - (long long)si * n_t);
            const DressedSys sy = p.systems[si];
            const double t = p.ta + (double)n * p.dt;
            double2 f[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) f[ch] = ch < sy.n_chan ? sample_ch(sy, ch, t) : c_zero();
            for (int e = lane; e < N * N; e += DW_THREADS) {
                const int r = e / N, c = e - r * N;
                const double2 a = sy.H0[r * N + c], b = sy.H0[c * N + r];
                double2 h = make_double2(a.x + b.x, a.y - b.y);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch)
                    if (ch < sy.n_chan) {
                        const double2* X = sy.X + (size_t)ch * N * N;
                        // (f X + conj(f) X^dagger)[r][c] = f X[r][c] + conj(f X[c][r]); twice its Hermitian part
                        const double2 u = c_mul(f[ch], X[r * N + c]), v = c_mul(f[ch], X[c * N + r]);
                        h.x += 2.0 * (u.x + v.x);
                        h.y += 2.0 * (u.y - v.y);
                    }
                h = c_scale(h, 0.5);
                if (r == c) h.y = 0.0;
                A[r * LD + c] = h;
                V[r * LD + c] = make_double2(r == c ? 1.0 : 0.0, 0.0);
            }
        }
        __syncthreads();

        // ---- 2. round-robin Jacobi
        double mine = 0.0;
        for (int e = lane; e < N * N; e += DW_THREADS) {
            const int r = e / N, c = e - r * N;
            const double2 a = A[r * LD + c];
            mine += a.x * a.x + a.y * a.y;
        }
        const double norm2 = wave_sum(mine);
        const bool finite = norm2 <= DBL_MAX;   // false for Inf and NaN
        const double thr = 4.0 * DBL_EPSILON * sqrt(norm2);
        bool done = !finite;
        for (int sweeps = 0;; ++sweeps) {
            double off = 0.0;
            for (int e = lane; e < N * N; e += DW_THREADS) {
                const int r = e / N, c = e - r * N;
                const double2 a = A[r * LD + c];
                off += r == c ? 0.0 : a.x * a.x + a.y * a.y;
            }
            off = sqrt(wave_sum(off));
            if (off <= thr) done = true;
            if (done || sweeps == DW_MAX_SWEEPS) break;   // uniform: every lane holds the same bits of off
            for (int rd = 0; rd < M; ++rd) {
                // phase 1: the slots' rotations from the pre-round matrix
                if (lane >= K0 && lane < NS) {
                    int a, b;
                    if (lane == 0) { a = rd; b = M; }
                    else { a = rd + lane; a -= a >= M ? M : 0; b = rd - lane; b += b < 0 ? M : 0; }
                    const int P = a < b ? a : b, Q = a < b ? b : a;
                    const double2 apq = A[P * LD + Q];
                    const double app = A[P * LD + P].x, aqq = A[Q * LD + Q].x;
                    const double m = hypot(apq.x, apq.y);
                    const bool on = m > 0.0;    // nothing to annihilate (also a NaN element: flagged below)
                    double c = 1.0;
                    double2 sw = c_zero();
                    if (on) {
                        const double2 w = make_double2(apq.x / m, apq.y / m);
                        const double tau = (aqq - app) / (2.0 * m);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        const double s = t * c;
                        sw = make_double2(s * w.x, s * w.y);
                    }
                    r_p[lane] = P; r_q[lane] = Q; r_on[lane] = on ? 1 : 0; r_c[lane] = c; r_sw[lane] = sw;
                }
                __syncthreads();
                // phase 2: columns of H and V: col_P' = c col_P - s conj(w) col_Q, col_Q' = s w col_P + c col_Q
                for (int e = lane; e < 2 * N * NK; e += DW_THREADS) {
                    const int h = e / (N * NK), e2 = e - h * (N * NK);
                    const int k = e2 / N, r = e2 - k * N;
                    const int sl = k + K0;
                    if (!r_on[sl]) continue;
                    double2* Mx = (h ? V : A) + r * LD;
                    const int P = r_p[sl], Q = r_q[sl];
                    const double c = r_c[sl];
                    const double2 sw = r_sw[sl];
                    const double2 x = Mx[P], y = Mx[Q];
                    double2 np = c_scale(x, c), nq = c_scale(y, c);
                    c_fma(np, make_double2(-sw.x, sw.y), y);
                    c_fma(nq, sw, x);
                    Mx[P] = np;
                    Mx[Q] = nq;
                }
                __syncthreads();
                // phase 3: rows of H: row_P' = c row_P - s w row_Q, row_Q' = s conj(w) row_P + c row_Q
                for (int e = lane; e < NK * N; e += DW_THREADS) {
                    const int k = e / N, j = e - k * N;
                    const int sl = k + K0;
                    if (!r_on[sl]) continue;
                    const int P = r_p[sl], Q = r_q[sl];
                    const double c = r_c[sl];
                    const double2 sw = r_sw[sl];
                    const double2 x = A[P * LD + j], y = A[Q * LD + j];
                    double2 np = c_scale(x, c), nq = c_scale(y, c);
                    c_fma(np, make_double2(-sw.x, -sw.y), y);
                    c_fma(nq, make_double2(sw.x, -sw.y), x);
                    // the annihilated pair is exactly zero, the diagonal exactly real
                    if (j == P) { nq = c_zero(); np.y = 0.0; }
                    if (j == Q) { np = c_zero(); nq.y = 0.0; }
                    A[P * LD + j] = np;
                    A[Q * LD + j] = nq;
                }
                __syncthreads();
            }
        }
        if (lane == 0 && (!finite || !done)) atomicOr(p.flags, finite ? 2u : 1u);

        // ---- 3. order, norm, phase: lane c takes column c; the H region becomes the staging, in output order
        if (lane < N) dg[lane] = A[lane * LD + lane].x;
        __syncthreads();
        double2* st = A;   // [rank][component], contiguous
        if (lane < N) {
            const int col = lane;
            const double d = dg[col];
            int rank = 0;
            for (int j = 0; j < N; ++j) {
                const double dj = dg[j];
                rank += (dj < d || (dj == d && j < col)) ? 1 : 0;
            }
            double nv = 0.0;
            for (int r = 0; r < N; ++r) {
                const double2 v = V[r * LD + col];
                nv += v.x * v.x + v.y * v.y;
            }
            const double inv = nv > 0.0 ? 1.0 / sqrt(nv) : 0.0;
            bool found = false;
            double2 ph = make_double2(1.0, 0.0);
            for (int r = 0; r < N; ++r) {
                const double2 v = c_scale(V[r * LD + col], inv);
                const double m = hypot(v.x, v.y);
                if (!found && m > 1e-12) {
                    found = true;
                    ph = make_double2(v.x / m, -v.y / m);
                }
            }
            found = false;
            for (int r = 0; r < N; ++r) {
                const double2 v = c_scale(V[r * LD + col], inv);
                const double m = hypot(v.x, v.y);
                const bool lead = !found && m > 1e-12;
                found = found || lead;
                const double2 z = c_mul(v, ph);
                st[rank * N + r] = lead ? make_double2(m, 0.0) : z;
            }
            st_val[rank] = d;
        }
        __syncthreads();
        if (p.evecs)
            for (int e = lane; e < N * N; e += DW_THREADS) p.evecs[(size_t)prob * N * N + e] = st[e];
        if (p.evals && lane < N) p.evals[(size_t)prob * N + lane] = st_val[lane];

        // ---- 4. occupations: occ[j] = Re sum_i v_j[i] sum_k conj(v_j[k]) R[i][k]; the V region holds R
        if (p.occ) {
            const double2* R = p.rho + (size_t)prob * N * N;
            for (int e = lane; e < N * N; e += DW_THREADS) {
                const int i = e / N, k = e - i * N;
                V[i * LD + k] = R[e];
            }
            __syncthreads();
            for (int e = lane; e < N * N; e += DW_THREADS) {
                const int j = e / N, i = e - j * N;
                double2 ti = c_zero();
                for (int k = 0; k < N; ++k) c_fma(ti, c_conj(st[j * N + k]), V[i * LD + k]);
                const double2 vi = st[j * N + i];
                part[e] = vi.x * ti.x - vi.y * ti.y;
            }
            __syncthreads();
            if (lane < N) {
                double oc = 0.0;
                for (int i = 0; i < N; ++i) oc += part[lane * N + i];
                p.occ[(size_t)prob * N + lane] = oc;
            }
        }
        __syncthreads();
    }
}

template <int N>
hipError_t launch_dressed_wide_n(const DressedParams& p, hipStream_t s) {
    const long long total = (long long)p.n_sys * ((long long)p.n_steps + 1);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(dressed_wide_kernel<N>, dim3((unsigned)std::min(total, DW_MAX_BLOCKS)), dim3(DW_THREADS), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dressed_wide(int N, const DressedParams& p, hipStream_t s) {
    switch (N) {
#define DW_CASE(n) case n: return launch_dressed_wide_n<n>(p, s);
        DW_CASE(7) DW_CASE(8) DW_CASE(9) DW_CASE(10) DW_CASE(11) DW_CASE(12) DW_CASE(13) DW_CASE(14) DW_CASE(15)
        DW_CASE(16) DW_CASE(17) DW_CASE(18) DW_CASE(19) DW_CASE(20) DW_CASE(21) DW_CASE(22) DW_CASE(23) DW_CASE(24)
#undef DW_CASE
        default: return hipErrorInvalidValue;
    }
}
