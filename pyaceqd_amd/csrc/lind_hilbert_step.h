// lind_hilbert_step.h — the Lindblad step in Hilbert space, once: the device code that lind_hilbert.hip (one
// trajectory per workgroup) and lind_hilbert_pt.hip (one bond slice per group of threads) both run. Only these two
// files include it. Every function is inlined into its caller; the callers keep their LDS maps, their loops over steps
// and slices, and the barriers around these calls.
//
// A factor exp(L(t_mid) w) is applied to rho, never built:
//   L(rho) = K rho + rho K^dag + sum_k gamma_k A_k rho A_k^dag,    K(t) = K0 + sum_p (f_p Xs_p + conj(f_p) Xt_p)
// (K0, Xs, Xt: HilbertSys; the Liouvillian of commutator / dissipator in pqd_host.cpp), as s scaled Taylor series
//   exp(L w) rho = (exp(L w / s))^s rho,    exp(L c) rho = sum_{m <= deg} c^m L^m rho / m!,  c = w / s.
// s and deg come from a bound of ||L w|| in the Frobenius norm of rho, ||K rho|| <= ||K||_F ||rho||_F and
// ||A rho A^dag|| <= ||A||_F^2 ||rho||_F:
//   theta = w (2 (||K0|| + sum_p |f_p(t_mid)| (||Xs_p|| + ||Xt_p||)) + sum_k |gamma_k| ||A_k||^2)
// s = ceil(theta) (at least 1, at most HB_SMAX), x = theta / s <= 1, deg = the smallest m <= HB_DEGMAX with
// x^(m+1) / (m+1)! (m+2) / (m+2-x) < 2^-56 (the remainder rule of free_prop.hip; x = 1 gives 18). Both depend on the
// system and the time only, never on rho, so every trajectory and every bond slice of a system runs the same
// arithmetic and its outputs are the same bits in any batch. A non-finite theta takes s = 1, deg = HB_DEGMAX: the
// kernel ends, the outputs are not finite, and pqd_plan_synchronize reports PQD_ERR_NUMERIC. Plan creation refuses a
// finite bound above HB_SMAX (pqd_host.cpp), so the cap on s is never what a finished run depended on.
//
// Thread e = i N + j of a matrix's owners holds element (i, j) of every matrix. One Taylor term is two passes:
//   1. B_k = A_k T for every jump operator, from the operator's nonzeros by rows;
//   2. Tn = c/m (K T + T K^dag + sum_k B_k (gamma_k A_k^dag)), R += Tn   (gamma_k conj(A_k) by the rows of A_k: valg),
// with a barrier after each. Jump operators are held as nonzero lists (a reference model's has at most N entries; a
// dense one has N^2 and costs N times as much, with the same code); a thread keeps the bounds of its two rows of every
// list (row i for pass 1, row j for pass 2) in registers. The lists are read from LDS when every system's fit
// HB_CSR_LDS bytes, else from global memory. Kd = K(t)^dag is kept beside K so that both products read consecutive
// addresses across lanes.
#pragma once
#include "pqd_common.h"

static_assert(HB_CSR_LDS % 16 == 0, "the nonzero lists start on a 16-byte boundary");

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

// the nonzero lists of a system's jump operators (HilbertSys: val, valg, col, rowptr)
struct HbLists {
    const double2* val;
    const double2* valg;
    const int* col;
    const int* rowptr;
};

// CSR_LDS: all nt threads copy the lists into LDS behind `base` (hilbert_csr_bytes: values, gamma conj(values),
// columns, row offsets); the caller's next barrier completes them. Else the global arrays.
template <bool CSR_LDS>
__device__ __forceinline__ HbLists hb_lists(const HilbertSys& sy, int nl, int N, double2* base, int tid, int nt) {
    if constexpr (CSR_LDS) {
        double2* lv = base;
        double2* lg = lv + sy.nnz;
        int* lc = reinterpret_cast<int*>(lg + sy.nnz);
        int* lr = lc + sy.nnz;
        for (int z = tid; z < sy.nnz; z += nt) { lv[z] = sy.val[z]; lg[z] = sy.valg[z]; lc[z] = sy.col[z]; }
        for (int z = tid; z < nl * (N + 1); z += nt) lr[z] = sy.rowptr[z];
        return {lv, lg, lc, lr};
    }
    return {sy.val, sy.valg, sy.col, sy.rowptr};
}

// the thread's rows of every jump operator's list: row i (pass 1), row j (pass 2)
struct HbRows {
    int ib[HB_LMAX], ie[HB_LMAX], jb[HB_LMAX], je[HB_LMAX];
};
__device__ __forceinline__ void hb_rows(HbRows& r, const int* rowptr, int nl, int N, int i, int j) {
#pragma unroll
    for (int k = 0; k < HB_LMAX; ++k) {
        r.ib[k] = r.ie[k] = r.jb[k] = r.je[k] = 0;
        if (k < nl) {
            const int* rp = rowptr + k * (N + 1);
            r.ib[k] = rp[i]; r.ie[k] = rp[i + 1]; r.jb[k] = rp[j]; r.je[k] = rp[j + 1];
        }
    }
}

// trajectory t: its output window, its events and its start time (MAP: HilbertParams, map mode), and the sub-step
struct HbTraj {
    int wb, we;
    long long wo;
    int ev_cur, ev_lim;
    double ta;
    int nsub;
    double w;  // dt / (2 n_sub)
};
template <bool MAP>
__device__ __forceinline__ HbTraj hb_traj(const HilbertParams& p, int t, int NN) {
    HbTraj r;
    r.wb = MAP ? 0 : p.wbeg[t];
    r.we = MAP ? p.map_steps : p.wend[t];
    r.wo = MAP ? (long long)t * p.map_steps * NN : p.woff[t];
    r.ev_cur = MAP ? 0 : p.ev_start[t];
    r.ev_lim = MAP ? p.map_nev : p.ev_start[t + 1];
    r.ta = MAP ? p.map_ta[t / NN] : p.ta;
    r.nsub = p.n_sub > 0 ? p.n_sub : 1;
    r.w = 0.5 * p.dt / r.nsub;
    return r;
}

// factors s and degree deg from the norm bound (header): uniform over the workgroup, independent of rho
__device__ __forceinline__ void hb_factor_rule(double theta, int& s, int& deg) {
    s = 1;
    deg = HB_DEGMAX;
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
}

// R <- (sum_{m <= deg} (cw L)^m / m!)^s R on one matrix, thread e = i N + j its element (act: the thread has one).
// K and Kd are complete on entry; the last barrier leaves R complete. 1 + deg (2 with jump operators, else 1) barriers
// a factor, the same for every thread of the workgroup. T and Tn trade places after every term: a factor opens with
// T = R, so which of the two buffers is which on entry never reaches a value.
__device__ __forceinline__ void hb_factors(bool act, int e, int i, int j, int N, int nl, double2* R, double2* T,
                                           double2* Tn, const double2* K, const double2* Kd, double2* B,
                                           const HbLists& L, const HbRows& r, int s, int deg, double cw) {
    const int NN = N * N;
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
                            for (int z = r.ib[k]; z < r.ie[k]; ++z) c_fma(acc, L.val[z], T[L.col[z] * N + j]);
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
                        for (int z = r.jb[k]; z < r.je[k]; ++z) c_fma(acc, Bk[L.col[z]], L.valg[z]);
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

// the output sums of the NN elements at src: wave v sums outputs v, v + n_waves, ...: lanes over the elements, then a
// butterfly (the same order in every run, whichever wave takes an output). out: the trajectory's n_out values of the step
__device__ __forceinline__ void hb_readout(const HilbertParams& p, const double2* src, int NN, int tid, int nt,
                                           double2* out) {
    const int lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    for (int k = wave; k < p.n_out; k += n_waves) {
        const double2* ov = p.ovec + (size_t)k * NN;
        double2 s = c_zero();
        for (int a = lane; a < NN; a += 64) c_fma(s, ov[a], src[a]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s = c_add(s, c_shfl_xor(s, m));
        if (lane == 0) out[k] = s;
    }
}

// element (i, j) of an MTO's result from the matrix at src (complete on entry): A src A^dag (kind 0), A src (1),
// src A (2). Kind 0 goes through T, with one barrier that every thread of the workgroup reaches (kind is uniform)
__device__ __forceinline__ double2 hb_mto(const double2* A, int kind, bool act, const double2* src, double2* T, int e,
                                          int N, int i, int j) {
    double2 v = c_zero();
    if (act) v = kind == 2 ? hb_dense<HB_RIGHT>(A, src, N, i, j) : hb_dense<HB_LEFT>(A, src, N, i, j);
    if (kind == 0) {  // (A src) A^dag through T
        if (act) T[e] = v;
        __syncthreads();
        if (act) v = hb_dense<HB_RIGHT_DAG>(A, T, N, i, j);
    }
    return v;
}
