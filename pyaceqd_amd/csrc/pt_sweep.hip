// pt_sweep.hip — the hot path: lock-step propagation of a batch of trajectories through the
// process-tensor MPO (PT contraction + symmetric-Trotter free half steps + MTOs + output traces).
//
// Replaces the per-step loop inside the external ACE binary that pyaceqd drives through
// system_ace_stream (general_system.py:227-343) and fans out one OS process per trajectory in the
// two-time sweeps (two_time/correlations.py:135-184, pol_entanglement/G2.py:439-533, ...).
//
// Work decomposition (MI355X: 256 CUs, 160 KiB LDS/CU, 64-wide waves, FP64 VALU = FP64 MFMA peak):
//   * one workgroup owns BT trajectories (8 at N2 <= 16, else 4) for the whole time range (persistent over
//     steps, no inter-workgroup traffic: trajectories are independent); 8 waves per workgroup (one per
//     trajectory at BT = 8, two per trajectory at BT = 4 and chi >= 32, see sweep_wpt);
//   * the augmented states Q_b[alpha][d] (N2 x CHI complex doubles, 16 KiB each at N=4, chi=64) stay
//     resident in LDS, rows padded to CHI+1 so column reads and row reads are bank-conflict free;
//   * free half steps / MTOs (N2 x N2 operator applied to every bond column): the waves of a trajectory
//     run the complex GEMM M . Q on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, 3 real MFMAs per complex
//     tile by default), no cross-wave traffic, no barrier inside the phase; steps without MTOs apply the
//     fused operator F(n) = M_a(n) M_b(n-1) once;
//   * PT contraction (row alpha of all BT trajectories times the chi x chi slice Q[g(alpha)]): waves take the
//     rows (or up to 4 rows sharing a dictionary slice) of a host-built unit list; v_mfma_f64_4x4x4_4b with
//     3 real products per complex product, every slice element read from L2 once per workgroup and step;
//   * closure + output traces only on steps inside some trajectory's output window.
// All PT slices / free propagators are shared by every workgroup at the same absolute step, so the
// dominant traffic is L2/MALL-resident; the kernel is FP64 matrix-core bound.
#include "pqd_common.h"
#include <climits>
#include <type_traits>

namespace {

template <int N2, int CHI, int BT>
struct SweepLayout {
    static constexpr int RS = CHI + 1;          // row stride (double2)
    static constexpr int TS = N2 * RS + 4;      // trajectory stride (+64 B: shifts banks per trajectory)
    static constexpr int KD = CHI / 16;         // PT output columns per lane
    static constexpr int NCOL = BT * CHI;       // column-phase work items
    static constexpr int WPT = sweep_wpt(N2, BT, CHI);  // waves per trajectory
    static constexpr int NW = BT * WPT;             // waves per workgroup
    static constexpr size_t LDS = (size_t)(BT * TS + BT * N2) * sizeof(double2);
};

typedef double dbl4 __attribute__((ext_vector_type(4)));

// load of launch-constant metadata at a wave-uniform address through the scalar cache
__device__ __forceinline__ int ldc(const int* q) { return *(const __attribute__((address_space(4))) int*)q; }
__device__ __forceinline__ int4 ldc(const int4* q) {
    const int* w = (const int*)q;
    return make_int4(ldc(w), ldc(w + 1), ldc(w + 2), ldc(w + 3));
}

// Column phase on the matrix cores: one wave applies the N2 x N2 operator Op (row-major, complex) to
// all CHI bond columns of its trajectory's augmented state S (LDS, row stride RS):
//   C[N2 x CHI] = Op[N2 x N2] . S[N2 x CHI]   as v_mfma_f64_16x16x4_f64 tiles,
// complex = 4 real MFMAs (Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br). Fragment maps (gfx950 f64):
// A[i = l&15][k = l>>4], B[k = l>>4][j = l&15], C[i = (l>>4) + 4 r][j = l&15].
// Column tiles are the outer loop, so each 16-column tile is read completely before it is written
// back in place. With WPT waves per trajectory, wave `half` takes every WPT-th tile (columns are
// independent). Rows/k beyond N2 are zero padding (N2 = 4, 9, 25, 36).
template <int N2, int CHI, int RS, int WPT = 1>
__device__ __forceinline__ void col_apply_mfma(const double2* __restrict__ Op, double2* S, int lane, int half = 0) {
    constexpr int MT = (N2 + 15) / 16;   // output row tiles
    constexpr int KS = (N2 + 3) / 4;     // k steps
    constexpr int NTL = CHI / 16;        // column tiles
    constexpr bool CACHE_A = KS * MT <= 8;
    constexpr int KSU = CACHE_A ? KS : 3;   // large N2: bounded unroll keeps the operator loads out of VGPRs
    const int li = lane & 15, lk = lane >> 4;
    double2 ac[CACHE_A ? KS * MT : 1];
    if constexpr (CACHE_A) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int r = 16 * mt + li, a = 4 * ks + lk;
                ac[ks * MT + mt] = (r < N2 && a < N2) ? Op[r * N2 + a] : c_zero();
            }
    }
#pragma unroll
    for (int j = 0; j < NTL / WPT; ++j) {   // this wave's column tiles: half, half + WPT, ...
        const int nt = j * WPT + half;
        dbl4 cr[MT], ci[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { cr[mt] = dbl4{0, 0, 0, 0}; ci[mt] = dbl4{0, 0, 0, 0}; }
#pragma unroll KSU
        for (int ks = 0; ks < KS; ++ks) {
            const int a = 4 * ks + lk;
            const double2 b = (a < N2) ? S[a * RS + 16 * nt + li] : c_zero();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                double2 m;
                if constexpr (CACHE_A) {
                    m = ac[ks * MT + mt];
                } else {
                    const int r = 16 * mt + li;
                    m = (r < N2 && a < N2) ? Op[r * N2 + a] : c_zero();
                }
                cr[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(m.x, b.x, cr[mt], 0, 0, 0);
                cr[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(-m.y, b.y, cr[mt], 0, 0, 0);
                ci[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(m.x, b.y, ci[mt], 0, 0, 0);
                ci[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(m.y, b.x, ci[mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + lk + 4 * r;
                if (row < N2) S[row * RS + 16 * nt + li] = make_double2(cr[mt][r], ci[mt][r]);
            }
    }
    // the next operator of this wave re-reads what other lanes just wrote
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Column phase with three real products per complex product ("3M"): P1 = Ar Br, P2 = Ai Bi,
// P3 = (Ar + Ai)(Br + Bi); Cr = P1 - P2, Ci = P3 - P1 - P2. Three MFMA chains instead of four, the sums are
// two VALU adds per operand fragment. Error bound eps (|Ar||Br| + |Ai||Bi| + |Ar + Ai||Br + Bi|) per product,
// i.e. the same order as the 4M form for these O(1) propagators.
template <int N2, int CHI, int RS, int WPT = 1>
__device__ __forceinline__ void col_apply_mfma3(const double2* __restrict__ Op, double2* S, int lane, int half = 0) {
    constexpr int MT = (N2 + 15) / 16;
    constexpr int KS = (N2 + 3) / 4;
    constexpr int NTL = CHI / 16;
    constexpr bool CACHE_A = KS * MT <= 8;
    constexpr int KSU = CACHE_A ? KS : 3;   // large N2: bounded unroll keeps the operator loads out of VGPRs
    const int li = lane & 15, lk = lane >> 4;
    double2 ac[CACHE_A ? KS * MT : 1];
    double as[CACHE_A ? KS * MT : 1];
    if constexpr (CACHE_A) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int r = 16 * mt + li, a = 4 * ks + lk;
                ac[ks * MT + mt] = (r < N2 && a < N2) ? Op[r * N2 + a] : c_zero();
                as[ks * MT + mt] = ac[ks * MT + mt].x + ac[ks * MT + mt].y;
            }
    }
#pragma unroll
    for (int j = 0; j < NTL / WPT; ++j) {   // this wave's column tiles: half, half + WPT, ...
        const int nt = j * WPT + half;
        dbl4 p1[MT], p2[MT], p3[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { p1[mt] = dbl4{0, 0, 0, 0}; p2[mt] = p1[mt]; p3[mt] = p1[mt]; }
#pragma unroll KSU
        for (int ks = 0; ks < KS; ++ks) {
            const int a = 4 * ks + lk;
            const double2 b = (a < N2) ? S[a * RS + 16 * nt + li] : c_zero();
            const double bs = b.x + b.y;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                double2 m;
                double ms;
                if constexpr (CACHE_A) {
                    m = ac[ks * MT + mt];
                    ms = as[ks * MT + mt];
                } else {
                    const int r = 16 * mt + li;
                    m = (r < N2 && a < N2) ? Op[r * N2 + a] : c_zero();
                    ms = m.x + m.y;
                }
                p1[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(m.x, b.x, p1[mt], 0, 0, 0);
                p2[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(m.y, b.y, p2[mt], 0, 0, 0);
                p3[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ms, bs, p3[mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + lk + 4 * r;
                if (row < N2)
                    S[row * RS + 16 * nt + li] = make_double2(p1[mt][r] - p2[mt][r], p3[mt][r] - p1[mt][r] - p2[mt][r]);
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// col_apply_mfma3 for large N2 (25, 36: the operator's fragments do not fit in VGPRs): all of this wave's column tiles
// in one pass over k, so every operator fragment is loaded from L2 once per call instead of once per tile, with the
// next k-step's fragments in flight while the current one's MFMAs run (the per-tile loop waited on each load:
// six-level scan, column phases ~24 us per step against ~9 us of MFMA work). Accumulators: 3 MT NTW tiles <= 18.
template <int N2, int CHI, int RS, int WPT>
constexpr bool col_big_ok() {
    return (N2 + 3) / 4 * ((N2 + 15) / 16) > 8 && 3 * ((N2 + 15) / 16) * (CHI / 16 / WPT) <= 18;
}
template <int N2, int CHI, int RS, int WPT>
__device__ __forceinline__ void col_apply_mfma3_big(const double2* __restrict__ Op, double2* S, int lane, int half) {
    constexpr int MT = (N2 + 15) / 16;
    constexpr int KS = (N2 + 3) / 4;
    constexpr int NTW = CHI / 16 / WPT;   // this wave's column tiles: half, half + WPT, ...
    const int li = lane & 15, lk = lane >> 4;
    dbl4 p1[MT][NTW], p2[MT][NTW], p3[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NTW; ++j) { p1[mt][j] = dbl4{0, 0, 0, 0}; p2[mt][j] = p1[mt][j]; p3[mt][j] = p1[mt][j]; }
    auto ldm = [&](int ks, int mt) {
        const int r = 16 * mt + li, a = 4 * ks + lk;
        return (r < N2 && a < N2) ? Op[r * N2 + a] : c_zero();
    };
    double2 mn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) mn[mt] = ldm(0, mt);
#pragma unroll 3
    for (int ks = 0; ks < KS; ++ks) {
        double2 m[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) m[mt] = mn[mt];
        if (ks + 1 < KS) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) mn[mt] = ldm(ks + 1, mt);
        }
        const int a = 4 * ks + lk;
        double2 b[NTW];
        double bs[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            b[j] = (a < N2) ? S[a * RS + 16 * (j * WPT + half) + li] : c_zero();
            bs[j] = b[j].x + b[j].y;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const double ms = m[mt].x + m[mt].y;
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                p1[mt][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[mt].x, b[j].x, p1[mt][j], 0, 0, 0);
                p2[mt][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(m[mt].y, b[j].y, p2[mt][j], 0, 0, 0);
                p3[mt][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ms, bs[j], p3[mt][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * mt + lk + 4 * r;
                if (row < N2)
                    S[row * RS + 16 * (j * WPT + half) + li] =
                        make_double2(p1[mt][j][r] - p2[mt][j][r], p3[mt][j][r] - p1[mt][j][r] - p2[mt][j][r]);
            }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// PT contraction of one Liouville row alpha on the matrix cores (v_mfma_f64_4x4x4_4b_f64):
//   C[BT x CHI] = X[BT x CHI] . Qg[CHI x CHI],  X = rows alpha of the BT trajectories.
// gfx950 lane map of the 4-block f64 MFMA (measured): lane l = 16 k + 4 blk + x holds A[blk][x][k],
// B[blk][k][x], D[blk][l>>4][x]. The 4 blocks of one instruction are 4 consecutive 4-column tiles,
// so lane l reads Qg[4 ks + (l>>4)][16 grp + (l & 15)] (256 contiguous bytes per 16 lanes) and ends up
// owning C[4 rb + (l>>4)][16 grp + (l & 15)]: no cross-lane reduction. Complex = 4 real MFMAs.
template <int CHI, int BT, int RS, int TS>
__device__ __forceinline__ void pt_row_mfma(const double2* __restrict__ Qg, double2* st, int a, int lane) {
    constexpr int RB = BT / 4, NG = CHI / 16, KSN = CHI / 4;
    const int x = lane & 3, kk = lane >> 4, c16 = lane & 15;
    double cr[RB][NG], ci[RB][NG];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int g = 0; g < NG; ++g) { cr[rb][g] = 0.0; ci[rb][g] = 0.0; }
    const double2* xr = st + a * RS + kk;          // + b*TS + 4 ks
    const double2* qp = Qg + (size_t)kk * CHI + c16;  // + 4 ks * CHI + 16 g
    double2 qn[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) qn[g] = qp[16 * g];
#pragma unroll 2
    for (int ks = 0; ks < KSN; ++ks) {
        double2 qv[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) qv[g] = qn[g];
        if (ks + 1 < KSN) {
#pragma unroll
            for (int g = 0; g < NG; ++g) qn[g] = qp[(size_t)4 * (ks + 1) * CHI + 16 * g];
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const double2 av = xr[(4 * rb + x) * TS + 4 * ks];
            const double ai_neg = -av.y;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                cr[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av.x, qv[g].x, cr[rb][g], 0, 0, 0);
                cr[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(ai_neg, qv[g].y, cr[rb][g], 0, 0, 0);
                ci[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av.x, qv[g].y, ci[rb][g], 0, 0, 0);
                ci[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av.y, qv[g].x, ci[rb][g], 0, 0, 0);
            }
        }
    }
    double2* wr = st + a * RS + c16;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int g = 0; g < NG; ++g) wr[(4 * rb + kk) * TS + 16 * g] = make_double2(cr[rb][g], ci[rb][g]);
}

// The same row on the VALU: lane l = 16 q + j accumulates input quarter q (bond indices 4 kk + q) of the KD = CHI / 16
// output columns j + 16 i of every trajectory, then the quarters are summed across the lanes.
template <int CHI, int BT, int RS, int TS, int KD>
__device__ __forceinline__ void pt_row_valu(const double2* __restrict__ Qg, double2* st, int a, int lane) {
    const int pj = lane & 15, pq = lane >> 4;
    Qg += pj;
    const double2* xr = st + a * RS + pq;
    double2 acc[BT][KD];
#pragma unroll
    for (int b = 0; b < BT; ++b)
#pragma unroll
        for (int i = 0; i < KD; ++i) acc[b][i] = c_zero();
    double2 qn[KD];
#pragma unroll
    for (int i = 0; i < KD; ++i) qn[i] = Qg[(size_t)pq * CHI + 16 * i];
#pragma unroll 2
    for (int kk = 0; kk < CHI / 4; ++kk) {
        double2 qv[KD];
#pragma unroll
        for (int i = 0; i < KD; ++i) qv[i] = qn[i];
        if (kk + 1 < CHI / 4) {
            const int dn = 4 * (kk + 1) + pq;
#pragma unroll
            for (int i = 0; i < KD; ++i) qn[i] = Qg[(size_t)dn * CHI + 16 * i];
        }
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const double2 x = xr[b * TS + 4 * kk];
#pragma unroll
            for (int i = 0; i < KD; ++i) c_fma(acc[b][i], x, qv[i]);
        }
    }
    // reduce the 4 input quarters (lanes j, j+16, j+32, j+48) and scatter the columns
    double2* wr = st + a * RS + pj;
    if constexpr (KD == 4) {
        const bool q0 = pq & 1, q1 = (pq >> 1) & 1;
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            double2 h[2];
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const double2 mine = q0 ? acc[b][2 * pi + 1] : acc[b][2 * pi];
                const double2 oth = q0 ? acc[b][2 * pi] : acc[b][2 * pi + 1];
                h[pi] = c_add(mine, c_shfl_xor(oth, 16));
            }
            const double2 mine = q1 ? h[1] : h[0];
            const double2 oth = q1 ? h[0] : h[1];
            wr[b * TS + 16 * pq] = c_add(mine, c_shfl_xor(oth, 32));
        }
    } else if constexpr (KD == 2) {
        const bool q0 = pq & 1;
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const double2 mine = q0 ? acc[b][1] : acc[b][0];
            const double2 oth = q0 ? acc[b][0] : acc[b][1];
            double2 h = c_add(mine, c_shfl_xor(oth, 16));
            h = c_add(h, c_shfl_xor(h, 32));
            if (pq < 2) wr[b * TS + 16 * pq] = h;
        }
    } else {
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            double2 h = c_add(acc[b][0], c_shfl_xor(acc[b][0], 16));
            h = c_add(h, c_shfl_xor(h, 32));
            if (pq == 0) wr[b * TS] = h;
        }
    }
}

// pt_row_mfma with three real products per complex product (3M, see col_apply_mfma3): 3 MFMA chains per
// (row block, column group) instead of 4; (Qr + Qi) and (Xr + Xi) are one VALU add per loaded element.
// PF = how many k-steps of the PT slice are in flight ahead of the MFMAs (L2 latency hiding).
// R > 1 contracts R Liouville rows that share one PT slice (dictionary PTs: rows with the same
// coupling-eigenvalue pair) in one pass, so each slice element loaded from L2 feeds R times the MFMAs.
// a0..a3 = the R row indices (unused ones ignored).
// RBN <= BT / 4: only the first RBN row blocks (4 trajectories each) are contracted — the later ones are dormant
// shared-trunk slots (their rows are left as they are until the slot is activated, pqd_host.cpp branch_slots).
template <int CHI, int BT, int RS, int TS, int PF = 1, int R = 1, int RBN = BT / 4>
__device__ __forceinline__ void pt_row_mfma3(const double2* __restrict__ Qg, double2* st, int a0, int a1, int a2,
                                             int a3, int lane) {
    constexpr int RB = RBN, NG = CHI / 16, KSN = CHI / 4;
    const int x = lane & 3, kk = lane >> 4, c16 = lane & 15;
    double p1[R][RB][NG], p2[R][RB][NG], p3[R][RB][NG];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int g = 0; g < NG; ++g) { p1[r][rb][g] = 0.0; p2[r][rb][g] = 0.0; p3[r][rb][g] = 0.0; }
    const double2* xr[R];
    xr[0] = st + a0 * RS + kk;
    if constexpr (R >= 2) xr[1] = st + a1 * RS + kk;
    if constexpr (R >= 3) xr[2] = st + a2 * RS + kk;
    if constexpr (R >= 4) xr[3] = st + a3 * RS + kk;
    const double2* qp = Qg + (size_t)kk * CHI + c16;
    double2 qn[PF][NG];
#pragma unroll
    for (int f = 0; f < PF; ++f)
#pragma unroll
        for (int g = 0; g < NG; ++g) qn[f][g] = qp[(size_t)4 * f * CHI + 16 * g];
#pragma unroll PF + 1
    for (int ks = 0; ks < KSN; ++ks) {
        double2 qv[NG];
        double qs[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) { qv[g] = qn[0][g]; qs[g] = qv[g].x + qv[g].y; }
#pragma unroll
        for (int f = 0; f + 1 < PF; ++f)
#pragma unroll
            for (int g = 0; g < NG; ++g) qn[f][g] = qn[f + 1][g];
        if (ks + PF < KSN) {
#pragma unroll
            for (int g = 0; g < NG; ++g) qn[PF - 1][g] = qp[(size_t)4 * (ks + PF) * CHI + 16 * g];
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const double2 av = xr[r][(4 * rb + x) * TS + 4 * ks];
                const double as = av.x + av.y;
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    p1[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av.x, qv[g].x, p1[r][rb][g], 0, 0, 0);
                    p2[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av.y, qv[g].y, p2[r][rb][g], 0, 0, 0);
                    p3[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(as, qs[g], p3[r][rb][g], 0, 0, 0);
                }
            }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double2* wr = st + (r == 0 ? a0 : r == 1 ? a1 : r == 2 ? a2 : a3) * RS + c16;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int g = 0; g < NG; ++g)
                wr[(4 * rb + kk) * TS + 16 * g] = make_double2(p1[r][rb][g] - p2[r][rb][g],
                                                               p3[r][rb][g] - p1[r][rb][g] - p2[r][rb][g]);
    }
}

// a unit of n rows sharing one slice (n <= sweep_rmax: the accumulators stay within 48 doubles)
template <int N2, int CHI, int BT, int RS, int TS, int PF, int RBN>
__device__ __forceinline__ void pt_rows3_n(const double2* __restrict__ Qg, double2* st, int4 e, int lane) {
    constexpr int RM = sweep_rmax(N2, BT, CHI);
    if constexpr (RM >= 4) {
        if (e.w >= 0) {  // rows 2 (and 3) in the low (high) 16 bits of w
            const int a2 = e.w & 0xFFFF, a3 = e.w >> 16;
            if (a3 != 0x7FFF) pt_row_mfma3<CHI, BT, RS, TS, PF, 4, RBN>(Qg, st, e.y, e.z, a2, a3, lane);
            else pt_row_mfma3<CHI, BT, RS, TS, PF, 3, RBN>(Qg, st, e.y, e.z, a2, a2, lane);
            return;
        }
    }
    if constexpr (RM >= 2) {
        if (e.z >= 0) pt_row_mfma3<CHI, BT, RS, TS, PF, 2, RBN>(Qg, st, e.y, e.z, e.z, e.z, lane);
        else pt_row_mfma3<CHI, BT, RS, TS, PF, 1, RBN>(Qg, st, e.y, e.y, e.y, e.y, lane);
    } else {
        pt_row_mfma3<CHI, BT, RS, TS, PF, 1, RBN>(Qg, st, e.y, e.y, e.y, e.y, lane);
    }
}

// all rows of the workgroup, dormant shared-trunk slots included (their rows are overwritten at activation):
// skipping a dormant row block through a second instance (RBN = 1) cost 0.7% on the bench workload, where blocks
// are dormant for a few steps only (profiles/r02/ab_rbn.log)
template <int N2, int CHI, int BT, int RS, int TS, int PF>
__device__ __forceinline__ void pt_rows3(const double2* __restrict__ Qg, double2* st, int4 e, int lane) {
    pt_rows3_n<N2, CHI, BT, RS, TS, PF, BT / 4>(Qg, st, e, lane);
}

// The PT phase of the lean instance (chi = 64, BT = 8: two row blocks, four column groups, 16 k-steps): the wave's one
// or two units in one routine, the k-steps of a unit fully unrolled. Same MFMAs with the same operands in the same order
// per accumulator, the same operand sums and the same combine as pt_row_mfma3, so the results are bit-identical to it.
// What differs is where the non-MFMA instructions go (they cost matrix-pipe time on gfx950):
//   * slice loads: wave-uniform 64-bit base (slice of the step's set, k-step folded in) + one 32-bit lane offset `qoff`
//     computed before the step loop + the column group as the instruction's immediate: no vector address arithmetic;
//   * state rows: one LDS address per row block and row of the unit, k-steps through the DS immediate (64 B each);
//   * the accumulators are born in k-step 0 (zero C operand), no zeroing moves and no copies at the end of the loop;
//   * k-step ks issues the slice loads of ks + PF and the LDS reads of ks + 1 before its own MFMAs (sched_barrier keeps
//     the k-steps apart; the waits the compiler derives in straight-line code are counted and reach 0 only where
//     nothing else is in flight: a step's first and a wave's last k-step);
//   * a wave with two units loads the second unit's first PF k-steps in the first unit's last PF k-steps, so the slice
//     pipeline runs through the first unit's combine and LDS writes; a wave with one unit loads nothing more.
// Bounds: every slice load is base-of-slice + qoff + constant with qoff <= 3 * CHI * 16 + 15 * 16 and the constant
// 4 ks CHI 16 + 256 g for ks < KSN, g < NG (static_assert below: the largest address is the slice's last element), and
// the prefetch across units reads k-steps 0 .. PF - 1 of the second unit's own slice, only where that unit exists.
// Nothing is loaded beyond the slice a unit contracts, whichever slice of the PT's buffer that is.
// A unit also takes a functor it calls once, in its first k-step between the slice wait and the MFMAs: the fast region
// issues the staging of the next step's column operands there (LeanStage below), everything else passes LeanNoStage.
struct LeanNoStage {
    static constexpr bool ACTIVE = false;
    __device__ __forceinline__ void operator()() const {}
};
template <int CHI, int RS, int TS, int PF>
struct LeanPt {
    static constexpr int RB = 2, NG = CHI / 16, KSN = CHI / 4;
    static constexpr unsigned KSB = 4 * CHI * sizeof(double2);   // bytes per k-step of a slice
    static_assert(PF >= 1 && PF < KSN, "k-steps in flight");
    static_assert((KSN - 1) * KSB + (NG - 1) * 256 + 3 * CHI * sizeof(double2) + 15 * sizeof(double2) ==
                      (size_t)CHI * CHI * sizeof(double2) - sizeof(double2), "the last load ends with the slice");

    typedef __attribute__((address_space(1))) char GlobalBytes;
    typedef double dbl2 __attribute__((ext_vector_type(2)));   // a complex double without the address-space-bound class
    typedef __attribute__((address_space(3))) dbl2 LdsC2;
    // k-step ks of the slice at the wave-uniform address Qu. The base of the k-step is pinned to scalar registers, so
    // the loads take the form (scalar base) + (32-bit lane offset) + immediate
    static __device__ __forceinline__ void ldq(dbl2 (&q)[NG], const double2* Qu, unsigned qoff, int ks) {
        unsigned long long b = (unsigned long long)Qu + (size_t)ks * KSB;
        asm("" : "+s"(b));
        asm("" : "+v"(qoff));   // keeps the offset's zero extension beside the loads (selects the scalar-base form)
        const GlobalBytes* bp = (const GlobalBytes*)b;
#pragma unroll
        for (int g = 0; g < NG; ++g) q[g] = *(const __attribute__((address_space(1))) dbl2*)(bp + (size_t)qoff + 256 * g);
    }
    static __device__ __forceinline__ void ldq_first(dbl2 (&qn)[PF][NG], const double2* Qu, unsigned qoff) {
#pragma unroll
        for (int f = 0; f < PF; ++f) ldq(qn[f], Qu, qoff, f);
    }

    // the pinned LDS address of row a of row block rb behind the lane's part p: one register per row and row block
    // (4 TS double2 apart: beyond the DS immediate), so that the k-steps and column groups stay in the immediates
    template <typename P>
    static __device__ __forceinline__ P* lds_row(P* p, int a, int rb) {
        unsigned v = (unsigned)(size_t)(p + a * RS + 4 * rb * TS);
        asm("" : "+v"(v));
        return (P*)v;
    }

    // one unit of R rows: qn holds k-steps 0 .. PF - 1 of its slice Qu on entry and, with MORE, those of the wave's
    // next unit (slice Qnext) on return: the last PF k-steps load them in place of their own slice's.
    // xr, wr: the rows' read and write addresses; avn: k-step 0 of the state rows (issued by the caller)
    // NXT > 0: the next unit is a partial one of NXT column groups, Qnext its slice from its first group on; its first
    // stage is loaded instead (ldq_part below)
    template <int R, bool MORE, typename ST, int NXT = 0>
    static __device__ __forceinline__ void unit(dbl2 (&qn)[PF][NG], const double2* Qu, const double2* Qnext,
                                                unsigned qoff, const LdsC2* (&xr)[R][RB], LdsC2* (&wr)[R][RB],
                                                dbl2 (&avn)[R][RB], const ST& stg) {
        static_assert(NXT == 0 || (MORE && PF == 1), "a partial successor is loaded one stage ahead");
        double p1[R][RB][NG], p2[R][RB][NG], p3[R][RB][NG];
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks) {
            __builtin_amdgcn_sched_barrier(0);
            dbl2 qv[NG], av[R][RB];
#pragma unroll
            for (int g = 0; g < NG; ++g) qv[g] = qn[0][g];
#pragma unroll
            for (int f = 0; f + 1 < PF; ++f)
#pragma unroll
                for (int g = 0; g < NG; ++g) qn[f][g] = qn[f + 1][g];
            if (ks + PF < KSN) ldq(qn[PF - 1], Qu, qoff, ks + PF);
            else if (MORE) {
                if constexpr (NXT == 0) ldq(qn[PF - 1], Qnext, qoff, ks + PF - KSN);
                else ldq_part<NXT>(qn[PF - 1], Qnext, qoff, 0);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    av[r][rb] = avn[r][rb];
                    if (ks + 1 < KSN) avn[r][rb] = xr[r][rb][4 * (ks + 1)];
                }
            double qs[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) qs[g] = qv[g].x + qv[g].y;
            if constexpr (ST::ACTIVE) {
                // behind the wait for this k-step's slice values (the sums above use them), so that wait does not cover
                // what stg issues; the next k-step's wait does
                if (ks == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    stg();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const double as = av[r][rb].x + av[r][rb].y;
#pragma unroll
                    for (int g = 0; g < NG; ++g) {
                        p1[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[r][rb].x, qv[g].x, ks ? p1[r][rb][g] : 0.0, 0, 0, 0);
                        p2[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[r][rb].y, qv[g].y, ks ? p2[r][rb][g] : 0.0, 0, 0, 0);
                        p3[r][rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(as, qs[g], ks ? p3[r][rb][g] : 0.0, 0, 0, 0);
                    }
                }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    wr[r][rb][16 * g] = dbl2{p1[r][rb][g] - p2[r][rb][g], p3[r][rb][g] - p1[r][rb][g] - p2[r][rb][g]};
    }
    // unit e = (slice, row 0, row 1 or -1, -) of one or two rows; en: the wave's next unit (MORE), a slice of the set Qns
    // (this step's, or the next step's for the first unit of that step). The first row's
    // addresses and its k-step 0 are common to both sizes and issued ahead of the branch (and of the first wait for
    // the slice, which the compiler places there)
    template <bool MORE, typename ST>
    static __device__ __forceinline__ void unit_r(dbl2 (&qn)[PF][NG], const double2* Qs, int4 e, int4 en, unsigned qoff,
                                                  const double2* xl, double2* wl, const double2* Qns, const ST& stg) {
        const double2* Qu = Qs + (size_t)e.x * CHI * CHI;
        const double2* Qnext = Qns + (size_t)(MORE ? en.x : e.x) * CHI * CHI;
        const LdsC2* x0[RB];
        LdsC2* w0[RB];
        dbl2 a0[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            x0[rb] = lds_row((const LdsC2*)xl, e.y, rb);
            w0[rb] = lds_row((LdsC2*)wl, e.y, rb);
            a0[rb] = x0[rb][0];
        }
        if (e.z >= 0) {
            const LdsC2* xr[2][RB];
            LdsC2* wr[2][RB];
            dbl2 avn[2][RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                xr[0][rb] = x0[rb]; wr[0][rb] = w0[rb]; avn[0][rb] = a0[rb];
                xr[1][rb] = lds_row((const LdsC2*)xl, e.z, rb);
                wr[1][rb] = lds_row((LdsC2*)wl, e.z, rb);
                avn[1][rb] = xr[1][rb][0];
            }
            unit<2, MORE>(qn, Qu, Qnext, qoff, xr, wr, avn, stg);
        } else {
            const LdsC2* xr[1][RB];
            LdsC2* wr[1][RB];
            dbl2 avn[1][RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) { xr[0][rb] = x0[rb]; wr[0][rb] = w0[rb]; avn[0][rb] = a0[rb]; }
            unit<1, MORE>(qn, Qu, Qnext, qoff, xr, wr, avn, stg);
        }
    }

    // run() with the slice pipeline kept full across steps (the fast region of the step loop): qn holds k-steps
    // 0 .. PF - 1 of u0's slice of this step's set Qs on entry and those of u0's slice of the next step's set Qn on return:
    // the wave's last unit loads them in its last PF k-steps, so no L2 round trip is exposed behind the barrier that opens
    // the next PT phase, and every unit body is "in flight at entry, loads a successor at exit". Bounds: k-steps
    // 0 .. PF - 1 of a slice the unit list names, in the set the schedule names for the next step; the caller runs this
    // only where that step is itself a PT step of the block (never in the block's last one)
    // stg (LeanStageOp or LeanNoStage) is called once per wave, in the first k-step of the wave's first unit. A wave
    // without units calls nothing: the host stages only where the six waves with a piece have units (blk_stage)
    template <typename ST>
    static __device__ __forceinline__ void run_pre(dbl2 (&qn)[PF][NG], const double2* Qs, const double2* Qn, int4 u0,
                                                   int4 u1, unsigned qoff, const double2* xl, double2* wl, ST stg) {
        if (u0.x < 0) return;
        int4 e = u0;
        if (u1.x >= 0) {
            unit_r<true>(qn, Qs, u0, u1, qoff, xl, wl, Qs, stg);
            e = u1;
            if constexpr (ST::ACTIVE) stg.ln = 0;
        }
        unit_r<true>(qn, Qs, e, u0, qoff, xl, wl, Qn, stg);
    }
    // the wave's units u0 and u1 (slice, row 0, row 1 or -1, -; slice < 0: none) on the step's slice set Qs
    static __device__ __forceinline__ void run(const double2* Qs, int4 u0, int4 u1, unsigned qoff, const double2* xl,
                                               double2* wl) {
        if (u0.x < 0) return;
        dbl2 qn[PF][NG];
        ldq_first(qn, Qs + (size_t)u0.x * CHI * CHI, qoff);
        int4 e = u0;
        if (u1.x >= 0) {
            unit_r<true>(qn, Qs, u0, u1, qoff, xl, wl, Qs, LeanNoStage{});
            e = u1;
        }
        unit_r<false>(qn, Qs, e, e, qoff, xl, wl, Qs, LeanNoStage{});
    }

    // ---- partial units (SweepParams::lean_parts): plans whose rows that stay zero get no unit deal the remaining rows
    // in quarters, so a wave's list is [partial unit,] one whole one-row unit (pqd_host.cpp lean_part_units).
    // A partial unit (slice, row, -1, g0 | NGU << 4) contracts the whole state row with the column groups
    // g0 .. g0 + NGU - 1 of the slice only (NGU = 1 or 2 of the NG = 4): the same MFMAs with the same operands in the
    // same k order per accumulator and the same combine as unit(), so its columns are bit-identical to a whole unit's.
    // It reads only those column groups: a row split over several waves costs no L2 bytes more than a whole one.
    // So that the pipeline keeps the whole unit's proportions (4 slice loads of 16 B, 24 MFMAs per scheduling region, one
    // region loaded ahead), a stage is KPS = NG / NGU k-steps of the unit's NGU groups: slot kk NGU + g of the stage
    // holds group g0 + g of k-step KPS st + kk. A k-step is KSB = 4 KiB on, beyond the load's immediate, so every k-step
    // of a stage has its own scalar base (scalar adds) and the groups stay in the immediate; the lane offset is qoff.
    // Bounds: Qp = slice + 16 g0 elements with g0 + NGU <= NG (part_g0 masks the descriptor to that), so a load is
    // slice + 256 (g0 + g) + KSB ks + qoff with g0 + g < NG and ks < KSN: the addresses unit() loads (static_assert above).
    // The rows of a split row are read by every wave that holds a part of it and written in place, so no part may be
    // written before all of them are read: the accumulators stay in registers across a workgroup barrier (run_parts).
    static_assert(NG == 4, "partial units: quarters of four column groups");
    template <int NGU>
    static __device__ __forceinline__ void ldq_part(dbl2 (&q)[NG], const double2* Qp, unsigned qoff, int st) {
        constexpr int KPS = NG / NGU;
#pragma unroll
        for (int kk = 0; kk < KPS; ++kk) {
            unsigned long long b = (unsigned long long)Qp + (size_t)(KPS * st + kk) * KSB;
            asm("" : "+s"(b));
            asm("" : "+v"(qoff));
            const GlobalBytes* bp = (const GlobalBytes*)b;
#pragma unroll
            for (int g = 0; g < NGU; ++g)
                q[kk * NGU + g] = *(const __attribute__((address_space(1))) dbl2*)(bp + (size_t)qoff + 256 * g);
        }
    }
    // first column group and group count of a partial unit's descriptor, forced into the slice whatever the word holds
    static __device__ __forceinline__ int part_ng(int4 e) { return (e.w >> 4) == 2 ? 2 : 1; }
    static __device__ __forceinline__ int part_g0(int4 e) { return part_ng(e) == 2 ? (e.w & 2) : (e.w & 3); }

    // the MFMAs of a partial unit. qn holds its stage 0 on entry and k-step 0 of the whole unit that follows it (slice
    // Qnext) on return. p1, p2, p3: its accumulators, combined and written by part_write behind the barrier
    template <int NGU, typename ST>
    static __device__ __forceinline__ void part(dbl2 (&qn)[PF][NG], const double2* Qp, const double2* Qnext, unsigned qoff,
                                                const LdsC2* (&xr)[RB], double (&p1)[RB][NGU], double (&p2)[RB][NGU],
                                                double (&p3)[RB][NGU], const ST& stg) {
        static_assert(PF == 1, "one stage in flight");
        constexpr int KPS = NG / NGU, NST = KSN / KPS;
        dbl2 avn[RB][KPS];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int kk = 0; kk < KPS; ++kk) avn[rb][kk] = xr[rb][4 * kk];
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            __builtin_amdgcn_sched_barrier(0);
            dbl2 qv[NG], av[RB][KPS];
#pragma unroll
            for (int j = 0; j < NG; ++j) qv[j] = qn[0][j];
            if (st + 1 < NST) ldq_part<NGU>(qn[0], Qp, qoff, st + 1);
            else ldq(qn[0], Qnext, qoff, 0);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int kk = 0; kk < KPS; ++kk) {
                    av[rb][kk] = avn[rb][kk];
                    if (st + 1 < NST) avn[rb][kk] = xr[rb][4 * (KPS * (st + 1) + kk)];
                }
            double qs[NG];
#pragma unroll
            for (int j = 0; j < NG; ++j) qs[j] = qv[j].x + qv[j].y;
            if constexpr (ST::ACTIVE) {
                if (st == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    stg();
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int kk = 0; kk < KPS; ++kk)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const double as = av[rb][kk].x + av[rb][kk].y;
                    const bool first = st == 0 && kk == 0;
#pragma unroll
                    for (int g = 0; g < NGU; ++g) {
                        const int j = kk * NGU + g;
                        p1[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[rb][kk].x, qv[j].x, first ? 0.0 : p1[rb][g], 0, 0, 0);
                        p2[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[rb][kk].y, qv[j].y, first ? 0.0 : p2[rb][g], 0, 0, 0);
                        p3[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(as, qs[j], first ? 0.0 : p3[rb][g], 0, 0, 0);
                    }
                }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // every part of a split row has been read (the caller's barrier): combine as unit() does and write the unit's columns
    template <int NGU>
    static __device__ __forceinline__ void part_write(LdsC2* (&wr)[RB], const double (&p1)[RB][NGU],
                                                      const double (&p2)[RB][NGU], const double (&p3)[RB][NGU]) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int g = 0; g < NGU; ++g)
                wr[rb][16 * g] = dbl2{p1[rb][g] - p2[rb][g], p3[rb][g] - p1[rb][g] - p2[rb][g]};
    }
    // The barrier between the partial units' reads and writes. Every wave of the workgroup passes exactly one per PT phase
    // (a wave without a partial unit at once). The reads have returned (lgkmcnt(0): their values fed MFMAs already, so
    // nothing is waited for), the slice loads in flight stay in flight: no vmcnt wait, unlike __syncthreads()
    static __device__ __forceinline__ void part_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

    // a partial unit e of NGU groups with its barrier and write; Qs: the step's slice set; en: the whole unit behind it
    template <int NGU, typename ST>
    static __device__ __forceinline__ void part_r(dbl2 (&qn)[PF][NG], const double2* Qs, int4 e, int4 en, unsigned qoff,
                                                  const double2* xl, double2* wl, const ST& stg) {
        const int g0 = part_g0(e);
        const double2* Qp = Qs + (size_t)e.x * CHI * CHI + 16 * g0;
        const double2* Qnext = Qs + (size_t)en.x * CHI * CHI;
        const LdsC2* xr[RB];
        LdsC2* wr[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            xr[rb] = lds_row((const LdsC2*)xl, e.y, rb);
            wr[rb] = lds_row((LdsC2*)wl + 16 * g0, e.y, rb);
        }
        double p1[RB][NGU], p2[RB][NGU], p3[RB][NGU];
        part<NGU>(qn, Qp, Qnext, qoff, xr, p1, p2, p3, stg);
        part_barrier();
        part_write<NGU>(wr, p1, p2, p3);
    }
    // the whole one-row unit e of a wave in a plan with partial units; NXT: what the wave's first unit of the next PT
    // phase is (0: e itself, a whole unit; 1, 2: a partial unit of that many groups, Qnext its slice from its first group)
    template <bool MORE, int NXT, typename ST>
    static __device__ __forceinline__ void whole1(dbl2 (&qn)[PF][NG], const double2* Qu, const double2* Qnext, int row,
                                                  unsigned qoff, const double2* xl, double2* wl, const ST& stg) {
        const LdsC2* xr[1][RB];
        LdsC2* wr[1][RB];
        dbl2 avn[1][RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            xr[0][rb] = lds_row((const LdsC2*)xl, row, rb);
            wr[0][rb] = lds_row((LdsC2*)wl, row, rb);
            avn[0][rb] = xr[0][rb][0];
        }
        unit<1, MORE, ST, NXT>(qn, Qu, Qnext, qoff, xr, wr, avn, stg);
    }
    // run_pre() for a plan with partial units: u0 is partial (u0.w >= 0) with the whole unit u1 behind it, or whole and
    // alone, or absent. qn: the first stage of u0 in this step's set Qs on entry, in the next step's set Qn on return
    template <typename ST>
    static __device__ __forceinline__ void run_pre_parts(dbl2 (&qn)[PF][NG], const double2* Qs, const double2* Qn, int4 u0,
                                                         int4 u1, unsigned qoff, const double2* xl, double2* wl, ST stg) {
        if (u0.x < 0 || u0.w < 0) {
            part_barrier();
            if (u0.x < 0) return;
            const double2* Qu = Qs + (size_t)u0.x * CHI * CHI;
            whole1<true, 0>(qn, Qu, Qn + (size_t)u0.x * CHI * CHI, u0.y, qoff, xl, wl, stg);
            return;
        }
        const double2* Qu = Qs + (size_t)u1.x * CHI * CHI;
        const double2* Qnext = Qn + (size_t)u0.x * CHI * CHI + 16 * part_g0(u0);
        if (part_ng(u0) == 2) {
            part_r<2>(qn, Qs, u0, u1, qoff, xl, wl, stg);
            whole1<true, 2>(qn, Qu, Qnext, u1.y, qoff, xl, wl, LeanNoStage{});
        } else {
            part_r<1>(qn, Qs, u0, u1, qoff, xl, wl, stg);
            whole1<true, 1>(qn, Qu, Qnext, u1.y, qoff, xl, wl, LeanNoStage{});
        }
    }
    // the first stage of the wave's first unit u0 in the set Qs (what run_pre_parts expects in qn)
    static __device__ __forceinline__ void ldq_first_parts(dbl2 (&qn)[PF][NG], const double2* Qs, int4 u0, unsigned qoff) {
        const double2* Qu = Qs + (size_t)u0.x * CHI * CHI;
        if (u0.w < 0) ldq(qn[0], Qu, qoff, 0);
        else if (part_ng(u0) == 2) ldq_part<2>(qn[0], Qu + 16 * part_g0(u0), qoff, 0);
        else ldq_part<1>(qn[0], Qu + 16 * part_g0(u0), qoff, 0);
    }
    // run() for a plan with partial units
    static __device__ __forceinline__ void run_parts(const double2* Qs, int4 u0, int4 u1, unsigned qoff, const double2* xl,
                                                     double2* wl) {
        if (u0.x < 0) {
            part_barrier();
            return;
        }
        dbl2 qn[PF][NG];
        ldq_first_parts(qn, Qs, u0, qoff);
        int4 e = u0;
        if (u0.w >= 0) {
            if (part_ng(u0) == 2) part_r<2>(qn, Qs, u0, u1, qoff, xl, wl, LeanNoStage{});
            else part_r<1>(qn, Qs, u0, u1, qoff, xl, wl, LeanNoStage{});
            e = u1;
        } else {
            part_barrier();
        }
        whole1<false, 0>(qn, Qs + (size_t)e.x * CHI * CHI, Qs, e.y, qoff, xl, wl, LeanNoStage{});
    }
};

// Two sums over lane pairs W = 16 or 32 apart in one step of a reduce-scatter: v_permlane16_swap exchanges the odd 16-lane
// rows of its first operand with the even rows of its second (v_permlane32_swap: the upper 32 lanes with the lower 32),
// so the sum of its two results is a[l] + a[l ^ W] in the lanes with bit W clear and b[l] + b[l ^ W] in the others
template <int W>
__device__ __forceinline__ double lean_pair(double a, double b) {
    static_assert(W == 32 || W == 16, "permlane swaps pair lanes 32 or 16 apart");
    const long long A = __double_as_longlong(a), B = __double_as_longlong(b);
    unsigned l0, l1, h0, h1;
    if constexpr (W == 32) {
        const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)A, (unsigned)B, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(A >> 32), (unsigned)(B >> 32), false, false);
        l0 = lo[0]; l1 = lo[1]; h0 = hi[0]; h1 = hi[1];
    } else {
        const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)A, (unsigned)B, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(A >> 32), (unsigned)(B >> 32), false, false);
        l0 = lo[0]; l1 = lo[1]; h0 = hi[0]; h1 = hi[1];
    }
    return __longlong_as_double(((long long)h0 << 32) | l0) + __longlong_as_double(((long long)h1 << 32) | l1);
}
// v[q] summed over the wave's four 16-lane rows (lanes l, l ^ 16, l ^ 32, l ^ 48), left in the lanes of row q
__device__ __forceinline__ double lean_rows4(const double (&v)[4]) {
    return lean_pair<32>(lean_pair<16>(v[0], v[1]), lean_pair<16>(v[2], v[3]));
}

// sum over each 16-lane row, left in all its lanes (c_group_sum<16> with bound_ctrl DPP moves: every lane of these
// permutations has a source, so no destination is initialised first)
template <int CTRL>
__device__ __forceinline__ double lean_dpp(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double2 lean_row_sum(double2 v) {
    v = c_add(v, make_double2(lean_dpp<0xB1>(v.x), lean_dpp<0xB1>(v.y)));    // quad_perm [1,0,3,2]
    v = c_add(v, make_double2(lean_dpp<0x4E>(v.x), lean_dpp<0x4E>(v.y)));    // quad_perm [2,3,0,1]
    v = c_add(v, make_double2(lean_dpp<0x141>(v.x), lean_dpp<0x141>(v.y)));  // row_half_mirror
    return c_add(v, make_double2(lean_dpp<0x140>(v.x), lean_dpp<0x140>(v.y)));  // row_mirror
}

// The compaction map of the lean column phase (SweepParams::lean_rho, pqd_host.cpp live_col_map): rho(c), c < 16, one
// nibble each, the live rows in increasing order followed by the rows that stay zero; every value is < 16.
__device__ __forceinline__ int lean_rho(unsigned long long rho, int c) { return (int)(rho >> (4 * c)) & 15; }
// A lane's addresses in the compacted column phase (LeanCol, KC < 4), fixed for the launch: cb[ks] = S[rho(4 ks + lk)][li]
// of the wave's trajectory (its B operand of compact k-step ks and, as accumulator ks, the row it writes), fo[ks] =
// rho(li) * 16 + rho(4 ks + lk), its element of F(n) where that is loaded from memory. Nothing at KC = 4.
typedef double lean_dbl2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) lean_dbl2 LeanLdsC2;
template <int KC>
struct LeanColMap {
    LeanLdsC2* cb[KC];
    int fo[KC];
};
template <>
struct LeanColMap<4> {};

// The column operands of the lean instance's next fast step, staged in LDS while the PT phase runs (the fast region of
// the step loop). LeanCol opens with 4 + 4 + 4 n_out loads per lane of bytes that are new every step, directly behind the
// barrier that ends the PT phase: both waves of every SIMD wait out that round trip together before their first MFMA.
// Fetching them a phase ahead through registers lost to the register file twice, so they go to LDS
// without passing one: global_load_lds_dwordx4 (16 bytes per lane, no data VGPR) writes lane-linearly from a
// wave-uniform LDS base, with a source address per lane. Six wave-instructions of at most 1 KiB hold a step's operands:
//   waves 0..3  F(n + 1) of the block's system in fragment order: wave ks, lane (li, lk) = (lane & 15, lane >> 4) sources
//               F[li * 16 + 4 ks + lk], the address that lane loads in LeanCol, so LeanCol reads ac[ks] as element
//               64 ks + lane (1 KiB contiguous per wave read);
//   wave 4      the 64 elements of the closure vector step n + 1 reads (slice set sched[n]), plainly;
//   wave 5      the 16 n_out elements of W(n + 1), plainly, by lanes < 16 n_out.
// The area lies behind rbuf in the dynamic LDS (OFF double2 from its start): F at 0, the closure vector at 256, W at 320
// (double2 elements), 6 KiB. One area holds one system's operands: a block whose slots mix systems does not stage
// (SweepParams::blk_stage).
// Ordering: the loads are issued in the PT phase of step n, behind the barrier that ends column phase n (whose reads of
// the area LeanCol's closing lgkmcnt(0) retired), in the first k-step of the issuing wave's first unit, after its slice
// wait and before its MFMAs (LeanPt::unit). Loads return in order, and the k-steps that follow consume slice values
// loaded behind the staged piece, so the piece has landed long before the wave reaches the barrier that ends the PT
// phase, and column phase n + 1 reads it behind that barrier. A wave without PT units has no such k-step: the host
// lets a plan stage only where waves 0..5 have units (pqd_host.cpp fill_sweep_params).
// The instruction stands in one asm statement: branch-free (the lanes that load are an exec mask, 0 for a wave with
// nothing to stage), with M0 and exec saved and restored around it, and outside the compiler's vmcnt bookkeeping. An
// uncounted older load only makes the compiler's counted waits wait for more; counted, the compiler drains vmcnt(0) at the
// next use of any load and before __syncthreads(), and with it the slice k-step that run_pre keeps in flight.
// Bounds: every source address is an index expression LeanCol or the step loop loads for a step the block runs (row
// li < 16, column 4 ks + lk < 16 of F(m), element lane < 64 of a closure vector, element lane < 16 n_out of W(m), for
// m = n + 1 <= n_end - 2 < n_steps); every destination is area + wave * 1 KiB + lane * 16 B with wave < 6: inside the
// 6 KiB (static_assert below; launch_sw adds BYTES to the instance's dynamic LDS).
template <int OFF>
struct LeanStage {
    static constexpr int N2 = 16, CHI = 64, KMAX = 4;
    static constexpr int F_AT = 0, C_AT = N2 * N2, W_AT = C_AT + CHI, ELEMS = W_AT + KMAX * N2;
    static constexpr size_t BYTES = (size_t)ELEMS * sizeof(double2);
    typedef double dbl2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) dbl2 LdsC2;
    static_assert(F_AT == 0 && C_AT == 4 * 64 && W_AT == 5 * 64 && ELEMS == 6 * 64 && BYTES == 6144,
                  "six pieces of 64 lanes x 16 B, wave w's at 64 w elements");
    static_assert(OFF >= 0 && sizeof(double2) == 16, "16-byte aligned destinations behind the 16-byte aligned smem");
    static_assert(OFF * sizeof(double2) + BYTES + 512 <= 160 * 1024, "the area fits the LDS beside the static tables");

    static __device__ __forceinline__ LdsC2* area(double2* smem) { return (LdsC2*)(smem + OFF); }
    // the wave's part, fixed for the launch: the lane's byte offset into its piece's source (F: row li, column
    // 4 wave + lk; closure vector and W: element lane), the piece's LDS byte address, the lanes that load
    // KC < 4 (compacted column phase, LeanCol): waves 0..KC-1 source F[rho(li) * 16 + rho(4 wave + lk)], the element
    // lane (li, lk) multiplies in compact k-step `wave`; wave 3 stages nothing (rho < 16: a row and a column of F(m))
    template <int KC = 4>
    static __device__ __forceinline__ unsigned lane_off(int wave, int lane, unsigned long long rho = 0) {
        if constexpr (KC == 4)
            return (unsigned)((wave < 4 ? (lane & 15) * N2 + 4 * wave + (lane >> 4) : lane) * sizeof(double2));
        else
            return (unsigned)((wave < KC ? lean_rho(rho, lane & 15) * N2 + lean_rho(rho, 4 * wave + (lane >> 4)) : lane) *
                              sizeof(double2));
    }
    static __device__ __forceinline__ unsigned dst(double2* smem, int wave) {
        return (unsigned)(size_t)(area(smem) + 64 * (wave < 6 ? wave : 0));
    }
    template <int KC = 4>
    static __device__ __forceinline__ unsigned long long lanes(int wave, int n_out) {
        if (KC < 4 && wave >= KC && wave < 4) return 0ull;
        return wave < 5 ? ~0ull : wave > 5 ? 0ull : n_out >= KMAX ? ~0ull : (1ull << (N2 * n_out)) - 1;
    }
    // the source of the wave's piece for step m: Fm, Wm: F(m), W(m) of the block's system; cv: the closure vector step m
    // reads (waves 6, 7 load no lane of it)
    static __device__ __forceinline__ const double2* src(int wave, const double2* Fm, const double2* cv, const double2* Wm) {
        return wave < 4 ? Fm : wave == 4 ? cv : Wm;
    }
    // one 16-byte element per lane of ln, from base + off (off per lane) to the LDS address to + 16 lane (base, to, ln
    // wave-uniform)
    static __device__ __forceinline__ void issue(const double2* base, unsigned off, unsigned to, unsigned long long ln) {
        unsigned long long keep_exec;
        unsigned keep_m0;
        asm volatile("s_mov_b64 %0, exec\n\ts_mov_b32 %1, m0\n\ts_mov_b64 exec, %5\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %1\n\ts_mov_b64 exec, %0"
                     : "=&s"(keep_exec), "=&s"(keep_m0)
                     : "v"(off), "s"(base), "s"(to), "s"(ln)
                     : "memory");
    }
};
// what a wave's first PT unit of a fast step issues behind its first slice wait (LeanPt::unit): its piece of the next
// step's column operands (ln = 0: nothing, the region's last step and waves 6, 7)
template <typename LS>
struct LeanStageOp {
    static constexpr bool ACTIVE = true;
    const double2* base;
    unsigned off, to;
    unsigned long long ln;
    __device__ __forceinline__ void operator()() const { LS::issue(base, off, to, ln); }
};

// The fused column operator F(n) of the lean instance with the step's outputs read on the way (N2 = 16, chi = 64, one
// wave per trajectory). The state the outputs of a fused step are read from is the one before F(n), and the wave that
// applies F(n) loads exactly those values as its B operands: lane (li, lk) = (lane & 15, lane >> 4) holds
// S[4 ks + lk][16 nt + li] for all 4 x 4 (ks, nt). So the closure r[a] = sum_d S[a][d] c[d] is one complex MAC per loaded
// value into r[ks] (the lane's part of rows 4 ks + lk), the trace t[k] = sum_a W(n)[k][a] r[a] 4 n_out MACs, and the sum
// over the 64 lanes a reduce-scatter of permlane swaps and a DPP row sum: no second pass over the states, no partials in
// LDS, no other wave involved. The MFMAs are those of col_apply_mfma3 with the same operands in the same order per
// accumulator and the same combine, so the states are bit-identical to it; the outputs differ from the closure pass of
// the step loop by the order of a 64-term and a 16-term sum.
// State addresses: one per-lane LDS base (row lk, column li of the wave's trajectory), every read S[4 ks + lk][16 nt + li]
// and every write S[lk + 4 r][16 nt + li] at base + (4 j RS + 16 nt) 16 B, j < 4: the DS immediate (largest 12 RS 16 + 768).
// Bounds: F, W and the closure vector are indexed as the step loop's own loads of them (row li < 16 and column
// 4 ks + lk < 16 of F(n), n < n_steps; W(n)[k][4 ks + lk], k < n_out; c[16 nt + li] < CHI of slice set sched[n - 1]).
// STAGED: Fn, cv and Wn are the parts of the LDS area LeanStage filled during the PT phase before (F in fragment order,
// element 64 ks + lane; the closure vector and W as in memory, the same indices as the global loads: < 64 and
// < 16 n_out <= 64), the same values in the same registers, so nothing downstream differs.
// KC: k-steps of the product. 4: all 16 rows, the code as it always was. 3 (plans whose 9 to 12 live rows the host
// compacted, SweepParams::lean_colk): the lane's MFMA operands are those of the compact index, A = F[rho(li)][rho(4 ks + lk)],
// B = S[rho(4 ks + lk)][16 nt + li], accumulator j < KC is row rho(lk + 4 j), written to the address it was read from
// (cm.cb[j]); accumulator 3 would be rows that stay zero and is not written. rho is increasing on the live rows and the
// f64 MFMA adds its k products as one ordered chain of FMAs (scripts/ubench_mfma_f64_korder.hip), so every live row
// gets the same products in the same order as at KC = 4, less terms that are exactly 0: the same bits. The outputs are
// then read from values loaded a second time in the layout of KC = 4 (rows 4 ks + lk through sb), with the same MACs
// in the same order: rows that stay zero add fma(w, 0, t) = t. Those loads of tile nt stand before the tile's writes in
// program order, and a wave's LDS operations complete in order, so they see the state before F(n) as the operands do.
// Bounds at KC = 3: rho < 16, so cm.cb[ks] + 16 nt is row rho < 16, column 16 nt + li < 64 of the wave's own trajectory
// and cm.fo[ks] < 256 an element of F(n); W and the closure vector are indexed as at KC = 4.
template <int RS, bool READOUT, bool STAGED = false, int KC = 4>
struct LeanCol {
    static constexpr int N2 = 16, CHI = 64, KS = 4, NTL = 4, KMAX = 4;   // KMAX: the lean instance's limit on n_out
    static_assert(KC == 3 || KC == 4, "three compact k-steps (9 to 12 live rows) or all four");
    typedef lean_dbl2 dbl2;
    typedef LeanLdsC2 LdsC2;
    static_assert((12 * RS + 48) * 16 + 15 < 65536, "tile and row offsets fit the DS immediate");
    // where the operands come from: global memory (restrict: nothing here writes it), or the staging area
    template <bool S, typename = void> struct SrcOf { typedef const double2* __restrict__ type; };
    template <typename V> struct SrcOf<true, V> { typedef const LdsC2* type; };
    typedef typename SrcOf<STAGED>::type Src;
    static __device__ __forceinline__ double2 ld(Src q, int i) {
        const auto v = q[i];
        return make_double2(v.x, v.y);
    }
    // the lane's B operand of k-step ks, tile nt (and where accumulator ks of that tile goes)
    static __device__ __forceinline__ LdsC2* opd(LdsC2* sb, const LeanColMap<KC>& cm, int ks, int nt) {
        if constexpr (KC == 4) return sb + 4 * ks * RS + 16 * nt;
        else return cm.cb[ks] + 16 * nt;
    }

    // (W(n) stays loaded ahead of the tiles in both forms: read from the staging area behind the last tile's operands
    // instead, it measured the same)
    // Fn: F(n) of the wave's system; cv: closure vector of the slice set of step n - 1; Wn: W(n) of the wave's system;
    // sb: the lane's LDS base; cm: its compacted addresses (KC < 4); out: where the slot's n_out outputs of step n go
    // (READOUT only)
    static __device__ __forceinline__ void run(Src Fn, Src cv, Src Wn, int n_out, LdsC2* sb, const LeanColMap<KC>& cm,
                                               double2* out, int lane) {
        const int li = lane & 15, lk = lane >> 4;
        double2 ac[KC], cl[NTL], w[KMAX][KS];
        double as[KC];
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) {
            if constexpr (KC == 4) ac[ks] = ld(Fn, STAGED ? 64 * ks + lane : li * N2 + 4 * ks + lk);
            else ac[ks] = ld(Fn, STAGED ? 64 * ks + lane : cm.fo[ks]);
        }
        if constexpr (READOUT) {
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt) cl[nt] = ld(cv, 16 * nt + li);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < n_out) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) w[k][ks] = ld(Wn, k * N2 + 4 * ks + lk);
                }
        }
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) as[ks] = ac[ks].x + ac[ks].y;
        double2 r[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) r[ks] = c_zero();
        // a tile's operand values are read while the tile before it runs its MFMAs (one LDS round trip exposed per
        // step, not one per value; tiles are disjoint columns, so the in-place writes of a tile touch nothing read later)
        dbl2 bn[KC];
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) bn[ks] = *opd(sb, cm, ks, 0);
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            dbl4 p1 = dbl4{0, 0, 0, 0}, p2 = p1, p3 = p1;
            dbl2 bq[KC], bo[KS];
            // KC < 4: the tile's values in the rows the outputs are summed over, issued ahead of the next tile's operands
            // and used behind this tile's first MFMAs
            if constexpr (KC < 4 && READOUT) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) bo[ks] = sb[4 * ks * RS + 16 * nt];
            }
#pragma unroll
            for (int ks = 0; ks < KC; ++ks) {
                bq[ks] = bn[ks];
                if (nt + 1 < NTL) bn[ks] = *opd(sb, cm, ks, nt + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < KC; ++ks) {
                const dbl2 bv = bq[ks];
                const double bs = bv.x + bv.y;
                p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[ks].x, bv.x, p1, 0, 0, 0);
                p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[ks].y, bv.y, p2, 0, 0, 0);
                p3 = __builtin_amdgcn_mfma_f64_16x16x4f64(as[ks], bs, p3, 0, 0, 0);
                if constexpr (READOUT) {
                    if constexpr (KC == 4) c_fma(r[ks], make_double2(bv.x, bv.y), cl[nt]);
                    else c_fma(r[ks], make_double2(bo[ks].x, bo[ks].y), cl[nt]);
                }
            }
            if constexpr (KC < 4 && READOUT) {
#pragma unroll
                for (int ks = KC; ks < KS; ++ks) c_fma(r[ks], make_double2(bo[ks].x, bo[ks].y), cl[nt]);
            }
#pragma unroll
            for (int j = 0; j < KC; ++j) *opd(sb, cm, j, nt) = dbl2{p1[j] - p2[j], p3[j] - p1[j] - p2[j]};
        }
        if constexpr (READOUT) {
            // t[k] over the lane's rows; re[k], im[k] = 0 for k >= n_out
            double re[KMAX], im[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                double2 t = c_zero();
                if (k < n_out) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) c_fma(t, w[k][ks], r[ks]);
                }
                re[k] = t.x;
                im[k] = t.y;
            }
            // the four 16-lane rows: after the swaps row q holds output q's sum over the rows (lean_rows4), then the
            // sum over the row's 16 lanes; lane 16 q stores output q
            double2 y = make_double2(lean_rows4(re), lean_rows4(im));
            y = lean_row_sum(y);
            if (li == 0 && lk < n_out) out[lk] = y;
        }
        // the PT phase reads what other lanes and waves wrote: the barrier that follows waits for these writes
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
};

// PT contraction of row alpha for BT = 8 on v_mfma_f64_16x16x4_f64 ("split complex"): the 16 MFMA rows are
// [Re X; Im X] of the 8 trajectories, so two real GEMMs P1 = [Xr; Xi] Qr and P2 = [Xr; Xi] Qi hold all four
// partial products: Cr = P1[top] - P2[bottom], Ci = P2[top] + P1[bottom]. C fragment rows (l>>4) + 4 r put
// row b (r = 0, 1) and row b + 8 (r + 2) in the same lane, so the recombination is lane-local. Same operand
// traffic as the 4x4x4 path, but the 16x16x4 instruction runs at the FP64 matrix peak and co-issues with VALU.
template <int CHI, int RS, int TS>
__device__ __forceinline__ void pt_row_mfma16(const double2* __restrict__ Qg, double2* st, int a, int lane) {
    constexpr int NTL = CHI / 16, KSN = CHI / 4;
    const int li = lane & 15, lk = lane >> 4;
    const bool imag_row = (li & 8) != 0;
    dbl4 p1[NTL], p2[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) { p1[t] = dbl4{0, 0, 0, 0}; p2[t] = dbl4{0, 0, 0, 0}; }
    const double2* xr = st + (li & 7) * TS + a * RS + lk;  // + 4 ks
    const double2* qp = Qg + (size_t)lk * CHI + li;         // + 4 ks * CHI + 16 t
    double2 qn[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) qn[t] = qp[16 * t];
#pragma unroll 2
    for (int ks = 0; ks < KSN; ++ks) {
        double2 qv[NTL];
#pragma unroll
        for (int t = 0; t < NTL; ++t) qv[t] = qn[t];
        if (ks + 1 < KSN) {
#pragma unroll
            for (int t = 0; t < NTL; ++t) qn[t] = qp[(size_t)4 * (ks + 1) * CHI + 16 * t];
        }
        const double2 xv = xr[4 * ks];
        const double av = imag_row ? xv.y : xv.x;
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
            p1[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, qv[t].x, p1[t], 0, 0, 0);
            p2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, qv[t].y, p2[t], 0, 0, 0);
        }
    }
    double2* wr = st + a * RS + li;
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int r = 0; r < 2; ++r)
            wr[(lk + 4 * r) * TS + 16 * t] = make_double2(p1[t][r] - p2[t][r + 2], p2[t][r] + p1[t][r + 2]);
}

// PT phase of the general instances: this wave's rows of every trajectory times the slices of the set Qs.
// pt_mode 0: VALU rows, 1: matrix-core rows (4x4x4_4b), 4: matrix-core rows with 3 real products per
// complex product (default), 3: split-complex 16x16x4 rows (BT = 8), 2: mixed (waves 0..NW/2-1 start on the matrix cores,
// the others on the VALU, alternating per row), so the two FP64 pipes of a SIMD run concurrently.
//
// SweepParams is taken by value: with a reference the instances <25, 64, 4> and <25, 64, 4, TRUNK> gain one VGPR
// spill each (profiles/r26/sweep_steps/README.md).
template <int N2, int CHI, int BT>
__device__ __forceinline__ void pt_phase(SweepParams p, const double2* Qs, double2* st, int wave, int lane) {
    using L = SweepLayout<N2, CHI, BT>;
    constexpr int RS = L::RS, TS = L::TS, WPT = L::WPT, NW = L::NW;
    int parity = (p.pt_mode == 2) ? ((wave >= NW / 2) ? 1 : 0) : 0;
    if (p.units && (p.pt_mode == 4 || p.pt_mode == 5)) {
        // 3M rows by the host's per-wave unit list: (slice, row 0, row 1 or -1, rows 2 | 3 << 16 or -1)
        const int4* U = p.units + (size_t)wave * p.umax;
        for (int u = 0; u < p.umax; ++u) {
            const int4 e = U[u];
            if (e.x < 0) break;
            const double2* Qg = Qs + (size_t)e.x * CHI * CHI;
            if (p.pt_mode == 5) pt_rows3<N2, CHI, BT, RS, TS, 2>(Qg, st, e, lane);
            else pt_rows3<N2, CHI, BT, RS, TS, 1>(Qg, st, e, lane);
        }
        return;
    }
    for (int a = wave; a < N2; a += NW) {
        const double2* Qg = Qs + (size_t)p.gmap[a] * CHI * CHI;
        const bool use_mfma = (p.pt_mode == 1) || (p.pt_mode == 2 && parity == 0);
        parity ^= 1;
        if (p.pt_mode == 4) {
            pt_row_mfma3<CHI, BT, RS, TS, 1>(Qg, st, a, a, a, a, lane);
            continue;
        }
        if (p.pt_mode == 5) {   // 3M with two k-steps of the slice in flight
            pt_row_mfma3<CHI, BT, RS, TS, 2>(Qg, st, a, a, a, a, lane);
            continue;
        }
        if constexpr (BT == 8) {
            if (p.pt_mode == 3) {
                pt_row_mfma16<CHI, RS, TS>(Qg, st, a, lane);
                continue;
            }
        }
        // the VALU rows are compiled for BT = 4, chi <= 64 and one wave per trajectory only: elsewhere
        // their accumulators cap the whole kernel's VGPR allocation and spill, so those run modes 0/2 on
        // the 4x4x4 path
        if (BT == 8 || CHI > 64 || WPT > 1 || use_mfma || p.pt_mode == 3) {
            pt_row_mfma<CHI, BT, RS, TS>(Qg, st, a, lane);
            continue;
        }
        if constexpr (BT == 4 && CHI <= 64 && WPT == 1) pt_row_valu<CHI, BT, RS, TS, L::KD>(Qg, st, a, lane);
    }
}

// TRUNK: the trunk pre-pass instance (writes checkpoints through p.ck_map); kept out of the main sweep's instance,
// where the extra live values cost VGPR spills
// Reads every half step's M, F, W as stored: plans running this kernel (main sweep or trunk pre-pass) build the free
// propagators without pulse windows (pqd_host.cpp). A window-select form of these loads measured 1.8% slower on the
// bench launch even with its selects folded away at compile time (202.3 vs 198.1 ms, profiles/r02/windows/).
// LEAN: the headline instance (N2 = 16, chi = 64, BT = 8) with the A/B switches of SweepParams fixed at their production
// values (3M unit-list PT rows, 3M columns, fused half steps, lane traces, no ablation), so its register allocation
// is that of the one path it runs and not the maximum over all of them; the host selects it only for plans with
// exactly that configuration (pqd_host.cpp sweep_lean_ok). With that room the wave's unit list and the slice schedule
// stay in scalar registers (200.3 -> 196.1 ms per bench launch; the instance alone gains nothing, and
// a register for the next event step or the first slice k-step loaded before the PT barrier measured slower).
// Its PT phase is LeanPt above (184.2 against 193.8 ms; the fused column operator loaded a phase ahead and a static
// s_setprio for waves 4-7 both measured slower on top of it and are not here). From a block's last MTO and activation on
// it reads the outputs inside the fused column operator (LeanCol above; the fast region of the step loop: 184.7 -> 178.9 ms).
// slice k-steps in flight in the lean instance's PT phase (2 measured the same within the spread and takes all 256 VGPRs)
constexpr int LEAN_PF = 1;
// PARTS: the lean instance for plans whose unit list holds partial units (SweepParams::lean_parts, LeanPt::run_parts);
// an instance of its own, so that a plan without them runs the code it always ran
template <int N2, int CHI, int BT, bool TRUNK, bool LEAN = false, bool PARTS = false>
__global__ __launch_bounds__(64 * BT * sweep_wpt(N2, BT, CHI)) void pt_sweep_kernel(SweepParams p, const double2* __restrict__ Mg,
                                                           const double2* __restrict__ Qg0, double2* __restrict__ outg,
                                                           const double2* __restrict__ Fg, const double2* __restrict__ Wg) {
    using L = SweepLayout<N2, CHI, BT>;
    static_assert(!LEAN || (N2 == 16 && CHI == 64 && BT == 8 && !TRUNK), "the lean instance is the headline shape only");
    static_assert(!PARTS || LEAN, "partial units exist in the lean instance only");
    constexpr int RS = L::RS, TS = L::TS, NCOL = L::NCOL;
    constexpr int WPT = L::WPT, NW = L::NW, NT = 64 * NW;  // waves per trajectory, waves, threads
    const int ablate = LEAN ? 0 : p.ablate;
    extern __shared__ __attribute__((aligned(16))) double2 smem[];
    double2* st = smem;
    double2* rbuf = smem + BT * TS;
    __shared__ int s_traj[BT], s_wb[BT], s_we[BT], s_fz[BT], s_sys[BT], s_act[BT], s_src[BT];
    __shared__ long long s_wo[BT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tw = wave % BT, half = wave / BT;  // column phases: trajectory of this wave, its column half

    if (tid < BT) {
        const int t = p.blk_traj[blockIdx.x * BT + tid];
        s_traj[tid] = t;
        s_wb[tid] = t >= 0 ? p.wbeg[t] : INT_MAX;
        s_we[tid] = t >= 0 ? p.wend[t] : -1;
        s_wo[tid] = t >= 0 ? p.woff[t] : 0;
        s_fz[tid] = 0;
        s_sys[tid] = t >= 0 ? p.traj_sys[t] : 0;
        s_act[tid] = p.blk_act[blockIdx.x * BT + tid];
        s_src[tid] = p.blk_src[blockIdx.x * BT + tid];
    }
    __syncthreads();
    // shared trunk (pqd_host.cpp branch_slots): a slot is dormant before its activation step, then copies the
    // (state, fused flag) of an earlier-activated slot of its workgroup or a trunk checkpoint. next_act: the next step
    // with activations
    const int my_act = __builtin_amdgcn_readfirstlane(s_act[tw]);
    auto next_activation = [&](int after) {
        int m = INT_MAX;
#pragma unroll
        for (int b = 0; b < BT; ++b)
            if (s_act[b] > after && s_act[b] < m) m = s_act[b];
        return m;
    };
    int n0 = INT_MAX;  // first step of the block: its earliest activation (0 unless every slot starts later)
#pragma unroll
    for (int b = 0; b < BT; ++b) n0 = s_act[b] < n0 ? s_act[b] : n0;
    if (n0 == INT_MAX) return;  // no trajectory in this workgroup (the whole block exits together)
    int next_act = n0 > 0 ? n0 : next_activation(0);
    const int n_end = p.blk_end[blockIdx.x];
    // a workgroup may mix systems (per-trajectory drives, e.g. one system per scan point): each wave reads the
    // free propagators of its own trajectory's system
    {
        const int sw = __builtin_amdgcn_readfirstlane(s_sys[tw]);
        Mg += (size_t)sw * p.m_stride;
        Fg += (size_t)sw * p.f_stride;
    }

    // ---- initial augmented states rho0 (x) bond0 (thread -> column)
    for (int c = tid; c < NCOL; c += NT) {
        const int cb = c / CHI, cd = c - (c / CHI) * CHI;
        const double2 b0 = p.bond0[cd];
#pragma unroll
        for (int a = 0; a < N2; ++a) st[cb * TS + a * RS + cd] = c_mul(p.rho0[a], b0);
    }
    __syncthreads();
    // ---- column phases: wave w owns trajectory w % BT (its free propagators, its MTO events), and with two
    // waves per trajectory the column tiles of half w / BT
    double2* stw = st + tw * TS;
    const bool c3 = LEAN || p.cmul3 != 0;
    const bool cbig = !LEAN && p.colbig != 0;
    auto col = [&](const double2* __restrict__ Op) {
        if (c3) {
            if constexpr (col_big_ok<N2, CHI, RS, WPT>()) {
                if (cbig) { col_apply_mfma3_big<N2, CHI, RS, WPT>(Op, stw, lane, half); return; }
            }
            col_apply_mfma3<N2, CHI, RS, WPT>(Op, stw, lane, half);
        } else {
            col_apply_mfma<N2, CHI, RS, WPT>(Op, stw, lane, half);
        }
    };
    int ev_cur = 0, ev_lim = 0;
    {
        const int t = s_traj[tw];
        if (t >= 0) { ev_cur = p.ev_start[t]; ev_lim = p.ev_start[t + 1]; }
        while (ev_cur < ev_lim) {  // applyBefore-true MTOs at step 0
            const int4 e = p.ev[ev_cur];
            if (e.x != 0 || e.y != 0) break;
            col(p.sop + (size_t)e.z * N2 * N2);
            ++ev_cur;
        }
    }
    __syncthreads();

    const int pj = lane & 15, pq = lane >> 4;
    // traces with one lane per (trajectory, output, row) when N2 is a power of two and they fit the workgroup
    // (16-lane reduction groups); each lane keeps the next step's W row element in a register
    const int ntr = BT * p.n_out * N2;
    const bool lanetr = LEAN || ((N2 == 4 || N2 == 16) && p.trpre && ntr <= NT);
    double2 wpre = c_zero();
    if (n0 > 0 && lanetr && tid < ntr) {  // the step the loop starts at: W(n0) row element, as fetched a step ahead
        const int a = tid % N2, bk = tid / N2, b = bk / p.n_out, k = bk - (bk / p.n_out) * p.n_out;
        wpre = Wg[(size_t)s_sys[b] * p.w_stride + ((size_t)n0 * p.n_out + k) * N2 + a];
    }
    bool fz = false;  // this wave's trajectory sits between M_b(n-1) and M_a(n) unapplied (fused step n)
    // lean: this wave's PT units (at most two, pqd_host.cpp) and the slice schedule around the current step, loaded
    // once or a step ahead through the scalar cache (the host wrote them before the launch; nothing here writes them)
    int4 u0 = make_int4(-1, 0, -1, -1), u1 = u0;
    int sc_prev = 0, sc_cur = 0, sc_nxt = 0;  // sched[n - 1], sched[n], sched[n + 1] (clamped to the schedule)
    if constexpr (LEAN) {
        u0 = ldc(p.units + (size_t)wave * p.umax);
        u1 = ldc(p.units + (size_t)wave * p.umax + 1);
        sc_prev = ldc(p.sched + (n0 > 0 ? n0 - 1 : 0));
        sc_cur = ldc(p.sched + (n0 < p.n_steps ? n0 : p.n_steps - 1));
    }
    // lean: the lane's part of the PT phase's addresses (slice offset in bytes, state-row read and write pointers)
    const unsigned lean_qoff = (unsigned)((pq * CHI + pj) * sizeof(double2));
    const double2* lean_xl = st + pq + (lane & 3) * TS;
    double2* lean_wl = st + pj + pq * TS;
    // lean: the fast region of the block (SweepParams::blk_fast) and, wave-uniform, the output window of this wave's slot
    // and its system's W rows, read once through the scalar cache
    int blk_fast = INT_MAX, w_beg = INT_MAX, w_end = -1;
    long long w_off = 0;
    const double2* Ww = Wg;
    if constexpr (LEAN) {
        if (p.blk_fast) blk_fast = ldc(p.blk_fast + blockIdx.x);
        const int t = __builtin_amdgcn_readfirstlane(s_traj[tw]);
        if (t >= 0) {
            w_beg = ldc(p.wbeg + t);
            w_end = ldc(p.wend + t);
            const int* wo = (const int*)(p.woff + t);
            w_off = (long long)(((unsigned long long)(unsigned)ldc(wo + 1) << 32) | (unsigned)ldc(wo));
            Ww += (size_t)ldc(p.traj_sys + t) * p.w_stride;
        }
    }
    for (int n = n0;; ++n) {
        // ------------------------------------------------------------ lean: the fast region, blk_fast <= n < n_end - 1
        // Every occupied slot is active, enters each of these steps fused and has no event left, so a step is the column
        // operator F(n) with the outputs read from its operands (LeanCol), a barrier, the PT phase and a barrier: no
        // closure pass, no partials in LDS, no fused flags written (they stay 1, as the last step before the region left
        // them) and no barrier at the end of the step (the column operator touches the wave's own trajectory only).
        // Every PT phase here loads the first slice k-step of the next one (LeanPt::run_pre), so the region ends a step
        // before the block's last PT step: steps n_end - 1 and n_end (outputs only) run below as before, the first of them
        // with its W row elements fetched here, and nothing is loaded for a step the block does not run.
        if constexpr (LEAN) {
            if (n >= blk_fast && n < n_end - 1) {
                using LC = LeanCol<RS, true>;
                typename LC::LdsC2* sb;
                {
                    unsigned v = (unsigned)(size_t)((typename LC::LdsC2*)stw + pq * RS + pj);
                    asm("" : "+v"(v));
                    sb = (typename LC::LdsC2*)v;
                }
                const bool occupied = my_act != INT_MAX;
                // A block whose slots share one system (SweepParams::blk_stage) takes F(n), the closure vector and W(n) from
                // LDS: the PT phase of step n - 1 staged them (LeanStage), and a prologue those of the region's first step.
                // The region's last PT phase stages nothing: step n_end - 1 loads for itself below. The two forms are two
                // loops (STG), so that neither carries the other's operands
                using LP = LeanPt<CHI, RS, TS, LEAN_PF>;
                using LS = LeanStage<BT * TS + BT * N2>;
                const int st_sys = p.blk_stage ? ldc(p.blk_stage + blockIdx.x) : -1;
                // PARTS: kcc is the number of k-steps of the column phase, 3 where the host compacted the live rows
                // (SweepParams::lean_colk, lean_rho), chosen once per launch like STG
                auto fast_steps = [&](auto stc, auto kcc) {
                    constexpr bool STG = decltype(stc)::value;
                    constexpr int KC = decltype(kcc)::value;
                    static_assert(KC == 4 || PARTS, "compacted rows come with partial units only");
                    typename LS::LdsC2* sg = LS::area(smem);
                    const double2* Fst = p.F + (size_t)(STG ? st_sys : 0) * p.f_stride;
                    const double2* Wst = Wg + (size_t)(STG ? st_sys : 0) * p.w_stride;
                    const unsigned st_off = LS::template lane_off<KC>(wave, lane, p.lean_rho), st_to = LS::dst(smem, wave);
                    const unsigned long long st_ln = LS::template lanes<KC>(wave, p.n_out);
                    // the lane's compacted addresses, pinned like sb (rho < 16: rows of the wave's own trajectory)
                    LeanColMap<KC> cm;
                    if constexpr (KC < 4) {
#pragma unroll
                        for (int ks = 0; ks < KC; ++ks) {
                            const int row = lean_rho(p.lean_rho, 4 * ks + pq);
                            unsigned v = (unsigned)(size_t)((typename LC::LdsC2*)stw + row * RS + pj);
                            int f = lean_rho(p.lean_rho, pj) * N2 + row;
                            asm("" : "+v"(v));
                            asm("" : "+v"(f));
                            cm.cb[ks] = (typename LC::LdsC2*)v;
                            cm.fo[ks] = f;
                        }
                    }
                    if constexpr (STG) {
                        LS::issue(LS::src(wave, Fst + (size_t)n * N2 * N2, p.closure + (size_t)sc_prev * CHI,
                                          Wst + (size_t)n * p.n_out * N2), st_off, st_to, st_ln);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __syncthreads();
                    }
                    // the first k-step of the wave's first unit, in flight from one step's PT phase to the next's
                    typename LP::dbl2 qn[LEAN_PF][CHI / 16];
                    if constexpr (PARTS) {
                        if (u0.x >= 0) LP::ldq_first_parts(qn, Qg0 + (size_t)sc_cur * p.D * CHI * CHI, u0, lean_qoff);
                    } else {
                        if (u0.x >= 0) LP::ldq_first(qn, Qg0 + ((size_t)sc_cur * p.D + u0.x) * CHI * CHI, lean_qoff);
                    }
                    for (; n < n_end - 1; ++n) {
                        sc_nxt = ldc(p.sched + (n + 1 < p.n_steps ? n + 1 : p.n_steps - 1));
                        if (occupied) {
                            const bool inwin = w_beg <= n && n <= w_end;   // the store's predicate: the slot's window, wave-uniform
                            if constexpr (STG) {
                                if (inwin)
                                    LeanCol<RS, true, true, KC>::run(sg + LS::F_AT, sg + LS::C_AT, sg + LS::W_AT, p.n_out, sb, cm,
                                                                     outg + w_off + (long long)(n - w_beg) * p.n_out, lane);
                                else
                                    LeanCol<RS, false, true, KC>::run(sg + LS::F_AT, nullptr, nullptr, 0, sb, cm, nullptr, lane);
                            } else {
                                const double2* Fn = Fg + (size_t)n * N2 * N2;
                                if (inwin)
                                    LeanCol<RS, true, false, KC>::run(Fn, p.closure + (size_t)sc_prev * CHI,
                                                                      Ww + (size_t)n * p.n_out * N2, p.n_out, sb, cm,
                                                                      outg + w_off + (long long)(n - w_beg) * p.n_out, lane);
                                else
                                    LeanCol<RS, false, false, KC>::run(Fn, nullptr, nullptr, 0, sb, cm, nullptr, lane);
                            }
                        }
                        __syncthreads();
                        if constexpr (STG) {
                            // step n + 1 <= n_end - 2 reads the closure vector of sched[n]
                            const LeanStageOp<LS> stg{LS::src(wave, Fst + (size_t)(n + 1) * N2 * N2,
                                                              p.closure + (size_t)sc_cur * CHI,
                                                              Wst + (size_t)(n + 1) * p.n_out * N2),
                                                      st_off, st_to, n + 2 < n_end ? st_ln : 0ull};
                            if constexpr (PARTS)
                                LP::run_pre_parts(qn, Qg0 + (size_t)sc_cur * p.D * CHI * CHI,
                                                  Qg0 + (size_t)sc_nxt * p.D * CHI * CHI, u0, u1, lean_qoff, lean_xl, lean_wl, stg);
                            else
                            LP::run_pre(qn, Qg0 + (size_t)sc_cur * p.D * CHI * CHI, Qg0 + (size_t)sc_nxt * p.D * CHI * CHI, u0,
                                        u1, lean_qoff, lean_xl, lean_wl, stg);
                        } else {
                            if constexpr (PARTS)
                                LP::run_pre_parts(qn, Qg0 + (size_t)sc_cur * p.D * CHI * CHI,
                                                  Qg0 + (size_t)sc_nxt * p.D * CHI * CHI, u0, u1, lean_qoff, lean_xl, lean_wl,
                                                  LeanNoStage{});
                            else
                            LP::run_pre(qn, Qg0 + (size_t)sc_cur * p.D * CHI * CHI, Qg0 + (size_t)sc_nxt * p.D * CHI * CHI, u0,
                                        u1, lean_qoff, lean_xl, lean_wl, LeanNoStage{});
                        }
                        __syncthreads();
                        sc_prev = sc_cur;
                        sc_cur = sc_nxt;
                    }
                };
                using KC4 = std::integral_constant<int, 4>;
                bool compact = false;
                if constexpr (PARTS) compact = p.lean_colk == 3;
                if (compact) {
                    if constexpr (PARTS) {
                        using KC3 = std::integral_constant<int, 3>;
                        if (st_sys >= 0) fast_steps(std::true_type{}, KC3{});
                        else fast_steps(std::false_type{}, KC3{});
                    }
                } else if (st_sys >= 0) fast_steps(std::true_type{}, KC4{});
                else fast_steps(std::false_type{}, KC4{});
                fz = true;
                if (tid < ntr) {  // W(n_end - 1) row element for the traces below
                    const int a = tid % N2, bk = tid / N2, b = bk / p.n_out, k = bk - (bk / p.n_out) * p.n_out;
                    wpre = Wg[(size_t)s_sys[b] * p.w_stride + ((size_t)n * p.n_out + k) * N2 + a];
                }
            }
        }
        // ------------------------------------------------------------ shared-trunk activations at step n
        if (n == next_act) {
            // a checkpoint (src <= -2) holds the trunk at the top of step n >= 1 with M_b(n-1) deferred (fused)
            if (tid < BT && s_act[tid] == n) s_fz[tid] = s_src[tid] >= 0 ? s_fz[s_src[tid]] : 1;
            for (int b = 0; b < BT; ++b) {
                if (s_act[b] != n) continue;
                double2* dp = st + b * TS;
                if (s_src[b] >= 0) {
                    const double2* sp = st + s_src[b] * TS;
                    for (int e = tid; e < N2 * CHI; e += NT) {
                        const int a = e / CHI, c = e - (e / CHI) * CHI;
                        dp[a * RS + c] = sp[a * RS + c];
                    }
                } else if (s_src[b] <= -2) {
                    const double2* cp = p.ck + (size_t)(-2 - s_src[b]) * N2 * CHI;
                    for (int e = tid; e < N2 * CHI; e += NT) {
                        const int a = e / CHI, c = e - (e / CHI) * CHI;
                        dp[a * RS + c] = cp[e];
                    }
                }
            }
            if (my_act == n) fz = s_src[tw] >= 0 ? (s_fz[s_src[tw]] != 0) : true;
            next_act = next_activation(n);
            __syncthreads();
        }
        // ------------------------------------------------------------ trunk pre-pass: checkpoints at step n
        if constexpr (TRUNK) {
            bool wrote = false;
            for (int b = 0; b < BT; ++b) {
                const int t = s_traj[b];
                const int c = t >= 0 ? p.ck_map[(size_t)t * p.ck_stride + n] : -1;
                if (c < 0) continue;
                wrote = true;
                double2* cp = p.ck + (size_t)c * N2 * CHI;
                for (int e = tid; e < N2 * CHI; e += NT) {
                    const int a = e / CHI, cc = e - (e / CHI) * CHI;
                    cp[e] = st[b * TS + a * RS + cc];
                }
            }
            if (wrote) __syncthreads();
        }
        // ------------------------------------------------------------ outputs at step n
        bool need = false;
#pragma unroll
        for (int b = 0; b < BT; ++b) need |= (s_wb[b] <= n) & (n <= s_we[b]);
        if (need && !(ablate & 4)) {
            const double2* cvec = (n == 0) ? p.closure0 : p.closure + (size_t)(LEAN ? sc_prev : p.sched[n - 1]) * CHI;
            constexpr int NPART = BT * N2 * 4;
            for (int it = 0; it < (NPART + NT - 1) / NT; ++it) {
                const int e = tid + NT * it;
                const int row = e >> 2, qr = e & 3;
                double2 s = c_zero();
                if (e < NPART) {
                    const int b = row / N2, a = row - (row / N2) * N2;
                    const double2* rp = st + b * TS + a * RS + qr;
#pragma unroll 4
                    for (int kk = 0; kk < CHI / 4; ++kk) c_fma(s, rp[4 * kk], cvec[4 * kk + qr]);
                }
                s = c_add(s, c_shfl_xor(s, 1));
                s = c_add(s, c_shfl_xor(s, 2));
                if (e < NPART && qr == 0) rbuf[row] = s;
            }
            __syncthreads();
            if (lanetr) {
                // one lane per (trajectory, output, row): the row element of W(n) was fetched a step ahead
                if (tid < ntr) {
                    const int a = tid % N2, bk = tid / N2, b = bk / p.n_out, k = bk - (bk / p.n_out) * p.n_out;
                    const double2 v = s_fz[b] ? wpre : p.ovec[k * N2 + a];
                    double2 x = c_mul(v, rbuf[b * N2 + a]);
#pragma unroll
                    for (int m = 1; m < N2; m <<= 1) x = c_add(x, c_shfl_xor(x, m));
                    if (a == 0 && s_wb[b] <= n && n <= s_we[b])
                        outg[s_wo[b] + (long long)(n - s_wb[b]) * p.n_out + k] = x;
                }
            } else
            for (int e = tid; e < BT * p.n_out; e += NT) {
                const int b = e / p.n_out, k = e - (e / p.n_out) * p.n_out;
                if (s_wb[b] <= n && n <= s_we[b]) {
                    double2 s = c_zero();
                    // fused trajectories still hold the state before M_b(n-1): read it through W(n)
                    const double2* ov = (s_fz[b] ? Wg + (size_t)s_sys[b] * p.w_stride + (size_t)n * p.n_out * N2
                                                 : p.ovec) + (size_t)k * N2;
                    // all of a chunk's row loads are issued before its first FMA (one memory round trip per
                    // chunk, not one per few elements: the scheduler otherwise interleaves them)
                    constexpr int CK = N2 <= 16 ? N2 : 9;
#pragma unroll
                    for (int a0 = 0; a0 < N2; a0 += CK) {
                        double2 ovr[CK];
#pragma unroll
                        for (int j = 0; j < CK; ++j) ovr[j] = (a0 + j < N2) ? ov[a0 + j] : c_zero();
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int j = 0; j < CK; ++j)
                            if (a0 + j < N2) c_fma(s, ovr[j], rbuf[b * N2 + a0 + j]);
                    }
                    outg[s_wo[b] + (long long)(n - s_wb[b]) * p.n_out + k] = s;
                }
            }
        }
        if (n >= n_end) break;
        if constexpr (LEAN) sc_nxt = ldc(p.sched + (n + 1 < p.n_steps ? n + 1 : p.n_steps - 1));
        if (lanetr && tid < ntr) {  // W(n + 1) row element for the next step's traces (fused trajectories)
            const int a = tid % N2, bk = tid / N2, b = bk / p.n_out, k = bk - (bk / p.n_out) * p.n_out;
            wpre = Wg[(size_t)s_sys[b] * p.w_stride + ((size_t)(n + 1) * p.n_out + k) * N2 + a];
        }

        // ------------------------------------------------------------ column phase A
        const double2* Ma = Mg + (size_t)(2 * n) * N2 * N2;
        if (!(ablate & 2) && n >= my_act) {
            const bool mto_now = ev_cur < ev_lim && p.ev[ev_cur].x == n;
            if (fz && !mto_now) {  // no MTO at step n: M_b(n-1) and M_a(n) in one operator
                col(Fg + (size_t)n * N2 * N2);
            } else {
                // a slot activated at n holds the trunk's state with M_b(n-1) still deferred, but has an MTO at n
                if (fz) col(Mg + (size_t)(2 * n - 1) * N2 * N2);
                while (ev_cur < ev_lim) {  // applyBefore-false MTOs at step n
                    const int4 e = p.ev[ev_cur];
                    if (e.x != n || e.y != 1) break;
                    col(p.sop + (size_t)e.z * N2 * N2);
                    ++ev_cur;
                }
                col(Ma);
            }
        }
        __syncthreads();

        // ------------------------------------------------------------ PT contraction
        if constexpr (LEAN) {
            // 3M rows of this wave's one or two units (LeanPt above)
            const double2* Qs = Qg0 + (size_t)sc_cur * p.D * CHI * CHI;
            if constexpr (PARTS) LeanPt<CHI, RS, TS, LEAN_PF>::run_parts(Qs, u0, u1, lean_qoff, lean_xl, lean_wl);
            else LeanPt<CHI, RS, TS, LEAN_PF>::run(Qs, u0, u1, lean_qoff, lean_xl, lean_wl);
        } else if (!(ablate & 1)) {
            pt_phase<N2, CHI, BT>(p, Qg0 + (size_t)p.sched[n] * p.D * CHI * CHI, st, wave, lane);
        }
        __syncthreads();

        // ------------------------------------------------------------ column phase B
        const double2* Mb = Ma + N2 * N2;
        // fuse M_b(n) into the next step's operator unless this trajectory has an MTO at step n+1
        fz = (LEAN || p.fuse) && !(ev_cur < ev_lim && p.ev[ev_cur].x == n + 1);
        if (!(ablate & 2) && !fz && n >= my_act) {
            col(Mb);
            while (ev_cur < ev_lim) {  // applyBefore-true MTOs at step n+1
                const int4 e = p.ev[ev_cur];
                if (e.x != n + 1 || e.y != 0) break;
                col(p.sop + (size_t)e.z * N2 * N2);
                ++ev_cur;
            }
        }
        if (lane == 0 && half == 0) s_fz[tw] = fz ? 1 : 0;
        if constexpr (LEAN) { sc_prev = sc_cur; sc_cur = sc_nxt; }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// chi = 1 (no environment): one wave per trajectory, lane r owns rho[r]; operators applied through
// cross-lane shuffles (no LDS, no barriers). Latency-bound by construction (C1: 1 trajectory).
// ------------------------------------------------------------------------------------------------
template <int N2>
__device__ __forceinline__ double2 lane_apply(const double2* __restrict__ Op, double2 own, int lane) {
    const int r = lane < N2 ? lane : N2 - 1;
    const double2* Or = Op + r * N2;
    double2 acc = c_zero();
#pragma unroll
    for (int a = 0; a < N2; ++a) {
        const double2 x = make_double2(__shfl(own.x, a), __shfl(own.y, a));
        c_fma(acc, Or[a], x);
    }
    return acc;
}

template <int N2>
__global__ __launch_bounds__(64) void sweep_nopt_kernel(SweepParams p) {
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    const int wb = p.wbeg[t], we = p.wend[t];
    const long long wo = p.woff[t];
    int ev_cur = p.ev_start[t];
    const int sy = p.traj_sys[t];
    const int2 wn = fw_win(p, sy);  // pulse windows (pqd_host.cpp: only plans whose kernels all read through them)
    const int ev_lim = p.ev_start[t + 1];
    double2 own = lane < N2 ? p.rho0[lane] : c_zero();
    while (ev_cur < ev_lim) {
        const int4 e = p.ev[ev_cur];
        if (e.x != 0 || e.y != 0) break;
        own = lane_apply<N2>(p.sop + (size_t)e.z * N2 * N2, own, lane);
        ++ev_cur;
    }
    for (int n = 0;; ++n) {
        if (wb <= n && n <= we) {
            // every lane gathers the state (all lanes take part in the shuffles), then lane k owns outputs
            // k, k + 64, ... (n_out may exceed the wave)
            double2 x[N2];
#pragma unroll
            for (int a = 0; a < N2; ++a) x[a] = make_double2(__shfl(own.x, a), __shfl(own.y, a));
            for (int k = lane; k < p.n_out; k += 64) {
                double2 s = c_zero();
                const double2* ov = p.ovec + (size_t)k * N2;
#pragma unroll
                for (int a = 0; a < N2; ++a) c_fma(s, ov[a], x[a]);
                p.out[wo + (long long)(n - wb) * p.n_out + k] = s;
            }
        }
        if (n >= we) break;
        while (ev_cur < ev_lim) {
            const int4 e = p.ev[ev_cur];
            if (e.x != n || e.y != 1) break;
            own = lane_apply<N2>(p.sop + (size_t)e.z * N2 * N2, own, lane);
            ++ev_cur;
        }
        own = lane_apply<N2>(fw_M(p, sy, wn, 2 * n, N2 * N2), own, lane);
        own = lane_apply<N2>(fw_M(p, sy, wn, 2 * n + 1, N2 * N2), own, lane);
        while (ev_cur < ev_lim) {
            const int4 e = p.ev[ev_cur];
            if (e.x != n + 1 || e.y != 0) break;
            own = lane_apply<N2>(p.sop + (size_t)e.z * N2 * N2, own, lane);
            ++ev_cur;
        }
    }
}

template <int N2, int CHI, int BT, bool TRUNK, bool LEAN = false, bool PARTS = false>
hipError_t launch_sw(int n_blocks, const SweepParams& p, hipStream_t s) {
    using L = SweepLayout<N2, CHI, BT>;
    // the lean instance: the staging area of its fast region behind rbuf (LeanStage; 6 KiB of the 27.8 KiB left)
    constexpr size_t LDS = L::LDS + (LEAN ? LeanStage<BT * L::TS + BT * N2>::BYTES : 0);
    static_assert((BT * L::TS + BT * N2) * sizeof(double2) == L::LDS, "the area starts where the states and rbuf end");
    static_assert(LDS + 512 <= 160 * 1024, "LDS budget (512 B: the kernel's static tables)");
    if (hipError_t e = allow_dyn_lds<&pt_sweep_kernel<N2, CHI, BT, TRUNK, LEAN, PARTS>>(LDS); e != hipSuccess) return e;
    hipLaunchKernelGGL((pt_sweep_kernel<N2, CHI, BT, TRUNK, LEAN, PARTS>), dim3(n_blocks), dim3(64 * L::NW), LDS, s, p, p.M,
                       p.Q, p.out, p.F, p.W);
    return hipGetLastError();
}

// the instance set: BT = 8 trajectories per workgroup fit the LDS up to N2 = 16, and chi = 128 keeps 4 augmented
// states of N2 <= 16 there (132 KiB); larger N2 or BT do not fit
constexpr int sw_max_bt(int N2) { return N2 <= 16 ? 8 : 4; }
constexpr bool sw_instance(int N2, int CHI, int BT) {
    return n2_listed(N2) && (BT == 4 || (BT == 8 && sw_max_bt(N2) == 8)) &&
           (CHI == 16 || CHI == 32 || CHI == 64 || (CHI == 128 && BT == 4 && N2 <= 16));
}

template <int N2, int BT, bool TRUNK = false>
hipError_t launch_sw_chi(int CHI, int n_blocks, const SweepParams& p, hipStream_t s) {
    return dispatch_list<16, 32, 64, 128>(CHI, [&](auto C) -> hipError_t {
        if constexpr (sw_instance(N2, KV(C), BT)) return launch_sw<N2, KV(C), BT, TRUNK>(n_blocks, p, s);
        else return hipErrorInvalidValue;
    });
}

}  // namespace

// (chi = 1: the kernel without a PT, launch_sweep_nopt)
bool sweep_supported(int N2, int CHI) { return n2_listed(N2) && (CHI == 1 || sw_instance(N2, CHI, 4)); }

// trajectories per workgroup that fit the LDS for this N2 (8 halves the per-trajectory PT-slice traffic)
int sweep_max_bt(int N2) { return sw_max_bt(N2); }

hipError_t launch_sweep(int N2, int CHI, int BT, int n_blocks, const SweepParams& p, hipStream_t s) {
    if (n_blocks <= 0) return hipSuccess;
    if (BT != 4 && (BT != 8 || p.ck_map)) return hipErrorInvalidValue;
    return dispatch_n2(N2, [&](auto NN) -> hipError_t {
        constexpr int N = KV(NN);
        if (p.ck_map) return launch_sw_chi<N, 4, true>(CHI, n_blocks, p, s);  // trunk pre-pass: four trunks per workgroup
        if (BT == 4) return launch_sw_chi<N, 4>(CHI, n_blocks, p, s);
        if constexpr (sw_max_bt(N) == 8) {
            if constexpr (N == 16) {
                if (p.lean && p.lean_parts && CHI == 64) return launch_sw<16, 64, 8, false, true, true>(n_blocks, p, s);
                if (p.lean && CHI == 64) return launch_sw<16, 64, 8, false, true>(n_blocks, p, s);
                if (p.lean_parts) return hipErrorInvalidValue;  // a list with partial units is the lean instance's alone
            }
            return launch_sw_chi<N, 8>(CHI, n_blocks, p, s);
        }
        return hipErrorInvalidValue;
    });
}

hipError_t launch_sweep_nopt(int N2, int n_traj, const SweepParams& p, hipStream_t s) {
    if (n_traj <= 0) return hipSuccess;
    return dispatch_n2(N2, [&](auto NN) {
        hipLaunchKernelGGL(sweep_nopt_kernel<KV(NN)>, dim3(n_traj), dim3(64), 0, s, p);
        return hipGetLastError();
    });
}
