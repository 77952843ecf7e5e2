// Does the f64 MFMA accumulate k as one ordered chain of FMAs (one rounding per product, k ascending, chained through
// the C operand from instruction to instruction)? The lean sweep's compacted column phase (pt_sweep.hip LeanCol, KC = 3)
// is bit-identical to the four-k-step form only if it does. Stand-alone, under a second:
//   hipcc --offload-arch=gfx950 -O2 scripts/ubench_mfma_f64_korder.hip -o ubench_mfma_f64_korder && ./ubench_mfma_f64_korder
// For v_mfma_f64_16x16x4_f64 and v_mfma_f64_4x4x4_4b_f64, over TRIALS sets of random finite operands:
//   (a) a 4-instruction chain over 16 k equals, bit for bit, the host's fma chain in k order;
//   (b) the same chain with the B values of k in {2, 6, 8, 9, 11, 14} zeroed equals the 3-instruction chain over the
//       10 other k in increasing order followed by two k whose B value is zero (the A values stay random, as F's
//       entries from a dead column may).
// The lane layout is not assumed beyond k = lane >> 4 for both operands: a first kernel multiplies unit vectors and
// records which D elements every (A lane, B lane) pair reaches; main() checks that the pairs of every D element are
// four, one per k.
// Exit status 0: all four checks hold; 1: one does not (the line says which); 2: layout or HIP error.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
typedef double dbl4 __attribute__((ext_vector_type(4)));

#define CHK(x)                                                                         \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);      \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

constexpr int TRIALS = 512, KSTEPS = 4, KC = 3;

// I = 0: 16x16x4 (4 D values per lane), I = 1: 4x4x4_4b (1 D value per lane)
template <int I> struct Acc;
template <> struct Acc<0> {
    static constexpr int R = 4;
    dbl4 v = dbl4{0, 0, 0, 0};
    __device__ void mac(double a, double b) { v = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, v, 0, 0, 0); }
    __device__ double get(int r) const { return v[r]; }
};
template <> struct Acc<1> {
    static constexpr int R = 1;
    double v = 0;
    __device__ void mac(double a, double b) { v = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, v, 0, 0, 0); }
    __device__ double get(int) const { return v; }
};

// reach[(la * 64 + lb) * R + r]: the lanes whose D value r receives A lane la times B lane lb
template <int I>
__global__ void reach_kernel(unsigned long long* reach) {
    const int l = threadIdx.x;
    for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb) {
            Acc<I> c;
            c.mac(l == la ? 1.0 : 0.0, l == lb ? 1.0 : 0.0);
            for (int r = 0; r < Acc<I>::R; ++r) {
                const unsigned long long m = __ballot(c.get(r) != 0.0);
                if (l == 0) reach[(la * 64 + lb) * Acc<I>::R + r] = m;
            }
        }
}

// one trial per block: d[(trial * 64 + lane) * R + r] after `steps` chained instructions on a, b[(trial * steps + s) * 64 + lane]
template <int I>
__global__ void chain_kernel(const double* a, const double* b, double* d, int steps) {
    const int l = threadIdx.x, t = blockIdx.x;
    Acc<I> c;
    for (int s = 0; s < steps; ++s) c.mac(a[(t * steps + s) * 64 + l], b[(t * steps + s) * 64 + l]);
    for (int r = 0; r < Acc<I>::R; ++r) d[(t * 64 + l) * Acc<I>::R + r] = c.get(r);
}

static uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

template <int I>
static int run(const char* name) {
    constexpr int R = Acc<I>::R;
    // ---- layout: the four (A lane, B lane) pairs of every D element, by k = lane >> 4
    unsigned long long* dreach;
    std::vector<unsigned long long> reach((size_t)64 * 64 * R);
    CHK(hipMalloc(&dreach, reach.size() * 8));
    hipLaunchKernelGGL(reach_kernel<I>, dim3(1), dim3(64), 0, 0, dreach);
    CHK(hipMemcpy(reach.data(), dreach, reach.size() * 8, hipMemcpyDeviceToHost));
    std::vector<int> pa((size_t)64 * R * 4, -1), pb((size_t)64 * R * 4, -1);  // [(lane * R + r) * 4 + k]
    for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb)
            for (int r = 0; r < R; ++r) {
                const unsigned long long m = reach[(la * 64 + lb) * R + r];
                for (int l = 0; l < 64; ++l) {
                    if (!((m >> l) & 1)) continue;
                    const int k = la >> 4;
                    if ((lb >> 4) != k || pa[(l * R + r) * 4 + k] >= 0) {
                        printf("%s: layout: D lane %d value %d gets A lane %d x B lane %d (not one pair per k = lane >> 4)\n",
                               name, l, r, la, lb);
                        return 2;
                    }
                    pa[(l * R + r) * 4 + k] = la;
                    pb[(l * R + r) * 4 + k] = lb;
                }
            }
    for (int v : pa)
        if (v < 0) { printf("%s: layout: a D element with fewer than four products\n", name); return 2; }

    // ---- operands: signs and exponents spread over +-20 binades, so that sums cancel and every rounding shows
    std::mt19937_64 rng(20260 + I);
    std::uniform_real_distribution<double> mant(1.0, 2.0);
    std::uniform_int_distribution<int> ex(-20, 20), sg(0, 1);
    auto rnd = [&] { return (sg(rng) ? -1.0 : 1.0) * std::ldexp(mant(rng), ex(rng)); };
    const size_t NF = (size_t)TRIALS * KSTEPS * 64, NCP = (size_t)TRIALS * KC * 64;
    std::vector<double> a(NF), b(NF), bz(NF), ac(NCP), bc(NCP);
    for (size_t i = 0; i < NF; ++i) { a[i] = rnd(); b[i] = rnd(); }
    const bool dead[16] = {0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0};
    int rho[16], nl = 0;
    for (int k = 0; k < 16; ++k) if (!dead[k]) rho[nl++] = k;
    for (int k = 0; k < 16; ++k) if (dead[k]) rho[nl++] = k;
    // zeroed: B of logical k = 4 s + (lane >> 4); compacted: compact k c takes the operands of k = rho[c], of the same
    // lane & 15
    for (int t = 0; t < TRIALS; ++t) {
        for (int s = 0; s < KSTEPS; ++s)
            for (int l = 0; l < 64; ++l) {
                const size_t i = ((size_t)t * KSTEPS + s) * 64 + l;
                bz[i] = dead[4 * s + (l >> 4)] ? 0.0 : b[i];
            }
        for (int s = 0; s < KC; ++s)
            for (int l = 0; l < 64; ++l) {
                const int k = rho[4 * s + (l >> 4)];
                const size_t from = ((size_t)t * KSTEPS + (k >> 2)) * 64 + 16 * (k & 3) + (l & 15);
                ac[((size_t)t * KC + s) * 64 + l] = a[from];
                bc[((size_t)t * KC + s) * 64 + l] = bz[from];
            }
    }
    double *da, *db, *dd;
    const size_t ND = (size_t)TRIALS * 64 * R;
    std::vector<double> d_full(ND), d_zero(ND), d_comp(ND);
    CHK(hipMalloc(&da, NF * 8));
    CHK(hipMalloc(&db, NF * 8));
    CHK(hipMalloc(&dd, ND * 8));
    auto chain = [&](const std::vector<double>& A, const std::vector<double>& B, int steps, std::vector<double>& D) {
        if (hipMemcpy(da, A.data(), A.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
        if (hipMemcpy(db, B.data(), B.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
        hipLaunchKernelGGL(chain_kernel<I>, dim3(TRIALS), dim3(64), 0, 0, da, db, dd, steps);
        return hipMemcpy(D.data(), dd, ND * 8, hipMemcpyDeviceToHost) == hipSuccess;
    };
    if (!chain(a, b, KSTEPS, d_full) || !chain(a, bz, KSTEPS, d_zero) || !chain(ac, bc, KC, d_comp)) {
        printf("%s: HIP error %s\n", name, hipGetErrorString(hipGetLastError()));
        return 2;
    }
    // ---- (a) against the host's k-ordered fma chain, for the full and the zeroed operands; (b) zeroed against compacted
    size_t bad_a = 0, bad_az = 0, bad_b = 0, nonzero = 0;
    for (int t = 0; t < TRIALS; ++t)
        for (int l = 0; l < 64; ++l)
            for (int r = 0; r < R; ++r) {
                double h = 0, hz = 0;
                for (int s = 0; s < KSTEPS; ++s)
                    for (int k = 0; k < 4; ++k) {
                        const size_t ia = ((size_t)t * KSTEPS + s) * 64 + pa[(l * R + r) * 4 + k];
                        const size_t ib = ((size_t)t * KSTEPS + s) * 64 + pb[(l * R + r) * 4 + k];
                        h = std::fma(a[ia], b[ib], h);
                        hz = std::fma(a[ia], bz[ib], hz);
                    }
                const size_t i = ((size_t)t * 64 + l) * R + r;
                bad_a += bits(h) != bits(d_full[i]);
                bad_az += bits(hz) != bits(d_zero[i]);
                bad_b += bits(d_zero[i]) != bits(d_comp[i]);
                nonzero += d_zero[i] != 0.0;
            }
    printf("%s: %zu D elements in %d trials (%zu nonzero with the six k zeroed)\n", name, ND, TRIALS, nonzero);
    printf("%s (a) 4-instruction chain over 16 k  vs host fma chain in k order: %zu differ -> %s\n", name, bad_a,
           bad_a ? "FAIL" : "bit-equal");
    printf("%s (a) the same with k in {2,6,8,9,11,14} zeroed vs host fma chain: %zu differ -> %s\n", name, bad_az,
           bad_az ? "FAIL" : "bit-equal");
    printf("%s (b) zeroed 4-instruction chain vs 3-instruction chain over the 10 compacted k + 2 zeros: %zu differ -> %s\n",
           name, bad_b, bad_b ? "FAIL" : "bit-equal");
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dd); (void)hipFree(dreach);
    return (bad_a || bad_az || bad_b) ? 1 : 0;
}

int main() {
    const int r0 = run<0>("v_mfma_f64_16x16x4_f64");
    const int r1 = run<1>("v_mfma_f64_4x4x4_4b_f64");
    printf("result: 16x16x4 %s, 4x4x4_4b %s\n", r0 == 0 ? "ordered fma chain" : r0 == 1 ? "NOT an ordered fma chain" : "error",
           r1 == 0 ? "ordered fma chain" : r1 == 1 ? "NOT an ordered fma chain" : "error");
    return r0 > r1 ? r0 : r1;
}
