// Streaming quantiles of a device-resident chain by the extended P² algorithm (include/nhp.h: nhp_cont_model_quantiles_*,
// nhp_disc_model_quantiles_*): the state, the one update every entry takes, and the sources of x.  What differs
// between the models is where an entry's value comes from -- the continuous parameter block, the discrete block, the product
// W∘θ of a standard discrete process -- so each is a small functor and the seam, the A·W product and the W∘θ product live in
// one place each; everything else is chain_quantiles.hip's, once.
#pragma once
#include "nhp_internal.h"

#define NHP_QUANT_KMAX (2 * NHP_QUANT_MAX + 3)

// the marker probabilities d_0 … d_{K−1}, made on the host as include/nhp.h writes them and handed to the kernel by value
struct nhp_quant_probs { double d[NHP_QUANT_KMAX]; };

struct nhp_quant_state {
    int32_t m = 0, every = 1, effective = 0;
    int64_t len = 0;                        // the sums' length (what _fetch is asked for)
    int64_t P = 0;                          // entries with a state; the scalar ρ's is entry P: the planes are P + 1 wide
    int64_t count = 0;                      // n: values every entry has seen
    int64_t kept = 0;                       // kept steps the driver has counted (it feeds those with kept % every == 0)
    double probs[NHP_QUANT_MAX] = {0.0, 0.0, 0.0, 0.0};
    nhp_quant_probs d;
    double *d_q = nullptr;                  // ONE allocation: heights [K][P + 1] fp64, then positions [K − 2][P + 1] int32
    int32_t *d_pos = nullptr;
};

// ---- the sources of x -----------------------------------------------------------------------------------------------------
// continuous: entry i of [λ0; θ | μ; τ; W]; with effective weights (A non-null) W[p,c] is fed as A[p,c]·W[p,c], one product
struct quant_src_cont {
    const double *params, *A;
    int64_t W;                              // first entry of W (it is the last table: W … P − 1)
    __device__ __forceinline__ double operator()(int64_t i) const
    {
#pragma clang fp contract(off)
        const double x = params[i];
        if (A && i >= W) { const double a = A[i - W]; return a * x; }
        return x;
    }
};

// discrete network process: entry i of the block [λ0; vec(W); vec(θ)]; effective weights as above
struct quant_src_disc_block {
    const double *block, *A;
    int64_t N, NN;
    __device__ __forceinline__ double operator()(int64_t i) const
    {
#pragma clang fp contract(off)
        const double x = block[i];
        if (A && i >= N && i < N + NN) { const double a = A[i - N]; return a * x; }
        return x;
    }
};

// discrete standard process: [λ0; vec(W∘θ)], x = W[p,c]·θ[p,c,b] as ONE rounded product -- the expression of disc_entry
// (disc_chain.hip), so the quantiles see the value the sums see, bit for bit
struct quant_src_disc_product {
    const double *block;
    int64_t N, NN;
    bool narrow;                            // 32-bit remainder where the indices fit
    __device__ __forceinline__ double operator()(int64_t i) const
    {
#pragma clang fp contract(off)
        if (i < N) return block[i];
        const int64_t j = i - N;            // p + N·c + N²·b
        const int64_t pc = narrow ? (int64_t)((uint32_t)j % (uint32_t)NN) : j % NN;
        const double w = block[N + pc], t = block[N + NN + j];
        const double x = w * t;
        return x;
    }
};

// ---- one value into one entry's markers ---------------------------------------------------------------------------------------
// Entry e of planes S wide; n = values seen before this one (the same for every entry: the warm-up branch is uniform).  All K
// heights and K − 2 positions sit in registers: every loop below has a compile-time trip count and every index is a constant
// after unrolling -- the search for k, the warm-up insertion and the choice of q_{i+s} / pos_{i+s} are compare/select chains,
// never an array indexed by a run-time value, which would go to scratch.  Expressions and their order: include/nhp.h.
template <int M>
__device__ __forceinline__ void quant_feed(double x, double *__restrict__ qp, int32_t *__restrict__ pp, int64_t S, int64_t e, int32_t n,
                                           const nhp_quant_probs &D)
{
#pragma clang fp contract(off)
    constexpr int K = 2 * M + 3;
    double q[K];
#pragma unroll
    for (int i = 0; i < K; ++i) q[i] = qp[(int64_t)i * S + e];
    if (n < K) {
        // warm-up: x goes behind the j values of the sorted prefix q_0 … q_{n−1} that are <= x
        int j = 0;
#pragma unroll
        for (int i = 0; i < K - 1; ++i) j += (i < n && q[i] <= x) ? 1 : 0;
#pragma unroll
        for (int i = K - 1; i >= 1; --i)
            if (i <= n) q[i] = i > j ? q[i - 1] : (i == j ? x : q[i]);
        if (j == 0) q[0] = x;
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (i <= n) qp[(int64_t)i * S + e] = q[i];
        if (n == K - 1) {
#pragma unroll
            for (int i = 1; i <= K - 2; ++i) pp[(int64_t)(i - 1) * S + e] = i + 1;
        }
        return;
    }
    int32_t pos[K];
    pos[0] = 1;
    pos[K - 1] = n;
#pragma unroll
    for (int i = 1; i <= K - 2; ++i) pos[i] = pp[(int64_t)(i - 1) * S + e];
    // 1. the cell x falls into; the extremes take x
    const bool lo = x < q[0], hi = !lo && x >= q[K - 1];
    int k = 0;
#pragma unroll
    for (int i = 1; i <= K - 2; ++i) k = q[i] <= x ? i : k;
    k = lo ? 0 : (hi ? K - 2 : k);
    q[0] = lo ? x : q[0];
    q[K - 1] = hi ? x : q[K - 1];
    // 2. the markers above the cell move up one place
#pragma unroll
    for (int i = 1; i <= K - 2; ++i) pos[i] += i > k ? 1 : 0;
    pos[K - 1] = n + 1;
    const double nm1 = (double)n;           // (n + 1) − 1
    // 3. each inner marker, in ascending order, one place towards its desired position when it is off by one or more
#pragma unroll
    for (int i = 1; i <= K - 2; ++i) {
        const double delta = (1.0 + nm1 * D.d[i]) - (double)pos[i];
        int s = 0;
        if (delta >= 1.0 && pos[i + 1] - pos[i] > 1) s = 1;
        else if (delta <= -1.0 && pos[i - 1] - pos[i] < -1) s = -1;
        if (s != 0) {
            const double sd = (double)s;
            const double a = (double)(pos[i] - pos[i - 1]), b = (double)(pos[i + 1] - pos[i]), c = (double)(pos[i + 1] - pos[i - 1]);
            const double t1 = ((a + sd) * (q[i + 1] - q[i])) / b;
            const double t2 = ((b - sd) * (q[i] - q[i - 1])) / a;
            const double qn = q[i] + (sd / c) * (t1 + t2);
            if (q[i - 1] < qn && qn < q[i + 1]) q[i] = qn;
            else {
                const double qs = s > 0 ? q[i + 1] : q[i - 1];
                const int32_t ps = s > 0 ? pos[i + 1] : pos[i - 1];
                q[i] = q[i] + (sd * (qs - q[i])) / (double)(ps - pos[i]);
            }
            pos[i] += s;
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) qp[(int64_t)i * S + e] = q[i];
#pragma unroll
    for (int i = 1; i <= K - 2; ++i) pp[(int64_t)(i - 1) * S + e] = pos[i];
}
