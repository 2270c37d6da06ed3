// The pieces of the generation-wise branching simulators shared by cont_simulate.hip (rand from time zero) and
// cont_forecast.hip (continuations of an observed history): the run scalars, the exact Poisson sampler, the row-prefix
// table of W∘A with the parameter checks, and the readback helpers.  Kernels are static: one copy per translation unit.
#pragma once
#include <math.h>

#include "nhp_dd.h"
#include "nhp_rng.h"

#define SIM_BLOCK 256
#define SIM_ROWS 64                                   // rows of the W∘A prefix table per workgroup (one wave)
#define SIM_CHUNK_MIN ((int64_t)1 << 12)
#define SIM_CHUNK_MAX ((int64_t)1 << 20)
#define SIM_PTRS_MIN 10.0                             // Poisson means from here on: PTRS; below: inversion
#define SIM_MAX_ATTEMPTS 4096u                        // PTRS attempts per draw (each accepts with probability > 0.9)

struct sim_scal {
    long long fill;                  // events kept so far (may pass max_events: nothing past it is written)
    unsigned long long next;         // child slots of the generation being stored
    int bad;                         // 1: weights / impulse parameters, 2: baseline
    int pad;
};

static __device__ __forceinline__ double sim_u01(double ua) { return ua - 0x1p-53; }        // (0,1] -> [0,1), exact

// log Γ(x) for x >= 1: the Stirling series at x0 = max(x, 7) and the recurrence down to x (the loggam of the PTRS
// literature; the library lgamma would cost every Poisson draw 340 bytes of scratch per lane)
static __device__ double sim_loggam(double x)
{
#pragma clang fp contract(off)
    if (x == 1.0 || x == 2.0) return 0.0;
    const int n = x < 7.0 ? (int)(7.0 - x) : 0;
    double x0 = x + n;
    const double x2 = (1.0 / x0) * (1.0 / x0);
    const double c[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                          8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                          1.796443723688307e-01, -1.39243221690590e+00};
    double g = c[9];
    for (int k = 8; k >= 0; --k) g = g * x2 + c[k];
    double gl = g / x0 + 0.5 * 1.8378770664093453e+00 + (x0 - 0.5) * nhp_log(x0) - x0;
    for (int k = 1; k <= n; ++k) { gl -= nhp_log(x0 - 1.0); x0 -= 1.0; }
    return gl;
}

// Poisson(mean), exact: inversion below SIM_PTRS_MIN (one uniform, attempt 0), PTRS above it (Hörmann 1993, the
// transformed rejection with squeeze; one Philox block per attempt: U from the first uniform, V from the second)
static __device__ double sim_poisson(double mean, uint64_t key, uint64_t step, uint64_t e)
{
#pragma clang fp contract(off)
    if (!(mean > 0.0)) return 0.0;
    double ua, ub;
    if (mean < SIM_PTRS_MIN) {
        philox_2u(key, step, e, 0, &ua, &ub);
        const double u = sim_u01(ua);
        double p = nhp_exp(-mean), F = p, k = 0.0;
        while (u >= F && k < 100.0) {
            k += 1.0;
            p = p * mean / k;
            F = F + p;
        }
        return k;
    }
    const double slam = sqrt(mean), loglam = nhp_log(mean);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    const double lia = nhp_log(invalpha);
    for (uint32_t att = 0; att < SIM_MAX_ATTEMPTS; ++att) {
        philox_2u(key, step, e, att, &ua, &ub);
        const double U = sim_u01(ua) - 0.5, V = ub;
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + mean + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (nhp_log(V) + lia - nhp_log(a / (us * us) + b) <= -mean + k * loglam - sim_loggam(k + 1.0)) return k;
    }
    return floor(mean);              // not reached: every attempt accepts with probability > 0.9
}

// wave sum of v, added to *dst by lane 0 (every lane of the wave calls it)
static __device__ __forceinline__ void sim_wave_add(unsigned long long v, unsigned long long *dst)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// ---- setup: the row-wise prefix table of W∘A, its row totals, and the parameter checks -----------------------------
// One lane per row p, a sequential running sum over c (so the table is monotone and a zero-weight entry equals the one
// before it exactly: it can never be chosen).  The model's tables are column-major: column c of 64 rows is one coalesced
// read; the running sums go through an LDS tile and leave row by row, again coalesced.
static __global__ void __launch_bounds__(SIM_ROWS) k_sim_rows(const double *__restrict__ W, const double *__restrict__ A,
                                                       const double *__restrict__ p1, const double *__restrict__ p2, int32_t N,
                                                       int32_t impulse_kind, double *__restrict__ G, double *__restrict__ R,
                                                       sim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    __shared__ double tile[SIM_ROWS][SIM_ROWS + 1];
    const int32_t p0 = blockIdx.x * SIM_ROWS, tx = threadIdx.x, p = p0 + tx;
    double run = 0.0;
    int bad = 0;
    for (int32_t c0 = 0; c0 < N; c0 += SIM_ROWS) {
        const int32_t nc = min(SIM_ROWS, N - c0);
        if (p < N) {
#pragma unroll 16
            for (int32_t k = 0; k < SIM_ROWS; ++k) {
                if (k < nc) {
                    const size_t q = (size_t)p + (size_t)(c0 + k) * N;
                    const double v = A ? W[q] * A[q] : W[q];
                    bad |= !(v >= 0.0 && v < INFINITY);
                    if (v > 0.0)
                        bad |= impulse_kind == NHP_IMPULSE_EXPONENTIAL ? !(p1[q] > 0.0 && p1[q] < INFINITY)
                                                                       : !(fabs(p1[q]) < INFINITY && p2[q] > 0.0 && p2[q] < INFINITY);
                    run = run + v;
                    tile[tx][k] = run;
                }
            }
        }
        __syncthreads();
        for (int32_t r = 0; r < SIM_ROWS && p0 + r < N; ++r)
            if (tx < nc) G[(size_t)(p0 + r) * N + c0 + tx] = tile[r][tx];
        __syncthreads();
    }
    if (p < N) {
        R[p] = run;
        bad |= !(run <= 4294967296.0);                // 2^32 children per event: the slot sums stay far inside int64
    }
    if (bad) atomicOr(&sc->bad, 1);
}

template <typename S>
struct sim_pinned {
    S *h = nullptr;
    ~sim_pinned() { if (h) (void)hipHostFree(h); }
};

template <typename S>
static nhp_status sim_read(nhp_ctx *ctx, S *h, const S *d)
{
    NHP_HIP(ctx, hipMemcpyAsync(h, d, sizeof(S), hipMemcpyDeviceToHost, ctx->main()));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    return NHP_OK;
}

static nhp_status sim_exploded(nhp_ctx *ctx)
{
    nhp_set_error(ctx, "branching process exploded (unstable weights?)");
    return NHP_ENOMEM;
}
