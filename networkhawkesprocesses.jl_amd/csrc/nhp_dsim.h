// The pieces of the discrete branching sampler shared by disc_simulate.hip (rand from bin 1) and disc_forecast.hip
// (continuations of an observed count matrix): the run scalars, the lag CDF, the link masses and their row prefixes with the
// parameter checks, the block-partial sums of the run scalars, the arena stores and the child draw.  A generator gives the
// three Philox keys of its draws (seed ^ family) in dsim_args.  Kernels are static: one copy per translation unit.
#pragma once
#include "nhp_sim.h"

#define DSIM_CELL_MAX 1048576.0                       // 2^20 expected events per cell at most

struct dsim_scal {
    long long fill;                  // arena entries so far (may pass max_events: nothing at or past it is written)
    unsigned long long next;         // child slots of the generation being stored
    unsigned long long events;       // events so far: Σ multiplicities, the entries that found no room included
    int bad;                         // 1: weights / basis parameters, 2: cell means, 4: history counts
    int pad;
};

struct dsim_args {
    const double *G, *R;             // row-major inclusive prefix of G [N*N], row totals R_p [N]
    const double *theta, *mb, *cdf;  // θ [N*N*B] column-major; m_b [B]; inclusive prefix of φ[·,b] over the lags [L*B], lag fastest
    int64_t T;                       // bins in all; a forecast: the horizon H, bins k + H·r belong to replica r
    int32_t N, B, L;
    uint64_t key_count, key_child;   // seed ^ family: child count of an arena entry; node, basis, lag of a child slot
};

// the lag CDF: one lane per basis b, a sequential running sum over the lags; m_b = dt·Σ_l φ[l,b]
static __global__ void k_dsim_lags(const double *__restrict__ phi, int32_t L, int32_t B, double dt, double *__restrict__ cdf,
                                   double *__restrict__ mb, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int32_t b = blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (b >= B) return;
    double run = 0.0;
    int bad = 0;
    for (int32_t l = 0; l < L; ++l) {
        const double v = phi[(size_t)b * L + l];
        bad |= !(v >= 0.0 && v < INFINITY);
        run = run + v;
        cdf[(size_t)b * L + l] = run;
    }
    mb[b] = run * dt;
    bad |= !(run < INFINITY);
    if (bad) atomicOr(&sc->bad, 1);
}

// the link masses V[p,c] = (W[p,c]·A[p,c])·Σ_b θ[p,c,b]·m_b (column-major, as W), one lane per link, with the parameter checks
static __global__ void __launch_bounds__(SIM_BLOCK) k_dsim_mass(const double *__restrict__ W, const double *__restrict__ A,
                                                                const double *__restrict__ theta, const double *__restrict__ mb,
                                                                int64_t NN, int32_t B, double *__restrict__ V,
                                                                dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (q >= NN) return;
    const double w = A ? W[q] * A[q] : W[q];
    double s = 0.0;
    int bad = 0;
    for (int32_t b = 0; b < B; ++b) {
        const double th = theta[q + NN * b];
        bad |= !(th >= 0.0 && th < INFINITY);
        s = s + th * mb[b];
    }
    const double v = w * s;
    bad |= !(W[q] >= 0.0 && w >= 0.0 && v >= 0.0 && v < INFINITY);
    V[q] = v;
    if (bad) atomicOr(&sc->bad, 1);
}

// k_sim_rows of nhp_sim.h over the link masses: one lane per row p, a sequential running sum over c (so the table is
// monotone and a zero-mass entry equals the one before it exactly: it can never be chosen); column c of 64 rows is one
// coalesced read, the running sums leave row by row through an LDS tile
static __global__ void __launch_bounds__(SIM_ROWS) k_dsim_rows(const double *__restrict__ V, int32_t N, double *__restrict__ G,
                                                               double *__restrict__ R, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    __shared__ double tile[SIM_ROWS][SIM_ROWS + 1];
    const int32_t p0 = blockIdx.x * SIM_ROWS, tx = threadIdx.x, p = p0 + tx;
    double run = 0.0;
    for (int32_t c0 = 0; c0 < N; c0 += SIM_ROWS) {
        const int32_t nc = min(SIM_ROWS, N - c0);
        if (p < N) {
#pragma unroll 16
            for (int32_t k = 0; k < SIM_ROWS; ++k) {
                if (k < nc) {
                    run = run + V[(size_t)p + (size_t)(c0 + k) * N];
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
        if (!(run <= 4294967296.0)) atomicOr(&sc->bad, 1);      // 2^32 children per event: the slot sums stay far inside int64
    }
}

// The run scalars are summed without atomics: a block leaves the sums of its lanes' a and b in pa[block], pb[block], and the
// one-block advance kernel behind it adds them up -- with an atomic per wave, the 16384 waves of a chunk queued on the two
// counters for 0.3 ms.  Block sums of a and b, valid in thread 0 (every thread of the block calls it):
static __device__ __forceinline__ void dsim_block_sums(unsigned long long &a, unsigned long long &b)
{
    __shared__ unsigned long long red[2][SIM_BLOCK / 64];
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < SIM_BLOCK / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    }
}

// one block: fill += kept entries, next += Σ pa (child slots), events += Σ pb (cells: the multiplicities; children: one each)
static __global__ void __launch_bounds__(SIM_BLOCK) k_dsim_advance(dsim_scal *__restrict__ sc, const uint32_t *__restrict__ kept,
                                                                   const unsigned long long *__restrict__ pa,
                                                                   const unsigned long long *__restrict__ pb, uint32_t nb,
                                                                   int children)
{
    unsigned long long a = 0, b = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += SIM_BLOCK) { a += pa[i]; b += pb[i]; }
    dsim_block_sums(a, b);
    if (threadIdx.x == 0) {
        sc->fill += *kept;
        sc->next += a;
        sc->events += children ? (unsigned long long)*kept : b;
    }
}

// the occupied cells of a chunk behind the fill counter (never at or past cap), with their child counts; background
static __global__ void __launch_bounds__(SIM_BLOCK) k_dsim_store_cells(dsim_args a, int64_t e0, int64_t m, const int32_t *__restrict__ kbuf,
                                                                       const uint32_t *__restrict__ flag,
                                                                       const uint32_t *__restrict__ pos, dsim_scal *__restrict__ sc,
                                                                       int64_t cap, int32_t *__restrict__ anode,
                                                                       int32_t *__restrict__ abin, int32_t *__restrict__ ak,
                                                                       int64_t *__restrict__ cnt, int64_t *__restrict__ background,
                                                                       unsigned long long *__restrict__ pa,
                                                                       unsigned long long *__restrict__ pb)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0, evs = 0;
    if (j < m) {
        const int64_t e = e0 + j;
        const int32_t k = kbuf[j];
        if (background) background[e] = k;
        if (flag[j]) {
            evs = (unsigned long long)k;
            const int64_t dst = (int64_t)sc->fill + pos[j];
            if (dst < cap) {
                const int64_t t = e / a.N;
                const int32_t c = (int32_t)(e - t * a.N);
                anode[dst] = c; abin[dst] = (int32_t)t; ak[dst] = k;
                const double n = sim_poisson((double)k * a.R[c], a.key_count, 0, (uint64_t)dst);
                cnt[dst] = (int64_t)n;
                kids = (unsigned long long)n;
            }
        }
    }
    dsim_block_sums(kids, evs);
    if (threadIdx.x == 0) { pa[blockIdx.x] = kids; pb[blockIdx.x] = evs; }
}

// child slot s = s0 + j of the current generation: parent, node, basis, lag, bin, keep flag.  REPLICAS: the T bins repeat,
// replica after replica, and a child stays only inside its parent's T bins; otherwise one run of T bins
template <bool REPLICAS>
static __global__ void __launch_bounds__(SIM_BLOCK) k_dsim_children(dsim_args a, uint64_t gen, int64_t s0, int64_t m,
                                                                    const int64_t *__restrict__ off, int64_t n_par, int64_t g0,
                                                                    const int32_t *__restrict__ anode, const int32_t *__restrict__ abin,
                                                                    int32_t *__restrict__ cn, int32_t *__restrict__ cb,
                                                                    uint32_t *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t s = s0 + j;
    int64_t lo = 0, hi = n_par;                       // last parent i with off[i] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= s) lo = mid; else hi = mid; }
    const int64_t par = g0 + lo;
    const int32_t p = anode[par], N = a.N, B = a.B, L = a.L;
    const uint64_t key = a.key_child;
    double ua, ub, uc, unused;
    philox_2u(key, gen, (uint64_t)s, 0, &ua, &ub);
    philox_2u(key, gen, (uint64_t)s, 1, &uc, &unused);
    const double *row = a.G + (size_t)p * N;
    double x = sim_u01(ua) * a.R[p];
    int32_t l = 0, h = N;                             // node: first c with row[c] > x
    while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] > x) h = mid; else l = mid + 1; }
    if (l == N) {                                     // x rounded up to R_p: the first entry reaching it (a positive mass)
        l = 0; h = N - 1;
        while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] >= x) h = mid; else l = mid + 1; }
    }
    const int32_t c = l;
    const double *th = a.theta + (size_t)p + (size_t)c * N;
    const size_t NN = (size_t)N * N;
    double tot = 0.0;
    for (int32_t b = 0; b < B; ++b) tot = tot + th[NN * b] * a.mb[b];
    x = sim_u01(ub) * tot;
    int32_t bs = -1, bg = -1;                         // basis: first b with prefix[b] > x (if none, the first prefix[b] >= x)
    double run = 0.0;
    for (int32_t b = 0; b < B; ++b) {
        run = run + th[NN * b] * a.mb[b];
        if (bs < 0 && run > x) bs = b;
        if (bg < 0 && run >= x) bg = b;
    }
    if (bs < 0) bs = bg < 0 ? B - 1 : bg;
    const double *col = a.cdf + (size_t)bs * L;
    x = sim_u01(uc) * col[L - 1];
    l = 0; h = L;                                     // lag: first l with col[l] > x
    while (l < h) { const int32_t mid = (l + h) >> 1; if (col[mid] > x) h = mid; else l = mid + 1; }
    if (l == L) {
        l = 0; h = L - 1;
        while (l < h) { const int32_t mid = (l + h) >> 1; if (col[mid] >= x) h = mid; else l = mid + 1; }
    }
    cn[j] = c;
    if (REPLICAS) {
        const int64_t tp = abin[par], k = tp % a.T + l + 1;        // lags are 1..L; k: the child's bin inside its replica
        cb[j] = (int32_t)(tp + (k < a.T ? l + 1 : 0));
        keep[j] = k < a.T;
    } else {
        const int64_t bin = (int64_t)abin[par] + l + 1;
        cb[j] = (int32_t)min(bin, a.T);
        keep[j] = bin < a.T;
    }
}

// survivors of a chunk behind the fill counter (never at or past cap), with their own child counts
static __global__ void __launch_bounds__(SIM_BLOCK) k_dsim_keep(dsim_args a, uint64_t gen_next, int64_t m, const uint32_t *__restrict__ keep,
                                                                const uint32_t *__restrict__ pos, const int32_t *__restrict__ cn,
                                                                const int32_t *__restrict__ cb, dsim_scal *__restrict__ sc, int64_t g1,
                                                                int64_t cap, int32_t *__restrict__ anode, int32_t *__restrict__ abin,
                                                                int32_t *__restrict__ ak, int64_t *__restrict__ cnt,
                                                                unsigned long long *__restrict__ pa, unsigned long long *__restrict__ pb)
{
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (j < m && keep[j]) {
        const int64_t dst = (int64_t)sc->fill + pos[j];
        if (dst < cap) {
            const int32_t c = cn[j];
            anode[dst] = c; abin[dst] = cb[j]; ak[dst] = 1;
            const double n = sim_poisson(a.R[c], a.key_count, gen_next, (uint64_t)dst);
            cnt[dst - g1] = (int64_t)n;
            kids = (unsigned long long)n;
        }
    }
    unsigned long long none = 0;
    dsim_block_sums(kids, none);
    if (threadIdx.x == 0) { pa[blockIdx.x] = kids; pb[blockIdx.x] = 0; }
}

static __global__ void k_dsim_clear_next(dsim_scal *__restrict__ sc) { sc->next = 0; }
