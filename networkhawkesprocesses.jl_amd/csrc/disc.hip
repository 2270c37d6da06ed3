// Discrete-time path: basis convolution, intensity / Poisson log-likelihood and the
// mean-field VB step (reference: convolve src/discrete.jl:146-151; basis
// src/impulses.jl:321-335; intensity src/discrete.jl:115-129 with bump :381-385,:511-516;
// loglikelihood :91-102; update! :369-375 = update_parents src/parents.jl:136-177 + the three
// component updates src/baselines.jl:444-456, src/weights.jl:70-97, src/impulses.jl:355-375).
//
// The reference's 4-deep scalar loop for λ and its T x N x (1+NB) responsibility array are one
// dense contraction:  with k = (p,b),  G = Ŝ viewed as T x (N·B)  and  E[k,c] the per-link
// factor,   Z = base ⊕ G·E   (GEMM-1, T x NB x N).  VB needs a second one,
// Γ = E ⊙ (Gᵀ·R) with R = data/Z (GEMM-2, NB x T x N); `u` (1.68 TB at N=512, B=8, T=1e5) is
// never formed.  This IS a dense GEMM, so it runs on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64): 128x128 block tile, 4 waves as 2x2, 64x64 per wave = 4x4 MFMA tiles
// (64 fp64 accumulators per lane), BK = 16 staged through padded LDS images that make every
// fragment read conflict-free, next tile prefetched into registers during the MFMAs.
#include <math.h>

#include <algorithm>

#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_netvb.h"           // DISC_CONV_CB
#include "nhp_disc_gemm.h"       // the GEMM of both contractions; the variational fits that share it: disc_vb.hip

// ---- small kernels ----------------------------------------------------------------------------

// data (N x T, node fastest, Int64) -> dataT (T x N, t fastest, f64) + per-node event totals
__global__ __launch_bounds__(256) void k_disc_transpose(const int64_t *__restrict__ data, int N, int64_t T,
                                                        double *__restrict__ dataT, uint8_t *__restrict__ data8)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    const int n0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + tx;
        const int64_t t = t0 + r;
        if (n < N && t < T) tile[r][tx] = (double)data[(size_t)n + (size_t)t * N];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r;
        const int64_t t = t0 + tx;
        if (n < N && t < T) {
            dataT[(size_t)t + (size_t)n * T] = tile[tx][r];
            if (data8) data8[(size_t)t + (size_t)n * T] = (uint8_t)tile[tx][r];
        }
    }
}

// per-node Σ_t data[n,t]  and  Σ_t loggamma(data[n,t] + 1)  -> out[n], out[N + n]
__global__ __launch_bounds__(256) void k_disc_colstats(const double *__restrict__ dataT, int N, int64_t T,
                                                       double *__restrict__ out)
{
    __shared__ double red[NHP_WAVES];
    const int n = blockIdx.x;
    double s = 0.0, lg = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) {
        const double v = dataT[(size_t)t + (size_t)n * T];
        s += v;
        if (v > 1.0) lg += lgamma(v + 1.0);
    }
    s = nhp_block_sum(s, red);
    lg = nhp_block_sum(lg, red);
    if (threadIdx.x == 0) { out[n] = s; out[N + n] = lg; }
}

// Ŝ[t,n,b] = max(0, Σ_{l=1..min(L,t)} data[n,t-l]·ϕ_b[l])   (0-based t; lag 0 excluded by the
// prepended 0.0 of the reference's conv kernel; direct form = the exact value its FFT approximates).
// A workgroup owns CONV_TB = 512 consecutive bins of one node, two per thread: the 512+L counts it needs sit in LDS (zeros
// before t = 0, which add exactly nothing) next to a bitmap of the NONZERO counts (one wave ballot per 64 bins), and the basis
// is transposed to ϕT[l][b] so one lag is a broadcast read.  A thread walks only the nonzero counts of its L-lag window
// (count data are sparse: BASELINE config 4 has 5 % occupied bins, 1.6 of 32 lags on average), most recent first, carrying
// CB basis sums at once.  Per basis the sum still runs l = 1..L in increasing order with separate multiply and add, and a
// skipped term is +0.0·ϕ -- which changes no bit of the running sum -- so the result is bit for bit the oracle's value.
// The two bins of a thread leave as ONE 16-byte non-temporal store per basis (8-byte stores ran at 1.8 TB/s; the 3.3 GB of
// Ŝ are re-read from HBM by the GEMMs whatever the cache policy).
#define CONV_CB DISC_CONV_CB         // nhp_netvb.h: k_disc_convolve_window (disc_vb.hip) and its LDS sizing use the same
#ifndef CONV_PP
#define CONV_PP 4                    // pairs of bins per thread: a workgroup's prologue (tile, bitmap, basis) serves 2048 bins
#endif
#define CONV_TB (512 * CONV_PP)
typedef double nhp_d2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_disc_convolve(const double *__restrict__ dataT, const uint8_t *__restrict__ data8, int N, int64_t T,
                                                       const double *__restrict__ phi, int L, int B,
                                                       double *__restrict__ conv, double *__restrict__ colpart)
{
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    double *tile = csm;                                  // [CONV_TB + L]: data[n, t0-L .. t0+CONV_TB-1]
    const int Bp = (B + CONV_CB - 1) / CONV_CB * CONV_CB;
    double *phiT = csm + CONV_TB + L;                    // [L][Bp], Bp = B rounded up to CONV_CB
    double *red = phiT + (size_t)L * Bp;                 // [4 waves][CONV_CB] column-sum staging
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(red + 4 * CONV_CB);   // [(CONV_TB + L) / 64 + 2]
    const int n = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * CONV_TB;
    const double *d = dataT + (size_t)n * T;
    const uint8_t *d8 = data8 ? data8 + (size_t)n * T : nullptr;    // the counts in bytes (exact: they are integers <= 255)
    const int span = CONV_TB + L, nwords = (span + 63) / 64 + 1;
    for (int i = tid; i < nwords * 64; i += 256) {       // whole 64-bin words, so every ballot is a full word
        const int64_t tt = t0 - L + i;
#if defined(CONV_FILL) && CONV_FILL >= 2                 // timing experiment: no count reads either
        const double x = 0.0; (void)tt; (void)d;
#else
        const double x = (i < span && tt >= 0 && tt < T) ? (d8 ? (double)d8[tt] : d[tt]) : 0.0;
#endif
        if (i < span) tile[i] = x;
        const unsigned long long bal = __ballot(x != 0.0);
        if ((tid & 63) == 0) bits[i >> 6] = bal;
    }
    for (int i = tid; i < L * Bp; i += 256) {
        const int l = i / Bp, b = i % Bp;
        phiT[i] = b < B ? phi[l + (size_t)b * L] : 0.0;
    }
    __syncthreads();
    const unsigned long long lmask = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    const bool pair = (T & 1) == 0;                      // every (t, t+1) store then is 16-byte aligned
    for (int b0 = 0; b0 < B; b0 += CONV_CB) {
        double cs[CONV_CB];                              // this thread's share of Σ_t Ŝ[t, n, b] (the column sums the
#pragma unroll                                           // discrete adjacency sweep needs: no second pass over 3.3 GB)
        for (int q = 0; q < CONV_CB; ++q) cs[q] = 0.0;
        for (int pp = 0; pp < CONV_PP; ++pp) {
            const int o = 2 * (tid + 256 * pp);          // local bin of this pair's first output (a wave stores 1 KB runs)
            const int64_t t = t0 + o;
            if (t >= T) break;
            double s[2][CONV_CB];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // bit k of m <-> tile[o + j + k] = data[n, t + j - (L - k)]: the lags l = L - k of output j
                const int pos = o + j, sh = pos & 63;
                const unsigned long long lo = bits[pos >> 6], hi = bits[(pos >> 6) + 1];
                unsigned long long m = ((lo >> sh) | (sh ? hi << (64 - sh) : 0ull)) & lmask;
#pragma unroll
                for (int q = 0; q < CONV_CB; ++q) s[j][q] = 0.0;
#ifdef CONV_FILL                                         // timing experiment (tools/): the stores alone
                m = 0;
#endif
                while (m) {                              // increasing lag = decreasing bit: highest set bit first
                    const int k = 63 - __builtin_clzll(m);
                    m &= ~(1ull << k);
                    const double x = tile[o + j + k];
                    const double *ph = phiT + (size_t)(L - k - 1) * Bp + b0;
#pragma unroll
                    for (int q = 0; q < CONV_CB; ++q) s[j][q] = s[j][q] + x * ph[q];
                }
            }
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q)
                if (b0 + q < B) {
                    double *dst = conv + (size_t)t + (size_t)n * T + (size_t)(b0 + q) * T * N;
                    const double v0 = s[0][q] > 0.0 ? s[0][q] : 0.0, v1 = (t + 1 < T && s[1][q] > 0.0) ? s[1][q] : 0.0;
                    cs[q] += v0 + v1;
                    if (pair) {
                        nhp_d2 v = {v0, v1};
#ifdef CONV_PLAIN
                        *reinterpret_cast<nhp_d2 *>(dst) = v;
#else
                        __builtin_nontemporal_store(v, reinterpret_cast<nhp_d2 *>(dst));
#endif
                    } else {
                        __builtin_nontemporal_store(v0, dst);
                        if (t + 1 < T) __builtin_nontemporal_store(v1, dst + 1);
                    }
                }
        }
        // per-workgroup column sums, waves in a fixed order (deterministic); k_disc_convsum_blocks adds the workgroups
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CONV_CB; ++q) {
            const double v = nhp_wave_sum(cs[q]);
            if ((tid & 63) == 0) red[(tid >> 6) * CONV_CB + q] = v;
        }
        __syncthreads();
        if (tid < CONV_CB && b0 + tid < B)
            colpart[((size_t)blockIdx.x * N + n) * B + b0 + tid] = (red[tid] + red[CONV_CB + tid]) + (red[2 * CONV_CB + tid] + red[3 * CONV_CB + tid]);
    }
}

// convsum[n + b·N] = Σ over the time blocks of colpart[blk][n][b], in block order
__global__ __launch_bounds__(256) void k_disc_convsum_blocks(const double *__restrict__ colpart, int nblk, int N, int B, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * B) return;
    const int n = i % N, b = i / N;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += colpart[((size_t)k * N + n) * B + b];
    out[i] = s;
}

// Dense form (every lag of every bin, 256 bins per workgroup, 8-byte stores): windows longer than the 64-lag bitmap.
__global__ __launch_bounds__(256) void k_disc_convolve_dense(const double *__restrict__ dataT, int N, int64_t T,
                                                       const double *__restrict__ phi, int L, int B,
                                                       double *__restrict__ conv)
{
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    double *tile = csm;                                  // [256 + L]: data[n, t0-L .. t0+255]
    double *phiT = csm + 256 + L;                        // [L][Bp], Bp = B rounded up to CONV_CB
    const int n = blockIdx.y, tid = threadIdx.x;
    const int Bp = (B + CONV_CB - 1) / CONV_CB * CONV_CB;
    const int64_t t0 = (int64_t)blockIdx.x * 256;
    const double *d = dataT + (size_t)n * T;
    for (int i = tid; i < 256 + L; i += 256) {
        const int64_t tt = t0 - L + i;
        tile[i] = (tt >= 0 && tt < T) ? d[tt] : 0.0;
    }
    for (int i = tid; i < L * Bp; i += 256) {
        const int l = i / Bp, b = i % Bp;
        phiT[i] = b < B ? phi[l + (size_t)b * L] : 0.0;
    }
    __syncthreads();
    const int64_t t = t0 + tid;
    for (int b0 = 0; b0 < B; b0 += CONV_CB) {
        double s[CONV_CB];
#pragma unroll
        for (int q = 0; q < CONV_CB; ++q) s[q] = 0.0;
        for (int l = 1; l <= L; ++l) {
            const double x = tile[tid + L - l];          // data[n, t - l]
            const double *ph = phiT + (size_t)(l - 1) * Bp + b0;
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q) s[q] = s[q] + x * ph[q];
        }
        if (t < T) {
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q)
                if (b0 + q < B) conv[(size_t)t + (size_t)n * T + (size_t)(b0 + q) * T * N] = s[q] > 0.0 ? s[q] : 0.0;
        }
    }
}

// ---- trials: independent recordings stacked along time (nhp_disc_dataset_set_trials) ----------------------------------
// Ŝ[t,n,b] = max(0, Σ_{l=1..min(L, t-o_r)} data[n,t-l]·ϕ_b[l]) for a bin t of the trial that starts at o_r: the lags stop
// at the trial's first bin.  `start` [T] is 1 at the first bin of every trial but the first.  k_disc_convolve with one
// more bitmap: the ballot loop that marks the nonzero counts also marks the trial starts, and an output bin clears from
// its count mask every lag that lies before the latest start inside its window -- one clz and one AND per output, one byte
// read per bin next to the 64·B stored.  The terms that remain are added as k_disc_convolve adds them, so a trial's rows
// are bit for bit the rows that kernel writes for the trial alone.  A boundary may fall anywhere in the tile and a stored
// pair (t, t+1) may straddle one: each output of the pair has its own mask.
__global__ __launch_bounds__(256) void k_disc_convolve_trials(const double *__restrict__ dataT, const uint8_t *__restrict__ data8,
                                                              const uint8_t *__restrict__ start, int N, int64_t T,
                                                              const double *__restrict__ phi, int L, int B,
                                                              double *__restrict__ conv, double *__restrict__ colpart)
{
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    double *tile = csm;                                  // [CONV_TB + L]: data[n, t0-L .. t0+CONV_TB-1]
    const int Bp = (B + CONV_CB - 1) / CONV_CB * CONV_CB;
    double *phiT = csm + CONV_TB + L;                    // [L][Bp]
    double *red = phiT + (size_t)L * Bp;                 // [4 waves][CONV_CB]
    const int span = CONV_TB + L, nwords = (span + 63) / 64 + 1;
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(red + 4 * CONV_CB);   // [nwords] nonzero counts
    unsigned long long *sbits = bits + nwords;                                              // [nwords] trial starts
    const int n = blockIdx.y, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * CONV_TB;
    const double *d = dataT + (size_t)n * T;
    const uint8_t *d8 = data8 ? data8 + (size_t)n * T : nullptr;
    for (int i = tid; i < nwords * 64; i += 256) {
        const int64_t tt = t0 - L + i;
        const bool in = i < span && tt >= 0 && tt < T;
        const double x = in ? (d8 ? (double)d8[tt] : d[tt]) : 0.0;
        const bool s = in && start[tt] != 0;
        if (i < span) tile[i] = x;
        const unsigned long long bal = __ballot(x != 0.0), sbal = __ballot(s);
        if ((tid & 63) == 0) { bits[i >> 6] = bal; sbits[i >> 6] = sbal; }
    }
    for (int i = tid; i < L * Bp; i += 256) {
        const int l = i / Bp, b = i % Bp;
        phiT[i] = b < B ? phi[l + (size_t)b * L] : 0.0;
    }
    __syncthreads();
    const unsigned long long lmask = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    const bool pair = (T & 1) == 0;
    for (int b0 = 0; b0 < B; b0 += CONV_CB) {
        double cs[CONV_CB];
#pragma unroll
        for (int q = 0; q < CONV_CB; ++q) cs[q] = 0.0;
        for (int pp = 0; pp < CONV_PP; ++pp) {
            const int o = 2 * (tid + 256 * pp);
            const int64_t t = t0 + o;
            if (t >= T) break;
            double s[2][CONV_CB];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // bit k of m <-> tile[o + j + k] = data[n, t + j - (L - k)]; bit k of sm <-> bin t + j - (L - 1 - k), the
                // window one bin later: it ends at the output bin itself, which as a trial's first bin has no lag at all
                const int pos = o + j, sh = pos & 63, spos = pos + 1, ssh = spos & 63;
                const unsigned long long lo = bits[pos >> 6], hi = bits[(pos >> 6) + 1];
                const unsigned long long slo = sbits[spos >> 6], shi = sbits[(spos >> 6) + 1];
                unsigned long long m = ((lo >> sh) | (sh ? hi << (64 - sh) : 0ull)) & lmask;
                const unsigned long long sm = ((slo >> ssh) | (ssh ? shi << (64 - ssh) : 0ull)) & lmask;
                if (sm) {                                // latest start at bit ks: the counts at bits 0..ks lie before it
                    const int ks = 63 - __builtin_clzll(sm);
                    m &= ~((2ull << ks) - 1ull);         // (ks = 63: 2 << 63 = 0, the mask is all ones)
                }
#pragma unroll
                for (int q = 0; q < CONV_CB; ++q) s[j][q] = 0.0;
                while (m) {
                    const int k = 63 - __builtin_clzll(m);
                    m &= ~(1ull << k);
                    const double x = tile[o + j + k];
                    const double *ph = phiT + (size_t)(L - k - 1) * Bp + b0;
#pragma unroll
                    for (int q = 0; q < CONV_CB; ++q) s[j][q] = s[j][q] + x * ph[q];
                }
            }
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q)
                if (b0 + q < B) {
                    double *dst = conv + (size_t)t + (size_t)n * T + (size_t)(b0 + q) * T * N;
                    const double v0 = s[0][q] > 0.0 ? s[0][q] : 0.0, v1 = (t + 1 < T && s[1][q] > 0.0) ? s[1][q] : 0.0;
                    cs[q] += v0 + v1;
                    if (pair) {
                        nhp_d2 v = {v0, v1};
                        __builtin_nontemporal_store(v, reinterpret_cast<nhp_d2 *>(dst));
                    } else {
                        __builtin_nontemporal_store(v0, dst);
                        if (t + 1 < T) __builtin_nontemporal_store(v1, dst + 1);
                    }
                }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < CONV_CB; ++q) {
            const double v = nhp_wave_sum(cs[q]);
            if ((tid & 63) == 0) red[(tid >> 6) * CONV_CB + q] = v;
        }
        __syncthreads();
        if (tid < CONV_CB && b0 + tid < B)
            colpart[((size_t)blockIdx.x * N + n) * B + b0 + tid] = (red[tid] + red[CONV_CB + tid]) + (red[2 * CONV_CB + tid] + red[3 * CONV_CB + tid]);
    }
}

// k_disc_convolve_dense for trials: the lag loop of bin t ends at min(L, t - o_r), found by walking the start flags of the
// bins t, t-1, ... in LDS (at most L of them, beside the L·B multiply-adds of the loop itself).
__global__ __launch_bounds__(256) void k_disc_convolve_dense_trials(const double *__restrict__ dataT, const uint8_t *__restrict__ start,
                                                                    int N, int64_t T, const double *__restrict__ phi, int L, int B,
                                                                    double *__restrict__ conv)
{
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    double *tile = csm;                                  // [256 + L]: data[n, t0-L .. t0+255]
    double *phiT = csm + 256 + L;                        // [L][Bp]
    const int n = blockIdx.y, tid = threadIdx.x;
    const int Bp = (B + CONV_CB - 1) / CONV_CB * CONV_CB;
    uint8_t *flag = reinterpret_cast<uint8_t *>(phiT + (size_t)L * Bp);     // [256 + L]: start[t0-L .. t0+255]
    const int64_t t0 = (int64_t)blockIdx.x * 256;
    const double *d = dataT + (size_t)n * T;
    for (int i = tid; i < 256 + L; i += 256) {
        const int64_t tt = t0 - L + i;
        const bool in = tt >= 0 && tt < T;
        tile[i] = in ? d[tt] : 0.0;
        flag[i] = in ? start[tt] : (uint8_t)0;
    }
    for (int i = tid; i < L * Bp; i += 256) {
        const int l = i / Bp, b = i % Bp;
        phiT[i] = b < B ? phi[l + (size_t)b * L] : 0.0;
    }
    __syncthreads();
    const int64_t t = t0 + tid;
    int lim = L;                                         // min(L, t - o_r): bin t - l is index tid + L - l
    for (int l = 0; l < L; ++l)
        if (flag[tid + L - l]) { lim = l; break; }
    for (int b0 = 0; b0 < B; b0 += CONV_CB) {
        double s[CONV_CB];
#pragma unroll
        for (int q = 0; q < CONV_CB; ++q) s[q] = 0.0;
        for (int l = 1; l <= lim; ++l) {
            const double x = tile[tid + L - l];          // data[n, t - l]
            const double *ph = phiT + (size_t)(l - 1) * Bp + b0;
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q) s[q] = s[q] + x * ph[q];
        }
        if (t < T) {
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q)
                if (b0 + q < B) conv[(size_t)t + (size_t)n * T + (size_t)(b0 + q) * T * N] = s[q] > 0.0 ? s[q] : 0.0;
        }
    }
}

// E[k + c·K], k = p + b·N:  bump = ((a·)w·θ)·dt   (src/discrete.jl:381-385,511-516);  base[c] = λ0[c]·dt
__global__ __launch_bounds__(256) void k_disc_bump(int N, int B, double dt, const double *__restrict__ lambda0,
                                                   const double *__restrict__ W, const double *__restrict__ theta,
                                                   const double *__restrict__ A, double *__restrict__ E,
                                                   double *__restrict__ base, int cat_order)
{
#pragma clang fp contract(off)
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NN * B) {
        const size_t b = i / NN, pc = i % NN, p = pc % N, c = pc / N;
        const double w = A ? A[pc] * W[pc] : W[pc];
        // cat_order: row q = p·B + b, the reference's parent-category order (src/parents.jl:108-112)
        E[(cat_order ? p * B + b : p + b * N) + c * K] = (w * theta[i]) * dt;
    }
    if (i < (size_t)N) base[i] = lambda0[i] * dt;
}

__global__ __launch_bounds__(256) void k_sum_pairs(const double *__restrict__ partials, int n, double lg_const,
                                                   double *__restrict__ out)
{
    __shared__ double red[NHP_WAVES];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
    a = nhp_block_sum(a, red);
    b = nhp_block_sum(b, red);
    if (threadIdx.x == 0) *out = a - b - lg_const;
}

// ---- host side -----------------------------------------------------------------------------------

extern "C" nhp_status nhp_disc_basis(int32_t L, int32_t B, double dt, double *phi)
{
    // basis(impulse): src/impulses.jl:321-335 (the exponent parses as -d²/(4σ))
    if (L < 1 || B < 1 || !phi) return NHP_EINVAL;
    const double sigma = (double)L / (double)(B - 1);
    const double coef = ((-1.0 / 2.0) * (1.0 / sigma)) / 2.0;
    for (int b = 0; b < B; ++b) {
        const int len = (B < L) ? B + 2 : B, i = (B < L) ? b + 1 : b;
        const double tt = (double)i / (double)(len > 1 ? len - 1 : 1);
        const double mu = (1.0 - tt) * 1.0 + tt * (double)L;
        double s = 0.0;
        for (int l = 0; l < L; ++l) {
            const double d = (double)(l + 1) - mu;
            phi[l + (size_t)b * L] = exp(coef * (d * d));
            s += phi[l + (size_t)b * L];
        }
        for (int l = 0; l < L; ++l) phi[l + (size_t)b * L] /= (s * dt);
    }
    return NHP_OK;
}

// convsum[k] = Σ_t Ŝ[t, k]  (one workgroup per (p, b) column, fixed-order block reduction)
__global__ __launch_bounds__(256) void k_disc_convsum(const double *__restrict__ conv, int64_t T, double *__restrict__ out)
{
    __shared__ double red[NHP_WAVES];
    const double *col = conv + (size_t)blockIdx.x * (size_t)T;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) s += col[t];
    s = nhp_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

extern "C" nhp_status nhp_disc_dataset_create(nhp_ctx *ctx, const int64_t *data, int32_t N, int64_t T,
                                              nhp_disc_dataset **out)
{
    if (!ctx || !out || !data || N < 1 || T < 1) return NHP_EINVAL;
    *out = nullptr;
    if (T >= ((int64_t)1 << 31) - BM) { nhp_set_error(ctx, "n_bins must be < 2^31"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_disc_dataset *ds = new nhp_disc_dataset();
    ds->ctx = ctx; ds->N = N; ds->T = T;
    const size_t NT = (size_t)N * (size_t)T;
    int64_t *d_raw = nullptr;
    hipStream_t st = ctx->main();
    hipError_t e;
    if ((e = hipMalloc(&d_raw, 8 * NT)) != hipSuccess || (e = hipMalloc(&ds->d_dataT, 8 * NT)) != hipSuccess ||
        (e = hipMalloc(&ds->d_colsum, 8 * 2 * (size_t)N)) != hipSuccess) {
        nhp_set_error(ctx, "hipMalloc failed: %s", hipGetErrorString(e));
        if (d_raw) (void)hipFree(d_raw);
        nhp_disc_dataset_destroy(ds);
        return NHP_ENOMEM;
    }
    NHP_HIP(ctx, hipMemcpyAsync(d_raw, data, 8 * NT, hipMemcpyHostToDevice, st));
    int64_t vmax = 0, vmin = 0;
    {   // occupied bins by span of the time axis, within a span by (node, bin); data is N x T column-major
        const int64_t want = 2 * (int64_t)ctx->cu_count, least = (T + NHP_DA_SPAN - 1) / NHP_DA_SPAN;
        int64_t nsp = std::max<int64_t>(std::min<int64_t>(want, T), least);
        if (const char *es = getenv("NHP_DADJ_SPANS")) { const int64_t v = atoll(es); if (v >= least && v <= T) nsp = v; }
        std::vector<int32_t> ot, oc, off((size_t)nsp + 1, 0), spt((size_t)nsp + 1, 0);
        std::vector<double> os;
        std::vector<int32_t> st_, sc_, cnt((size_t)N + 1);
        std::vector<double> ss_;
        int64_t nocc = 0;
        for (int64_t k = 0; k < nsp; ++k) {
            const int64_t ta = k * T / nsp, tb = (k + 1) * T / nsp;              // (tb - ta <= ceil(T / nsp) <= NHP_DA_SPAN)
            spt[(size_t)k] = (int32_t)ta;
            off[(size_t)k] = (int32_t)ot.size();
            st_.clear(); sc_.clear(); ss_.clear();
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t t = ta; t < tb; ++t)
                for (int32_t n = 0; n < N; ++n) {
                    const int64_t v = data[(size_t)n + (size_t)t * N];
                    if (v > 0) { st_.push_back((int32_t)t); sc_.push_back(n); ss_.push_back((double)v); ++cnt[(size_t)n + 1]; }
                    if (v > vmax) vmax = v;
                    if (v < vmin) vmin = v;
                }
            for (int32_t n = 0; n < N; ++n) cnt[(size_t)n + 1] += cnt[(size_t)n];
            const size_t base = ot.size(), m = st_.size(), mp = (m + 3) / 4 * 4;
            ot.resize(base + mp, (int32_t)ta); oc.resize(base + mp, 0); os.resize(base + mp, 0.0);      // (padding: bin ta, node 0, count 0)
            for (size_t i = 0; i < m; ++i) {                                       // stable by node: bins stay ascending
                const size_t d = base + (size_t)cnt[(size_t)sc_[i]]++;
                ot[d] = st_[i]; oc[d] = sc_[i]; os[d] = ss_[i];
            }
            nocc += (int64_t)m;
            ds->da_max_entries = std::max<int32_t>(ds->da_max_entries, (int32_t)mp);
            if (ot.size() >= ((size_t)1 << 31)) break;
        }
        off[(size_t)nsp] = (int32_t)ot.size();
        spt[(size_t)nsp] = (int32_t)T;
        ds->nocc = nocc;
        ds->nocc_pad = (int64_t)ot.size();
        ds->da_nspans = (int32_t)nsp;
        // any negative entry, not a negative node total: [-1, 0, 5, ...] would pass the kernels as a finite, wrong likelihood
        if (vmin < 0) { (void)hipFree(d_raw); nhp_set_error(ctx, "counts must be non-negative"); nhp_disc_dataset_destroy(ds); return NHP_EDOMAIN; }
        if (ot.size() >= ((size_t)1 << 31)) { (void)hipFree(d_raw); nhp_set_error(ctx, "too many occupied bins"); nhp_disc_dataset_destroy(ds); return NHP_ENOTIMPL; }
        const size_t no = ot.size() ? ot.size() : 4;
        if (hipMalloc(&ds->d_occ_t, 4 * no) != hipSuccess || hipMalloc(&ds->d_occ_c, 4 * no) != hipSuccess ||
            hipMalloc(&ds->d_occ_s, 8 * no) != hipSuccess || hipMalloc(&ds->d_occ_off, 4 * off.size()) != hipSuccess ||
            hipMalloc(&ds->d_span_t, 4 * spt.size()) != hipSuccess) {
            (void)hipFree(d_raw); nhp_set_error(ctx, "out of device memory (occupied-bin list)"); nhp_disc_dataset_destroy(ds); return NHP_ENOMEM;
        }
        if (!ot.empty()) {
            NHP_HIP(ctx, hipMemcpy(ds->d_occ_t, ot.data(), 4 * ot.size(), hipMemcpyHostToDevice));
            NHP_HIP(ctx, hipMemcpy(ds->d_occ_c, oc.data(), 4 * oc.size(), hipMemcpyHostToDevice));
            NHP_HIP(ctx, hipMemcpy(ds->d_occ_s, os.data(), 8 * os.size(), hipMemcpyHostToDevice));
        }
        NHP_HIP(ctx, hipMemcpy(ds->d_occ_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
        NHP_HIP(ctx, hipMemcpy(ds->d_span_t, spt.data(), 4 * spt.size(), hipMemcpyHostToDevice));
        // the adjacency sweep's entry word: node (16 bits) | count (8 bits) | bin % 256 (a span is at most 256 bins)
        static_assert(NHP_DA_SPAN == 256, "the packed entry keeps 8 bits of the bin");
        if (N <= 65536 && vmax < 256 && !ot.empty() && hipMalloc((void **)&ds->d_occ_pack, 4 * no) == hipSuccess) {
            std::vector<uint32_t> pk(ot.size());
            for (size_t i = 0; i < ot.size(); ++i)
                pk[i] = ((uint32_t)oc[i] << 16) | ((uint32_t)os[i] << 8) | (uint32_t)(ot[i] % NHP_DA_SPAN);
            NHP_HIP(ctx, hipMemcpy(ds->d_occ_pack, pk.data(), 4 * pk.size(), hipMemcpyHostToDevice));
        } else {
            (void)hipGetLastError();
            ds->d_occ_pack = nullptr;
        }
    }
    // counts that fit a byte are kept in bytes too: the convolution then reads 1/8 of the bytes next to its 3.3 GB of stores
    if (vmin >= 0 && vmax <= 255 && hipMalloc((void **)&ds->d_data8, NT) != hipSuccess) ds->d_data8 = nullptr;
    dim3 tg((unsigned)((T + 31) / 32), (unsigned)((N + 31) / 32));
    hipLaunchKernelGGL(k_disc_transpose, tg, dim3(256), 0, st, d_raw, N, T, ds->d_dataT, ds->d_data8);
    hipLaunchKernelGGL(k_disc_colstats, dim3((unsigned)N), dim3(256), 0, st, ds->d_dataT, N, T, ds->d_colsum);
    NHP_HIP(ctx, hipGetLastError());
    std::vector<double> h(2 * (size_t)N);
    NHP_HIP(ctx, hipMemcpyAsync(h.data(), ds->d_colsum, 8 * 2 * (size_t)N, hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    (void)hipFree(d_raw);
    ds->lgamma_sum = 0.0;
    for (int n = 0; n < N; ++n) ds->lgamma_sum += h[(size_t)N + n];
    *out = ds;
    return NHP_OK;
}

extern "C" void nhp_disc_dataset_destroy(nhp_disc_dataset *ds)
{
    if (!ds) return;
    (void)hipSetDevice(ds->ctx->device);
    (void)hipStreamSynchronize(ds->ctx->main());
    (void)hipFree(ds->d_dataT); (void)hipFree(ds->d_data8); (void)hipFree(ds->d_conv); (void)hipFree(ds->d_colsum);
    (void)hipFree(ds->d_occ_t); (void)hipFree(ds->d_occ_c); (void)hipFree(ds->d_occ_s); (void)hipFree(ds->d_occ_off); (void)hipFree(ds->d_occ_pack); (void)hipFree(ds->d_span_t);
    (void)hipFree(ds->d_convsum); (void)hipFree(ds->d_baseT); (void)hipFree(ds->d_base_counts); (void)hipFree(ds->d_trial_start);
    delete ds;
}

// Trials r = 0..R-1 stacked along time: offsets [R + 1] = first bin of each trial, then T.  Drops Ŝ and its column sums
// (the convolution depends on the boundaries); R = 1 puts the dataset back to one recording.
extern "C" nhp_status nhp_disc_dataset_set_trials(nhp_ctx *ctx, nhp_disc_dataset *ds, const int64_t *offsets, int32_t n_trials)
{
    if (!ctx || !ds || !offsets) return NHP_EINVAL;
    if (n_trials < 1) { nhp_set_error(ctx, "set_trials: n_trials = %d must be at least 1", n_trials); return NHP_EINVAL; }
    if (offsets[0] != 0) { nhp_set_error(ctx, "set_trials: offsets[0] = %lld must be 0", (long long)offsets[0]); return NHP_EINVAL; }
    for (int32_t r = 1; r <= n_trials; ++r)
        if (offsets[r] <= offsets[r - 1]) {
            nhp_set_error(ctx, "set_trials: offsets[%d] = %lld is not above offsets[%d] = %lld (a trial holds at least one bin)", r,
                          (long long)offsets[r], r - 1, (long long)offsets[r - 1]);
            return NHP_EINVAL;
        }
    if (offsets[n_trials] != ds->T) {
        nhp_set_error(ctx, "set_trials: offsets[%d] = %lld must be the dataset's %lld bins", n_trials, (long long)offsets[n_trials], (long long)ds->T);
        return NHP_EINVAL;
    }
    if (ds->d_baseT && n_trials > 1) {
        nhp_set_error(ctx, "set_trials: the dataset carries an LGCP baseline, whose grid is a function of time across the trials");
        return NHP_ENOTIMPL;
    }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipStreamSynchronize(st));
    uint8_t *d_start = nullptr;
    if (n_trials > 1) {
        std::vector<uint8_t> h((size_t)ds->T, 0);
        for (int32_t r = 1; r < n_trials; ++r) h[(size_t)offsets[r]] = 1;
        if (hipMalloc((void **)&d_start, (size_t)ds->T) != hipSuccess) { nhp_set_error(ctx, "out of device memory (trial starts)"); return NHP_ENOMEM; }
        if (hipMemcpy(d_start, h.data(), (size_t)ds->T, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d_start); nhp_set_error(ctx, "set_trials: the upload of the trial starts failed"); return NHP_EHIP;
        }
    }
    (void)hipFree(ds->d_trial_start);
    ds->d_trial_start = d_start;
    if (n_trials > 1) ds->trial_off.assign(offsets, offsets + n_trials + 1);
    else ds->trial_off.clear();
    (void)hipFree(ds->d_conv); ds->d_conv = nullptr;
    (void)hipFree(ds->d_convsum); ds->d_convsum = nullptr;
    ds->B = 0; ds->L = 0;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_dataset_get_trials(const nhp_disc_dataset *ds, int32_t *n_trials, int64_t *offsets)
{
    if (!ds || !n_trials) return NHP_EINVAL;
    const bool one = ds->trial_off.empty();
    *n_trials = one ? 1 : (int32_t)ds->trial_off.size() - 1;
    if (offsets) {
        if (one) { offsets[0] = 0; offsets[1] = ds->T; }
        else std::copy(ds->trial_off.begin(), ds->trial_off.end(), offsets);
    }
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_convolve(nhp_ctx *ctx, nhp_disc_dataset *ds, const double *phi, int32_t L,
                                        int32_t B, double *out)
{
    if (!ctx || !ds || !phi || L < 1 || B < 1) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t TNB = (size_t)ds->T * ds->N * B;
    hipStream_t st = ctx->main();
    if (ds->B != B || !ds->d_conv) {
        NHP_HIP(ctx, hipStreamSynchronize(st));
        if (ds->d_conv) (void)hipFree(ds->d_conv);
        ds->d_conv = nullptr;
        if (hipMalloc(&ds->d_conv, 8 * TNB) != hipSuccess) { nhp_set_error(ctx, "out of device memory for the %zu-byte convolution", 8 * TNB); return NHP_ENOMEM; }
    }
    ds->B = B; ds->L = L;
    const size_t part = (size_t)((ds->T + CONV_TB - 1) / CONV_TB) * ds->N * B;       // per-workgroup column sums (sparse kernel)
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * ((size_t)L * B + part)));
    double *d_phi = (double *)ctx->d_scratch, *d_part = d_phi + (size_t)L * B;
    NHP_HIP(ctx, hipMemcpyAsync(d_phi, phi, 8 * (size_t)L * B, hipMemcpyHostToDevice, st));
    // sparse walk (nonzero counts of the lag window only) for count data as sparse as the models assume; a dense matrix
    // (more than ~1 in 8 bins occupied) or more than 64 lags takes the dense kernel
    const bool sparse = L <= 64 && !getenv("NHP_CONV_DENSE") && (double)ds->nocc < 0.125 * (double)ds->N * (double)ds->T;
    const int tb = sparse ? CONV_TB : 256;
    dim3 grid((unsigned)((ds->T + tb - 1) / tb), (unsigned)ds->N);
    const uint8_t *d_start = ds->d_trial_start;                    // trials: the lags stop at a trial's first bin
    const size_t lds_conv = 8 * ((size_t)tb + L + (size_t)L * ((B + CONV_CB - 1) / CONV_CB * CONV_CB) +
                                 (sparse ? 4 * CONV_CB + (d_start ? 2 : 1) * ((CONV_TB + L + 63) / 64 + 2) : (d_start ? (256 + L + 7) / 8 : 0)));
    if (lds_conv > 64 * 1024) { nhp_set_error(ctx, "convolve: nlags * nbasis = %d * %d exceeds the LDS budget", L, B); return NHP_ENOTIMPL; }
    if (ds->d_convsum) { (void)hipFree(ds->d_convsum); ds->d_convsum = nullptr; }
    if (hipMalloc(&ds->d_convsum, 8 * (size_t)ds->N * B) != hipSuccess) { nhp_set_error(ctx, "out of device memory"); return NHP_ENOMEM; }
    if (sparse) {
        if (d_start) {
            hipLaunchKernelGGL(k_disc_convolve_trials, grid, dim3(256), lds_conv, st, ds->d_dataT, (const uint8_t *)ds->d_data8, d_start, ds->N, ds->T, d_phi, L, B, ds->d_conv, d_part);
        } else {
            hipLaunchKernelGGL(k_disc_convolve, grid, dim3(256), lds_conv, st, ds->d_dataT, (const uint8_t *)ds->d_data8, ds->N, ds->T, d_phi, L, B, ds->d_conv, d_part);
        }
        NHP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_disc_convsum_blocks, dim3((unsigned)(((size_t)ds->N * B + 255) / 256)), dim3(256), 0, st, d_part, (int)grid.x, ds->N, B, ds->d_convsum);
    } else {
        if (d_start) {
            hipLaunchKernelGGL(k_disc_convolve_dense_trials, grid, dim3(256), lds_conv, st, ds->d_dataT, d_start, ds->N, ds->T, d_phi, L, B, ds->d_conv);
        } else {
            hipLaunchKernelGGL(k_disc_convolve_dense, grid, dim3(256), lds_conv, st, ds->d_dataT, ds->N, ds->T, d_phi, L, B, ds->d_conv);
        }
        NHP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_disc_convsum, dim3((unsigned)((size_t)ds->N * B)), dim3(256), 0, st, ds->d_conv, ds->T, ds->d_convsum);
    }
    NHP_HIP(ctx, hipGetLastError());
    if (out) NHP_HIP(ctx, hipMemcpyAsync(out, ds->d_conv, 8 * TNB, hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}

// Σ_t Ŝ[t, n, b] as the convolution left it on the device -> out [N*B], node fastest
extern "C" nhp_status nhp_disc_dataset_get_convsum(nhp_ctx *ctx, const nhp_disc_dataset *ds, double *out)
{
    if (!ctx || !ds || !out) return NHP_EINVAL;
    if (!ds->d_convsum) { nhp_set_error(ctx, "get_convsum: convolve(process, data) must run first"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    NHP_HIP(ctx, hipMemcpy(out, ds->d_convsum, 8 * (size_t)ds->N * ds->B, hipMemcpyDeviceToHost));
    return NHP_OK;
}

// uploads the model pieces, builds E and base on the device; returns pointers into scratch
nhp_status nhp_disc_stage_bump(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W,
                               const double *theta, const double *A, double dt, double **E, double **base, size_t extra,
                               double **extra_ptr, int cat_order, bool on_device)
{
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!ds->d_conv) { nhp_set_error(ctx, "convolve(process, data) must run before intensity / loglikelihood"); return NHP_EINVAL; }
    if (!W || !theta) return NHP_EINVAL;
    if (!lambda0 && !ds->d_baseT) { nhp_set_error(ctx, "lambda0 is NULL and the dataset has no LGCP baseline (nhp_disc_set_lgcp_baseline)"); return NHP_EINVAL; }
    const size_t N = (size_t)ds->N, NN = N * N, B = (size_t)ds->B, K = N * B;
    const size_t need = 8 * (K * N + N + N + NN + NN * B + NN + extra);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, need));
    double *p = (double *)ctx->d_scratch;
    double *dE = p; p += K * N;
    double *dbase = p; p += N;
    double *dl0 = p; p += N;
    double *dW = p; p += NN;
    double *dth = p; p += NN * B;
    double *dA = p; p += NN;
    *extra_ptr = p;
    hipStream_t st = ctx->main();
    if (lambda0) NHP_HIP(ctx, hipMemcpyAsync(dl0, lambda0, 8 * N, kind, st));
    else NHP_HIP(ctx, hipMemsetAsync(dl0, 0, 8 * N, st));          // per-bin baseline comes from ds->d_baseT
    NHP_HIP(ctx, hipMemcpyAsync(dW, W, 8 * NN, kind, st));
    NHP_HIP(ctx, hipMemcpyAsync(dth, theta, 8 * NN * B, kind, st));
    if (A) NHP_HIP(ctx, hipMemcpyAsync(dA, A, 8 * NN, kind, st));
    hipLaunchKernelGGL(k_disc_bump, dim3((unsigned)((NN * B + 255) / 256)), dim3(256), 0, st, (int)N, (int)B, dt, dl0, dW,
                       dth, A ? dA : nullptr, dE, dbase, cat_order);
    NHP_HIP(ctx, hipGetLastError());
    *E = dE; *base = dbase;
    return NHP_OK;
}

// λ = base ⊕ G·E into dlam [T x N] (GEMM-1 with the plain epilogue); shared with the adjacency sweep
nhp_status nhp_disc_launch_intensity(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base,
                                     bool per_bin_baseline, double *dlam)
{
    gemm_args g{};
    g.A = ds->d_conv; g.lda = (size_t)ds->T; g.B = E; g.ldb = (size_t)ds->N * ds->B;
    g.M = (int)ds->T; g.N = ds->N; g.K = ds->N * ds->B; g.k_chunk = g.K;
    g.base = base; g.baseT = per_bin_baseline ? ds->d_baseT : nullptr; g.out = dlam;
    launch_gemm<true, EPI_INTENSITY>(g, 1, ctx->main(), gemm1_tile_m(g.M, g.N, ctx->cu_count));
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// rows [t0, t0 + R) of the same product: the A operand starts t0 rows down its columns (lda stays T), the output is R x N
nhp_status nhp_disc_launch_intensity_rows(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base, int64_t t0,
                                          int64_t R, double *dlam)
{
    if (t0 < 0 || R < 1 || t0 + R > ds->T) { nhp_set_error(ctx, "intensity rows [%lld, %lld) outside the dataset", (long long)t0, (long long)(t0 + R)); return NHP_EINVAL; }
    gemm_args g{};
    g.A = ds->d_conv + t0; g.lda = (size_t)ds->T; g.B = E; g.ldb = (size_t)ds->N * ds->B;
    g.M = (int)R; g.N = ds->N; g.K = ds->N * ds->B; g.k_chunk = g.K;
    g.base = base; g.baseT = nullptr; g.out = dlam;
    launch_gemm<true, EPI_INTENSITY>(g, 1, ctx->main(), gemm1_tile_m(g.M, g.N, ctx->cu_count));
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_intensity(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                         const double *W, const double *theta, const double *A, double dt,
                                         double *lam)
{
    if (!ctx || !ds || !lam) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t TN = (size_t)ds->T * ds->N;
    double *E, *base, *dlam;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, A, dt, &E, &base, TN, &dlam));
    gemm_args g{};
    g.A = ds->d_conv; g.lda = (size_t)ds->T; g.B = E; g.ldb = (size_t)ds->N * ds->B;
    g.M = (int)ds->T; g.N = ds->N; g.K = ds->N * ds->B; g.k_chunk = g.K;
    g.base = base; g.baseT = lambda0 ? nullptr : ds->d_baseT; g.out = dlam;
    launch_gemm<true, EPI_INTENSITY>(g, 1, ctx->main(), gemm1_tile_m(g.M, g.N, ctx->cu_count));
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipMemcpyAsync(lam, dlam, 8 * TN, hipMemcpyDeviceToHost, ctx->main()));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                      const double *W, const double *theta, const double *A, double dt, double *ll)
{
    if (!ctx || !ds || !ll) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    double *E, *base, *unused;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, A, dt, &E, &base, 0, &unused));
    gemm_args g{};
    g.A = ds->d_conv; g.lda = (size_t)ds->T; g.B = E; g.ldb = (size_t)ds->N * ds->B;
    g.M = (int)ds->T; g.N = ds->N; g.K = ds->N * ds->B; g.k_chunk = g.K;
    g.base = base; g.baseT = lambda0 ? nullptr : ds->d_baseT; g.dataT = ds->d_dataT;
    const int bm = gemm1_tile_m(g.M, g.N, ctx->cu_count);
    const int blocks = ((g.M + bm - 1) / bm) * ((g.N + BN - 1) / BN);
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)blocks));
    g.partials = ctx->d_partials;
    launch_gemm<true, EPI_LOGLIK>(g, 1, ctx->main(), bm);
    NHP_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sum_pairs, dim3(1), dim3(256), 0, ctx->main(), ctx->d_partials, blocks, ds->lgamma_sum, ctx->d_results);
    NHP_HIP(ctx, hipGetLastError());
    return nhp_ctx_fetch(ctx, 0, 1, ll);
}

// ---- DiscreteLogGaussianCoxProcess baseline (reference src/baselines.jl:461-609).  intensity(p, ts) is the
// piecewise-linear interpolation of (x, λ[:, n]·dt); the process intensity evaluates it at ts = 1..T
// (src/discrete.jl:117), the baseline's own likelihood at range(p) = x[1] : dt : x[end]-dt (:553-584).
__device__ __forceinline__ void disc_interp_cell(const double *x, int G, double t, int *lo, double *wlo, double *whi)
{
    // src/utils/interpolation.jl:26-35: x0 in [x[i], x[i+1]) -> cell i; x0 >= x[end] -> last value
    int a = 0, b = G - 1;
    if (!(t < x[b])) { *lo = b; *wlo = 1.0; *whi = 0.0; return; }
    while (b - a > 1) { const int mid = (a + b) >> 1; if (t >= x[mid]) a = mid; else b = mid; }
    const double w = x[a + 1] - x[a];
    *lo = a; *wlo = (x[a + 1] - t) / w; *whi = (t - x[a]) / w;
}

// baseT[t + T·c] = interp(x, lam[:, c]·dt)(t + 1)
__global__ __launch_bounds__(256) void k_disc_base_interp(const double *__restrict__ x, int G, const double *__restrict__ lam,
                                                          double dt, int64_t T, double *__restrict__ baseT)
{
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (t >= T) return;
    const double time = (double)(t + 1);
    const double *y = lam + (size_t)c * G;
    int lo; double wlo, whi;
    disc_interp_cell(x, G, time, &lo, &wlo, &whi);
    double v;
    if (lo == G - 1) v = y[G - 1] * dt;
    else v = ((y[lo + 1] * dt) * (time - x[lo]) + (y[lo] * dt) * (x[lo + 1] - time)) / (x[lo + 1] - x[lo]);
    baseT[(size_t)t + (size_t)T * c] = v;
}

// grad[g + G·c] += dt Σ_t (R[t,c] - 1) w_g(t + 1)
__global__ __launch_bounds__(256) void k_disc_grad_lgcp(const double *__restrict__ R, int64_t T, int G, const double *__restrict__ x,
                                                        double dt, double *__restrict__ grad)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (t >= T) return;
    const double r = (R[(size_t)t + (size_t)T * c] - 1.0) * dt;
    int lo; double wlo, whi;
    disc_interp_cell(x, G, (double)(t + 1), &lo, &wlo, &whi);
    atomicAdd(&grad[(size_t)c * G + lo], r * wlo);
    if (whi != 0.0) atomicAdd(&grad[(size_t)c * G + lo + 1], r * whi);
}

// ll[c] = Σ_t log pdf(Poisson(λ_t), s0[t,c]),  λ_t = interp(x, cand[:, c]·dt)(x[0] + t·dt)   (src/baselines.jl:571-584)
__global__ __launch_bounds__(256) void k_disc_lgcp_ll(const int *__restrict__ s0, int64_t T, int G, const double *__restrict__ x,
                                                      const double *__restrict__ cand, double dt, double *__restrict__ ll)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const int c = blockIdx.x;
    const double *y = cand + (size_t)c * G;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) {
        const double time = x[0] + (double)t * dt;
        int lo; double wlo, whi;
        disc_interp_cell(x, G, time, &lo, &wlo, &whi);
        double lam;
        if (lo == G - 1) lam = y[G - 1] * dt;
        else lam = ((y[lo + 1] * dt) * (time - x[lo]) + (y[lo] * dt) * (x[lo + 1] - time)) / (x[lo + 1] - x[lo]);
        const double s = (double)s0[(size_t)t + (size_t)T * c];
        acc += (s == 0.0 ? 0.0 : s * nhp_log(lam)) - lam - lgamma(s + 1.0);
    }
    acc = nhp_block_sum(acc, red);
    if (threadIdx.x == 0) ll[c] = acc;
}

// ---- gradient of the discrete log-likelihood in the reference's mle! parameters [λ0; η = W∘θ]
// (params / params! src/discrete.jl:174-201; the reference hands Optim no gradient -- its d_loglikelihood
// :298-314 is commented out of mle! -- so one gradient costs it 2(N + N²B) objective calls):
//     ∂ll/∂λ0[c] = dt Σ_t (s_tc/λ_tc - 1),      ∂ll/∂η[p,c,b] = dt Σ_t (s_tc/λ_tc - 1) Ŝ[t,p,b]
// i.e. with R = data/Z from GEMM-1:  dt (colsum R - T)  and  dt (Gᵀ·R - Σ_t Ŝ) -- the VB step's two GEMMs
// with a different last kernel.
__global__ __launch_bounds__(256) void k_disc_grad_finish(int N, int B, int splits, int row_blocks, double dt, double Tbins,
                                                          const double *__restrict__ slabs, const double *__restrict__ colp,
                                                          const double *__restrict__ convsum, double *__restrict__ grad)
{
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NN * B) {
        const size_t b = i / NN, pc = i % NN, p = pc % N, c = pc / N, k = p + b * N;
        double g = 0.0;
        for (int z = 0; z < splits; ++z) g += slabs[(size_t)z * K * N + k + c * K];      // fixed order
        grad[N + i] = dt * (g - convsum[k]);
    }
    if (i < (size_t)N) {
        double r = 0.0;
        for (int rb = 0; rb < row_blocks; ++rb) r += colp[(size_t)rb * N + i];
        grad[i] = dt * (r - Tbins);
    }
}

// Sizes of one (log-likelihood, gradient) evaluation and its scratch behind the bump table
struct disc_grad_plan {
    size_t N, NN, B, K, T, G, nbase;
    int bm, row_blocks, splits, k_chunk;
    size_t extra() const { return T * N + (size_t)row_blocks * N + (size_t)splits * K * N + nbase + NN * B + G; }
};

static disc_grad_plan disc_grad_sizes(nhp_ctx *ctx, const nhp_disc_dataset *ds, bool homogeneous)
{
    disc_grad_plan q{};
    q.N = (size_t)ds->N; q.NN = q.N * q.N; q.B = (size_t)ds->B; q.K = q.N * q.B; q.T = (size_t)ds->T;
    q.G = homogeneous ? 0 : ds->h_grid_x.size();
    q.nbase = homogeneous ? q.N : q.G * q.N;                     // params(baseline): λ or vec(λ) (G x N)
    q.bm = gemm1_tile_m((int64_t)q.T, (int)q.N, ctx->cu_count);
    q.row_blocks = (int)((q.T + q.bm - 1) / q.bm);
    const int tiles2 = (int)(((q.K + BM - 1) / BM) * ((q.N + BN - 1) / BN));
    int splits = (2 * ctx->cu_count + tiles2 - 1) / tiles2;
    splits = std::max(1, std::min(splits, (int)((q.T + 4 * BK - 1) / (4 * BK))));
    int k_chunk = (int)((q.T + splits - 1) / splits);
    k_chunk = ((k_chunk + BK - 1) / BK) * BK;
    q.k_chunk = k_chunk;
    q.splits = (int)((q.T + k_chunk - 1) / k_chunk);
    return q;
}

// log-likelihood -> ctx->d_results[0], gradient in [params(baseline); vec(W .* θ)] order -> *dgrad_out (inside `x`, the
// scratch behind the bump table E / base); asynchronous
static nhp_status disc_grad_enqueue(nhp_ctx *ctx, const nhp_disc_dataset *ds, const disc_grad_plan &q, bool homogeneous, const double *E,
                                    const double *base, double *x, double dt, double **dgrad_out)
{
    const size_t N = q.N, NN = q.NN, B = q.B, K = q.K, T = q.T, G = q.G, nbase = q.nbase;
    double *dR = x; x += T * N;
    double *dcolp = x; x += (size_t)q.row_blocks * N;
    double *dslab = x; x += (size_t)q.splits * K * N;
    double *dgrad = x;
    hipStream_t st = ctx->main();
    // GEMM-1 once, with both epilogues: the Poisson log-likelihood partials AND R = data / Z with its column sums
    gemm_args g{};
    g.A = ds->d_conv; g.lda = T; g.B = E; g.ldb = K; g.M = (int)T; g.N = (int)N; g.K = (int)K; g.k_chunk = (int)K;
    g.base = base; g.baseT = homogeneous ? nullptr : ds->d_baseT; g.dataT = ds->d_dataT;
    const int blocks = ((g.M + q.bm - 1) / q.bm) * ((g.N + BN - 1) / BN);
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)blocks));
    g.partials2 = ctx->d_partials;
    g.out = dR; g.partials = dcolp;
    launch_gemm<true, EPI_GRAD>(g, 1, st, q.bm);
    hipLaunchKernelGGL(k_sum_pairs, dim3(1), dim3(256), 0, st, ctx->d_partials, blocks, ds->lgamma_sum, ctx->d_results);
    // then Gᵀ·R in T-slabs
    gemm_args g2{};
    g2.A = ds->d_conv; g2.lda = T; g2.B = dR; g2.ldb = T; g2.M = (int)K; g2.N = (int)N; g2.K = (int)T; g2.k_chunk = q.k_chunk;
    g2.out = dslab;
    launch_gemm<false, EPI_SLAB>(g2, q.splits, st);
    hipLaunchKernelGGL(k_disc_grad_finish, dim3((unsigned)((NN * B + 255) / 256)), dim3(256), 0, st, (int)N, (int)B, q.splits, q.row_blocks,
                       dt, (double)T, dslab, dcolp, ds->d_convsum, dgrad + (nbase - N));
    if (!homogeneous) {
        // LGCP: ∂λ_base[t,c]/∂λgrid[g,c] = dt·w_g(t) (interpolation weights at bin time t+1), so the baseline block
        // is dt Σ_t (R - 1)[t,c] w_g -- it overwrites the N homogeneous entries k_disc_grad_finish left at its end
        double *dgx = dgrad + nbase + NN * B;
        NHP_HIP(ctx, hipMemcpyAsync(dgx, ds->h_grid_x.data(), 8 * G, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemsetAsync(dgrad, 0, 8 * nbase, st));
        hipLaunchKernelGGL(k_disc_grad_lgcp, dim3((unsigned)((T + 255) / 256), (unsigned)N), dim3(256), 0, st, dR, (int64_t)T, (int)G,
                           dgx, dt, dgrad);
    }
    NHP_HIP(ctx, hipGetLastError());
    *dgrad_out = dgrad;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_loglik_grad(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                           const double *W, const double *theta, double dt, double *ll, double *grad,
                                           int64_t grad_len)
{
    if (!ctx || !ds || !ll || !grad) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const disc_grad_plan q = disc_grad_sizes(ctx, ds, lambda0 != nullptr);
    if ((size_t)grad_len != q.nbase + q.NN * q.B) { nhp_set_error(ctx, "Parameter vector length does not match model parameter length."); return NHP_ESHAPE; }
    if (!ds->d_convsum) { nhp_set_error(ctx, "convolve(process, data) must run before the gradient"); return NHP_EINVAL; }
    double *E, *base, *x, *dgrad;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, nullptr, dt, &E, &base, q.extra(), &x));
    NHP_TRY(disc_grad_enqueue(ctx, ds, q, lambda0 != nullptr, E, base, x, dt, &dgrad));
    NHP_HIP(ctx, hipMemcpyAsync(grad, dgrad, 8 * (q.nbase + q.NN * q.B), hipMemcpyDeviceToHost, ctx->main()));
    return nhp_ctx_fetch(ctx, 0, 1, ll);
}

// ---- thin launchers for disc_information.hip (declared in nhp_internal.h): the two GEMM launches it re-drives ----
// the Poisson log-likelihood of a staged bump table -> ctx->d_results[0]: nhp_disc_loglik's own launch pair, so its bits
nhp_status nhp_disc_launch_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base)
{
    gemm_args g{};
    g.A = ds->d_conv; g.lda = (size_t)ds->T; g.B = E; g.ldb = (size_t)ds->N * ds->B;
    g.M = (int)ds->T; g.N = ds->N; g.K = ds->N * ds->B; g.k_chunk = g.K;
    g.base = base; g.baseT = nullptr; g.dataT = ds->d_dataT;
    const int bm = gemm1_tile_m(g.M, g.N, ctx->cu_count);
    const int blocks = ((g.M + bm - 1) / bm) * ((g.N + BN - 1) / BN);
    NHP_TRY(nhp_ctx_reserve_partials(ctx, 2 * (size_t)blocks));
    g.partials = ctx->d_partials;
    launch_gemm<true, EPI_LOGLIK>(g, 1, ctx->main(), bm);
    NHP_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sum_pairs, dim3(1), dim3(256), 0, ctx->main(), ctx->d_partials, blocks, ds->lgamma_sum, ctx->d_results);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// the T-slabs of the gradient's Gᵀ·R: how many, and their length
void nhp_disc_gtr_plan(nhp_ctx *ctx, const nhp_disc_dataset *ds, int *splits, int *k_chunk)
{
    const disc_grad_plan q = disc_grad_sizes(ctx, ds, true);
    *splits = q.splits; *k_chunk = q.k_chunk;
}

// slabs[z][k + c·K] = Σ_{t in slab z} Ŝ[t,k]·R[t,c]   (R is T x N, t fastest; the caller sums the slabs in order)
nhp_status nhp_disc_launch_gtr(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *dR, int splits, int k_chunk, double *dslab)
{
    gemm_args g2{};
    g2.A = ds->d_conv; g2.lda = (size_t)ds->T; g2.B = dR; g2.ldb = (size_t)ds->T;
    g2.M = ds->N * ds->B; g2.N = ds->N; g2.K = (int)ds->T; g2.k_chunk = k_chunk;
    g2.out = dslab;
    launch_gemm<false, EPI_SLAB>(g2, splits, ctx->main());
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// ---- mle!(process::DiscreteStandardHawkesProcess, data) with the optimizer's state on the device (src/discrete.jl:211-296) ----
// x = params(process) = [λ0; vec(W .* θ)] (src/discrete.jl:178-182).  params!(process, x) (:195-203) splits the second block
// into W = Σ_b x[p,c,b] and θ = x ./ W, and the objective's bump is (W·θ)·dt (:381-385): the same three roundings here, from
// the DEVICE vector.  E[k + c·K], k = p + b·N; base[c] = λ0[c]·dt.
__global__ __launch_bounds__(256) void k_disc_bump_from_x(int N, int B, double dt, const double *__restrict__ x, double *__restrict__ E,
                                                          double *__restrict__ base)
{
#pragma clang fp contract(off)
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t pc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pc < NN) {
        const size_t p = pc % N, c = pc / N;
        const double *xw = x + N;
        double w = 0.0;
        for (int b = 0; b < B; ++b) w += xw[pc + (size_t)b * NN];
        for (int b = 0; b < B; ++b) {
            const double th = xw[pc + (size_t)b * NN] / w;
            E[p + (size_t)b * N + c * K] = (w * th) * dt;
        }
    }
    if (pc < (size_t)N) base[pc] = x[pc] * dt;
}

#include "nhp_lbfgs.h"

extern "C" nhp_status nhp_disc_mle_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt, double lower, double upper, double f_abstol,
                                       int32_t max_steps, double *x, int64_t P, double *loss, int32_t *steps_out, int32_t *converged_out,
                                       int32_t *evals_out)
{
    if (!ctx || !ds || !x || !loss || !steps_out || !converged_out) return NHP_EINVAL;
    if (!(lower < upper) || max_steps < 0 || !(dt > 0.0)) return NHP_EDOMAIN;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    if (!ds->d_conv || !ds->d_convsum) { nhp_set_error(ctx, "convolve(process, data) must run before mle!"); return NHP_EINVAL; }
    const disc_grad_plan q = disc_grad_sizes(ctx, ds, true);
    if ((size_t)P != q.nbase + q.NN * q.B) { nhp_set_error(ctx, "Parameter vector length does not match model parameter length."); return NHP_ESHAPE; }
    // scratch: E | base | the evaluation's buffers (nhp_disc_stage_bump's layout without its host-side copies)
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (q.K * q.N + q.N + q.extra())));
    auto eval = [&](const double *d_x, double *d_g, bool /*commit*/) -> nhp_status {
        hipStream_t st = ctx->main();
        double *E = (double *)ctx->d_scratch, *base = E + q.K * q.N, *xs = base + q.N, *dgrad = nullptr;
        hipLaunchKernelGGL(k_disc_bump_from_x, dim3((unsigned)((q.NN + 255) / 256)), dim3(256), 0, st, (int)q.N, (int)q.B, dt, d_x, E, base);
        NHP_TRY(disc_grad_enqueue(ctx, ds, q, true, E, base, xs, dt, &dgrad));
        hipLaunchKernelGGL(k_mle_neg, dim3((unsigned)std::min<int64_t>(2048, (P + 255) / 256)), dim3(256), 0, st, d_g, (const double *)dgrad, P);
        NHP_HIP(ctx, hipGetLastError());
        return NHP_OK;
    };
    return nhp_lbfgs_box(ctx, P, lower, upper, f_abstol, max_steps, eval, x, loss, steps_out, converged_out, evals_out);
}

// DiscreteLogGaussianCoxProcess(x, λ, Σ, m, dt) as the baseline of this dataset's process (src/baselines.jl:461-509):
// builds the per-bin baseline intensity on the device; later calls that pass lambda0 = NULL use it.
extern "C" nhp_status nhp_disc_set_lgcp_baseline(nhp_ctx *ctx, nhp_disc_dataset *ds, const double *grid_x, int32_t grid_n,
                                                 const double *lam, double dt)
{
    if (!ctx || !ds || !grid_x || !lam || grid_n < 2) return NHP_EINVAL;
    if (ds->d_trial_start) { nhp_set_error(ctx, "set_lgcp_baseline: the grid is a function of time and the dataset holds several trials"); return NHP_ENOTIMPL; }
    for (int g = 0; g + 1 < grid_n; ++g)
        if (!(grid_x[g + 1] > grid_x[g])) { nhp_set_error(ctx, "grid points must be strictly increasing"); return NHP_EDOMAIN; }
    // the interpolator throws outside [x[1], x[end]] (src/utils/interpolation.jl:27); bins are evaluated at 1..T
    if (grid_x[0] > 1.0 || grid_x[grid_n - 1] < (double)ds->T) {
        nhp_set_error(ctx, "bin times 1..%lld fall outside the grid support [%g, %g]", (long long)ds->T, grid_x[0], grid_x[grid_n - 1]);
        return NHP_EDOMAIN;
    }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)ds->N, T = (size_t)ds->T, G = (size_t)grid_n;
    if (!ds->d_baseT && hipMalloc(&ds->d_baseT, 8 * T * N) != hipSuccess) { nhp_set_error(ctx, "out of device memory (baseline matrix)"); return NHP_ENOMEM; }
    if (!ds->d_base_counts && hipMalloc(&ds->d_base_counts, 4 * T * N) != hipSuccess) { nhp_set_error(ctx, "out of device memory (baseline counts)"); return NHP_ENOMEM; }
    ds->h_grid_x.assign(grid_x, grid_x + grid_n);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (G + G * N)));
    double *dx = (double *)ctx->d_scratch, *dl = dx + G;
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(dx, grid_x, 8 * G, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(dl, lam, 8 * G * N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_disc_base_interp, dim3((unsigned)((T + 255) / 256), (unsigned)N), dim3(256), 0, st, dx, grid_n, dl, dt, ds->T, ds->d_baseT);
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}

// loglikelihood(p::DiscreteLogGaussianCoxProcess, data, node, y) for all nodes (src/baselines.jl:571-584), data =
// the per-bin baseline counts parents[:, :, 1] of the latest nhp_disc_resample_parents on this dataset; cand [G*N]
// holds exp.(m .+ y) per node.
extern "C" nhp_status nhp_disc_lgcp_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *cand, double dt, double *ll)
{
    if (!ctx || !ds || !cand || !ll) return NHP_EINVAL;
    if (!ds->d_base_counts || !ds->base_counts_valid) { nhp_set_error(ctx, "lgcp_loglik: run resample_parents with the LGCP baseline first"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N = (size_t)ds->N, G = ds->h_grid_x.size();
    // range(p) = x[1] : dt : x[end] - dt must have T points inside the support
    if (ds->h_grid_x[0] + (double)(ds->T - 1) * dt > ds->h_grid_x[G - 1]) { nhp_set_error(ctx, "lgcp_loglik: bins fall outside the grid support"); return NHP_EDOMAIN; }
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (G + G * N + N)));
    double *dx = (double *)ctx->d_scratch, *dc = dx + G, *dll = dc + G * N;
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(dx, ds->h_grid_x.data(), 8 * G, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(dc, cand, 8 * G * N, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_disc_lgcp_ll, dim3((unsigned)N), dim3(256), 0, st, ds->d_base_counts, ds->T, (int)G, dx, dc, dt, dll);
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipMemcpyAsync(ll, dll, 8 * N, hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}

