// LatentDistanceNetworkModel: resample!(network, A) on the device (the reference leaves the model an empty stub at the end
// of src/networks.jl).
//
//   z_n ~ N(0, σ² I_D), b ~ N(μb, σb²), η[p,c] = b - ‖z_p - z_c‖², A[p,c] ~ Bernoulli(1 / (1 + exp(-η[p,c]))) (diagonal included)
//
// One resample is (1) a sweep over the positions, node after node, each by elliptical slice sampling on its conditional
// L_n(z) = Σ_{j≠n} s_nj η_j - 2 softplus(η_j), s_nj = A[n,j] + A[j,n], and (2) elliptical slice sampling of b - μb on the full
// log-likelihood.  Both follow the rule of the reference's elliptical_slice (src/baselines.jl:287-326): threshold
// L(current) + log u0, θ1 = 2π u1 with the bracket [θ1 - 2π, θ1], a rejected θ < 0 becomes the lower end and any other the
// upper end, the next θ is uniform in the bracket, the first candidate with L >= threshold is accepted, 100 attempts.
//
// The bracket moves by the sign of the rejected angle only, so the candidate angles of a step are a function of its
// uniforms and of no likelihood: k_lat_prepare turns every step's draws into log u0, the scaled normals and the cosines and
// sines of all 100 angles before the chain starts, and a step evaluates a batch of candidates at once and takes the first
// that passes (further batches only when none does).
//
// The position sweep is a chain of N dependent steps and runs in ONE workgroup (k_lat_sweep): the positions stay in LDS,
// the threads split the other nodes j between them, each carries the partial sums of the whole batch, and the sums are
// reduced inside a wave by DPP and across the waves through LDS in wave order -- no floating-point atomics, one
// workgroup barrier per step.  The bit rows and columns of A (k_sbm_pack) and the prepared draws of the next step are
// requested one step ahead.
#include <algorithm>
#include <cmath>
#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_rng.h"

#define LAT_MAX_D 8
#define LAT_MAX_ATT 100                    // attempts of one slice step, as in the reference
#ifndef LAT_BLOCK
#define LAT_BLOCK 512                      // threads of the position sweep's workgroup (measured against 256 and 1024)
#endif
#define LAT_J 8                            // candidates per batch of a position step (the first batch: the current position + 7)
#define LAT_JB 16                          // candidates per batch of the offset step
#define LAT_MAX_WORDS 256                  // bit words per column: N <= 8192
#define LAT_LDS_BUDGET (160 * 1024)
#define LAT_REC 209                        // prepared draws of a step: log u0; ν [8]; (cos θ_c, sin θ_c), c = 1..100
#define LAT_HEAD (9 + 2 * (LAT_J - 1))     // the part of a record the first batch needs
#define LAT_OFF_BLOCKS 256                 // workgroups of the offset pass at most
#define LAT_CHUNK_STEPS 32768              // steps whose draws a stand-alone call holds on the device at a time

struct lat_off {                           // the offset step's state between its batches
    int done, pad;
    double thr;
};

struct nhp_latent_state {
    int32_t D = 0;
    double sigma = 1.0, mu_b = 0.0, sigma_b = 1.0;
    int32_t positions_every = 1;
    double *d_z = nullptr;              // [N*D] column-major: z_n[d] at n + N·d
    double *d_b = nullptr;              // [1]
    double *d_P = nullptr;              // [N*N] link probabilities of the latest step for the adjacency sweep; between the
                                        // position sweep and the next fill it holds ‖z_p - z_c‖² for the offset update
    double *d_sum = nullptr;            // [2] Σb, Σb² over the kept steps
    double *d_psum = nullptr;           // [N*N] Σ link probability over the kept steps
    double *d_raw = nullptr;            // [N*(D+101) + 102] the step's draws
    double *d_prep = nullptr;           // [(N+1)*LAT_REC] ... prepared
    double *d_partial = nullptr;        // [LAT_OFF_BLOCKS*LAT_JB]
    uint32_t *d_bits = nullptr;         // [2][N*W] A by column, A by row
    lat_off *d_off = nullptr;
    long long *d_exh = nullptr;         // slice steps that used up their 100 attempts and kept their value
};

// ---- device helpers -------------------------------------------------------------------------------------------------
// log1p(t) for t in [0, 1] as 2·atanh(s), s = t / (2 + t) <= 1/3, by the odd series up to s^33: the first term left out is
// below 2e-18 of the result.  With nhp_exp_neg this is half the instructions of the library's log1p(exp(·)), which the
// position sweep spends nearly all its time in; both stay within a few 1e-16 of them.
__device__ __forceinline__ double lat_log1p01(double t)
{
    const double s = t * rng_rcp(2.0 + t), w = s * s;
    double p = 1.0 / 33.0;
    p = fma(p, w, 1.0 / 31.0); p = fma(p, w, 1.0 / 29.0); p = fma(p, w, 1.0 / 27.0); p = fma(p, w, 1.0 / 25.0);
    p = fma(p, w, 1.0 / 23.0); p = fma(p, w, 1.0 / 21.0); p = fma(p, w, 1.0 / 19.0); p = fma(p, w, 1.0 / 17.0);
    p = fma(p, w, 1.0 / 15.0); p = fma(p, w, 1.0 / 13.0); p = fma(p, w, 1.0 / 11.0); p = fma(p, w, 1.0 / 9.0);
    p = fma(p, w, 1.0 / 7.0); p = fma(p, w, 1.0 / 5.0); p = fma(p, w, 1.0 / 3.0); p = fma(p, w, 1.0);
    return 2.0 * s * p;
}
// softplus(η) = max(η, 0) + log1p(exp(-|η|))
__device__ __forceinline__ double lat_softplus(double eta) { return fmax(eta, 0.0) + lat_log1p01(nhp_exp_neg(-fabs(eta))); }

__device__ __forceinline__ double lat_dist2(const double *__restrict__ z, int N, int D, int p, int c)
{
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) { const double x = z[p + (size_t)N * d] - z[c + (size_t)N * d]; d2 += x * x; }
    return d2;
}

__device__ __forceinline__ double lat_dpp(double v, const int ctrl)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    switch (ctrl) {          // the control word is an immediate
    case 0xB1: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true));
    case 0x4E: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true));
    case 0x141: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true));
    default: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true));
    }
}
__device__ __forceinline__ double lat_lane(double v, const int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Sum over the 64 lanes, the same value in every lane: butterflies inside rows of 16 lanes (both operands of every add are
// the same pair in either lane, so the lanes of a row agree bit for bit), then the four rows in row order.
__device__ __forceinline__ double lat_wave_sum(double v)
{
    v += lat_dpp(v, 0xB1);          // quad_perm [1,0,3,2]
    v += lat_dpp(v, 0x4E);          // quad_perm [2,3,0,1]
    v += lat_dpp(v, 0x141);         // row_half_mirror
    v += lat_dpp(v, 0x140);         // row_mirror
    return ((lat_lane(v, 0) + lat_lane(v, 16)) + lat_lane(v, 32)) + lat_lane(v, 48);
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// The draw stream of `nsw` sweeps from sweep `sweep0` on (layout: nhp.h): element e of sweep s is a normal or a uniform of
// global step g = s·(N+1) + n (n = N: the offset step).  Keys: nhp_rng.h.
__global__ __launch_bounds__(256) void k_lat_draws(double *__restrict__ raw, int N, int Np, int D, uint64_t seed, uint64_t step, int64_t sweep0,
                                                   int64_t count)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const int64_t RS = (int64_t)Np * (D + 101) + 102, sl = e / RS, pos = e % RS;
    int n, k, dims;
    if (pos < (int64_t)Np * (D + 101)) { n = (int)(pos / (D + 101)); k = (int)(pos % (D + 101)); dims = D; }
    else { n = N; k = (int)(pos - (int64_t)Np * (D + 101)); dims = 1; }
    const uint64_t g = (uint64_t)(sweep0 + sl) * (uint64_t)(N + 1) + (uint64_t)n;
    raw[e] = k < dims ? dev_normal(seed ^ NHP_KEY_LAT_NORMAL, step, g * 8 + (uint64_t)k, 0)
                      : nhp_philox_uniform(seed ^ NHP_KEY_LAT_UNIFORM, step, g * 101 + (uint64_t)(k - dims));
}

// One thread per step: its draws [normals; u0; u1..u100] -> its record [log u0; scale·normals; (cos θ_c, sin θ_c)].
__global__ __launch_bounds__(64) void k_lat_prepare(const double *__restrict__ raw, double *__restrict__ prep, int Np, int D, double sigma,
                                                    double sigma_b, int64_t records)
{
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= records) return;
    const int64_t RS = (int64_t)Np * (D + 101) + 102, sl = r / (Np + 1);
    const int n = (int)(r % (Np + 1));
    const int dims = n < Np ? D : 1;
    const double scale = n < Np ? sigma : sigma_b;
    const double *u = raw + sl * RS + (int64_t)n * (D + 101);
    double *o = prep + r * LAT_REC;
    for (int d = 0; d < LAT_MAX_D; ++d) o[1 + d] = d < dims ? scale * u[d] : 0.0;
    u += dims;
    o[0] = log(u[0]);
    const double two_pi = 6.283185307179586;
    double th = two_pi * u[1], tmin = th - two_pi, tmax = th;
    for (int c = 1; c <= LAT_MAX_ATT; ++c) {
        if (c > 1) {
            if (th < 0.0) tmin = th; else tmax = th;
            th = tmin + (tmax - tmin) * u[c];
        }
        double sn, cs;
        sincos(th, &sn, &cs);
        o[9 + 2 * (c - 1)] = cs; o[10 + 2 * (c - 1)] = sn;
    }
}

// The position sweep.  Dynamic LDS: Z [D][N] doubles, the waves' partial sums [2][waves][J], the head of the current, the
// next and the previous step's record [3][LAT_HEAD], the bits of their node's column and row [3][2][W].  Step i of the
// launch uses record / attempts / trace slot (i / N)·stride + i % N.
template <int D>
__global__ __launch_bounds__(LAT_BLOCK) void k_lat_sweep(int N, int W, int n_sweeps, int stride, double *__restrict__ z, const double *__restrict__ bp,
                                                     const uint32_t *__restrict__ colb, const uint32_t *__restrict__ rowb,
                                                     const double *__restrict__ prep, int32_t *__restrict__ attempts,
                                                     double *__restrict__ trace, long long *__restrict__ exhausted)
{
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int BLOCK = LAT_BLOCK, NW = LAT_BLOCK / 64, J = LAT_J, HEAD = LAT_HEAD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *Z = reinterpret_cast<double *>(smem), *part = Z + (size_t)N * D, *rec = part + 2 * NW * J;
    uint32_t *bits = reinterpret_cast<uint32_t *>(rec + 3 * HEAD);
    for (int i = tid; i < N * D; i += BLOCK) Z[i] = z[i];
    if (tid < HEAD) rec[tid] = prep[tid];
    if (tid < W) { bits[tid] = colb[tid]; bits[W + tid] = rowb[tid]; }
    const double b = *bp;
    __syncthreads();
    double zc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) zc[d] = Z[d * N];
    const int64_t total = (int64_t)n_sweeps * N;
    long long nex = 0;
    int n = 0, pb = 0;
    int64_t sweep = 0;
    for (int64_t i = 0; i < total; ++i) {
        const int64_t g = sweep * stride + n;
        const int nn = n + 1 < N ? n + 1 : 0;
        const int64_t gn = nn ? g + 1 : (sweep + 1) * stride;
        const bool more = i + 1 < total;
        // ---- requests for the next step (data only)
        uint32_t pc = 0u, pr = 0u;
        double pd = 0.0;
        if (more) {
            if (tid < W) { pc = colb[(size_t)nn * W + tid]; pr = rowb[(size_t)nn * W + tid]; }
            if (tid < HEAD) pd = prep[gn * LAT_REC + tid];
        }
        const int slot = (int)(i % 3), nslot = (int)((i + 1) % 3);
        const double *rc = rec + slot * HEAD;
        const uint32_t *cb = bits + slot * 2 * W, *rb = cb + W;
        double nu[D], znew[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { nu[d] = rc[1 + d]; znew[d] = zc[d]; }
        const double lu0 = rc[0];
        double thr = 0.0;
        int accepted = 0;
        // ---- batches of candidates c0 .. c0+J-1; candidate 0 is the current position (θ = 0)
        for (int c0 = 0; c0 <= LAT_MAX_ATT && !accepted; c0 += J) {
            double cs[J], sn[J], acc[J];
#pragma unroll
            for (int s = 0; s < J; ++s) {
                const int c = c0 + s;
                cs[s] = 1.0; sn[s] = 0.0; acc[s] = 0.0;
                if (c >= 1 && c <= LAT_MAX_ATT) {
                    const double *src = c0 == 0 ? rc : prep + g * LAT_REC;          // later batches: straight from global memory
                    cs[s] = src[9 + 2 * (c - 1)]; sn[s] = src[10 + 2 * (c - 1)];
                }
            }
            for (int j = tid; j < N; j += BLOCK) {
                if (j == n) continue;
                const double sb = (double)(int)(((cb[j >> 5] >> (j & 31)) & 1u) + ((rb[j >> 5] >> (j & 31)) & 1u));
                double zj[D];
#pragma unroll
                for (int d = 0; d < D; ++d) zj[d] = Z[d * N + j];
#pragma unroll
                for (int s = 0; s < J; ++s) {
                    double d2 = 0.0;
#pragma unroll
                    for (int d = 0; d < D; ++d) { const double x = fma(sn[s], nu[d], cs[s] * zc[d]) - zj[d]; d2 = fma(x, x, d2); }
                    const double eta = b - d2;
                    acc[s] += sb * eta - 2.0 * lat_softplus(eta);
                }
            }
#pragma unroll
            for (int s = 0; s < J; ++s) acc[s] = lat_wave_sum(acc[s]);
            double *pw = part + (pb & 1) * NW * J;
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < J; ++s) pw[wave * J + s] = acc[s];
            }
            if (c0 == 0 && more) {
                if (tid < W) { bits[nslot * 2 * W + tid] = pc; bits[nslot * 2 * W + W + tid] = pr; }
                if (tid < HEAD) rec[nslot * HEAD + tid] = pd;
            }
            __syncthreads();
            // ---- every wave sums the waves' parts in wave order: lane s holds L of candidate c0 + s
            double v = 0.0;
            if (lane < J)
                for (int w = 0; w < NW; ++w) v += pw[w * J + lane];
            ++pb;
            double L[J];
#pragma unroll
            for (int s = 0; s < J; ++s) L[s] = lat_lane(v, s);
            if (c0 == 0) thr = L[0] + lu0;
#pragma unroll
            for (int s = 0; s < J; ++s) {
                const int c = c0 + s;
                if (!accepted && c >= 1 && c <= LAT_MAX_ATT && L[s] >= thr) {
                    accepted = c;
#pragma unroll
                    for (int d = 0; d < D; ++d) znew[d] = fma(sn[s], nu[d], cs[s] * zc[d]);
                }
            }
            if (tid == 0 && trace) {
                if (c0 == 0) trace[g * 101] = thr;
#pragma unroll
                for (int s = 0; s < J; ++s)
                    if (c0 + s >= 1 && c0 + s <= LAT_MAX_ATT) trace[g * 101 + c0 + s] = L[s];
            }
        }
        if (!accepted) ++nex;                                  // 100 attempts used up: the node keeps its position
        if (tid == n % BLOCK) {                                // the thread that reads Z[.][n] in the other nodes' steps
#pragma unroll
            for (int d = 0; d < D; ++d) Z[d * N + n] = znew[d];
        }
        if (tid == 0 && attempts) attempts[g] = accepted ? accepted : LAT_MAX_ATT + 1;
        // (Z[.][nn] was last written before this step's barrier; its next write follows the next step's)
#pragma unroll
        for (int d = 0; d < D; ++d) zc[d] = N == 1 ? znew[d] : Z[d * N + nn];
        n = nn;
        if (!nn) ++sweep;
    }
    __syncthreads();
    for (int i = tid; i < N * D; i += BLOCK) z[i] = Z[i];
    if (tid == 0 && nex) atomicAdd(reinterpret_cast<unsigned long long *>(exhausted), (unsigned long long)nex);
}

__global__ __launch_bounds__(256) void k_lat_d2(int N, int D, const double *__restrict__ z, double *__restrict__ d2)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * N) return;
    d2[i] = lat_dist2(z, N, D, (int)(i % N), (int)(i / N));
}

__global__ __launch_bounds__(256) void k_lat_fill(int N, int D, const double *__restrict__ z, const double *__restrict__ bp, double *__restrict__ P)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * N) return;
    P[i] = 1.0 / (1.0 + exp(lat_dist2(z, N, D, (int)(i % N), (int)(i / N)) - *bp));
}

__global__ __launch_bounds__(256) void k_lat_moments(int N, int D, const double *__restrict__ z, const double *__restrict__ bp,
                                                     double *__restrict__ sum, double *__restrict__ psum)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * N) return;
    const double b = *bp;
    if (i == 0) { sum[0] += b; sum[1] += b * b; }
    psum[i] += 1.0 / (1.0 + exp(lat_dist2(z, N, D, (int)(i % N), (int)(i / N)) - b));
}

// candidate c of the offset step: μb + (b - μb) cos θ_c + ν sin θ_c; the current offset for c = 0 and without a record
__device__ __forceinline__ double lat_off_candidate(const double *__restrict__ rec, int c, double b, double mu_b)
{
    if (!rec || c < 1 || c > LAT_MAX_ATT) return b;
    return mu_b + fma(rec[10 + 2 * (c - 1)], rec[1], rec[9 + 2 * (c - 1)] * (b - mu_b));
}

// Σ_{p,c} A η - softplus(η) at the candidates c0 .. c0+JB-1 over this workgroup's pairs -> partial[blockIdx.x][JB]
__global__ __launch_bounds__(256) void k_lat_off_pass(int N, int W, const double *__restrict__ d2, const uint32_t *__restrict__ colb,
                                                      const double *__restrict__ bp, double mu_b, const double *__restrict__ rec, int c0,
                                                      const lat_off *__restrict__ st, double *__restrict__ partial)
{
    constexpr int JB = LAT_JB;
    __shared__ double red[4][JB];
    if (c0 > 0 && st->done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double b = *bp;
    double bc[JB], acc[JB];
#pragma unroll
    for (int s = 0; s < JB; ++s) { bc[s] = lat_off_candidate(rec, c0 + s, b, mu_b); acc[s] = 0.0; }
    const size_t NN = (size_t)N * N;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < NN; i += (size_t)gridDim.x * 256) {
        const int p = (int)(i % N), c = (int)(i / N);
        const bool a = (colb[(size_t)c * W + (p >> 5)] >> (p & 31)) & 1u;
        const double dd = d2[i];
#pragma unroll
        for (int s = 0; s < JB; ++s) {
            const double eta = bc[s] - dd;
            acc[s] += (a ? eta : 0.0) - lat_softplus(eta);
        }
    }
#pragma unroll
    for (int s = 0; s < JB; ++s) acc[s] = lat_wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < JB; ++s) red[wave][s] = acc[s];
    }
    __syncthreads();
    if (tid < JB) partial[(size_t)blockIdx.x * JB + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// The workgroups' partials in workgroup order, then the acceptance rule; `last`: the batch that ends the 100 attempts
__global__ __launch_bounds__(64) void k_lat_off_finish(int nblk, const double *__restrict__ partial, double *__restrict__ bp, double mu_b,
                                                       const double *__restrict__ rec, int c0, int last, lat_off *__restrict__ st,
                                                       int32_t *__restrict__ attempts, double *__restrict__ trace,
                                                       long long *__restrict__ exhausted, double *__restrict__ ll_out)
{
    constexpr int JB = LAT_JB;
    __shared__ double L[JB];
    if (c0 > 0 && st->done) return;
    const int tid = threadIdx.x;
    if (tid < JB) {
        double v = 0.0;
        for (int k = 0; k < nblk; ++k) v += partial[(size_t)k * JB + tid];
        L[tid] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    if (ll_out) { *ll_out = L[0]; return; }
    const double b = *bp;
    const double thr = c0 == 0 ? L[0] + rec[0] : st->thr;
    int accepted = 0;
    for (int s = 0; s < JB; ++s) {
        const int c = c0 + s;
        if (c < 1 || c > LAT_MAX_ATT) continue;
        if (trace) trace[c] = L[s];
        if (!accepted && L[s] >= thr) accepted = c;
    }
    if (c0 == 0) { st->thr = thr; if (trace) trace[0] = thr; }
    if (accepted) *bp = lat_off_candidate(rec, accepted, b, mu_b);
    else if (last) *exhausted += 1;                            // the offset keeps its value
    st->done = accepted || last;
    if (attempts && (accepted || last)) *attempts = accepted ? accepted : LAT_MAX_ATT + 1;
}

// workgroup n: L_n = Σ_{j≠n} s_nj η_j - 2 softplus(η_j) at the current state
__global__ __launch_bounds__(256) void k_lat_cond(int N, int W, int D, const double *__restrict__ z, const double *__restrict__ bp,
                                                  const uint32_t *__restrict__ colb, const uint32_t *__restrict__ rowb, double *__restrict__ out)
{
    __shared__ double red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const double b = *bp;
    double acc = 0.0;
    for (int j = tid; j < N; j += 256) {
        if (j == n) continue;
        const size_t w = (size_t)n * W + (j >> 5);
        const double sb = (double)(int)(((colb[w] >> (j & 31)) & 1u) + ((rowb[w] >> (j & 31)) & 1u));
        const double eta = b - lat_dist2(z, N, D, n, j);
        acc += sb * eta - 2.0 * lat_softplus(eta);
    }
    acc = lat_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) out[n] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- host side ----------------------------------------------------------------------------------------------------
static size_t lat_sweep_lds(int N, int D)
{
    const size_t W = ((size_t)N + 31) / 32;
    return 8 * (size_t)N * D + 8 * (2 * (LAT_BLOCK / 64) * LAT_J + 3 * LAT_HEAD) + 24 * W;
}

static nhp_status lat_check_shape(nhp_ctx *ctx, const char *what, int N, int D)
{
    if (N < 1) { nhp_set_error(ctx, "%s: n_nodes = %d must be positive", what, N); return NHP_EINVAL; }
    if (D < 1) { nhp_set_error(ctx, "%s: n_dims = %d must lie in 1..%d", what, D, LAT_MAX_D); return NHP_EINVAL; }
    if (D > LAT_MAX_D) { nhp_set_error(ctx, "%s: n_dims = %d must lie in 1..%d (the position sweep is built for these)", what, D, LAT_MAX_D); return NHP_ENOTIMPL; }
    if ((N + 31) / 32 > LAT_MAX_WORDS || lat_sweep_lds(N, D) > LAT_LDS_BUDGET) {
        nhp_set_error(ctx, "%s: n_nodes = %d with n_dims = %d exceeds the position sweep's LDS "
                           "(8·N·D + 24·ceil(N/32) + %d bytes <= 160 KiB and N <= %d)", what, N, D,
                      8 * (2 * (LAT_BLOCK / 64) * LAT_J + 3 * LAT_HEAD), 32 * LAT_MAX_WORDS);
        return NHP_ENOTIMPL;
    }
    return NHP_OK;
}

static nhp_status lat_check_state(nhp_ctx *ctx, const char *what, const double *z, int N, int D, double b)
{
    for (size_t i = 0; i < (size_t)N * D; ++i)
        if (!std::isfinite(z[i])) { nhp_set_error(ctx, "%s: position z[%zu,%zu] is not finite", what, i % N, i / N); return NHP_EDOMAIN; }
    if (!std::isfinite(b)) { nhp_set_error(ctx, "%s: the offset b is not finite", what); return NHP_EDOMAIN; }
    return NHP_OK;
}

static nhp_status lat_check_priors(nhp_ctx *ctx, const char *what, double sigma, double mu_b, double sigma_b)
{
    if (!(sigma > 0.0 && sigma_b > 0.0 && std::isfinite(sigma) && std::isfinite(sigma_b) && std::isfinite(mu_b))) {
        nhp_set_error(ctx, "%s: the priors need sigma, sigma_b > 0 and a finite mu_b (got %g, %g, %g)", what, sigma, sigma_b, mu_b);
        return NHP_EDOMAIN;
    }
    return NHP_OK;
}

static size_t lat_align(size_t b) { return (b + 255) & ~(size_t)255; }
static unsigned lat_blocks(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }
static int lat_off_blocks(int N) { return (int)std::min<size_t>(LAT_OFF_BLOCKS, ((size_t)N * N + 1023) / 1024); }

struct lat_buffers {
    double *z, *b, *d2, *raw, *prep, *partial;
    const uint32_t *colb, *rowb;
    lat_off *off;
    long long *exh;
    int32_t *att;              // nullable
    double *trace;             // nullable
};

template <int D>
static nhp_status lat_launch_sweep(nhp_ctx *ctx, int N, int n_sweeps, const lat_buffers &q, int64_t rec0)
{
    const size_t lds = lat_sweep_lds(N, D);
    const int W = (N + 31) / 32;
    if (lds > 64 * 1024) NHP_HIP(ctx, hipFuncSetAttribute((const void *)k_lat_sweep<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_lat_sweep<D>, dim3(1), dim3(LAT_BLOCK), lds, ctx->main(), N, W, n_sweeps, N + 1, q.z, q.b, q.colb, q.rowb,
                       q.prep + rec0 * LAT_REC, q.att ? q.att + rec0 : nullptr, q.trace ? q.trace + rec0 * 101 : nullptr, q.exh);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

static nhp_status lat_enqueue_sweep(nhp_ctx *ctx, int N, int D, int n_sweeps, const lat_buffers &q, int64_t rec0)
{
    switch (D) {
    case 1: return lat_launch_sweep<1>(ctx, N, n_sweeps, q, rec0);
    case 2: return lat_launch_sweep<2>(ctx, N, n_sweeps, q, rec0);
    case 3: return lat_launch_sweep<3>(ctx, N, n_sweeps, q, rec0);
    case 4: return lat_launch_sweep<4>(ctx, N, n_sweeps, q, rec0);
    case 5: return lat_launch_sweep<5>(ctx, N, n_sweeps, q, rec0);
    case 6: return lat_launch_sweep<6>(ctx, N, n_sweeps, q, rec0);
    case 7: return lat_launch_sweep<7>(ctx, N, n_sweeps, q, rec0);
    default: return lat_launch_sweep<8>(ctx, N, n_sweeps, q, rec0);
    }
}

// The full log-likelihood at the offsets of one batch: ‖z_p - z_c‖² must be in q.d2
static void lat_launch_pass(nhp_ctx *ctx, int N, const lat_buffers &q, double mu_b, const double *rec, int c0)
{
    hipLaunchKernelGGL(k_lat_off_pass, dim3((unsigned)lat_off_blocks(N)), dim3(256), 0, ctx->main(), N, (N + 31) / 32, q.d2, q.colb, q.b, mu_b,
                       rec, c0, q.off, q.partial);
}

// ESS of the offset with record `r`: the distances once, then the batches; a batch after the accepted one returns at once
static nhp_status lat_enqueue_offset(nhp_ctx *ctx, int N, int D, const lat_buffers &q, double mu_b, int64_t r)
{
    hipStream_t st = ctx->main();
    hipLaunchKernelGGL(k_lat_d2, dim3(lat_blocks((size_t)N * N, 256)), dim3(256), 0, st, N, D, q.z, q.d2);
    NHP_HIP(ctx, hipGetLastError());
    const double *rec = q.prep + r * LAT_REC;
    for (int c0 = 0; c0 <= LAT_MAX_ATT; c0 += LAT_JB) {
        lat_launch_pass(ctx, N, q, mu_b, rec, c0);
        hipLaunchKernelGGL(k_lat_off_finish, dim3(1), dim3(64), 0, st, lat_off_blocks(N), q.partial, q.b, mu_b, rec, c0,
                           c0 + LAT_JB > LAT_MAX_ATT ? 1 : 0, q.off, q.att ? q.att + r : nullptr, q.trace ? q.trace + r * 101 : nullptr, q.exh,
                           (double *)nullptr);
        NHP_HIP(ctx, hipGetLastError());
    }
    return NHP_OK;
}

// `nsw` sweeps of Np node steps (N or 0) and one offset step each, from the draws in q.raw (all asynchronous)
static nhp_status lat_enqueue_resample(nhp_ctx *ctx, int N, int D, int Np, int64_t nsw, bool do_offset, const lat_buffers &q, double sigma,
                                       double mu_b, double sigma_b)
{
    const int64_t records = nsw * (Np + 1);
    hipLaunchKernelGGL(k_lat_prepare, dim3(lat_blocks((size_t)records, 64)), dim3(64), 0, ctx->main(), q.raw, q.prep, Np, D, sigma, sigma_b, records);
    NHP_HIP(ctx, hipGetLastError());
    if (Np && !do_offset) return lat_enqueue_sweep(ctx, N, D, (int)nsw, q, 0);
    for (int64_t s = 0; s < nsw; ++s) {
        if (Np) NHP_TRY(lat_enqueue_sweep(ctx, N, D, 1, q, s * (Np + 1)));
        if (do_offset) NHP_TRY(lat_enqueue_offset(ctx, N, D, q, mu_b, s * (Np + 1) + Np));
    }
    return NHP_OK;
}

static nhp_status lat_enqueue_draws(nhp_ctx *ctx, double *d_raw, int N, int Np, int D, uint64_t seed, uint64_t step, int64_t sweep0, int64_t nsw)
{
    const int64_t count = nsw * ((int64_t)Np * (D + 101) + 102);
    hipLaunchKernelGGL(k_lat_draws, dim3(lat_blocks((size_t)count, 256)), dim3(256), 0, ctx->main(), d_raw, N, Np, D, seed, step, sweep0, count);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// ---- stand-alone entries on a host A ------------------------------------------------------------------------------------
extern "C" nhp_status nhp_latent_loglik(nhp_ctx *ctx, const double *A, int32_t N, int32_t D, const double *z, double b, double *out)
{
    if (!ctx || !A || !z || !out) return NHP_EINVAL;
    NHP_TRY(lat_check_shape(ctx, "latent_loglik", N, D));
    NHP_TRY(lat_check_state(ctx, "latent_loglik", z, N, D, b));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t NN = (size_t)N * N, W = ((size_t)N + 31) / 32;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t r = off; off += lat_align(bytes); return r; };
    const size_t o_A = carve(8 * NN), o_bits = carve(8 * (size_t)N * W), o_z = carve(8 * (size_t)N * D), o_b = carve(8), o_d2 = carve(8 * NN);
    const size_t o_part = carve(8 * LAT_OFF_BLOCKS * LAT_JB), o_off = carve(sizeof(lat_off)), o_out = carve(8 * ((size_t)N + 1));
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, off));
    char *base = (char *)ctx->d_scratch;
    hipStream_t st = ctx->main();
    lat_buffers q = {};
    uint32_t *bits = (uint32_t *)(base + o_bits);
    q.z = (double *)(base + o_z); q.b = (double *)(base + o_b); q.d2 = (double *)(base + o_d2); q.partial = (double *)(base + o_part);
    q.colb = bits; q.rowb = bits + (size_t)N * W; q.off = (lat_off *)(base + o_off);
    double *d_out = (double *)(base + o_out);
    NHP_HIP(ctx, hipMemcpyAsync(base + o_A, A, 8 * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(q.z, z, 8 * (size_t)N * D, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(q.b, &b, 8, hipMemcpyHostToDevice, st));
    NHP_TRY(nhp_sbm_enqueue_pack(ctx, (const double *)(base + o_A), N, bits, bits + (size_t)N * W));
    hipLaunchKernelGGL(k_lat_d2, dim3(lat_blocks(NN, 256)), dim3(256), 0, st, N, D, q.z, q.d2);
    NHP_HIP(ctx, hipGetLastError());
    lat_launch_pass(ctx, N, q, 0.0, nullptr, 0);
    hipLaunchKernelGGL(k_lat_off_finish, dim3(1), dim3(64), 0, st, lat_off_blocks(N), q.partial, q.b, 0.0, (const double *)nullptr, 0, 0, q.off,
                       (int32_t *)nullptr, (double *)nullptr, (long long *)nullptr, d_out);
    hipLaunchKernelGGL(k_lat_cond, dim3((unsigned)N), dim3(256), 0, st, N, (int)W, D, q.z, q.b, q.colb, q.rowb, d_out + 1);
    NHP_HIP(ctx, hipGetLastError());
    return nhp_download(ctx, out, d_out, 8 * ((size_t)N + 1));          // (waits for the stream: `b` is a stack value)
}

extern "C" nhp_status nhp_latent_resample(nhp_ctx *ctx, const double *A, int32_t N, int32_t D, double *z, double *b, double sigma, double mu_b,
                                          double sigma_b, const double *draws, uint64_t seed, uint64_t step, int32_t n_sweeps,
                                          int32_t do_offset, double *draws_used, int32_t *attempts, double *ll_trace, int64_t *exhausted)
{
    if (!ctx || !A || !z || !b) return NHP_EINVAL;
    NHP_TRY(lat_check_shape(ctx, "latent_resample", N, D));
    if (n_sweeps < 0 || (n_sweeps == 0 && !do_offset)) {
        nhp_set_error(ctx, "latent_resample: n_sweeps = %d must be positive (0: the offset update alone)", n_sweeps);
        return NHP_EINVAL;
    }
    NHP_TRY(lat_check_state(ctx, "latent_resample", z, N, D, *b));
    NHP_TRY(lat_check_priors(ctx, "latent_resample", sigma, mu_b, sigma_b));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const int Np = n_sweeps ? N : 0;
    const int64_t nsw = n_sweeps ? n_sweeps : 1, RS = (int64_t)Np * (D + 101) + 102;
    const int64_t chunk = std::min<int64_t>(nsw, std::max<int64_t>(1, LAT_CHUNK_STEPS / (Np + 1))), crec = chunk * (Np + 1);
    const size_t NN = (size_t)N * N, W = ((size_t)N + 31) / 32;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t r = off; off += lat_align(bytes); return r; };
    const size_t o_A = carve(8 * NN), o_bits = carve(8 * (size_t)N * W), o_z = carve(8 * (size_t)N * D), o_b = carve(8), o_d2 = carve(8 * NN);
    const size_t o_part = carve(8 * LAT_OFF_BLOCKS * LAT_JB), o_off = carve(sizeof(lat_off)), o_exh = carve(8);
    const size_t o_raw = carve(8 * (size_t)(chunk * RS)), o_prep = carve(8 * (size_t)crec * LAT_REC), o_att = carve(4 * (size_t)crec);
    const size_t o_tr = carve(ll_trace ? 8 * (size_t)crec * 101 : 8);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, off));
    char *base = (char *)ctx->d_scratch;
    hipStream_t st = ctx->main();
    lat_buffers q = {};
    uint32_t *bits = (uint32_t *)(base + o_bits);
    q.z = (double *)(base + o_z); q.b = (double *)(base + o_b); q.d2 = (double *)(base + o_d2); q.partial = (double *)(base + o_part);
    q.raw = (double *)(base + o_raw); q.prep = (double *)(base + o_prep);
    q.colb = bits; q.rowb = bits + (size_t)N * W; q.off = (lat_off *)(base + o_off); q.exh = (long long *)(base + o_exh);
    q.att = (int32_t *)(base + o_att); q.trace = ll_trace ? (double *)(base + o_tr) : nullptr;
    NHP_HIP(ctx, hipMemcpyAsync(base + o_A, A, 8 * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(q.z, z, 8 * (size_t)N * D, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(q.b, b, 8, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemsetAsync(q.exh, 0, 8, st));
    NHP_TRY(nhp_sbm_enqueue_pack(ctx, (const double *)(base + o_A), N, bits, bits + (size_t)N * W));
    for (int64_t s0 = 0; s0 < nsw; s0 += chunk) {
        const int64_t ns = std::min(chunk, nsw - s0), nrec = ns * (Np + 1);
        if (draws) NHP_HIP(ctx, hipMemcpyAsync(q.raw, draws + s0 * RS, 8 * (size_t)(ns * RS), hipMemcpyHostToDevice, st));
        else NHP_TRY(lat_enqueue_draws(ctx, q.raw, N, Np, D, seed, step, s0, ns));
        NHP_HIP(ctx, hipMemsetAsync(q.att, 0, 4 * (size_t)nrec, st));          // (the slots of steps that do not run stay 0)
        NHP_TRY(lat_enqueue_resample(ctx, N, D, Np, ns, do_offset != 0, q, sigma, mu_b, sigma_b));
        if (draws_used) NHP_TRY(nhp_download(ctx, draws_used + s0 * RS, q.raw, 8 * (size_t)(ns * RS)));
        if (attempts) NHP_TRY(nhp_download(ctx, attempts + s0 * (Np + 1), q.att, 4 * (size_t)nrec));
        if (ll_trace) NHP_TRY(nhp_download(ctx, ll_trace + s0 * (Np + 1) * 101, q.trace, 8 * (size_t)nrec * 101));
    }
    NHP_TRY(nhp_download(ctx, z, q.z, 8 * (size_t)N * D));
    NHP_TRY(nhp_download(ctx, b, q.b, 8));
    long long ex = 0;
    NHP_TRY(nhp_download(ctx, &ex, q.exh, 8));
    if (exhausted) *exhausted = ex;
    return NHP_OK;
}

// ---- device-resident state, kept next to the continuous model -----------------------------------------------------------
void nhp_latent_free(nhp_cont_model *m)
{
    nhp_latent_state *s = m->latent;
    if (!s) return;
    (void)hipFree(s->d_z); (void)hipFree(s->d_b); (void)hipFree(s->d_P); (void)hipFree(s->d_sum); (void)hipFree(s->d_psum);
    (void)hipFree(s->d_raw); (void)hipFree(s->d_prep); (void)hipFree(s->d_partial); (void)hipFree(s->d_bits); (void)hipFree(s->d_off);
    (void)hipFree(s->d_exh);
    delete s;
    m->latent = nullptr;
}

// A model whose network is no latent distance model (any more): nhp_cont_model_set_rho and _set_sbm call this
nhp_status nhp_latent_detach(nhp_ctx *ctx, nhp_cont_model *m)
{
    if (!m->latent) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    nhp_latent_free(m);
    return NHP_OK;
}

static nhp_status lat_model_check(nhp_ctx *ctx, const nhp_cont_model *m, const char *what, bool need_state)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    if (need_state && !m->latent) {
        nhp_set_error(ctx, "%s: the model has no latent distance network (nhp_cont_model_set_latent)", what);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

nhp_status nhp_latent_moments_reset(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_latent_state *s = m->latent;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_HIP(ctx, hipMemsetAsync(s->d_sum, 0, 16, ctx->main()));
    NHP_HIP(ctx, hipMemsetAsync(s->d_psum, 0, 8 * (size_t)m->N * m->N, ctx->main()));
    return NHP_OK;
}

nhp_status nhp_latent_moments_accumulate(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_latent_state *s = m->latent;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_lat_moments, dim3(lat_blocks((size_t)m->N * m->N, 256)), dim3(256), 0, ctx->main(), m->N, s->D, s->d_z, s->d_b, s->d_sum,
                       s->d_psum);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_set_latent(nhp_ctx *ctx, nhp_cont_model *m, int32_t D, const double *z, double b, double sigma, double mu_b,
                                                double sigma_b)
{
    NHP_TRY(lat_model_check(ctx, m, "set_latent", false));
    if (!z) return NHP_EINVAL;
    if (!m->has_A) { nhp_set_error(ctx, "set_latent: the model has no adjacency matrix"); return NHP_EINVAL; }
    const int N = m->N;
    NHP_TRY(lat_check_shape(ctx, "set_latent", N, D));
    NHP_TRY(lat_check_state(ctx, "set_latent", z, N, D, b));
    NHP_TRY(lat_check_priors(ctx, "set_latent", sigma, mu_b, sigma_b));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_sbm_detach(ctx, m));                          // one structured network at a time
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    if (m->latent && m->latent->D != D) nhp_latent_free(m);
    const size_t NN = (size_t)N * N, W = ((size_t)N + 31) / 32;
    if (!m->latent) {
        nhp_latent_state *s = new nhp_latent_state;
        s->D = D;
        m->latent = s;
        if (hipMalloc((void **)&s->d_z, 8 * (size_t)N * D) != hipSuccess || hipMalloc((void **)&s->d_b, 8) != hipSuccess ||
            hipMalloc((void **)&s->d_P, 8 * NN) != hipSuccess || hipMalloc((void **)&s->d_sum, 16) != hipSuccess ||
            hipMalloc((void **)&s->d_psum, 8 * NN) != hipSuccess || hipMalloc((void **)&s->d_raw, 8 * ((size_t)N * (D + 101) + 102)) != hipSuccess ||
            hipMalloc((void **)&s->d_prep, 8 * ((size_t)N + 1) * LAT_REC) != hipSuccess ||
            hipMalloc((void **)&s->d_partial, 8 * LAT_OFF_BLOCKS * LAT_JB) != hipSuccess || hipMalloc((void **)&s->d_bits, 8 * (size_t)N * W) != hipSuccess ||
            hipMalloc((void **)&s->d_off, sizeof(lat_off)) != hipSuccess || hipMalloc((void **)&s->d_exh, 8) != hipSuccess) {
            (void)hipGetLastError();
            nhp_latent_free(m);
            nhp_set_error(ctx, "out of device memory (latent distance network state)");
            return NHP_ENOMEM;
        }
        NHP_TRY(nhp_latent_moments_reset(ctx, m));
    }
    nhp_latent_state *s = m->latent;
    s->sigma = sigma; s->mu_b = mu_b; s->sigma_b = sigma_b;
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(s->d_z, z, 8 * (size_t)N * D, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(s->d_b, &b, 8, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemsetAsync(s->d_exh, 0, 8, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));                   // `b` is a stack value
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_set_latent_positions_every(nhp_ctx *ctx, nhp_cont_model *m, int32_t every)
{
    NHP_TRY(lat_model_check(ctx, m, "set_latent_positions_every", true));
    if (every < 1) { nhp_set_error(ctx, "set_latent_positions_every: every = %d must be positive", every); return NHP_EINVAL; }
    m->latent->positions_every = every;
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_get_latent(nhp_ctx *ctx, const nhp_cont_model *m, double *z, double *b, double *sums, double *p_sum,
                                                int64_t *exhausted)
{
    NHP_TRY(lat_model_check(ctx, m, "get_latent", true));
    const nhp_latent_state *s = m->latent;
    const size_t N = (size_t)m->N;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    if (z) NHP_TRY(nhp_download(ctx, z, s->d_z, 8 * N * s->D));
    if (b) NHP_TRY(nhp_download(ctx, b, s->d_b, 8));
    if (sums) NHP_TRY(nhp_download(ctx, sums, s->d_sum, 16));
    if (p_sum) NHP_TRY(nhp_download(ctx, p_sum, s->d_psum, 8 * N * N));
    if (exhausted) {
        long long ex = 0;
        NHP_TRY(nhp_download(ctx, &ex, s->d_exh, 8));
        *exhausted = ex;
    }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_latent_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, uint64_t seed, uint64_t step)
{
    NHP_TRY(lat_model_check(ctx, m, "latent_step", true));
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "latent_step: not available on a column shard (the positions need every column of A)");
        return NHP_ENOTIMPL;
    }
    nhp_latent_state *s = m->latent;
    const int N = m->N, D = s->D, W = (N + 31) / 32;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->main();
    // link probabilities from the current (z, b), the adjacency sweep, then resample!(network, A)
    hipLaunchKernelGGL(k_lat_fill, dim3(lat_blocks((size_t)N * N, 256)), dim3(256), 0, st, N, D, s->d_z, s->d_b, s->d_P);
    NHP_HIP(ctx, hipGetLastError());
    double *d_links = nullptr;
    NHP_TRY(nhp_adj_enqueue(ctx, ds, m, nullptr, 0.5, nullptr, nullptr, seed, step, &d_links, s->d_P));
    NHP_TRY(nhp_sbm_enqueue_pack(ctx, m->d_A, N, s->d_bits, s->d_bits + (size_t)N * W));
    lat_buffers q = {};
    q.z = s->d_z; q.b = s->d_b; q.d2 = s->d_P; q.raw = s->d_raw; q.prep = s->d_prep; q.partial = s->d_partial;
    q.colb = s->d_bits; q.rowb = s->d_bits + (size_t)N * W; q.off = s->d_off; q.exh = s->d_exh;
    const int Np = step % (uint64_t)s->positions_every == 0 ? N : 0;
    NHP_TRY(lat_enqueue_draws(ctx, q.raw, N, Np, D, seed, step, 0, 1));
    return lat_enqueue_resample(ctx, N, D, Np, 1, true, q, s->sigma, s->mu_b, s->sigma_b);
}
