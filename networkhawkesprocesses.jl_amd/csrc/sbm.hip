// StochasticBlockNetworkModel: resample!(network, A) on the device (the reference leaves the model an empty stub at the
// end of src/networks.jl).
//
//   z_n ~ Categorical(π), π ~ Dirichlet(γ·1_K), ρ[k,l] ~ Beta(α, β), A[p,c] ~ Bernoulli(ρ[z_p, z_c]) (diagonal included)
//
// One resample is (1) block counts L[k,l] = Σ A[p,c]·[z_p = k][z_c = l] and sizes n_k, (2) ρ[k,l] ~ Beta(α + L, β + n_k n_l - L),
// (3) π ~ Dirichlet(γ + n), (4) one collapsed-Gibbs sweep over the labels, node after node, each conditional on the
// current labels of all others.
//
// The adjacency matrix is first packed into bits, once by column and once by row (k_sbm_pack: N²/4 bytes for both, 256 KiB
// at N = 1024 against the 8 MiB of doubles), so everything below reads words that stay in L2.  k_sbm_tables -- one
// workgroup per node -- counts a node's links into and out of every block (diagonal excluded) and, from the same pass,
// the block counts: integer atomics only, so the sums are exact whatever their order.
//
// The label sweep is a chain of N dependent steps and runs in ONE workgroup (k_sbm_sweep).  The per-node tables
// out[n][l] = #{c != n: A[n,c], z_c = l} and in[n][l] = #{p != n: A[p,n], z_p = l}, log ρ and log(1 - ρ) stay in LDS for
// the whole sweep.  A step costs O(K²) for the K scores (lane k owns block k), a few wave reductions for the softmax and
// the inverse-cdf draw, and -- only when the node changes block -- O(N) table updates spread over the workgroup's
// threads.  What a step needs from global memory is data only (the bits of the node's column and row, its uniform): it
// is requested one step ahead and lands in LDS under the current step's arithmetic, so no global round trip sits on the
// chain.  Every wave computes the scores and the decision itself (same operations on the same LDS words, hence the same
// bits), which leaves one workgroup barrier per step.
#include <algorithm>
#include <vector>
#include <math.h>
#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_rng.h"

#define SBM_MAX_K 64
#define SBM_BLOCK 256                     // threads of the label sweep's workgroup (four waves: DESIGN 3.18)
#define SBM_MAX_WORDS SBM_BLOCK           // bit words per column: N <= 8192 (k_sbm_sweep keeps one of them per thread in flight)
#define SBM_LDS_BUDGET (160 * 1024)

struct nhp_sbm_state {
    int32_t K = 0;
    double alpha = 1.0, beta = 1.0, gamma = 1.0;
    int32_t labels_every = 1;
    int32_t *d_z = nullptr;             // [N]
    double *d_rho = nullptr;            // [K*K] column-major: ρ[k,l] at k + K·l
    double *d_pi = nullptr;             // [K]
    double *d_P = nullptr;              // [N*N] link probabilities ρ[z_p, z_c] of the latest step
    double *d_sum = nullptr;            // [2K² + 2K] Σρ, Σρ², Σπ, Σπ² over the kept steps
    long long *d_bc = nullptr;          // [N*K] kept steps node n spent in block k (n + N·k)
    uint32_t *d_bits = nullptr;         // [2][N*W] A by column, A by row
    int32_t *d_tab = nullptr;           // [2][N*K] out, in
    long long *d_cnt = nullptr;         // [K*K + K] L, n
    double *d_u = nullptr;              // [N]
};

// ---- kernels ------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: colb[n*W + w] bit j = A[32w + j, n];  1: rowb[n*W + w] bit j = A[n, 32w + j]
__global__ __launch_bounds__(256) void k_sbm_pack(const double *__restrict__ A, int N, int W, uint32_t *__restrict__ colb,
                                                  uint32_t *__restrict__ rowb)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)N * W) return;
    uint32_t bits = 0;
    if (blockIdx.y == 0) {
        const int n = (int)(t / W), w = (int)(t % W);
        for (int j = 0; j < 32; ++j) {
            const int m = 32 * w + j;
            if (m < N && A[(size_t)m + (size_t)n * N] != 0.0) bits |= 1u << j;
        }
        colb[(size_t)n * W + w] = bits;
    } else {
        const int w = (int)(t / N), n = (int)(t % N);          // consecutive threads: consecutive rows of one column
        for (int j = 0; j < 32; ++j) {
            const int m = 32 * w + j;
            if (m < N && A[(size_t)n + (size_t)m * N] != 0.0) bits |= 1u << j;
        }
        rowb[(size_t)n * W + w] = bits;
    }
}

// workgroup m: out[m][l], in[m][l] over the other nodes; L and sizes (nullable) get node m's share, diagonal included
__global__ __launch_bounds__(64) void k_sbm_tables(const uint32_t *__restrict__ colb, const uint32_t *__restrict__ rowb,
                                                   const int32_t *__restrict__ z, int N, int W, int K, int32_t *__restrict__ out,
                                                   int32_t *__restrict__ in, long long *__restrict__ L, long long *__restrict__ sizes)
{
    __shared__ int co[SBM_MAX_K], ci[SBM_MAX_K];
    const int m = blockIdx.x, lane = threadIdx.x;
    co[lane] = 0; ci[lane] = 0;
    __syncthreads();
    for (int w = lane; w < W; w += 64) {
        const uint32_t self = (m >> 5) == w ? ~(1u << (m & 31)) : ~0u;
        uint32_t r = rowb[(size_t)m * W + w] & self, c = colb[(size_t)m * W + w] & self;
        while (r) { const int j = __ffs(r) - 1; r &= r - 1; atomicAdd(&co[z[32 * w + j]], 1); }
        while (c) { const int j = __ffs(c) - 1; c &= c - 1; atomicAdd(&ci[z[32 * w + j]], 1); }
    }
    __syncthreads();
    if (lane < K) {
        out[(size_t)m * K + lane] = co[lane];
        in[(size_t)m * K + lane] = ci[lane];
        if (L) {
            const int zm = z[m];
            const int diag = (colb[(size_t)m * W + (m >> 5)] >> (m & 31)) & 1;
            const long long v = co[lane] + (lane == zm ? diag : 0);
            if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&L[zm + K * lane]), (unsigned long long)v);
            if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&sizes[zm]), 1ull);
        }
    }
}

// ρ[k,l] = X/(X+Y), X ~ Gamma(α + L), Y ~ Gamma(β + n_k n_l - L) (elements 2i, 2i+1 of the ρ family, i = k + K·l);
// π = g / Σg, g_k ~ Gamma(γ + n_k) (element k of the π family), Σ in index order.  Keys: nhp_rng.h.
__global__ __launch_bounds__(256) void k_sbm_draw(int K, const long long *__restrict__ L, const long long *__restrict__ sizes, double alpha,
                                                  double beta, double gamma, uint64_t seed, uint64_t step, double *__restrict__ rho,
                                                  double *__restrict__ pi)
{
    __shared__ double g[SBM_MAX_K];
    const int tid = threadIdx.x;
    for (int i = tid; i < K * K; i += 256) {
        const double l = (double)L[i], nn = (double)sizes[i % K] * (double)sizes[i / K];
        const double x = dev_gamma(alpha + l, 1.0, seed ^ NHP_KEY_SBM_RHO, step, (uint64_t)(2 * i));
        const double y = dev_gamma(beta + nn - l, 1.0, seed ^ NHP_KEY_SBM_RHO, step, (uint64_t)(2 * i + 1));
        const double r = x / (x + y);
        rho[i] = fmin(fmax(r, 1e-300), 1.0 - 0x1p-53);            // open interval: the sweep takes log ρ and log(1 - ρ)
    }
    if (tid < K) g[tid] = dev_gamma(gamma + (double)sizes[tid], 1.0, seed ^ NHP_KEY_SBM_PI, step, (uint64_t)tid);
    __syncthreads();
    if (tid < K) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += g[k];
        pi[tid] = g[tid] / s;
    }
}

__global__ __launch_bounds__(256) void k_sbm_fill(int N, int K, const int32_t *__restrict__ z, const double *__restrict__ rho,
                                                  double *__restrict__ P)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * N) return;
    P[i] = rho[z[i % N] + K * z[i / N]];
}

__global__ __launch_bounds__(256) void k_sbm_uniforms(double *__restrict__ dst, uint64_t seed, uint64_t step, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = nhp_philox_uniform(seed ^ NHP_KEY_SBM_LABEL, step, (uint64_t)i);
}

__global__ __launch_bounds__(256) void k_sbm_moments(int N, int K, const int32_t *__restrict__ z, const double *__restrict__ rho,
                                                     const double *__restrict__ pi, double *__restrict__ sum, long long *__restrict__ bc)
{
    const int i = blockIdx.x * 256 + threadIdx.x, KK = K * K;
    if (i < KK) { const double r = rho[i]; sum[i] += r; sum[KK + i] += r * r; }
    if (i < K) { const double p = pi[i]; sum[2 * KK + i] += p; sum[2 * KK + K + i] += p * p; }
    if (i < N) bc[(size_t)i + (size_t)N * z[i]] += 1;
}

// Wave-wide maximum and inclusive prefix sum of one double per lane in the VALU (DPP inside rows of 16 lanes, scalar lane
// reads across the four rows): no LDS round trips on the sweep's chain.  `rows` = rows that hold live lanes (wave-uniform).
__device__ __forceinline__ double sbm_dpp(double v, const int ctrl)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    switch (ctrl) {          // the control word is an immediate
    case 0xB1: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true));
    case 0x4E: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true));
    case 0x141: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true));
    case 0x140: return __hiloint2double(__builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true));
    // row_shr:n -- lanes whose source lies outside the row read 0.0
    case 0x111: return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x111, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xF, 0xF, false));
    case 0x112: return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x112, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xF, 0xF, false));
    case 0x114: return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x114, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xF, 0xF, false));
    default: return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, 0x118, 0xF, 0xF, false), __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xF, 0xF, false));
    }
}
__device__ __forceinline__ double sbm_lane(double v, const int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double sbm_wave_max(double v, const int rows)
{
    v = fmax(v, sbm_dpp(v, 0xB1));          // quad_perm [1,0,3,2]
    v = fmax(v, sbm_dpp(v, 0x4E));          // quad_perm [2,3,0,1]
    v = fmax(v, sbm_dpp(v, 0x141));         // row_half_mirror
    v = fmax(v, sbm_dpp(v, 0x140));         // row_mirror
    double r = sbm_lane(v, 0);
    if (rows > 1) r = fmax(r, sbm_lane(v, 16));
    if (rows > 2) r = fmax(fmax(r, sbm_lane(v, 32)), sbm_lane(v, 48));
    return r;
}
__device__ __forceinline__ double sbm_wave_scan(double v, const int rows, const int lane)
{
    v += sbm_dpp(v, 0x111);
    v += sbm_dpp(v, 0x112);
    v += sbm_dpp(v, 0x114);
    v += sbm_dpp(v, 0x118);
    if (rows > 1) {                                // the totals of the rows below, in row order
        const double t0 = sbm_lane(v, 15), t1 = t0 + sbm_lane(v, 31), t2 = t1 + sbm_lane(v, 47);
        const int row = lane >> 4;
        v += row == 0 ? 0.0 : row == 1 ? t0 : row == 2 ? t1 : t2;
    }
    return v;
}

// The label sweep.  Dynamic LDS: log ρ, log(1 - ρ) [K][K|1] doubles each (odd row stride: lane k reads row k and column
// k without bank conflicts), out, in [K][N] int32, the bits of the current and the next node's column and row
// [2][2][W], the labels [N] bytes.  u [n_sweeps·N]; probs (nullable) [n_sweeps·N·K], the conditional of step i at i·K.
__global__ __launch_bounds__(SBM_BLOCK) void k_sbm_sweep(int N, int W, int K, int n_sweeps, int32_t *__restrict__ z,
                                                     const double *__restrict__ rho, const double *__restrict__ pi,
                                                     const uint32_t *__restrict__ colb, const uint32_t *__restrict__ rowb,
                                                     const int32_t *__restrict__ out_g, const int32_t *__restrict__ in_g,
                                                     const long long *__restrict__ sizes, const double *__restrict__ u,
                                                     double *__restrict__ probs)
{
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int BLOCK = SBM_BLOCK;
    const int KP = K | 1, tid = threadIdx.x, lane = tid & 63;
    double *lr = reinterpret_cast<double *>(smem), *l1r = lr + K * KP;
    int32_t *out = reinterpret_cast<int32_t *>(l1r + K * KP), *in = out + (size_t)N * K;
    uint32_t *bits = reinterpret_cast<uint32_t *>(in + (size_t)N * K);
    uint8_t *zl = reinterpret_cast<uint8_t *>(bits + 4 * W);
    for (int i = tid; i < K * K; i += BLOCK) {
        const double r = rho[i];
        lr[(i % K) * KP + i / K] = log(r);
        l1r[(i % K) * KP + i / K] = log(1.0 - r);
    }
    for (int i = tid; i < N * K; i += BLOCK) {                   // [N][K] in global memory -> [K][N] here: the updates of a step touch consecutive words
        const int m = i / K, l = i % K;
        out[l * N + m] = out_g[i]; in[l * N + m] = in_g[i];
    }
    for (int i = tid; i < N; i += BLOCK) zl[i] = (uint8_t)z[i];
    for (int w = tid; w < W; w += BLOCK) { bits[w] = colb[w]; bits[W + w] = rowb[w]; }
    const int kk = lane < K ? lane : K - 1;                       // lanes past K repeat block K-1 and are masked out
    const int rows = (K + 15) >> 4;
    const double lpi = log(pi[kk]);
    int sz = lane < K ? (int)sizes[lane] : 0;                    // lane k: size of block k (every wave keeps its own copy)
    __syncthreads();
    int a = zl[0];
    const int64_t total = (int64_t)n_sweeps * N;
    double u_cur = u[0];
    int n = 0;
    for (int64_t i = 0; i < total; ++i) {
        // ---- requests for the next step (data only)
        const int nn = n + 1 < N ? n + 1 : 0;
        const uint32_t pc = tid < W ? colb[(size_t)nn * W + tid] : 0u;     // W <= SBM_MAX_WORDS = SBM_BLOCK: one word of each per thread
        const uint32_t pr = tid < W ? rowb[(size_t)nn * W + tid] : 0u;
        const double u_next = i + 1 < total ? u[i + 1] : 0.0;
        const uint32_t *cur = bits + (i & 1) * 2 * W;
        uint32_t *nxt = bits + ((i + 1) & 1) * 2 * W;
        const int a_next = zl[nn];
        // ---- scores of node n: lane k holds s_k
        const int diag = (cur[n >> 5] >> (n & 31)) & 1;
        const double *lrk = lr + kk * KP, *l1rk = l1r + kk * KP;
        double s = lpi + (diag ? lrk[kk] : l1rk[kk]), s2 = 0.0;      // two chains: the links out of n, the links into n
        for (int l0 = 0; l0 < K; l0 += 4) {                           // four blocks at a time: their LDS reads are issued together
            int o[4], q[4];
            double x1[4], x2[4], x3[4], x4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = l0 + j < K ? l0 + j : K - 1;
                o[j] = out[l * N + n]; q[j] = in[l * N + n];
                x1[j] = lrk[l]; x2[j] = l1rk[l]; x3[j] = lr[l * KP + kk]; x4[j] = l1r[l * KP + kk];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (l0 + j < K) {
                    const int c = __builtin_amdgcn_readlane(sz, l0 + j) - (l0 + j == a ? 1 : 0);
                    s += (double)o[j] * x1[j] + (double)(c - o[j]) * x2[j];
                    s2 += (double)q[j] * x3[j] + (double)(c - q[j]) * x4[j];
                }
            }
        }
        s += s2;
        // ---- p = softmax(s); z_n = first k with u <= p_0 + ... + p_k, the last block catches rounding
        const double mx = sbm_wave_max(lane < K ? s : -__builtin_inf(), rows);
        const double e = lane < K ? exp(s - mx) : 0.0;
        const double p = e / sbm_lane(sbm_wave_scan(e, rows, lane), K - 1);
        const double cum = sbm_wave_scan(p, rows, lane);
        const unsigned long long hits = __ballot(lane < K && u_cur <= cum);
        const int b = hits ? __ffsll((long long)hits) - 1 : K - 1;
        if (probs && tid < K) probs[i * K + tid] = p;
        // ---- the node moved: every other node's counts of blocks a and b follow
        if (b != a) {
            for (int m = tid; m < N; m += BLOCK) {                    // (a != b: the four words are distinct; reads first, then writes)
                const int cb = m == n ? 0 : (cur[m >> 5] >> (m & 31)) & 1;          // A[m,n]
                const int rb = m == n ? 0 : (cur[W + (m >> 5)] >> (m & 31)) & 1;    // A[n,m]
                const int oa = out[a * N + m], ob = out[b * N + m], ia = in[a * N + m], ib = in[b * N + m];
                out[a * N + m] = oa - cb; out[b * N + m] = ob + cb;
                in[a * N + m] = ia - rb; in[b * N + m] = ib + rb;
            }
            if (lane == a) --sz;
            if (lane == b) ++sz;
            if (tid == 0) { zl[n] = (uint8_t)b; z[n] = b; }
        }
        if (tid < W) { nxt[tid] = pc; nxt[W + tid] = pr; }
        a = N == 1 ? b : a_next;
        u_cur = u_next;
        n = nn;
        __syncthreads();
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct sbm_work {
    uint32_t *colb, *rowb;
    int32_t *out, *in;
    long long *L, *sizes;
};

static size_t sbm_sweep_lds(int N, int K)
{
    const size_t W = ((size_t)N + 31) / 32;
    return 16 * (size_t)K * (size_t)(K | 1) + 8 * (size_t)N * K + 16 * W + (size_t)N + 16;
}

static nhp_status sbm_check_shape(nhp_ctx *ctx, const char *what, int N, int K)
{
    if (K < 1 || K > SBM_MAX_K) { nhp_set_error(ctx, "%s: n_blocks = %d must lie in 1..%d", what, K, SBM_MAX_K); return NHP_EINVAL; }
    if (N < 1) { nhp_set_error(ctx, "%s: n_nodes = %d must be positive", what, N); return NHP_EINVAL; }
    return NHP_OK;
}

// the label sweep's limits: the tables of every node stay in LDS
static nhp_status sbm_check_sweep(nhp_ctx *ctx, int N, int K)
{
    if ((N + 31) / 32 > SBM_MAX_WORDS || sbm_sweep_lds(N, K) > SBM_LDS_BUDGET) {
        nhp_set_error(ctx, "block labels: n_nodes = %d with n_blocks = %d exceeds the label sweep's LDS tables "
                           "(8·N·K + 16·K·(K|1) + N/2 + N + 16 bytes <= 160 KiB and N <= %d)", N, K, 32 * SBM_MAX_WORDS);
        return NHP_ENOTIMPL;
    }
    return NHP_OK;
}

static nhp_status sbm_check_labels(nhp_ctx *ctx, const char *what, const int32_t *z, int N, int K)
{
    for (int n = 0; n < N; ++n)
        if (z[n] < 0 || z[n] >= K) { nhp_set_error(ctx, "%s: label z[%d] = %d outside 0..%d", what, n, z[n], K - 1); return NHP_EDOMAIN; }
    return NHP_OK;
}

static nhp_status sbm_check_rho_pi(nhp_ctx *ctx, const char *what, const double *rho, const double *pi, int K)
{
    for (int i = 0; i < K * K; ++i)
        if (!(rho[i] > 0.0 && rho[i] < 1.0)) {
            nhp_set_error(ctx, "%s: rho[%d,%d] = %g must lie in the open interval (0, 1)", what, i % K, i / K, rho[i]);
            return NHP_EDOMAIN;
        }
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        if (!(pi[k] > 0.0)) { nhp_set_error(ctx, "%s: pi[%d] = %g must be positive", what, k, pi[k]); return NHP_EDOMAIN; }
        s += pi[k];
    }
    if (!(fabs(s - 1.0) <= 1e-12)) { nhp_set_error(ctx, "%s: pi sums to %.17g, not to 1 within 1e-12", what, s); return NHP_EDOMAIN; }
    return NHP_OK;
}

static nhp_status sbm_check_priors(nhp_ctx *ctx, const char *what, double alpha, double beta, double gamma)
{
    if (!(alpha > 0.0 && beta > 0.0 && gamma > 0.0)) {
        nhp_set_error(ctx, "%s: the priors need alpha, beta, gamma > 0 (got %g, %g, %g)", what, alpha, beta, gamma);
        return NHP_EDOMAIN;
    }
    return NHP_OK;
}

static size_t sbm_align(size_t b) { return (b + 255) & ~(size_t)255; }

// bytes of the work arrays for (N, K), and their places inside `base`
static size_t sbm_work_bytes(int N, int K)
{
    const size_t W = ((size_t)N + 31) / 32;
    return 2 * sbm_align(4 * (size_t)N * W) + 2 * sbm_align(4 * (size_t)N * K) + sbm_align(8 * ((size_t)K * K + K));
}

static sbm_work sbm_carve(char *base, int N, int K)
{
    const size_t W = ((size_t)N + 31) / 32, nb = sbm_align(4 * (size_t)N * W), nt = sbm_align(4 * (size_t)N * K);
    sbm_work w;
    w.colb = (uint32_t *)base; w.rowb = (uint32_t *)(base + nb);
    w.out = (int32_t *)(base + 2 * nb); w.in = (int32_t *)(base + 2 * nb + nt);
    w.L = (long long *)(base + 2 * nb + 2 * nt); w.sizes = w.L + (size_t)K * K;
    return w;
}

// A -> its bit rows and columns (asynchronous); the latent distance model (latent.hip) reads the same words
nhp_status nhp_sbm_enqueue_pack(nhp_ctx *ctx, const double *d_A, int N, uint32_t *colb, uint32_t *rowb)
{
    const int W = (N + 31) / 32;
    hipLaunchKernelGGL(k_sbm_pack, dim3((unsigned)(((size_t)N * W + 255) / 256), 2), dim3(256), 0, ctx->main(), d_A, N, W, colb, rowb);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// bits of A, the per-node tables and the block counts for the labels d_z (all on the device, asynchronous)
static nhp_status sbm_enqueue_tables(nhp_ctx *ctx, const double *d_A, int N, int K, const int32_t *d_z, const sbm_work &w, bool pack)
{
    hipStream_t st = ctx->main();
    const int W = (N + 31) / 32;
    if (pack) NHP_TRY(nhp_sbm_enqueue_pack(ctx, d_A, N, w.colb, w.rowb));
    NHP_HIP(ctx, hipMemsetAsync(w.L, 0, 8 * ((size_t)K * K + K), st));
    hipLaunchKernelGGL(k_sbm_tables, dim3((unsigned)N), dim3(64), 0, st, w.colb, w.rowb, d_z, N, W, K, w.out, w.in, w.L, w.sizes);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

static nhp_status sbm_enqueue_sweep(nhp_ctx *ctx, int N, int K, int n_sweeps, int32_t *d_z, const double *d_rho, const double *d_pi,
                                    const sbm_work &w, const double *d_u, double *d_probs)
{
    NHP_TRY(sbm_check_sweep(ctx, N, K));
    const size_t lds = sbm_sweep_lds(N, K);
    const int W = (N + 31) / 32;
    hipStream_t st = ctx->main();
    if (lds > 64 * 1024) NHP_HIP(ctx, hipFuncSetAttribute((const void *)k_sbm_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_sbm_sweep, dim3(1), dim3(SBM_BLOCK), lds, st, N, W, K, n_sweeps, d_z, d_rho, d_pi, w.colb, w.rowb, w.out,
                       w.in, w.sizes, d_u, d_probs);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// ---- stand-alone entries on a host A ------------------------------------------------------------------------------------
extern "C" nhp_status nhp_sbm_block_counts(nhp_ctx *ctx, const double *A, int32_t N, int32_t K, const int32_t *z, int64_t *links,
                                           int64_t *sizes)
{
    if (!ctx || !A || !z || !links || !sizes) return NHP_EINVAL;
    NHP_TRY(sbm_check_shape(ctx, "sbm_block_counts", N, K));
    NHP_TRY(sbm_check_labels(ctx, "sbm_block_counts", z, N, K));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t NN = (size_t)N * N, o_z = sbm_align(8 * NN), o_w = o_z + sbm_align(4 * (size_t)N);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, o_w + sbm_work_bytes(N, K)));
    char *base = (char *)ctx->d_scratch;
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(base, A, 8 * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(base + o_z, z, 4 * (size_t)N, hipMemcpyHostToDevice, st));
    const sbm_work w = sbm_carve(base + o_w, N, K);
    NHP_TRY(sbm_enqueue_tables(ctx, (const double *)base, N, K, (const int32_t *)(base + o_z), w, true));
    std::vector<long long> h((size_t)K * K + K);
    NHP_HIP(ctx, hipMemcpyAsync(h.data(), w.L, 8 * h.size(), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < K * K; ++i) links[i] = h[i];
    for (int k = 0; k < K; ++k) sizes[k] = h[(size_t)K * K + k];
    return NHP_OK;
}

extern "C" nhp_status nhp_sbm_draw(nhp_ctx *ctx, int32_t K, const int64_t *links, const int64_t *sizes, double alpha, double beta,
                                   double gamma, uint64_t seed, uint64_t step, double *rho_out, double *pi_out)
{
    if (!ctx || !links || !sizes || !rho_out || !pi_out) return NHP_EINVAL;
    NHP_TRY(sbm_check_shape(ctx, "sbm_draw", 1, K));
    NHP_TRY(sbm_check_priors(ctx, "sbm_draw", alpha, beta, gamma));
    for (int k = 0; k < K; ++k)
        if (sizes[k] < 0) { nhp_set_error(ctx, "sbm_draw: sizes[%d] is negative", k); return NHP_EDOMAIN; }
    for (int i = 0; i < K * K; ++i)
        if (links[i] < 0 || links[i] > sizes[i % K] * sizes[i / K]) {
            nhp_set_error(ctx, "sbm_draw: links[%d,%d] = %lld outside 0..n_k·n_l", i % K, i / K, (long long)links[i]);
            return NHP_EDOMAIN;
        }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nc = (size_t)K * K + K;
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 2 * sbm_align(8 * nc)));
    long long *d_cnt = (long long *)ctx->d_scratch;
    double *d_out = (double *)((char *)ctx->d_scratch + sbm_align(8 * nc));
    std::vector<long long> h(nc);
    for (int i = 0; i < K * K; ++i) h[i] = links[i];
    for (int k = 0; k < K; ++k) h[(size_t)K * K + k] = sizes[k];
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(d_cnt, h.data(), 8 * nc, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sbm_draw, dim3(1), dim3(256), 0, st, K, d_cnt, d_cnt + (size_t)K * K, alpha, beta, gamma, seed, step, d_out,
                       d_out + (size_t)K * K);
    NHP_HIP(ctx, hipGetLastError());
    std::vector<double> o(nc);
    NHP_HIP(ctx, hipMemcpyAsync(o.data(), d_out, 8 * nc, hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    std::copy(o.begin(), o.begin() + (size_t)K * K, rho_out);
    std::copy(o.begin() + (size_t)K * K, o.end(), pi_out);
    return NHP_OK;
}

extern "C" nhp_status nhp_sbm_resample_blocks(nhp_ctx *ctx, const double *A, int32_t N, int32_t K, int32_t *z, const double *rho,
                                              const double *pi, const double *u, uint64_t seed, uint64_t step, int32_t n_sweeps,
                                              double *u_used, double *probs)
{
    if (!ctx || !A || !z || !rho || !pi) return NHP_EINVAL;
    NHP_TRY(sbm_check_shape(ctx, "sbm_resample_blocks", N, K));
    if (n_sweeps < 1) { nhp_set_error(ctx, "sbm_resample_blocks: n_sweeps = %d must be positive", n_sweeps); return NHP_EINVAL; }
    NHP_TRY(sbm_check_labels(ctx, "sbm_resample_blocks", z, N, K));
    NHP_TRY(sbm_check_rho_pi(ctx, "sbm_resample_blocks", rho, pi, K));
    NHP_TRY(sbm_check_sweep(ctx, N, K));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const size_t NN = (size_t)N * N, steps = (size_t)n_sweeps * N, KK = (size_t)K * K;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t r = off; off += sbm_align(bytes); return r; };
    const size_t o_A = carve(8 * NN), o_z = carve(4 * (size_t)N), o_rho = carve(8 * (KK + K)), o_u = carve(8 * steps);
    const size_t o_pr = carve(probs ? 8 * steps * K : 8), o_w = carve(sbm_work_bytes(N, K));
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, off));
    char *base = (char *)ctx->d_scratch;
    hipStream_t st = ctx->main();
    int32_t *d_z = (int32_t *)(base + o_z);
    double *d_rho = (double *)(base + o_rho), *d_pi = d_rho + KK, *d_u = (double *)(base + o_u);
    double *d_probs = probs ? (double *)(base + o_pr) : nullptr;
    NHP_HIP(ctx, hipMemcpyAsync(base + o_A, A, 8 * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_z, z, 4 * (size_t)N, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_rho, rho, 8 * KK, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_pi, pi, 8 * (size_t)K, hipMemcpyHostToDevice, st));
    if (u) NHP_HIP(ctx, hipMemcpyAsync(d_u, u, 8 * steps, hipMemcpyHostToDevice, st));
    else {
        hipLaunchKernelGGL(k_sbm_uniforms, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, st, d_u, seed, step, (int64_t)steps);
        NHP_HIP(ctx, hipGetLastError());
    }
    const sbm_work w = sbm_carve(base + o_w, N, K);
    NHP_TRY(sbm_enqueue_tables(ctx, (const double *)(base + o_A), N, K, d_z, w, true));
    NHP_TRY(sbm_enqueue_sweep(ctx, N, K, n_sweeps, d_z, d_rho, d_pi, w, d_u, d_probs));
    NHP_HIP(ctx, hipMemcpyAsync(z, d_z, 4 * (size_t)N, hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    if (u_used) NHP_TRY(nhp_download(ctx, u_used, d_u, 8 * steps));
    if (probs) NHP_TRY(nhp_download(ctx, probs, d_probs, 8 * steps * K));
    return NHP_OK;
}

// ---- device-resident state, kept next to the continuous model -----------------------------------------------------------
void nhp_sbm_free(nhp_cont_model *m)
{
    nhp_sbm_state *s = m->sbm;
    if (!s) return;
    (void)hipFree(s->d_z); (void)hipFree(s->d_rho); (void)hipFree(s->d_pi); (void)hipFree(s->d_P); (void)hipFree(s->d_sum);
    (void)hipFree(s->d_bc); (void)hipFree(s->d_bits); (void)hipFree(s->d_tab); (void)hipFree(s->d_cnt); (void)hipFree(s->d_u);
    delete s;
    m->sbm = nullptr;
}

// A model whose network is not a block model: drop the block state, so that the chain driver takes the Bernoulli / dense step
// again (nhp_cont_model_set_rho calls this; waits for work that may still read the state)
nhp_status nhp_sbm_detach(nhp_ctx *ctx, nhp_cont_model *m)
{
    if (!m->sbm) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    nhp_sbm_free(m);
    return NHP_OK;
}

static nhp_status sbm_model_check(nhp_ctx *ctx, const nhp_cont_model *m, const char *what, bool need_state)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    if (need_state && !m->sbm) { nhp_set_error(ctx, "%s: the model has no block network (nhp_cont_model_set_sbm)", what); return NHP_EINVAL; }
    return NHP_OK;
}

nhp_status nhp_sbm_moments_reset(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_sbm_state *s = m->sbm;
    const size_t K = (size_t)s->K;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_HIP(ctx, hipMemsetAsync(s->d_sum, 0, 8 * (2 * K * K + 2 * K), ctx->main()));
    NHP_HIP(ctx, hipMemsetAsync(s->d_bc, 0, 8 * (size_t)m->N * K, ctx->main()));
    return NHP_OK;
}

nhp_status nhp_sbm_moments_accumulate(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_sbm_state *s = m->sbm;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const int n = std::max(m->N, s->K * s->K);
    hipLaunchKernelGGL(k_sbm_moments, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->main(), m->N, s->K, s->d_z, s->d_rho, s->d_pi,
                       s->d_sum, s->d_bc);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_set_sbm(nhp_ctx *ctx, nhp_cont_model *m, int32_t K, const int32_t *z, const double *rho,
                                             const double *pi, double alpha, double beta, double gamma)
{
    NHP_TRY(sbm_model_check(ctx, m, "set_sbm", false));
    if (!z || !rho || !pi) return NHP_EINVAL;
    if (!m->has_A) { nhp_set_error(ctx, "set_sbm: the model has no adjacency matrix"); return NHP_EINVAL; }
    const int N = m->N;
    NHP_TRY(sbm_check_shape(ctx, "set_sbm", N, K));
    NHP_TRY(sbm_check_labels(ctx, "set_sbm", z, N, K));
    NHP_TRY(sbm_check_rho_pi(ctx, "set_sbm", rho, pi, K));
    NHP_TRY(sbm_check_priors(ctx, "set_sbm", alpha, beta, gamma));
    NHP_TRY(sbm_check_sweep(ctx, N, K));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_latent_detach(ctx, m));                       // one structured network at a time
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));
    if (m->sbm && m->sbm->K != K) nhp_sbm_free(m);
    const size_t KK = (size_t)K * K, W = ((size_t)N + 31) / 32;
    if (!m->sbm) {
        nhp_sbm_state *s = new nhp_sbm_state;
        s->K = K;
        m->sbm = s;
        if (hipMalloc((void **)&s->d_z, 4 * (size_t)N) != hipSuccess || hipMalloc((void **)&s->d_rho, 8 * KK) != hipSuccess ||
            hipMalloc((void **)&s->d_pi, 8 * (size_t)K) != hipSuccess || hipMalloc((void **)&s->d_P, 8 * (size_t)N * N) != hipSuccess ||
            hipMalloc((void **)&s->d_sum, 8 * (2 * KK + 2 * K)) != hipSuccess || hipMalloc((void **)&s->d_bc, 8 * (size_t)N * K) != hipSuccess ||
            hipMalloc((void **)&s->d_bits, 8 * (size_t)N * W) != hipSuccess || hipMalloc((void **)&s->d_tab, 8 * (size_t)N * K) != hipSuccess ||
            hipMalloc((void **)&s->d_cnt, 8 * (KK + K)) != hipSuccess || hipMalloc((void **)&s->d_u, 8 * (size_t)N) != hipSuccess) {
            (void)hipGetLastError();
            nhp_sbm_free(m);
            nhp_set_error(ctx, "out of device memory (block network state)");
            return NHP_ENOMEM;
        }
        NHP_TRY(nhp_sbm_moments_reset(ctx, m));
    }
    nhp_sbm_state *s = m->sbm;
    s->alpha = alpha; s->beta = beta; s->gamma = gamma;
    hipStream_t st = ctx->main();
    NHP_HIP(ctx, hipMemcpyAsync(s->d_z, z, 4 * (size_t)N, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(s->d_rho, rho, 8 * KK, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(s->d_pi, pi, 8 * (size_t)K, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_set_sbm_labels_every(nhp_ctx *ctx, nhp_cont_model *m, int32_t every)
{
    NHP_TRY(sbm_model_check(ctx, m, "set_sbm_labels_every", true));
    if (every < 1) { nhp_set_error(ctx, "set_sbm_labels_every: every = %d must be positive", every); return NHP_EINVAL; }
    m->sbm->labels_every = every;
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_get_sbm(nhp_ctx *ctx, const nhp_cont_model *m, int32_t *z, double *rho, double *pi, double *sums,
                                             int64_t *block_counts)
{
    NHP_TRY(sbm_model_check(ctx, m, "get_sbm", true));
    const nhp_sbm_state *s = m->sbm;
    const size_t K = (size_t)s->K, N = (size_t)m->N;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    if (z) NHP_TRY(nhp_download(ctx, z, s->d_z, 4 * N));
    if (rho) NHP_TRY(nhp_download(ctx, rho, s->d_rho, 8 * K * K));
    if (pi) NHP_TRY(nhp_download(ctx, pi, s->d_pi, 8 * K));
    if (sums) NHP_TRY(nhp_download(ctx, sums, s->d_sum, 8 * (2 * K * K + 2 * K)));
    if (block_counts) NHP_TRY(nhp_download(ctx, block_counts, s->d_bc, 8 * N * K));
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_sbm_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, uint64_t seed, uint64_t step)
{
    NHP_TRY(sbm_model_check(ctx, m, "sbm_step", true));
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "sbm_step: not available on a column shard (the block labels need every column of A)");
        return NHP_ENOTIMPL;
    }
    nhp_sbm_state *s = m->sbm;
    const int N = m->N, K = s->K, W = (N + 31) / 32;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->main();
    // link probabilities from the current (z, ρ), the adjacency sweep, then resample!(network, A)
    hipLaunchKernelGGL(k_sbm_fill, dim3((unsigned)(((size_t)N * N + 255) / 256)), dim3(256), 0, st, N, K, s->d_z, s->d_rho, s->d_P);
    NHP_HIP(ctx, hipGetLastError());
    double *d_links = nullptr;
    NHP_TRY(nhp_adj_enqueue(ctx, ds, m, nullptr, 0.5, nullptr, nullptr, seed, step, &d_links, s->d_P));
    sbm_work w;
    w.colb = s->d_bits; w.rowb = s->d_bits + (size_t)N * W;
    w.out = s->d_tab; w.in = s->d_tab + (size_t)N * K;
    w.L = s->d_cnt; w.sizes = s->d_cnt + (size_t)K * K;
    NHP_TRY(sbm_enqueue_tables(ctx, m->d_A, N, K, s->d_z, w, true));
    hipLaunchKernelGGL(k_sbm_draw, dim3(1), dim3(256), 0, st, K, w.L, w.sizes, s->alpha, s->beta, s->gamma, seed, step, s->d_rho, s->d_pi);
    NHP_HIP(ctx, hipGetLastError());
    if (step % (uint64_t)s->labels_every == 0) {
        hipLaunchKernelGGL(k_sbm_uniforms, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, s->d_u, seed, step, (int64_t)N);
        NHP_HIP(ctx, hipGetLastError());
        NHP_TRY(sbm_enqueue_sweep(ctx, N, K, 1, s->d_z, s->d_rho, s->d_pi, w, s->d_u, nullptr));
    }
    return NHP_OK;
}
