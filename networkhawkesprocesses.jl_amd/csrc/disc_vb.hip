// The discrete variational fits: mean-field VB (update!, vb!) and SVI (svi!) of the standard process, of the
// network process (§3.19) and of the block network (§3.21).  One iteration serves all of them (§3.32):
//   factors from the OLD parameters -> (SVI: the window's image and counts) -> GEMM-1 with EPI_VB_Z -> GEMM-2 with EPI_SLAB
//   -> baseline kernel -> finish kernel -> (network: the ρv reduction, or the block model's tables and sweep)
// written once as disc_vb_drive; a fit (dense_vb_fit, netvb_fit) supplies its sizing, carving, planes, factors and finish.
// Reference: update! src/discrete.jl:369-375 = update_parents src/parents.jl:136-177 + the three component updates
// src/baselines.jl:444-456, src/weights.jl:70-97, src/impulses.jl:355-375.  The GEMM and its epilogues: nhp_disc_gemm.h.
#include <math.h>

#include <algorithm>

#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_disc_gemm.h"
#include "nhp_netvb.h"
#include "nhp_sbmvb.h"
#include "nhp_sbmvb_dev.h"
#include "nhp_vb_bump.h"

#define CONV_CB DISC_CONV_CB         // basis columns per pass of the convolution kernels, disc.hip's too (nhp_netvb.h)

// VB factors from the OLD variational parameters (src/parents.jl:169-177), one link (p, c) with its ElogW:
// E[k + c·K] = exp(ψ(γv[p,c,b]) - ψ(Σ_b γv[p,c,·]) + ElogW);  e0[c] = exp(ψ(αv) - log βv)
__device__ __forceinline__ void vb_factors_link(int N, int B, size_t pc, double elw, const double *__restrict__ gamma_v,
                                                double *__restrict__ E)
{
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t p = pc % N, c = pc / N;
    double gs = 0.0;
    for (int b = 0; b < B; ++b) gs += gamma_v[pc + (size_t)b * NN];
    const double dgs = nhp_digamma(gs);
    for (int b = 0; b < B; ++b) {
        const double elt = nhp_digamma(gamma_v[pc + (size_t)b * NN]) - dgs;
        E[p + (size_t)b * N + c * K] = nhp_exp(elt + elw);
    }
}
__device__ __forceinline__ double vb_factor_base(double alpha_v, double beta_v) { return nhp_exp(nhp_digamma(alpha_v) - nhp_log(beta_v)); }

// the standard process: ElogW = ψ(κv[p,c]) - log νv[p,c]
__global__ __launch_bounds__(256) void k_vb_factors(int N, int B, const double *__restrict__ alpha_v,
                                                    const double *__restrict__ beta_v,
                                                    const double *__restrict__ kappa_v,
                                                    const double *__restrict__ nu_v,
                                                    const double *__restrict__ gamma_v,
                                                    double *__restrict__ E, double *__restrict__ e0)
{
    const size_t pc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pc < (size_t)N * N) vb_factors_link(N, B, pc, nhp_digamma(kappa_v[pc]) - nhp_log(nu_v[pc]), gamma_v, E);
    if (pc < (size_t)N) e0[pc] = vb_factor_base(alpha_v[pc], beta_v[pc]);
}

// ---- stochastic variational inference (svi!: a stub in the reference, src/inference.jl:190) ----
// One step = the mean-field update! with every sum over t restricted to one block of bins, the block statistics scaled by
// the number of blocks nb, and the result blended into the current parameters with weight ρ.  The two GEMMs are the VB
// step's, on the block's rows of Ŝ (pointer offset t0, lda = T) or of a block-sized image convolved on the fly.

// Ŝ rows [t0, t0 + rows) of every (node, basis) into out[(t - t0) + n·ldo + b·ldo·N]: k_disc_convolve_dense with a window.
// Counts are read from t0 - L on, zeros before bin 0; a bin's sum runs l = 1..L in increasing order with separate multiply
// and add, so a row is bit for bit the row nhp_disc_convolve writes (either of its kernels: a skipped term is +0.0·ϕ).
__global__ __launch_bounds__(256) void k_disc_convolve_window(const double *__restrict__ dataT, int N, int64_t T,
                                                              const double *__restrict__ phi, int L, int B, int64_t t0, int rows,
                                                              size_t ldo, double *__restrict__ out)
{
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    double *tile = csm;                                  // [256 + L]: data[n, tb-L .. tb+255], tb = t0 + 256·blockIdx.x
    double *phiT = csm + 256 + L;                        // [L][Bp], Bp = B rounded up to CONV_CB
    const int n = blockIdx.y, tid = threadIdx.x;
    const int Bp = (B + CONV_CB - 1) / CONV_CB * CONV_CB;
    const int r0 = blockIdx.x * 256;
    const double *d = dataT + (size_t)n * T;
    for (int i = tid; i < 256 + L; i += 256) {
        const int64_t tt = t0 + r0 - L + i;
        tile[i] = (tt >= 0 && tt < T) ? d[tt] : 0.0;
    }
    for (int i = tid; i < L * Bp; i += 256) {
        const int l = i / Bp, b = i % Bp;
        phiT[i] = b < B ? phi[l + (size_t)b * L] : 0.0;
    }
    __syncthreads();
    const int r = r0 + tid;
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
        if (r < rows) {
#pragma unroll
            for (int q = 0; q < CONV_CB; ++q)
                if (b0 + q < B) out[(size_t)r + (size_t)n * ldo + (size_t)(b0 + q) * ldo * N] = s[q] > 0.0 ? s[q] : 0.0;
        }
    }
}

// the block's counts as a compact rows x N matrix (the GEMM epilogue indexes its count operand with the output's shape)
__global__ __launch_bounds__(256) void k_svi_block_data(const double *__restrict__ dataT, int64_t T, int64_t t0, int rows, int N,
                                                        double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * N) return;
    const size_t r = i % rows, c = i / rows;
    out[i] = dataT[(size_t)t0 + r + c * (size_t)T];
}

// The γ loop of every finish kernel, once: for each basis b of link (p, c), Γ = E ⊙ Σ_z slab_z (slabs in increasing z), then
//   VB:   γv = γ + Γ,  and Γ joins the sum;
//   SVI:  γ' = γ + Γ,  γ̂ = γ + nb (γ' - γ),  γ̂ - γ joins the sum,  γv <- keep γv + r γ̂.
// Returns Σ_b of what joined, in increasing b.  k_vb_finish<SVI> and every k_netvb_finish<SVI, SBM> call it, so a dense
// network executes the γ statements of the standard process.
template <bool SVI>
__device__ __forceinline__ double vb_gamma_link(int N, int B, size_t pc, int n_slabs, const double *__restrict__ slabs,
                                                const double *__restrict__ E, double gamma, double nb, double keep, double r,
                                                double *__restrict__ gamma_v)
{
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t p = pc % N, c = pc / N;
    double ksum = 0.0;
    for (int b = 0; b < B; ++b) {
        const size_t o = p + (size_t)b * N + c * K;
        double s = 0.0;
        for (int z = 0; z < n_slabs; ++z) s += slabs[(size_t)z * K * N + o];
        if (SVI) {
            const double gp = gamma + E[o] * s;
            const double gh = gamma + nb * (gp - gamma);
            ksum += gh - gamma;
            gamma_v[pc + (size_t)b * NN] = keep * gamma_v[pc + (size_t)b * NN] + r * gh;
        } else {
            const double G = E[o] * s;
            gamma_v[pc + (size_t)b * NN] = gamma + G;
            ksum += G;
        }
    }
    return ksum;
}

// After GEMM-2: the γ loop, then κ̂ = κ + Σ_b (γ̂ - γ), ν̂[p,c] = ν + Σ_t data[p,t] (whole data);  VB writes the hats, SVI
// blends x <- (1 - ρ) x + ρ x̂.  Fixed summation order, no atomics.  The κv blend is written as the fma the SVI kernel has
// always executed, fma(ρ, κ̂, keep κv): left as `keep κv + ρ κ̂` the compiler picks the product to fuse by the code around it,
// and with the γ loop inlined it picks the other one (the last bit of κv moves).
template <bool SVI>
__global__ __launch_bounds__(256) void k_vb_finish(int N, int B, int n_slabs, const double *__restrict__ slabs,
                                                   const double *__restrict__ E, const double *__restrict__ colsum,
                                                   double kappa, double nu, double gamma, double nb, double rho,
                                                   double *__restrict__ kappa_v, double *__restrict__ nu_v,
                                                   double *__restrict__ gamma_v)
{
    const size_t pc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pc >= (size_t)N * N) return;
    const size_t p = pc % N;
    const double keep = 1.0 - rho;
    const double ksum = vb_gamma_link<SVI>(N, B, pc, n_slabs, slabs, E, gamma, nb, keep, rho, gamma_v);
    if (SVI) {
        kappa_v[pc] = __builtin_fma(rho, kappa + ksum, keep * kappa_v[pc]);
        nu_v[pc] = keep * nu_v[pc] + rho * (nu + colsum[p]);
    } else {
        kappa_v[pc] = kappa + ksum;
        nu_v[pc] = nu + colsum[p];
    }
}

// α' = α0 + e0[c]·Σ_{t in window} R[t,c],  β' = 1/β0 + T·dt (whole T; src/baselines.jl:444-452, D14 literal);  VB writes them,
// SVI blends α̂ = α0 + nb (α' - α0) and β'
template <bool SVI>
__global__ __launch_bounds__(256) void k_vb_baseline(int N, int row_blocks, const double *__restrict__ colpart,
                                                     const double *__restrict__ e0, double alpha0, double beta0, double Tdt,
                                                     double nb, double rho, double *__restrict__ alpha_v, double *__restrict__ beta_v)
{
    // 256 threads = 64 columns x 4 row-slices; fixed-order combine keeps the sum deterministic
    __shared__ double part[4][64];
    const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double s = 0.0;
    if (c < N)
        for (int r = sl; r < row_blocks; r += 4) s += colpart[(size_t)r * N + c];
    part[sl][cl] = s;
    __syncthreads();
    if (sl == 0 && c < N) {
        if (SVI) {
            const double ap = alpha0 + e0[c] * (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]);
            const double keep = 1.0 - rho;
            alpha_v[c] = keep * alpha_v[c] + rho * (alpha0 + nb * (ap - alpha0));
            beta_v[c] = keep * beta_v[c] + rho * (1.0 / beta0 + Tdt);
        } else {
            alpha_v[c] = alpha0 + e0[c] * (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]);
            beta_v[c] = 1.0 / beta0 + Tdt;
        }
    }
}

// Block of step i (global, 1-based): floor(nb·u), u the Philox4x32-10 uniform with key seed ^ SVI_KEY and counter
// (event 0, step i) -- a function of (seed, i) alone, so a run cut into chunks draws the same sequence.
#define SVI_KEY 0x5C1B10C5D2A7E391ull
static inline int32_t svi_block_of(uint64_t seed, uint64_t i, int32_t nb)
{
    const int32_t j = (int32_t)(nhp_philox_uniform(seed ^ SVI_KEY, i, 0) * (double)nb);
    return j < nb ? j : nb - 1;
}

extern "C" nhp_status nhp_disc_svi_blocks(uint64_t seed, int64_t step0, int64_t n, int32_t nb, int32_t *out)
{
    if (!out || n < 0 || step0 < 0 || nb < 1) return NHP_EINVAL;
    for (int64_t k = 0; k < n; ++k) out[k] = svi_block_of(seed, (uint64_t)(step0 + k + 1), nb);
    return NHP_OK;
}

// GEMM-2's split of a `len`-long reduction (the VB step's rule).  svi_split_cap is the most slabs the rule can give: it is
// monotone in len, so the cap of a whole block bounds every block, whole or short, and sizes the slab scratch.
static int svi_split_cap(int64_t len, int tiles2, int cu_count)
{
    return std::max(1, std::min((2 * cu_count + tiles2 - 1) / tiles2, (int)((len + 4 * BK - 1) / (4 * BK))));
}
static void svi_split(int64_t len, int tiles2, int cu_count, int *splits, int *k_chunk)
{
    const int s = svi_split_cap(len, tiles2, cu_count);
    int kc = (int)((len + s - 1) / s);
    kc = ((kc + BK - 1) / BK) * BK;
    *k_chunk = kc;
    *splits = (int)((len + kc - 1) / kc);              // <= s: rounding the chunk up only removes slabs
}

// ---- VB and SVI for the network process: spike-and-slab weights around the two GEMMs above ----
// q(A[p,c] = 1) = ρv[p,c], q(W | A = a) = Gamma(κv_a, νv_a); the reference writes every formula (src/weights.jl:141-173,
// src/discrete.jl:482-492, src/networks.jl:80-93) and throws on the wiring.  The GEMMs, their epilogues and the baseline
// kernels are the dense step's; the three kernels below are the per-link layer around them.

// E[(p,b), c] = exp(ψ(γv[p,c,b]) - ψ(Σ_b γv) + ElogW),  ElogW = (1 - ρv)(ψ(κv0) - log νv0) + ρv (ψ(κv1) - log νv1): two
// products and one sum, never contracted, so ρv = 1 leaves the slab's term exactly (the dense step's factor bit for bit)
__global__ __launch_bounds__(256) void k_netvb_factors(int N, int B, const double *__restrict__ alpha_v,
                                                       const double *__restrict__ beta_v,
                                                       const double *__restrict__ kappa_v0, const double *__restrict__ nu_v0,
                                                       const double *__restrict__ kappa_v1, const double *__restrict__ nu_v1,
                                                       const double *__restrict__ gamma_v, const double *__restrict__ rho_v,
                                                       double *__restrict__ E, double *__restrict__ e0)
{
    const size_t pc = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pc < (size_t)N * N) {
        double elw;
        {
#pragma clang fp contract(off)
            const double r = rho_v[pc];
            const double elw0 = nhp_digamma(kappa_v0[pc]) - nhp_log(nu_v0[pc]);
            const double elw1 = nhp_digamma(kappa_v1[pc]) - nhp_log(nu_v1[pc]);
            elw = (1.0 - r) * elw0 + r * elw1;
        }
        vb_factors_link(N, B, pc, elw, gamma_v, E);
    }
    if (pc < (size_t)N) e0[pc] = vb_factor_base(alpha_v[pc], beta_v[pc]);
}

// (netvb_lgamma_diff, netvb_logit, netvb_sigmoid: nhp_math.h, shared with cont_netvb.hip)

// After GEMM-2: Γ = E ⊙ Σ_z slab_z and the hats γ̂ = γ + nb Γ, κ̂_a = κ_a + Σ_b (γ̂ - γ), ν̂_a[p,c] = ν_a + Σ_t data[p,t]
// (VB: nb = 1 and γ̂ = γ + Γ as k_vb_finish writes it); ρ̂ from the logit at the hats and the OLD network parameters
// netp = (αv, βv); then x <- x̂ (VB) or x <- (1 - r) x + r x̂ (SVI), ρv included.  Every workgroup leaves the pair
// (Σ ρ̂, Σ (1 - ρ̂)) of its 256 links in partials[2·blockIdx.x ..]: the order inside nhp_block_sum2_n is fixed.
// What the finish kernel reads for a block network: net[p,c] = Σ_l (m·D)[p,l] m[c,l] off the diagonal and
// Σ_k m[p,k] D[k,k] on it (a node has one label), D = ψ(αv) - ψ(βv) per pair of blocks; an SVI step also keeps ρ̂.
// (sbmvb_link, sbmvb_net: nhp_sbmvb_dev.h, shared with cont_netvb.hip)

template <bool SVI, bool SBM = false>
__global__ __launch_bounds__(256) void k_netvb_finish(int N, int B, int n_slabs, const double *__restrict__ slabs,
                                                      const double *__restrict__ E, const double *__restrict__ colsum,
                                                      double kappa0, double nu0, double kappa1, double nu1, double gamma,
                                                      double nb, double r, int net_kind, double prior,
                                                      const double *__restrict__ netp,
                                                      double *__restrict__ kappa_v0, double *__restrict__ nu_v0,
                                                      double *__restrict__ kappa_v1, double *__restrict__ nu_v1,
                                                      double *__restrict__ gamma_v, double *__restrict__ rho_v,
                                                      double *__restrict__ partials, sbmvb_link blk)
{
    __shared__ double red[2 * NHP_WAVES];
    const size_t NN = (size_t)N * N;
    const size_t pc = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double keep = 1.0 - r;
    double rh = 0.0, rc = 0.0;                         // ρ̂ and 1 - ρ̂ of this link; a thread past the end adds nothing
    if (pc < NN) {
        const size_t p = pc % N, c = pc / N;
        const double ksum = vb_gamma_link<SVI>(N, B, pc, n_slabs, slabs, E, gamma, nb, keep, r, gamma_v);
        const double k0h = kappa0 + ksum, k1h = kappa1 + ksum, n0h = nu0 + colsum[p], n1h = nu1 + colsum[p];
        if (net_kind == 0) {
            rh = 1.0;
        } else {
            const double net = SBM ? sbmvb_net(blk, (size_t)N, p, c) : nhp_digamma(netp[0]) - nhp_digamma(netp[1]);
            rh = netvb_sigmoid(netvb_logit(net, prior, kappa1 - kappa0, nu1 - nu0, k0h, n0h, n1h));
            if (SBM && SVI) blk.rho_hat[pc] = rh;
        }
        rc = 1.0 - rh;
        if (SVI) {
            kappa_v0[pc] = keep * kappa_v0[pc] + r * k0h;
            nu_v0[pc] = keep * nu_v0[pc] + r * n0h;
            kappa_v1[pc] = keep * kappa_v1[pc] + r * k1h;
            nu_v1[pc] = keep * nu_v1[pc] + r * n1h;
            rho_v[pc] = net_kind ? keep * rho_v[pc] + r * rh : 1.0;
        } else {
            kappa_v0[pc] = k0h; nu_v0[pc] = n0h; kappa_v1[pc] = k1h; nu_v1[pc] = n1h;
            rho_v[pc] = rh;
        }
    }
    nhp_block_sum2_n<NHP_WAVES>(rh, rc, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = rh; partials[2 * (size_t)blockIdx.x + 1] = rc; }
}

// One workgroup: thread i adds the pairs i, i + 256, ... in increasing order, nhp_block_sum2_n joins the 256 threads in
// its fixed order; αv = α + Σρ̂, βv = β + Σ(1 - ρ̂) over all N² links, the diagonal included (src/networks.jl:86-90)
template <bool SVI>
__global__ __launch_bounds__(256) void k_netvb_network(int n_pairs, const double *__restrict__ partials, double alpha, double beta,
                                                       double r, double *__restrict__ netp)
{
    __shared__ double red[2 * NHP_WAVES];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_pairs; i += 256) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
    nhp_block_sum2_n<NHP_WAVES>(a, b, red);
    if (threadIdx.x == 0) {
        const double ah = alpha + a, bh = beta + b;
        if (SVI) {
            const double keep = 1.0 - r;
            netp[0] = keep * netp[0] + r * ah;
            netp[1] = keep * netp[1] + r * bh;
        } else {
            netp[0] = ah; netp[1] = bh;
        }
    }
}

// (k_sbmvb_expect, k_sbmvb_md, k_sbmvb_u, k_sbmvb_tables, k_sbmvb_sweep and its launcher, sbmvb_bufs: nhp_sbmvb_dev.h, shared
// with cont_netvb.hip)

// x <- (1 - r) x + r x̂ over the block model's state (m, αv, βv, γv, contiguous): a convex combination keeps m on the simplex
__global__ __launch_bounds__(256) void k_sbmvb_blend(size_t n, double r, const double *__restrict__ hat, double *__restrict__ x)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double keep = 1.0 - r;
    if (i < n) x[i] = keep * x[i] + r * hat[i];
}

// the block model's part of a run: the priors, the schedule of the sweep and the caller's in/out arrays
struct sbmvb_args {
    int32_t K;
    double alpha, beta, gamma;
    int32_t labels_every;
    int64_t step0;                                     // VB: steps already taken (SVI has its own step0)
    double *m, *alpha_v, *beta_v, *gamma_v;
};

static sbmvb_bufs sbmvb_carve(vb_bump &p, size_t N, size_t K, bool svi)
{
    const size_t NK = N * K, KK = K * K;
    sbmvb_bufs s;
    s.m = p.take(NK); s.av = p.take(KK); s.bv = p.take(KK); s.gv = p.take(K);
    s.mh = p.take(NK); s.avh = p.take(KK); s.bvh = p.take(KK); s.gvh = p.take(K);
    s.D = p.take(KK);
    s.tabs = p.take(4 * KK);                           // E1, E0, E1ᵀ, E0ᵀ
    s.Epi = p.take(K); s.mD = p.take(NK); s.U1 = p.take(NK); s.U0 = p.take(NK);
    s.rho_hat = p.take(svi ? N * N : 0);
    s.end = p.p;
    return s;
}

static nhp_status sbmvb_check(nhp_ctx *ctx, const char *what, int64_t N, const sbmvb_args &a)
{
    char msg[256];
    const int rc = sbmvb_check_args(what, N, a.K, a.alpha, a.beta, a.gamma, a.labels_every, a.m, a.alpha_v, a.beta_v, a.gamma_v, msg, sizeof msg);
    if (rc == NETVB_OK) return NHP_OK;
    nhp_set_error(ctx, "%s", msg);
    return rc == NETVB_ENOTIMPL ? NHP_ENOTIMPL : NHP_EINVAL;
}

static nhp_status sbmvb_copy(nhp_ctx *ctx, hipStream_t st, const sbmvb_bufs &s, const sbmvb_args &a, size_t N, bool up)
{
    const size_t K = (size_t)a.K;
    double *dev[4] = {s.m, s.av, s.bv, s.gv}, *host[4] = {a.m, a.alpha_v, a.beta_v, a.gamma_v};
    const size_t bytes[4] = {8 * N * K, 8 * K * K, 8 * K * K, 8 * K};
    for (int i = 0; i < 4; ++i)
        NHP_HIP(ctx, up ? hipMemcpyAsync(dev[i], host[i], bytes[i], hipMemcpyHostToDevice, st)
                        : hipMemcpyAsync(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost, st));
    return NHP_OK;
}

// before the finish kernel: D from the OLD tables and m·D from the OLD m
static void sbmvb_before_finish(hipStream_t st, const sbmvb_bufs &s, size_t N, size_t K)
{
    hipLaunchKernelGGL(k_sbmvb_expect, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, st, (int)K, s.av, s.bv, s.gv, s.D, s.tabs,
                       s.Epi);
    hipLaunchKernelGGL(k_sbmvb_md, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, (int)N, (int)K, s.m, s.D, s.mD);
}

// after the finish kernel: the tables from the NEW ρv (SVI: ρ̂v) and the current m, then the sweep when this step has one.
// VB writes the state itself; SVI writes the hats, sweeps a copy of m and blends.
static nhp_status sbmvb_after_finish(nhp_ctx *ctx, hipStream_t st, const sbmvb_bufs &s, const sbmvb_args &a, size_t N, const double *rho,
                                     bool svi, bool sweep, double r)
{
    const size_t K = (size_t)a.K, NK = N * K;
    double *av = svi ? s.avh : s.av, *bv = svi ? s.bvh : s.bv, *gv = svi ? s.gvh : s.gv, *m = svi ? s.mh : s.m;
    hipLaunchKernelGGL(k_sbmvb_u, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, st, (int)N, (int)K, rho, s.m, s.U1, s.U0);
    hipLaunchKernelGGL(k_sbmvb_tables, dim3((unsigned)(K * K)), dim3(256), 0, st, (int)N, (int)K, rho, s.m, s.U1, s.U0, a.alpha, a.beta,
                       a.gamma, av, bv, gv);
    if (sweep) {
        if (svi) NHP_HIP(ctx, hipMemcpyAsync(s.mh, s.m, 8 * NK, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_sbmvb_expect, dim3((unsigned)((K * K + 255) / 256)), dim3(256), 0, st, (int)K, av, bv, gv, s.D, s.tabs,
                           s.Epi);
        NHP_TRY(sbmvb_launch_sweep(ctx, st, s, N, K, rho, m));
    }
    if (svi) {                                         // a step without a sweep has no m̂: m stays bit for bit, the tables blend
        const size_t skip = sweep ? 0 : NK, n = sbmvb_state_doubles(N, K) - skip;
        hipLaunchKernelGGL(k_sbmvb_blend, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, r, s.mh + skip, s.m + skip);
    }
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// ---- one step's launch plan and its two GEMMs ----

// a window of `len` bins: GEMM-1's tile height and row blocks (= column partials), GEMM-2's split of the len-long reduction
struct disc_vb_plan { int bm, row_blocks, splits, k_chunk; };
static int disc_vb_tiles2(size_t N, size_t K) { return (int)(((K + BM - 1) / BM) * ((N + BN - 1) / BN)); }
static disc_vb_plan disc_vb_plan_of(int64_t len, size_t N, size_t K, int cu_count)
{
    disc_vb_plan q;
    q.bm = gemm1_tile_m(len, (int)N, cu_count);
    q.row_blocks = (int)((len + q.bm - 1) / q.bm);
    svi_split(len, disc_vb_tiles2(N, K), cu_count, &q.splits, &q.k_chunk);
    return q;
}

// rows of Ŝ (G, leading dimension ldg) and of the counts (D, compact when the window is not the whole data)
struct disc_vb_window { const double *G; size_t ldg; const double *D; int64_t len; };

// GEMM-1: Z = e0 ⊕ G·E, R = D / Z, column sums of R;  GEMM-2: slabs_z = Gᵀ·R over chunk z of the window
static nhp_status disc_vb_gemms(nhp_ctx *ctx, hipStream_t st, const disc_vb_window &w, const disc_vb_plan &q, size_t N, size_t K,
                                const double *E, const double *e0, double *R, double *colp, double *slabs)
{
    gemm_args g1{};
    g1.A = w.G; g1.lda = w.ldg; g1.B = E; g1.ldb = K; g1.M = (int)w.len; g1.N = (int)N; g1.K = (int)K; g1.k_chunk = (int)K;
    g1.base = e0; g1.dataT = w.D; g1.out = R; g1.partials = colp;
    launch_gemm<true, EPI_VB_Z>(g1, 1, st, q.bm);
    NHP_HIP(ctx, hipGetLastError());
    gemm_args g2{};
    g2.A = w.G; g2.lda = w.ldg; g2.B = R; g2.ldb = (size_t)w.len; g2.M = (int)K; g2.N = (int)N; g2.K = (int)w.len; g2.k_chunk = q.k_chunk;
    g2.out = slabs;
    launch_gemm<false, EPI_SLAB>(g2, q.splits, st);
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

// ---- the fits: plain structs the loop below is instantiated with ----
//   N, B, alpha0, beta0        the shape and the baseline's prior (the baseline kernel is the loop's)
//   E, e0, av, bv              what the GEMMs and the baseline kernel read and write
//   reserve_doubles(dims)      the sizing function (nhp_netvb.h) of what carve + the window's buffers + carve_tail take
//   carve(mem), carve_tail(mem, svi)
//   upload(ctx, st), download(ctx, st)    the caller's arrays, through the fit's planes
//   factors(st)                E, e0 from the OLD parameters
//   finish(ctx, st, slabs, n_slabs, svi, nb, rho, step)   the finish kernel and what follows it; consults hipGetLastError

struct disc_vb_plane { double *user, *dev; size_t n; };
static nhp_status disc_vb_copy(nhp_ctx *ctx, hipStream_t st, const disc_vb_plane *pl, int n, bool up)
{
    for (int i = 0; i < n; ++i)
        NHP_HIP(ctx, up ? hipMemcpyAsync(pl[i].dev, pl[i].user, 8 * pl[i].n, hipMemcpyHostToDevice, st)
                        : hipMemcpyAsync(pl[i].user, pl[i].dev, 8 * pl[i].n, hipMemcpyDeviceToHost, st));
    return NHP_OK;
}

struct dense_vb_fit {
    size_t N, B;
    double alpha0, beta0, kappa, nu, gamma;
    double *alpha_v, *beta_v, *kappa_v, *nu_v, *gamma_v;          // the caller's arrays
    const double *colsum;
    double *E, *e0, *av, *bv, *kv, *nv, *gv;

    size_t reserve_doubles(const disc_vb_dims &d) const { return dense_vb_reserve_doubles(d); }
    void carve(vb_bump &m)
    {
        const size_t NN = N * N;
        E = m.take(N * B * N); e0 = m.take(N); av = m.take(N); bv = m.take(N); kv = m.take(NN); nv = m.take(NN); gv = m.take(NN * B);
    }
    void carve_tail(vb_bump &, bool) {}
    nhp_status copy(nhp_ctx *ctx, hipStream_t st, bool up) const
    {
        const size_t NN = N * N;
        const disc_vb_plane pl[5] = {{alpha_v, av, N}, {beta_v, bv, N}, {kappa_v, kv, NN}, {nu_v, nv, NN}, {gamma_v, gv, NN * B}};
        return disc_vb_copy(ctx, st, pl, 5, up);
    }
    nhp_status upload(nhp_ctx *ctx, hipStream_t st) { return copy(ctx, st, true); }
    nhp_status download(nhp_ctx *ctx, hipStream_t st)
    {
        NHP_TRY(copy(ctx, st, false));
        NHP_HIP(ctx, hipStreamSynchronize(st));
        return NHP_OK;
    }
    void factors(hipStream_t st) const
    {
        hipLaunchKernelGGL(k_vb_factors, dim3((unsigned)((N * N + 255) / 256)), dim3(256), 0, st, (int)N, (int)B, av, bv, kv, nv, gv, E, e0);
    }
    nhp_status finish(nhp_ctx *ctx, hipStream_t st, const double *slabs, int n_slabs, bool svi, double nb, double rho, uint64_t) const
    {
        hipLaunchKernelGGL(svi ? k_vb_finish<true> : k_vb_finish<false>, dim3((unsigned)((N * N + 255) / 256)), dim3(256), 0, st, (int)N,
                           (int)B, n_slabs, slabs, E, colsum, kappa, nu, gamma, nb, rho, kv, nv, gv);
        NHP_HIP(ctx, hipGetLastError());
        return NHP_OK;
    }
};

struct netvb_host {
    double *alpha_v, *beta_v, *kappa_v0, *nu_v0, *kappa_v1, *nu_v1, *gamma_v, *rho_v, *net_alpha_v, *net_beta_v;
};

// A dense or Bernoulli network (sb = nullptr) or a block network (sb: net_kind is 1 for the checks and the kernels, the
// scalar network parameters are placeholders nobody reads).  The device block is in the order netvb_param_doubles counts.
struct netvb_fit {
    size_t N, B;
    netvb_priors q;
    double alpha0, beta0, prior;
    netvb_host h;
    const sbmvb_args *sb;
    const double *colsum;
    double *E, *e0, *av, *bv, *kv0, *nv0, *kv1, *nv1, *gv, *rho, *netp, *part;
    sbmvb_bufs s;
    double net_stage[2];

    size_t KB() const { return sb ? (size_t)sb->K : 0; }
    unsigned link_blocks() const { return (unsigned)netvb_link_blocks(N); }
    size_t reserve_doubles(const disc_vb_dims &d) const { return netvb_reserve_doubles(d, sb ? sbmvb_param_doubles(N, KB(), d.svi) : 0); }
    void carve(vb_bump &m)
    {
        const size_t NN = N * N;
        E = m.take(N * B * N); e0 = m.take(N); av = m.take(N); bv = m.take(N);
        kv0 = m.take(NN); nv0 = m.take(NN); kv1 = m.take(NN); nv1 = m.take(NN); gv = m.take(NN * B); rho = m.take(NN);
        netp = m.take(2); part = m.take(2 * netvb_link_blocks(N));
    }
    void carve_tail(vb_bump &m, bool svi)
    {
        if (!sb) return;
        s = sbmvb_carve(m, N, KB(), svi);
    }
    nhp_status copy(nhp_ctx *ctx, hipStream_t st, bool up)
    {
        const size_t NN = N * N;
        const disc_vb_plane pl[9] = {{h.alpha_v, av, N}, {h.beta_v, bv, N}, {h.kappa_v0, kv0, NN}, {h.nu_v0, nv0, NN}, {h.kappa_v1, kv1, NN},
                                     {h.nu_v1, nv1, NN}, {h.gamma_v, gv, NN * B}, {h.rho_v, rho, NN}, {net_stage, netp, 2}};
        return disc_vb_copy(ctx, st, pl, 9, up);
    }
    // a dense network's ρv is 1 whatever the caller's array holds; the network's two scalars travel through net_stage
    nhp_status upload(nhp_ctx *ctx, hipStream_t st)
    {
        if (q.net_kind == 0)
            for (size_t i = 0; i < N * N; ++i) h.rho_v[i] = 1.0;
        net_stage[0] = q.net_kind ? *h.net_alpha_v : 1.0;
        net_stage[1] = q.net_kind ? *h.net_beta_v : 1.0;
        NHP_TRY(copy(ctx, st, true));
        if (sb) NHP_TRY(sbmvb_copy(ctx, st, s, *sb, N, true));
        return NHP_OK;
    }
    nhp_status download(nhp_ctx *ctx, hipStream_t st)
    {
        if (sb) NHP_TRY(sbmvb_copy(ctx, st, s, *sb, N, false));
        NHP_TRY(copy(ctx, st, false));
        NHP_HIP(ctx, hipStreamSynchronize(st));
        if (q.net_kind) { *h.net_alpha_v = net_stage[0]; *h.net_beta_v = net_stage[1]; }
        return NHP_OK;
    }
    void factors(hipStream_t st) const
    {
        hipLaunchKernelGGL(k_netvb_factors, dim3(link_blocks()), dim3(256), 0, st, (int)N, (int)B, av, bv, kv0, nv0, kv1, nv1, gv, rho, E, e0);
    }
    template <bool SBM>
    void launch_finish(hipStream_t st, const double *slabs, int n_slabs, bool svi, double nb, double r, const sbmvb_link &blk) const
    {
        hipLaunchKernelGGL((svi ? k_netvb_finish<true, SBM> : k_netvb_finish<false, SBM>), dim3(link_blocks()), dim3(256), 0, st, (int)N,
                           (int)B, n_slabs, slabs, E, colsum, q.kappa0, q.nu0, q.kappa1, q.nu1, q.gamma, nb, r, (int)q.net_kind, prior, netp,
                           kv0, nv0, kv1, nv1, gv, rho, part, blk);
    }
    nhp_status finish(nhp_ctx *ctx, hipStream_t st, const double *slabs, int n_slabs, bool svi, double nb, double r, uint64_t step) const
    {
        if (sb) {       // the block network: a per-link term in; the tables (SVI: the hats from ρ̂v), the sweep and the blend after
            sbmvb_before_finish(st, s, N, KB());
            launch_finish<true>(st, slabs, n_slabs, svi, nb, r, sbmvb_link{(int)KB(), s.m, s.mD, s.D, svi ? s.rho_hat : nullptr});
            const bool sweep = ((uint64_t)sb->step0 + step) % (uint64_t)sb->labels_every == 0;
            return sbmvb_after_finish(ctx, st, s, *sb, N, svi ? s.rho_hat : rho, svi, sweep, r);
        }
        launch_finish<false>(st, slabs, n_slabs, svi, nb, r, sbmvb_link{});
        if (q.net_kind) {
            hipLaunchKernelGGL(svi ? k_netvb_network<true> : k_netvb_network<false>, dim3(1), dim3(256), 0, st, (int)link_blocks(), part,
                               q.net_alpha, q.net_beta, r, netp);
        }
        NHP_HIP(ctx, hipGetLastError());
        return NHP_OK;
    }
};

// ---- the loop: every entry point below reaches it after its own argument checks ----
// sc = nullptr is a VB run: one window, the whole resident Ŝ, nb = 1 and the kernels that write the hats.  With a schedule,
// step i (global, 1-based) works on block j of Tb bins (short at the end of the data) and blends with ρ_i = (i + delay)^-forgetting.
template <class FIT>
static nhp_status disc_vb_drive(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt, FIT &f, int32_t n_steps, const svi_schedule *sc)
{
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    const bool svi = sc != nullptr, streamed = svi && sc->streamed;
    const size_t N = f.N, B = f.B, K = N * B, T = (size_t)ds->T, L = streamed ? (size_t)sc->rq.n_lags : 0;
    const int64_t Tn = ds->T, Tb = svi ? sc->Tb : Tn;
    const int32_t nb = svi ? sc->nb : 1;
    // VB sizes the column partials and the slabs by the plan of its one window; SVI by the caps of a whole block, which bound
    // every block, whole or short
    disc_vb_plan whole{};
    disc_vb_dims d{N, B, (size_t)Tb, 0, 0, svi, L};
    if (svi) {
        d.row_blocks = (size_t)((Tb + BM - 1) / BM);
        d.splits = (size_t)svi_split_cap(Tb, disc_vb_tiles2(N, K), ctx->cu_count);
    } else {
        whole = disc_vb_plan_of(Tn, N, K, ctx->cu_count);
        d.row_blocks = (size_t)whole.row_blocks;
        d.splits = (size_t)whole.splits;
    }
    const size_t want = f.reserve_doubles(d);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * want));
    vb_bump mem((double *)ctx->d_scratch);
    f.carve(mem);
    double *dD = mem.take(svi ? d.rows * N : 0), *dR = mem.take(d.rows * N), *dcolp = mem.take(d.row_blocks * N);
    double *dslab = mem.take(d.splits * K * N), *dimg = mem.take(streamed ? d.rows * K : 0), *dphi = mem.take(L * B);
    f.carve_tail(mem, svi);
    if (mem.used() != want) {
        nhp_set_error(ctx, "variational state: carved %zu doubles of %zu reserved (sizing and carving disagree)", mem.used(), want);
        return NHP_EINVAL;
    }
    hipStream_t st = ctx->main();
    NHP_TRY(f.upload(ctx, st));
    if (streamed) NHP_HIP(ctx, hipMemcpyAsync(dphi, sc->rq.phi, 8 * L * B, hipMemcpyHostToDevice, st));
    const size_t lds_conv = svi_window_lds_bytes(L, B);
    for (int32_t k = 0; k < n_steps; ++k) {           // every parameter stays on the device between steps
        const uint64_t i = (uint64_t)(svi ? sc->rq.step0 : 0) + (uint64_t)k + 1;
        int64_t t0 = 0, len = Tn;
        double rho = 1.0;
        if (svi) {
            const int64_t j = sc->rq.blocks ? sc->rq.blocks[k] : svi_block_of(sc->rq.seed, i, nb);
            t0 = j * Tb; len = std::min<int64_t>(Tn, t0 + Tb) - t0;
            rho = pow((double)i + sc->rq.delay, -sc->rq.forgetting);
        }
        const disc_vb_plan q = svi ? disc_vb_plan_of(len, N, K, ctx->cu_count) : whole;
        f.factors(st);
        disc_vb_window w{ds->d_conv + t0, T, ds->d_dataT, len};
        if (streamed) {
            hipLaunchKernelGGL(k_disc_convolve_window, dim3((unsigned)((len + 255) / 256), (unsigned)N), dim3(256), lds_conv, st, ds->d_dataT, (int)N,
                               Tn, dphi, (int)L, (int)B, t0, (int)len, (size_t)len, dimg);
            w.G = dimg; w.ldg = (size_t)len;
        }
        if (len < Tn) {
            hipLaunchKernelGGL(k_svi_block_data, dim3((unsigned)(((size_t)len * N + 255) / 256)), dim3(256), 0, st, ds->d_dataT, Tn, t0, (int)len,
                               (int)N, dD);
            w.D = dD;
        }
        NHP_HIP(ctx, hipGetLastError());
        NHP_TRY(disc_vb_gemms(ctx, st, w, q, N, K, f.E, f.e0, dR, dcolp, dslab));
        hipLaunchKernelGGL(svi ? k_vb_baseline<true> : k_vb_baseline<false>, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, st, (int)N,
                           q.row_blocks, dcolp, f.e0, f.alpha0, f.beta0, (double)T * dt, (double)nb, rho, f.av, f.bv);
        NHP_TRY(f.finish(ctx, st, dslab, q.splits, svi, (double)nb, rho, i));
    }
    return f.download(ctx, st);
}

// ---- entry points: their own argument checks, then the loop ----

static nhp_status disc_vb_status(nhp_ctx *ctx, int rc, const char *msg)
{
    if (rc == NETVB_OK) return NHP_OK;
    nhp_set_error(ctx, "%s", msg);
    return rc == NETVB_ENOTIMPL ? NHP_ENOTIMPL : NHP_EINVAL;
}

static nhp_status svi_check(nhp_ctx *ctx, const char *what, const nhp_disc_dataset *ds, const svi_request &rq, int32_t n_steps,
                            svi_schedule *sc)
{
    char msg[256];
    return disc_vb_status(ctx, svi_check_schedule(what, rq, n_steps, ds->T, ds->d_baseT != nullptr, ds->d_trial_start != nullptr,
                                                  ds->d_conv != nullptr, sc, msg, sizeof msg), msg);
}

// (nhp_disc_vb_run is declared in include/nhp.h)
extern "C" nhp_status nhp_disc_vb_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                       double alpha0, double beta0, double kappa, double nu, double gamma,
                                       double *alpha_v, double *beta_v, double *kappa_v, double *nu_v, double *gamma_v)
{
    return nhp_disc_vb_run(ctx, ds, dt, alpha0, beta0, kappa, nu, gamma, 1, alpha_v, beta_v, kappa_v, nu_v, gamma_v);
}

extern "C" nhp_status nhp_disc_vb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                      double alpha0, double beta0, double kappa, double nu, double gamma, int32_t n_steps,
                                      double *alpha_v, double *beta_v, double *kappa_v, double *nu_v, double *gamma_v)
{
    if (n_steps < 1) return NHP_EINVAL;
    if (!ctx || !ds || !alpha_v || !beta_v || !kappa_v || !nu_v || !gamma_v) return NHP_EINVAL;
    if (!ds->d_conv) { nhp_set_error(ctx, "convolve(process, data) must run before update!"); return NHP_EINVAL; }
    dense_vb_fit f{(size_t)ds->N, (size_t)ds->B, alpha0, beta0, kappa, nu, gamma, alpha_v, beta_v, kappa_v, nu_v, gamma_v, ds->d_colsum};
    return disc_vb_drive(ctx, ds, dt, f, n_steps, nullptr);
}

extern "C" nhp_status nhp_disc_svi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                       double alpha0, double beta0, double kappa, double nu, double gamma,
                                       int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0,
                                       int32_t n_steps, const int32_t *blocks, const double *phi, int32_t n_lags, int32_t n_basis,
                                       double *alpha_v, double *beta_v, double *kappa_v, double *nu_v, double *gamma_v)
{
    if (!ctx || !ds || !alpha_v || !beta_v || !kappa_v || !nu_v || !gamma_v) return NHP_EINVAL;
    if (!(dt > 0.0)) { nhp_set_error(ctx, "svi: dt must be positive"); return NHP_EINVAL; }
    svi_schedule sc;
    NHP_TRY(svi_check(ctx, "svi", ds, svi_request{batch_bins, delay, forgetting, seed, step0, blocks, phi, n_lags, n_basis}, n_steps, &sc));
    dense_vb_fit f{(size_t)ds->N, (size_t)(sc.streamed ? n_basis : ds->B), alpha0, beta0, kappa, nu, gamma, alpha_v, beta_v, kappa_v, nu_v,
                   gamma_v, ds->d_colsum};
    return disc_vb_drive(ctx, ds, dt, f, n_steps, &sc);
}

static nhp_status netvb_check(nhp_ctx *ctx, const char *what, const nhp_disc_dataset *ds, const netvb_priors &q, double dt, int64_t B,
                              int32_t n_steps, const netvb_host &h)
{
    char msg[256];
    return disc_vb_status(ctx, netvb_check_args(what, q, dt, ds->N, B, n_steps, h.alpha_v, h.beta_v, h.kappa_v0, h.nu_v0, h.kappa_v1, h.nu_v1,
                                                h.gamma_v, h.rho_v, h.net_alpha_v, h.net_beta_v, msg, sizeof msg), msg);
}

// The run of a dense or Bernoulli network (sb = nullptr) or of a block network; rq = nullptr: VB, else SVI
static nhp_status netvb_run_impl(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt, const netvb_priors &q, const netvb_host &h,
                                 int32_t n_steps, const sbmvb_args *sb, const svi_request *rq)
{
    if (!ctx || !ds) return NHP_EINVAL;
    const char *what = rq ? (sb ? "sbmsvi" : "netsvi") : (sb ? "sbmvb" : "netvb");
    svi_schedule sc;
    if (rq) {
        NHP_TRY(svi_check(ctx, what, ds, *rq, n_steps, &sc));
    } else {
        if (!ds->d_conv) { nhp_set_error(ctx, "%s: convolve(process, data) must run before update!", what); return NHP_EINVAL; }
        if (ds->d_baseT) { nhp_set_error(ctx, "%s: defined for DiscreteHomogeneousProcess baselines only", what); return NHP_ENOTIMPL; }
    }
    const int64_t B = rq && sc.streamed ? rq->n_basis : ds->B;
    NHP_TRY(netvb_check(ctx, what, ds, q, dt, B, n_steps, h));
    if (sb) NHP_TRY(sbmvb_check(ctx, what, ds->N, *sb));
    netvb_fit f{(size_t)ds->N, (size_t)B, q, q.alpha0, q.beta0, netvb_prior_logit(q), h, sb, ds->d_colsum};
    return disc_vb_drive(ctx, ds, dt, f, n_steps, rq ? &sc : nullptr);
}

extern "C" nhp_status nhp_disc_netvb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                         double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                                         int32_t net_kind, double net_alpha, double net_beta, int32_t n_steps,
                                         double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                                         double *nu_v1, double *gamma_v, double *rho_v, double *net_alpha_v, double *net_beta_v)
{
    return netvb_run_impl(ctx, ds, dt, netvb_priors{alpha0, beta0, kappa0, nu0, kappa1, nu1, gamma, net_kind, net_alpha, net_beta},
                          netvb_host{alpha_v, beta_v, kappa_v0, nu_v0, kappa_v1, nu_v1, gamma_v, rho_v, net_alpha_v, net_beta_v}, n_steps,
                          nullptr, nullptr);
}

// update! / vb! with a StochasticBlockNetworkModel
extern "C" nhp_status nhp_disc_sbmvb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                         double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                                         int32_t n_blocks, double net_alpha, double net_beta, double net_gamma, int32_t labels_every,
                                         int64_t step0, int32_t n_steps, double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0,
                                         double *kappa_v1, double *nu_v1, double *gamma_v, double *rho_v, double *m,
                                         double *net_alpha_v, double *net_beta_v, double *gamma_v_net)
{
    if (ctx && step0 < 0) { nhp_set_error(ctx, "sbmvb: step0 = %lld must be >= 0", (long long)step0); return NHP_EINVAL; }
    const sbmvb_args sb{n_blocks, net_alpha, net_beta, net_gamma, labels_every, step0, m, net_alpha_v, net_beta_v, gamma_v_net};
    double one_a = 1.0, one_b = 1.0;                  // what the Bernoulli checks and the upload read in place of (αv, βv)
    return netvb_run_impl(ctx, ds, dt, netvb_priors{alpha0, beta0, kappa0, nu0, kappa1, nu1, gamma, 1, 1.0, 1.0},
                          netvb_host{alpha_v, beta_v, kappa_v0, nu_v0, kappa_v1, nu_v1, gamma_v, rho_v, &one_a, &one_b}, n_steps, &sb, nullptr);
}

extern "C" nhp_status nhp_disc_netsvi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                          double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                                          int32_t net_kind, double net_alpha, double net_beta,
                                          int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0,
                                          int32_t n_steps, const int32_t *blocks, const double *phi, int32_t n_lags, int32_t n_basis,
                                          double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                                          double *nu_v1, double *gamma_v, double *rho_v, double *net_alpha_v, double *net_beta_v)
{
    const svi_request rq{batch_bins, delay, forgetting, seed, step0, blocks, phi, n_lags, n_basis};
    return netvb_run_impl(ctx, ds, dt, netvb_priors{alpha0, beta0, kappa0, nu0, kappa1, nu1, gamma, net_kind, net_alpha, net_beta},
                          netvb_host{alpha_v, beta_v, kappa_v0, nu_v0, kappa_v1, nu_v1, gamma_v, rho_v, net_alpha_v, net_beta_v}, n_steps,
                          nullptr, &rq);
}

// svi! with a StochasticBlockNetworkModel; the sweep's schedule counts the run's own step0
extern "C" nhp_status nhp_disc_sbmsvi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                                          double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                                          int32_t n_blocks, double net_alpha, double net_beta, double net_gamma, int32_t labels_every,
                                          int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0,
                                          int32_t n_steps, const int32_t *blocks, const double *phi, int32_t n_lags, int32_t n_basis,
                                          double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                                          double *nu_v1, double *gamma_v, double *rho_v, double *m, double *net_alpha_v,
                                          double *net_beta_v, double *gamma_v_net)
{
    const sbmvb_args sb{n_blocks, net_alpha, net_beta, net_gamma, labels_every, 0, m, net_alpha_v, net_beta_v, gamma_v_net};
    const svi_request rq{batch_bins, delay, forgetting, seed, step0, blocks, phi, n_lags, n_basis};
    double one_a = 1.0, one_b = 1.0;
    return netvb_run_impl(ctx, ds, dt, netvb_priors{alpha0, beta0, kappa0, nu0, kappa1, nu1, gamma, 1, 1.0, 1.0},
                          netvb_host{alpha_v, beta_v, kappa_v0, nu_v0, kappa_v1, nu_v1, gamma_v, rho_v, &one_a, &one_b}, n_steps, &sb, &rq);
}
