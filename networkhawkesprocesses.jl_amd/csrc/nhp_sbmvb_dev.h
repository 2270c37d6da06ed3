// Device side of the block network's variational layer, shared by the discrete fit (disc.hip) and the continuous
// one (cont_netvb.hip): the expectation tables, m·D, the link sums U1 / U0, the tables' update and THE label
// sweep with its launcher, and the device block they work in.  Everything has internal linkage (one copy per file that
// includes it); the text is what disc.hip held.
#pragma once
#include <cmath>

#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_sbmvb.h"

namespace {

// A link's network term, net[p,c] = Σ_l (m·D)[p,l] m[c,l] off the diagonal and Σ_k m[p,k] D[k,k] on it: what the per-link
// kernels read (disc.hip's k_netvb_finish, which also keeps ρ̂ for an SVI step; cont_netvb.hip's k_csbmvb_update).  A thread
// handles link p + c·N with p fastest, so (m·D)[p,l] is read coalesced per l and m[c,l] is one address for the wave.
struct sbmvb_link {
    int K;
    const double *m, *mD, *D;
    double *rho_hat;
};
__device__ __forceinline__ double sbmvb_net(const sbmvb_link &s, size_t N, size_t p, size_t c)
{
    double net = 0.0;
    if (p == c)
        for (int k = 0; k < s.K; ++k) net += s.m[p + (size_t)k * N] * s.D[(size_t)k * s.K + k];
    else
        for (int l = 0; l < s.K; ++l) net += s.mD[p + (size_t)l * N] * s.m[c + (size_t)l * N];
    return net;
}

// ---- the block network's variational layer: q(z_n) = Categorical(m[n,:]), q(π) = Dirichlet(γv),
// q(ρ[k,l]) = Beta(αv[k,l], βv[k,l]) around the per-link step above.  m is [n, k] and the K x K tables [k, l], column-major.

// The expectations of one set of tables: D = ψ(αv) - ψ(βv) (= E1 - E0, the ψ(αv + βv) cancels and is never formed),
// E1 = ψ(αv) - ψ(αv + βv), E0 = ψ(βv) - ψ(αv + βv), their transposes (the sweep reads a row and a column of each, both
// with consecutive threads on consecutive addresses) and Eπ = ψ(γv) - ψ(Σγv), γv added in increasing k.
__global__ __launch_bounds__(256) void k_sbmvb_expect(int K, const double *__restrict__ alpha_v, const double *__restrict__ beta_v,
                                                      const double *__restrict__ gamma_v, double *__restrict__ D,
                                                      double *__restrict__ tabs, double *__restrict__ Epi)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    double *E1 = tabs, *E0 = tabs + K * K, *E1T = tabs + 2 * K * K, *E0T = tabs + 3 * K * K;   // the layout k_sbmvb_sweep reads
    if (i < K * K) {
        const int k = i % K, l = i / K;
        const double da = nhp_digamma(alpha_v[i]), db = nhp_digamma(beta_v[i]), ds = nhp_digamma(alpha_v[i] + beta_v[i]);
        D[i] = da - db;
        E1[i] = da - ds; E0[i] = db - ds;
        E1T[l + k * K] = da - ds; E0T[l + k * K] = db - ds;
    }
    if (i < K) {
        double gs = 0.0;
        for (int k = 0; k < K; ++k) gs += gamma_v[k];
        Epi[i] = nhp_digamma(gamma_v[i]) - nhp_digamma(gs);
    }
}

// (m·D)[n, l] = Σ_k m[n,k] D[k,l], k increasing: after it a link's network term costs K multiply-adds
__global__ __launch_bounds__(256) void k_sbmvb_md(int N, int K, const double *__restrict__ m, const double *__restrict__ D,
                                                  double *__restrict__ mD)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * K) return;
    const size_t n = i % N, l = i / N;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += m[n + (size_t)k * N] * D[k + l * K];
    mD[i] = s;
}

// U1[p, l] = Σ_{c≠p} ρv[p,c] m[c,l] and U0[p, l] = Σ_{c≠p} (1 - ρv[p,c]) m[c,l], c increasing.  One thread per (p, l) with
// p fastest: a wave reads 64 consecutive p of column c of ρv (ρv is [p, c] column-major) and one m[c, l], so the product
// that walks ρv along its rows is coalesced as it stands and ρvᵀ is never needed.  The diagonal is left out here and
// enters the tables with its own weight.
__global__ __launch_bounds__(256) void k_sbmvb_u(int N, int K, const double *__restrict__ rho, const double *__restrict__ m,
                                                 double *__restrict__ U1, double *__restrict__ U0)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * K) return;
    const size_t p = i % N, l = i / N;
    double u1 = 0.0, u0 = 0.0;
    for (size_t c = 0; c < (size_t)N; ++c) {
        if (c == p) continue;
        const double r = rho[p + c * N], mm = m[c + l * N];
        u1 += r * mm;
        u0 += (1.0 - r) * mm;
    }
    U1[i] = u1; U0[i] = u0;
}

// One workgroup per pair (k, l): αv[k,l] = α + Σ_p m[p,k] (U1[p,l] + δ_kl ρv[p,p]), βv likewise from U0 and 1 - ρv[p,p]
// (ω[p,p,k,l] = m[p,k] δ_kl: a node has one label), and for l = 0 also γv[k] = γ + Σ_p m[p,k].  Thread i adds the nodes
// i, i + 256, ... in increasing order and nhp_block_sum2_n joins the threads in its fixed order; every term is >= 0.
__global__ __launch_bounds__(256) void k_sbmvb_tables(int N, int K, const double *__restrict__ rho, const double *__restrict__ m,
                                                      const double *__restrict__ U1, const double *__restrict__ U0,
                                                      double alpha, double beta, double gamma, double *__restrict__ alpha_v,
                                                      double *__restrict__ beta_v, double *__restrict__ gamma_v)
{
    __shared__ double red[2 * NHP_WAVES];
    const size_t k = blockIdx.x % K, l = blockIdx.x / K;
    double a = 0.0, b = 0.0, g = 0.0;
    for (size_t p = threadIdx.x; p < (size_t)N; p += 256) {
        const double mk = m[p + k * N];
        double u1 = U1[p + l * N], u0 = U0[p + l * N];
        if (k == l) { const double r = rho[p + p * N]; u1 += r; u0 += 1.0 - r; }
        a += mk * u1;
        b += mk * u0;
        g += mk;
    }
    nhp_block_sum2_n<NHP_WAVES>(a, b, red);
    if (threadIdx.x == 0) { alpha_v[blockIdx.x] = alpha + a; beta_v[blockIdx.x] = beta + b; }
    if (l == 0) {
        g = nhp_block_sum_n<NHP_WAVES>(g, red);
        if (threadIdx.x == 0) gamma_v[k] = gamma + g;
    }
}

// The label sweep: sequential coordinate ascent over the nodes 0 .. N-1 in ONE workgroup, each node reading the current m
// of all others.  m lives in LDS as [n][k]; row n and column n of ρv are in LDS too and those of node n + 1 are requested
// into registers before node n's sums start (they do not change during a sweep), so their latency hides behind the sums.
// For node n the 256 threads are dealt as (l, g), l < Kp (the next power of two of K), g < 256/Kp: thread (l, g) adds, over
// the nodes c = g, g + 256/Kp, ... ≠ n in increasing order, the four sums
//   A1[l] = Σ ρv[n,c] m[c,l],  A0[l] = Σ (1 - ρv[n,c]) m[c,l],  B1[l] = Σ ρv[c,n] m[c,l],  B0[l] = Σ (1 - ρv[c,n]) m[c,l]
// fresh from the LDS copy of m (no second table, nothing accumulates from node to node); a butterfly over the lanes of
// equal l, one LDS pass over the four waves in increasing order, and the first K lanes of wave 0 hold
//   s_k = Eπ[k] + ρv[n,n] E1[k,k] + (1 - ρv[n,n]) E0[k,k] + Σ_l (A1[l] E1[k,l] + A0[l] E0[k,l] + B1[l] E1[l,k] + B0[l] E0[l,k]),
// m[n,:] = softmax(s) shifted by its maximum: an entry may underflow to exactly 0, the largest is exp(0) = 1, so the
// normaliser is >= 1 and nothing is NaN.  Every order is fixed: the sweep is reproducible bit for bit.
// `tabs` is ONE block of 4·K² doubles, E1, E0, E1ᵀ, E0ᵀ in that order (sbmvb_bufs::tabs, the only pointer to them that
// is handed out).  TAB: the block is copied to LDS once per sweep, when it fits next to the rest; a score then waits on
// LDS and not, K times in a row, on global loads.
template <int NPT, bool TAB>
__global__ __launch_bounds__(256) void k_sbmvb_sweep(int N, int K, int Kp, const double *__restrict__ rho,
                                                     const double *__restrict__ tabs, const double *__restrict__ Epi,
                                                     double *__restrict__ m)
{
    extern __shared__ double sbmvb_lds[];
    double *ml = sbmvb_lds;                            // m[n*K + k]
    double *row = ml + (size_t)N * K;                  // ρv[n, c] of the current node
    double *col = row + N;                             // ρv[p, n]
    double *wsum = col + N;                            // [(wave*4 + q)*Kp + l]
    double *fin = wsum + SBMVB_WAVES * 4 * Kp;         // [q*Kp + l]
    double *tab = fin + 4 * Kp;                        // TAB: the four tables, K² each
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int l = t & (Kp - 1), g = t / Kp, G = 256 / Kp;
    const int KK = K * K;
    if (TAB)
        for (int i = t; i < 4 * KK; i += 256) tab[i] = tabs[i];
    const double *tb = TAB ? tab : tabs;
    const double *e1 = tb, *e0 = tb + KK, *e1t = tb + 2 * KK, *e0t = tb + 3 * KK;
    for (int i = t; i < N * K; i += 256) ml[(i % N) * K + i / N] = m[i];
    for (int c = t; c < N; c += 256) { row[c] = rho[(size_t)c * N]; col[c] = rho[c]; }
    const double epi = t < K ? Epi[t] : 0.0;           // lane k of wave 0 keeps Eπ[k] for the whole sweep
    __syncthreads();
    for (int n = 0; n < N; ++n) {
        double nr[NPT], nc[NPT];
        if (n + 1 < N) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const int c = t + i * 256;
                if (c < N) { nr[i] = rho[(size_t)(n + 1) + (size_t)c * N]; nc[i] = rho[(size_t)c + (size_t)(n + 1) * N]; }
            }
        }
        double a1 = 0.0, a0 = 0.0, b1 = 0.0, b0 = 0.0;
#pragma unroll 4
        for (int c = g; c < N; c += G) {               // node n itself enters with weight 0: no branch in the loop
            const double mm = (l < K && c != n) ? ml[c * K + l] : 0.0;
            const double r = row[c], q = col[c];
            a1 += r * mm;
            a0 += (1.0 - r) * mm;
            b1 += q * mm;
            b0 += (1.0 - q) * mm;
        }
        const double rnn = row[n];
        for (int off = Kp; off < 64; off <<= 1) {
            a1 += __shfl_xor(a1, off);
            a0 += __shfl_xor(a0, off);
            b1 += __shfl_xor(b1, off);
            b0 += __shfl_xor(b0, off);
        }
        if (lane < Kp) {
            wsum[(w * 4 + 0) * Kp + lane] = a1;
            wsum[(w * 4 + 1) * Kp + lane] = a0;
            wsum[(w * 4 + 2) * Kp + lane] = b1;
            wsum[(w * 4 + 3) * Kp + lane] = b0;
        }
        __syncthreads();                               // every read of row / col for node n is done
        if (n + 1 < N) {
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                const int c = t + i * 256;
                if (c < N) { row[c] = nr[i]; col[c] = nc[i]; }
            }
        }
        if (t < 4 * Kp) {                              // t = q*Kp + l
            double s = 0.0;
            for (int v = 0; v < SBMVB_WAVES; ++v) s += wsum[v * 4 * Kp + t];
            fin[t] = s;
        }
        __syncthreads();
        if (w == 0) {
            double s = -INFINITY;
            if (lane < K) {
                const int k = lane;
                s = epi + (rnn * e1[k + k * K] + (1.0 - rnn) * e0[k + k * K]);
                for (int j = 0; j < K; ++j)
                    s += (fin[j] * e1[k + j * K] + fin[Kp + j] * e0[k + j * K]) +
                         (fin[2 * Kp + j] * e1t[k + j * K] + fin[3 * Kp + j] * e0t[k + j * K]);
            }
            double mx = s;                             // butterflies over the first Kp lanes only: log2(Kp) stages
            for (int off = Kp >> 1; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
            const double e = lane < K ? nhp_exp(s - mx) : 0.0;
            double z = e;
            for (int off = Kp >> 1; off > 0; off >>= 1) z += __shfl_xor(z, off);
            if (lane < K) {
                const double v = e / z;
                ml[n * K + lane] = v;
                m[(size_t)n + (size_t)lane * N] = v;
            }
        }
        __syncthreads();
    }
}

// its device block, after the network run's own (netvb_bufs::end), in the order sbmvb_param_doubles counts it
struct sbmvb_bufs {
    double *m, *av, *bv, *gv, *mh, *avh, *bvh, *gvh, *D, *tabs, *Epi, *mD, *U1, *U0, *rho_hat, *end;
};
static nhp_status sbmvb_launch_sweep(nhp_ctx *ctx, hipStream_t st, const sbmvb_bufs &s, size_t N, size_t K, const double *rho, double *m)
{
    const size_t need = sbmvb_sweep_lds_bytes(N, K), with_tables = need + sbmvb_sweep_table_bytes(K);
    const bool tab = with_tables <= (size_t)SBMVB_LDS_LIMIT;      // the tables ride along when they fit; the limit is `need`
    const size_t lds = tab ? with_tables : need;
    const int Kp = (int)sbmvb_pow2(K);
#define NHP_SBMVB_SWEEP_(npt, tb)                                                                                                    \
    do {                                                                                                                             \
        if (lds > 64 * 1024)                                                                                                         \
            NHP_HIP(ctx, hipFuncSetAttribute((const void *)k_sbmvb_sweep<npt, tb>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL((k_sbmvb_sweep<npt, tb>), dim3(1), dim3(SBMVB_THREADS), lds, st, (int)N, (int)K, Kp, rho, s.tabs, s.Epi, m); \
    } while (0)
#define NHP_SBMVB_SWEEP(npt) do { if (tab) NHP_SBMVB_SWEEP_(npt, true); else NHP_SBMVB_SWEEP_(npt, false); } while (0)
    if (N <= 256) NHP_SBMVB_SWEEP(1);
    else if (N <= 1024) NHP_SBMVB_SWEEP(4);
    else if (N <= 4096) NHP_SBMVB_SWEEP(16);
    else NHP_SBMVB_SWEEP(32);                          // the LDS limit keeps N below 8192
#undef NHP_SBMVB_SWEEP
#undef NHP_SBMVB_SWEEP_
    return NHP_OK;
}

}   // namespace
