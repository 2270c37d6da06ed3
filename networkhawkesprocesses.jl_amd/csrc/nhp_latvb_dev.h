// Device side of the latent distance network's variational layer (the definition is in include/nhp.h,
// nhp_cont_latvb_run): the link's network term η[p,c] = b - ‖z_p - z_c‖², C = ρv + ρvᵀ, and the monotone ascent of
//   F(z, b) = Σ_pc [ρv η - softplus(η)] - ‖z‖²/(2σ²) - (b - μb)²/(2σb²) = ½ Σ_nj [C[j,n] η_nj - 2 softplus(η_nj)] - ...
// over the positions and the offset: the gradient, the ladder of step sizes along it, the one-workgroup finish that picks a rung,
// and the move.  Positions are N x D column-major (z_n[d] at n + N·d) with the offset behind them: Z = [vec z; b], and G = ∇F has
// the same layout.  No atomics and no host round trip: every sum has one fixed order -- a thread adds its entries in increasing
// order, nhp_block_sum_n joins the threads, and the finish adds the nodes' sums the same way.  Everything has internal linkage.
#pragma once
#include <cmath>

#include "nhp_clatvb.h"
#include "nhp_internal.h"
#include "nhp_math.h"

namespace {

constexpr int LATVB_TILE = 32;                                     // the transpose tile of k_latvb_sym (LDS rows padded by one)

// softplus(η) = max(η, 0) + log1p(exp(-|η|))
__device__ __forceinline__ double latvb_softplus(double eta) { return fmax(eta, 0.0) + log1p(nhp_exp(-fabs(eta))); }

// ‖z_p - z_c‖², d increasing
__device__ __forceinline__ double latvb_dist2(const double *__restrict__ z, size_t N, int D, size_t p, size_t c)
{
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
        const double v = z[p + (size_t)d * N] - z[c + (size_t)d * N];
        d2 += v * v;
    }
    return d2;
}

// A link's network term: what cont_netvb.hip's O(P) pass reads.  A thread handles link p + c·N with p fastest, so z[p, d] is
// read coalesced per d and z[c, d] is one address for (almost) the whole wave; D <= 8 values, no N² table.
struct latvb_link {
    int D;
    const double *Z;                                               // [vec z; b] of the state stepped FROM
};
__device__ __forceinline__ double latvb_eta(const latvb_link &s, size_t N, size_t p, size_t c)
{
    return s.Z[N * (size_t)s.D] - latvb_dist2(s.Z, N, s.D, p, c);
}

// C[i,j] = ρv[i,j] + ρv[j,i], once per step: the ascent reads C alone.  ρv is column-major, so a row of it is strided; both
// tiles (i-block, j-block) and (j-block, i-block) are loaded along their columns, coalesced, and the second is read transposed
// from LDS (rows of 33 doubles: the column read walks banks 2 apart, no conflict inside a half wave).
__global__ __launch_bounds__(256) void k_latvb_sym(int N, const double *__restrict__ rho, double *__restrict__ C)
{
    __shared__ double t1[LATVB_TILE][LATVB_TILE + 1];
    __shared__ double t2[LATVB_TILE][LATVB_TILE + 1];
    const int i0 = blockIdx.x * LATVB_TILE, j0 = blockIdx.y * LATVB_TILE;
    const int tx = threadIdx.x % LATVB_TILE, ty = threadIdx.x / LATVB_TILE;       // ty in 0..7
    for (int r = ty; r < LATVB_TILE; r += 256 / LATVB_TILE) {
        // t1[r][tx] = ρv[i0 + tx, j0 + r];  t2[r][tx] = ρv[j0 + tx, i0 + r]
        t1[r][tx] = (i0 + tx < N && j0 + r < N) ? rho[(size_t)(i0 + tx) + (size_t)(j0 + r) * N] : 0.0;
        t2[r][tx] = (j0 + tx < N && i0 + r < N) ? rho[(size_t)(j0 + tx) + (size_t)(i0 + r) * N] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < LATVB_TILE; r += 256 / LATVB_TILE)
        if (i0 + tx < N && j0 + r < N) C[(size_t)(i0 + tx) + (size_t)(j0 + r) * N] = t1[r][tx] + t2[tx][r];
}

// Workgroup n: with w_j = C[j,n] - 2 s(η_nj) over ALL j (the diagonal has z_n - z_j = 0 and η = b),
//   G[n,d] = -2 Σ_j w_j (z_n[d] - z_j[d]) - z_n[d]/σ²,      hb[n] = Σ_j w_j   (∂F/∂b = ½ Σ_n hb[n] - (b - μb)/σb²: k_latvb_gb).
// Lanes run over j: column n of C and the columns of z load coalesced; z_n is one address for the workgroup.
__global__ __launch_bounds__(256) void k_latvb_grad(int N, int D, double inv_s2, const double *__restrict__ C, const double *__restrict__ Z,
                                                    double *__restrict__ G, double *__restrict__ hb)
{
    __shared__ double red[4];
    const size_t n = blockIdx.x, Ns = (size_t)N;
    const double b = Z[Ns * D];
    double zn[CLATVB_MAX_DIMS], acc[CLATVB_MAX_DIMS], accb = 0.0;
#pragma unroll
    for (int d = 0; d < CLATVB_MAX_DIMS; ++d) { zn[d] = d < D ? Z[n + (size_t)d * Ns] : 0.0; acc[d] = 0.0; }
    for (size_t j = threadIdx.x; j < Ns; j += 256) {
        double dz[CLATVB_MAX_DIMS], d2 = 0.0;
#pragma unroll
        for (int d = 0; d < CLATVB_MAX_DIMS; ++d) {
            dz[d] = d < D ? zn[d] - Z[j + (size_t)d * Ns] : 0.0;
            d2 += dz[d] * dz[d];
        }
        const double w = C[j + n * Ns] - 2.0 * netvb_sigmoid(b - d2);
#pragma unroll
        for (int d = 0; d < CLATVB_MAX_DIMS; ++d) acc[d] += w * dz[d];
        accb += w;
    }
#pragma unroll
    for (int d = 0; d < CLATVB_MAX_DIMS; ++d) {
        if (d < D) {                                               // (uniform)
            const double s = nhp_block_sum_n<4>(acc[d], red);
            if (threadIdx.x == 0) G[n + (size_t)d * Ns] = -2.0 * s - zn[d] * inv_s2;
        }
    }
    accb = nhp_block_sum_n<4>(accb, red);
    if (threadIdx.x == 0) hb[n] = accb;
}

// G[N·D] = ∂F/∂b = ½ Σ_n hb[n] - (b - μb)/σb²; one workgroup, thread i adds the nodes i, i + 256, ... in increasing order
__global__ __launch_bounds__(256) void k_latvb_gb(int N, int D, double mu_b, double inv_sb2, const double *__restrict__ Z,
                                                  const double *__restrict__ hb, double *__restrict__ G)
{
    __shared__ double red[4];
    double v = 0.0;
    for (int n = threadIdx.x; n < N; n += 256) v += hb[n];
    v = nhp_block_sum_n<4>(v, red);
    if (threadIdx.x == 0) G[(size_t)N * D] = 0.5 * v - (Z[(size_t)N * D] - mu_b) * inv_sb2;
}

// the step sizes of one pass: t[0 .. n-1]
struct latvb_steps { int n; double t[CLATVB_SLOTS]; };

// Workgroup n: out[n·stride + r] = Σ_j [C[j,n] η_nj(t_r) - 2 softplus(η_nj(t_r))] over ALL j at the point (z, b) + t_r·G, for every
// step size of `ts` in ONE pass: along the ray ‖Δz + tΔg‖² = a + 2t·bb + t²·c, so a pair costs one (a, bb, c) and ts.n softplus.
// G = NULL: the point itself (every t is taken as 0 and G is not read) -- a state's own link sums.
__global__ __launch_bounds__(256) void k_latvb_ladder(int N, int D, latvb_steps ts, const double *__restrict__ C, const double *__restrict__ Z,
                                                      const double *__restrict__ G, double *__restrict__ out, int stride)
{
    __shared__ double red[4];
    const size_t n = blockIdx.x, Ns = (size_t)N;
    const bool ray = G != nullptr;
    const double b = Z[Ns * D], gb = ray ? G[Ns * D] : 0.0;
    double zn[CLATVB_MAX_DIMS], gn[CLATVB_MAX_DIMS], acc[CLATVB_SLOTS];
#pragma unroll
    for (int d = 0; d < CLATVB_MAX_DIMS; ++d) {
        zn[d] = d < D ? Z[n + (size_t)d * Ns] : 0.0;
        gn[d] = (ray && d < D) ? G[n + (size_t)d * Ns] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < CLATVB_SLOTS; ++r) acc[r] = 0.0;
    for (size_t j = threadIdx.x; j < Ns; j += 256) {
        double a = 0.0, bb = 0.0, c = 0.0;
#pragma unroll
        for (int d = 0; d < CLATVB_MAX_DIMS; ++d) {
            const double dz = d < D ? zn[d] - Z[j + (size_t)d * Ns] : 0.0;
            const double dg = (ray && d < D) ? gn[d] - G[j + (size_t)d * Ns] : 0.0;
            a += dz * dz; bb += dz * dg; c += dg * dg;
        }
        const double cj = C[j + n * Ns];
#pragma unroll
        for (int r = 0; r < CLATVB_SLOTS; ++r) {
            if (r < ts.n) {                                        // (uniform)
                const double t = ray ? ts.t[r] : 0.0;
                const double eta = (b + t * gb) - (a + t * (2.0 * bb + t * c));
                acc[r] += cj * eta - 2.0 * latvb_softplus(eta);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CLATVB_SLOTS; ++r) {
        if (r < ts.n) {
            const double s = nhp_block_sum_n<4>(acc[r], red);
            if (threadIdx.x == 0) out[n * (size_t)stride + r] = s;
        }
    }
}

struct latvb_prior { double inv_s2, mu_b, inv_sb2; };             // 1/σ², μb, 1/σb²

// One workgroup.  F at every slot r of `ts` (the last slot is the current point, t = 0):
//   F_r = ½ Σ_n lad[n·stride + r] - (Σz² + 2t Σz·g + t² Σg²)/(2σ²) - (b + t·gb - μb)²/(2σb²),
// the sums over nodes and over the N·D positions in the fixed order of k_latvb_gb.  The best of the rungs r < ts.n - 1, the lowest
// index on ties, is taken if it EXCEEDS the current F; otherwise the point stays.  sc = [t taken (0: stays), its rung (-1: stays),
// F_0 .. F_{n-1}]; rung (nullable) receives the rung's index as a double.  G = NULL: every t is taken as 0 (F of the point itself).
__global__ __launch_bounds__(256) void k_latvb_finish(int N, int D, latvb_steps ts, latvb_prior pr, const double *__restrict__ lad,
                                                      int stride, const double *__restrict__ Z, const double *__restrict__ G,
                                                      double *__restrict__ sc, double *__restrict__ rung)
{
    __shared__ double red[4];
    __shared__ double S[CLATVB_SLOTS];
    const size_t ND = (size_t)N * D;
    for (int r = 0; r < ts.n; ++r) {
        double v = 0.0;
        for (int n = threadIdx.x; n < N; n += 256) v += lad[(size_t)n * stride + r];
        v = nhp_block_sum_n<4>(v, red);
        if (threadIdx.x == 0) S[r] = 0.5 * v;
    }
    double zz = 0.0, zg = 0.0, gg = 0.0;
    for (size_t i = threadIdx.x; i < ND; i += 256) {
        const double z = Z[i], g = G ? G[i] : 0.0;
        zz += z * z; zg += z * g; gg += g * g;
    }
    zz = nhp_block_sum_n<4>(zz, red);
    zg = nhp_block_sum_n<4>(zg, red);
    gg = nhp_block_sum_n<4>(gg, red);
    if (threadIdx.x == 0) {
        const double b = Z[ND], gb = G ? G[ND] : 0.0;
        int best = -1;
        double fbest = 0.0;
        for (int r = 0; r < ts.n; ++r) {
            const double t = G ? ts.t[r] : 0.0, db = (b + t * gb) - pr.mu_b;
            const double f = (S[r] - 0.5 * pr.inv_s2 * (zz + t * (2.0 * zg + t * gg))) - 0.5 * pr.inv_sb2 * (db * db);
            sc[2 + r] = f;
            if (r < ts.n - 1 && (best < 0 || f > fbest)) { best = r; fbest = f; }
            if (r == ts.n - 1 && !(best >= 0 && fbest > f)) best = -1;           // the last slot is the current point
        }
        sc[0] = best >= 0 ? ts.t[best] : 0.0;
        sc[1] = (double)best;
        if (rung) *rung = (double)best;
    }
}

// (z, b) += t·G with the t the finish left in sc[0]; t = 0 leaves every bit as it is
__global__ __launch_bounds__(256) void k_latvb_apply(size_t n, const double *__restrict__ sc, const double *__restrict__ G, double *__restrict__ Z)
{
    const double t = sc[0];
    if (t == 0.0) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) Z[i] += t * G[i];
}

}   // namespace
