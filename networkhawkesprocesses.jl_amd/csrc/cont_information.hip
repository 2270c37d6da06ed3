// Observed information (minus the Hessian of the log-likelihood) and Hessian-vector products of the continuous processes.
//
// The objective separates by child node c, so its Hessian is block diagonal: one block per column over the D = 1 + kinds·N
// parameters [λ0[c]; θ[:,c] | μ[:,c]; τ[:,c]; W[:,c]] (kinds = 2 exponential, 3 logit-normal).  Every integral term is linear
// in the parameters; only Σ_i log λ_i has curvature.  With g_i = 1/λ_i, a = A[p,c] (1 for a standard process), w = W[p,c]
// and u_i = ∂λ_i/∂(column parameters) -- 1 on λ0, a·Σ_{j∈p} ħ_ij on W[p], a·w·Σ_{j∈p} ∂_qħ_ij on impulse parameter q of p --
//
//     J_c = -H_c = Σ_{i on c} g_i²·u_i u_iᵀ  -  Σ_{i on c} g_i·∇²λ_i
//     ∇²λ_i:  (W[p], q[p]) = a·Σ_{j∈p} ∂_qħ        (q[p], q'[p]) = a·w·Σ_{j∈p} ∂²_{qq'}ħ        everything else 0
//
//     exponential   ħ = θe^{-θΔ}:   ∂_θħ = (1 - θΔ)e^{-θΔ}        ∂²_θθħ = -Δ(2 - θΔ)e^{-θΔ}
//     logit-normal  δ = ℓ - μ, ℓ = logit(Δ/Δtmax), counted for 0 < x < 1:
//                   ∂_μħ = ħτδ             ∂_τħ = ħ(1/(2τ) - δ²/2)
//                   ∂²_μμħ = ħ(τ²δ² - τ)   ∂²_μτħ = ħδ(3/2 - τδ²/2)   ∂²_ττħ = ħ((1/(2τ) - δ²/2)² - 1/(2τ²))
//
// Pass A is the log-likelihood launch on the exact 16-byte records, which stores λ_i (nhp_launch_event_intensity_as: the
// Δtmax windows, or the truncated windows of the recursive objective).  Both kernels below revisit each child's window with
// g_i known, on the same records, so every delay is exact.
//
// k_info_blocks: one workgroup per (item, tile), a wave per child.  The wave sums u_i by parent node in its own LDS scratch
// (a list of the parents its window touched keeps that O(window)), turns the touched entries into the rows and the columns
// that fall into the workgroup's tile and adds their g²-scaled products into the tile's accumulator with LDS fp64 adds; the
// curvature sums Σ g·∂ħ, Σ g·∂²ħ are column accumulators as in k_grad_windowed.  A tile is a pair (ta >= tb) of runs of
// `tile_nodes` parent nodes: all parameter kinds of the nodes of ta against those of tb, λ0 with the run that holds parent 0;
// ta == tb keeps a packed lower triangle.  With one run the tile is the whole block.  One flush per workgroup into one
// triangle of the column's block (global fp64 atomics), mirrored by k_info_mirror afterwards, so blocks are exactly symmetric.
//
// k_info_hvp: G lanes per child, two walks of the window: the first sums s_i = u_i·v, the second accumulates per parent node
//     Σ g²s·ħ, Σ g²s·∂_qħ, Σ g·∂_qħ, Σ g·∂²_{qq'}ħ,
// from which the column's entries of H·v follow with the column's constants.  No block is stored.
#include <algorithm>

#include "nhp_internal.h"
#include "nhp_math.h"

namespace {

template <int IMP> struct info_kinds { static constexpr int KI = IMP == NHP_IMPULSE_EXPONENTIAL ? 1 : 2; };

// one pair's impulse value, its first derivatives d[q] and second derivatives dd (exponential: θθ; logit-normal: μμ, μτ, ττ)
struct info_pair {
    double h, d[2], dd[3];
    bool live;
};

// c1 = {θ, -θ·64/ln 2} | {μ, sqrt τ};  c2 = {τ, 1/(2τ)} (logit-normal only)
template <int IMP>
__device__ __forceinline__ info_pair info_eval(double dt, double inv_dtmax, const double2 c1, const double2 c2, const double *etab)
{
    info_pair r;
    if (IMP == NHP_IMPULSE_EXPONENTIAL) {
        const double e = nhp_exp_neg_tab_scaled(c1.y * dt, etab);
        const double td = c1.x * dt;
        r.h = c1.x * e;
        r.d[0] = (1.0 - td) * e;
        r.dd[0] = -(dt * ((2.0 - td) * e));
        r.d[1] = r.dd[1] = r.dd[2] = 0.0;
        r.live = true;
    } else {
        const double x = dt * inv_dtmax;
        r.live = x > 0.0 && x < 1.0;
        r.h = r.d[0] = r.d[1] = r.dd[0] = r.dd[1] = r.dd[2] = 0.0;
        if (r.live) {
            const double o = 1.0 - x, qq = 1.0 / (x * o);
            const double dl = nhp_log((x * x) * qq) - c1.x;
            const double z = dl * c1.y;
            const double h = (nhp_exp_neg(-0.5 * (z * z)) * (NHP_INVSQRT2PI * c1.y)) * qq;
            const double tau = c2.x, i2t = c2.y, hd2 = 0.5 * (dl * dl);
            const double k = i2t - hd2;                          // 1/(2τ) - δ²/2
            r.h = h;
            r.d[0] = h * (tau * dl);
            r.d[1] = h * k;
            r.dd[0] = h * (tau * (tau * (dl * dl) - 1.0));
            r.dd[1] = h * (dl * (1.5 - tau * hd2));
            r.dd[2] = h * (k * k - 2.0 * (i2t * i2t));
        }
    }
    return r;
}

// ---- LDS layout of k_info_blocks, shared by the kernel and its launcher ---------------------------------------------------
struct info_tile {
    int a0, na, szA, b0, nb, szB, diag, accN;
};
__host__ __device__ inline info_tile info_tile_of(int N, int KK, int tn, int ta, int tb)
{
    info_tile t;
    t.a0 = ta * tn; t.na = (t.a0 + tn < N ? t.a0 + tn : N) - t.a0; t.szA = KK * t.na + (ta == 0 ? 1 : 0);
    t.b0 = tb * tn; t.nb = (t.b0 + tn < N ? t.b0 + tn : N) - t.b0; t.szB = KK * t.nb + (tb == 0 ? 1 : 0);
    t.diag = ta == tb;
    t.accN = t.diag ? t.szA * (t.szA + 1) / 2 : t.szA * t.szB;
    return t;
}
// bytes of one wave's scratch: u [KK·N] doubles, row / column values [szA] / [szB], their local indices, flag [N], list [N], 4 counters
__host__ __device__ inline size_t info_wave_bytes(int N, int KK, int szA, int szB)
{
    const size_t b = 8 * (size_t)KK * N + 12 * ((size_t)szA + szB) + 8 * (size_t)N + 16;
    return (b + 15) & ~(size_t)15;
}
constexpr int INFO_WAVES = 4;
// shared part: 64 spare, c1 [N] double2, c2 [N] double2 (logit), scale [N] double2 {a, a·w}, curvature sums [ND·N], exp table
__host__ __device__ inline size_t info_shared_bytes(int N, bool expo)
{
    return 64 + 16 * (size_t)N * (expo ? 2 : 3) + 8 * (size_t)N * (expo ? 2 : 5) + (expo ? 512 : 0);
}
inline size_t info_lds_bytes(int N, bool expo, int tn)
{
    const int KK = expo ? 2 : 3;
    const int nt = (N + tn - 1) / tn;
    // the largest tile: tile 0 carries λ0; off-diagonal rectangles are larger than a triangle
    const info_tile d = info_tile_of(N, KK, tn, 0, 0);
    size_t acc = (size_t)d.accN, sa = (size_t)d.szA, sb = (size_t)d.szB;
    if (nt > 1) { const info_tile r = info_tile_of(N, KK, tn, 1, 0); acc = std::max(acc, (size_t)r.accN); sa = std::max(sa, (size_t)r.szA); }
    return info_shared_bytes(N, expo) + 8 * acc + INFO_WAVES * info_wave_bytes(N, KK, (int)sa, (int)sb);
}

__device__ __forceinline__ int info_global_index(int l, int p0, int n, int KK, int N)
{
    if (l == KK * n) return 0;                                   // λ0, kept behind the tile's nodes
    return 1 + (l / n) * N + p0 + l % n;
}

template <int IMP>
__global__ __launch_bounds__(64 * INFO_WAVES) void k_info_blocks(nhp_cont_args a, const double *__restrict__ lambda,
                                                                  const int32_t *__restrict__ colmap, int tn, double *__restrict__ blocks)
{
    constexpr bool EXPO = IMP == NHP_IMPULSE_EXPONENTIAL;
    constexpr int KI = info_kinds<IMP>::KI, KK = KI + 1, ND = EXPO ? 2 : 5;
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = colmap[c];
    if (slot < 0 || it.kbeg >= it.kend) return;                  // (uniform over the workgroup)
    int ta = 0;
    while ((ta + 1) * (ta + 2) / 2 <= (int)blockIdx.y) ++ta;
    const int tb = (int)blockIdx.y - ta * (ta + 1) / 2;
    const info_tile T = info_tile_of(N, KK, tn, ta, tb);
    const int a1 = T.a0 + T.na, b1 = T.b0 + T.nb;

    extern __shared__ __align__(16) unsigned char smem[];
    double2 *c1 = reinterpret_cast<double2 *>(smem + 64);
    double2 *c2 = c1 + (EXPO ? 0 : N);                           // (exponential: unused, aliases c1)
    double2 *sc = c2 + N;
    double *dacc = reinterpret_cast<double *>(sc + N);           // [ND][N]
    double *etab = dacc + (size_t)ND * N;
    double *acc = etab + (EXPO ? 64 : 0);
    unsigned char *wbase = reinterpret_cast<unsigned char *>(acc + T.accN) + (size_t)wv * info_wave_bytes(N, KK, T.szA, T.szB);
    double *u = reinterpret_cast<double *>(wbase);               // [KK][N]: Σ ħ, Σ ∂_qħ by parent node, this child
    double *rv = u + (size_t)KK * N, *cv = rv + T.szA;           // values of the rows / columns of this child
    int *rl = reinterpret_cast<int *>(cv + T.szB), *cl = rl + T.szA;     // their local indices
    int *flag = cl + T.szB, *list = flag + N, *cnt = list + N;   // touched parents; {touched, rows, columns}

    if (EXPO) nhp_exp_tab_init(etab);
    for (int p = tid; p < N; p += 64 * INFO_WAVES) {
        const size_t k = (size_t)p + (size_t)c * N;
        const double av = a.A ? a.A[k] : 1.0;
        if (EXPO) c1[p] = make_double2(a.p1[k], -(a.p1[k] * 92.33248261689366));
        else {
            c1[p] = make_double2(a.p1[k], __builtin_sqrt(a.p2[k]));
            c2[p] = make_double2(a.p2[k], 0.5 / a.p2[k]);
        }
        sc[p] = make_double2(av, av * a.W[k]);
        for (int q = 0; q < ND; ++q) dacc[(size_t)q * N + p] = 0.0;
    }
    for (int i = tid; i < T.accN; i += 64 * INFO_WAVES) acc[i] = 0.0;
    for (int p = lane; p < N; p += 64) {
        for (int q = 0; q < KK; ++q) u[(size_t)q * N + p] = 0.0;
        flag[p] = 0;
    }
    if (lane < 4) cnt[lane] = 0;
    __syncthreads();

    for (int k = it.kbeg + wv; k < it.kend; k += INFO_WAVES) {
        const nhp_child ch = a.child[k];
        const double g = 1.0 / lambda[ch.idx];
        // ---- u_i by parent node (only the nodes of this tile), the curvature sums of the diagonal tiles
        for (int j = ch.idx - 1 - lane; j >= ch.first; j -= 64) {
            const nhp_event e = a.ev[j];
            const int p = e.node;
            if (!((p >= T.a0 && p < a1) || (p >= T.b0 && p < b1))) continue;
            const info_pair r = info_eval<IMP>(ch.t - e.t, a.inv_dtmax, c1[p], c2[p], etab);
            if (!r.live) continue;
            atomicAdd(&u[p], r.h);
            atomicAdd(&u[N + p], r.d[0]);
            if (!EXPO) atomicAdd(&u[2 * N + p], r.d[1]);
            if (atomicAdd(&flag[p], 1) == 0) list[atomicAdd(&cnt[0], 1)] = p;
            if (T.diag) {
                if (EXPO) {
                    atomicAdd(&dacc[p], g * r.d[0]);
                    atomicAdd(&dacc[N + p], g * r.dd[0]);
                } else {
                    atomicAdd(&dacc[p], g * r.d[0]);
                    atomicAdd(&dacc[N + p], g * r.d[1]);
                    atomicAdd(&dacc[2 * N + p], g * r.dd[0]);
                    atomicAdd(&dacc[3 * N + p], g * r.dd[1]);
                    atomicAdd(&dacc[4 * N + p], g * r.dd[2]);
                }
            }
        }
        NHP_LDS_SYNC();
        const int nt = cnt[0];
        // ---- the child's rows and columns inside the tile: g·u entry by entry (λ0 first, then {W, q...} of every touched parent)
        for (int x = lane; x < 1 + nt * KK; x += 64) {
            double val = g;
            int la = -1, lb = -1;
            if (x == 0) {
                if (ta == 0) la = KK * T.na;
                if (tb == 0) lb = KK * T.nb;
            } else {
                const int t = (x - 1) / KK, s = (x - 1) % KK;
                const int p = list[t];
                const int ks = s == 0 ? KI : s - 1;              // block order: impulse kinds, then W
                val = g * (s == 0 ? sc[p].x * u[p] : sc[p].y * u[(size_t)s * N + p]);
                if (p >= T.a0 && p < a1) la = ks * T.na + (p - T.a0);
                if (p >= T.b0 && p < b1) lb = ks * T.nb + (p - T.b0);
            }
            if (la >= 0) { const int r = atomicAdd(&cnt[1], 1); rv[r] = val; rl[r] = la; }
            if (lb >= 0) { const int r = atomicAdd(&cnt[2], 1); cv[r] = val; cl[r] = lb; }
        }
        NHP_LDS_SYNC();
        const int nA = cnt[1], nB = cnt[2];
        for (int i = lane; i < nA * nB; i += 64) {
            const int r = i / nB, q = i - r * nB;
            const int la = rl[r], lb = cl[q];
            if (T.diag) {
                if (la >= lb) atomicAdd(&acc[la * (la + 1) / 2 + lb], rv[r] * cv[q]);
            } else {
                atomicAdd(&acc[la * T.szB + lb], rv[r] * cv[q]);
            }
        }
        // ---- the scratch back to zero for the wave's next child
        for (int t = lane; t < nt; t += 64) {
            const int p = list[t];
            for (int q = 0; q < KK; ++q) u[(size_t)q * N + p] = 0.0;
            flag[p] = 0;
        }
        if (lane < 4) cnt[lane] = 0;
        NHP_LDS_SYNC();
    }
    __syncthreads();
    if (T.diag) {                                                // - Σ g·∇²λ: inside one parent's own parameters
        for (int pp = tid; pp < T.na; pp += 64 * INFO_WAVES) {
            const int p = T.a0 + pp;
            const double av = sc[p].x, aw = sc[p].y;
            const int lW = KI * T.na + pp, l0 = pp, l1 = T.na + pp;       // W; θ | μ; τ
            if (EXPO) {
                acc[lW * (lW + 1) / 2 + l0] -= av * dacc[p];
                acc[l0 * (l0 + 1) / 2 + l0] -= aw * dacc[N + p];
            } else {
                acc[lW * (lW + 1) / 2 + l0] -= av * dacc[p];
                acc[lW * (lW + 1) / 2 + l1] -= av * dacc[N + p];
                acc[l0 * (l0 + 1) / 2 + l0] -= aw * dacc[2 * N + p];
                acc[l1 * (l1 + 1) / 2 + l0] -= aw * dacc[3 * N + p];
                acc[l1 * (l1 + 1) / 2 + l1] -= aw * dacc[4 * N + p];
            }
        }
        __syncthreads();
    }
    const size_t D = 1 + (size_t)KK * N;
    double *blk = blocks + (size_t)slot * D * D;
    for (int i = tid; i < T.accN; i += 64 * INFO_WAVES) {
        const double v = acc[i];
        if (v == 0.0) continue;
        int la, lb;
        if (T.diag) {
            la = (int)((__builtin_sqrt(8.0 * (double)i + 1.0) - 1.0) * 0.5);
            while ((la + 1) * (la + 2) / 2 <= i) ++la;
            while (la * (la + 1) / 2 > i) --la;
            lb = i - la * (la + 1) / 2;
        } else {
            la = i / T.szB; lb = i - la * T.szB;
        }
        const int gr = info_global_index(la, T.a0, T.na, KK, N), gc = info_global_index(lb, T.b0, T.nb, KK, N);
        // into the upper triangle (column-major): consecutive lanes of a packed row add to consecutive doubles
        const size_t r = gr < gc ? gr : gc, q = gr < gc ? gc : gr;
        atomicAdd(&blk[r + q * D], v);
    }
}

// lower triangle <- upper triangle of every block
__global__ __launch_bounds__(256) void k_info_mirror(double *__restrict__ blocks, size_t D, size_t nblk)
{
    const size_t DD = D * D, total = nblk * DD;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / DD, e = i - b * DD, r = e % D, q = e / D;
        if (r > q) blocks[i] = blocks[b * DD + q + r * D];
    }
}

// ---- Hessian-vector product --------------------------------------------------------------------------------------------
__host__ __device__ inline size_t hvp_lds_bytes(int N, bool expo)
{
    // 64 spare, c1 [N] double2, c2 [N] double2 (logit), a·v by kind [KK][N], the sums [4 | 8][N], the exponential's table
    return 64 + 16 * (size_t)N * (expo ? 1 : 2) + 8 * (size_t)N * (expo ? 2 + 4 : 3 + 8) + (expo ? 512 : 0);
}

template <int IMP, int G>
__global__ __launch_bounds__(256) void k_info_hvp(nhp_cont_args a, const double *__restrict__ lambda, const double *__restrict__ v,
                                                  double *__restrict__ out)
{
    constexpr bool EXPO = IMP == NHP_IMPULSE_EXPONENTIAL;
    constexpr int KI = info_kinds<IMP>::KI, KK = KI + 1, NA = EXPO ? 4 : 8, TH = 256;
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = reinterpret_cast<double *>(smem);
    double2 *c1 = reinterpret_cast<double2 *>(smem + 64);
    double2 *c2 = c1 + (EXPO ? 0 : a.N);
    double *cvv = reinterpret_cast<double *>(c2 + a.N);          // [KK][N]: a·v_W, a·w·v_q
    double *A = cvv + (size_t)KK * a.N;                          // [NA][N]
    double *etab = A + (size_t)NA * a.N;
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N, tid = threadIdx.x;
    const nhp_layout L(a);
    if (EXPO) nhp_exp_tab_init(etab);
    for (int p = tid; p < N; p += TH) {
        const size_t k = (size_t)p + (size_t)c * N;
        const double av = a.A ? a.A[k] : 1.0, aw = av * a.W[k];
        if (EXPO) c1[p] = make_double2(a.p1[k], -(a.p1[k] * 92.33248261689366));
        else {
            c1[p] = make_double2(a.p1[k], __builtin_sqrt(a.p2[k]));
            c2[p] = make_double2(a.p2[k], 0.5 / a.p2[k]);
        }
        cvv[p] = av * v[L.W + k];
        cvv[N + p] = aw * v[L.p1 + k];
        if (!EXPO) cvv[2 * N + p] = aw * v[L.p2 + k];
        for (int q = 0; q < NA; ++q) A[(size_t)q * N + p] = 0.0;
    }
    __syncthreads();
    const double v0 = v[c];
    constexpr int GROUPS = TH / G;
    const int gid = tid / G, gl = tid % G;
    double l0 = 0.0;
    for (int k = it.kbeg + gid; k < it.kend; k += GROUPS) {
        const nhp_child ch = a.child[k];
        const double g = 1.0 / lambda[ch.idx];
        double s = 0.0;
        for (int j = ch.idx - 1 - gl; j >= ch.first; j -= G) {
            const nhp_event e = a.ev[j];
            const int p = e.node;
            const info_pair r = info_eval<IMP>(ch.t - e.t, a.inv_dtmax, c1[p], c2[p], etab);
            if (!r.live) continue;
            s += r.h * cvv[p] + r.d[0] * cvv[N + p];
            if (!EXPO) s += r.d[1] * cvv[2 * N + p];
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        s += v0;
        const double g2s = g * g * s;
        if (gl == 0) l0 -= g2s;
        for (int j = ch.idx - 1 - gl; j >= ch.first; j -= G) {
            const nhp_event e = a.ev[j];
            const int p = e.node;
            const info_pair r = info_eval<IMP>(ch.t - e.t, a.inv_dtmax, c1[p], c2[p], etab);
            if (!r.live) continue;
            if (EXPO) {
                atomicAdd(&A[p], g2s * r.h);
                atomicAdd(&A[N + p], g * r.d[0]);
                atomicAdd(&A[2 * N + p], g2s * r.d[0]);
                atomicAdd(&A[3 * N + p], g * r.dd[0]);
            } else {
                atomicAdd(&A[p], g2s * r.h);
                atomicAdd(&A[N + p], g2s * r.d[0]);
                atomicAdd(&A[2 * N + p], g2s * r.d[1]);
                atomicAdd(&A[3 * N + p], g * r.d[0]);
                atomicAdd(&A[4 * N + p], g * r.d[1]);
                atomicAdd(&A[5 * N + p], g * r.dd[0]);
                atomicAdd(&A[6 * N + p], g * r.dd[1]);
                atomicAdd(&A[7 * N + p], g * r.dd[2]);
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < N; p += TH) {
        const size_t k = (size_t)p + (size_t)c * N;
        const double av = a.A ? a.A[k] : 1.0, w = a.W[k], vW = v[L.W + k];
        if (EXPO) {
            const double vt = v[L.p1 + k];
            const double oW = av * (A[N + p] * vt - A[p]);
            const double ot = av * (vW * A[N + p] + w * (vt * A[3 * N + p] - A[2 * N + p]));
            if (oW != 0.0) atomicAdd(&out[L.W + k], oW);
            if (ot != 0.0) atomicAdd(&out[L.p1 + k], ot);
        } else {
            const double vm = v[L.p1 + k], vt = v[L.p2 + k];
            const double oW = av * ((A[3 * N + p] * vm + A[4 * N + p] * vt) - A[p]);
            const double om = av * (vW * A[3 * N + p] + w * ((vm * A[5 * N + p] + vt * A[6 * N + p]) - A[N + p]));
            const double ot = av * (vW * A[4 * N + p] + w * ((vm * A[6 * N + p] + vt * A[7 * N + p]) - A[2 * N + p]));
            if (oW != 0.0) atomicAdd(&out[L.W + k], oW);
            if (om != 0.0) atomicAdd(&out[L.p1 + k], om);
            if (ot != 0.0) atomicAdd(&out[L.p2 + k], ot);
        }
    }
    const double ls = nhp_block_sum_n<TH / 64>(l0, red);
    if (tid == 0 && ls != 0.0) atomicAdd(&out[c], ls);
}

template <int IMP>
void launch_hvp(int G, dim3 grid, size_t lds, hipStream_t st, const nhp_cont_args &a, const double *lambda, const double *v, double *out)
{
#define NHP_CASE(g)                                                                                                               \
    case g:                                                                                                                       \
        if (lds > 64 * 1024)                                                                                                      \
            (void)hipFuncSetAttribute((const void *)k_info_hvp<IMP, g>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
        hipLaunchKernelGGL((k_info_hvp<IMP, g>), grid, dim3(256), lds, st, a, lambda, v, out);                                    \
        break;
    switch (G) {
        NHP_CASE(1) NHP_CASE(2) NHP_CASE(4) NHP_CASE(8) NHP_CASE(16) NHP_CASE(32)
    default:
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute((const void *)k_info_hvp<IMP, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((k_info_hvp<IMP, 64>), grid, dim3(256), lds, st, a, lambda, v, out);
    }
#undef NHP_CASE
}

// What both entry points refuse, before anything is written; then the windows the objective sums over.
nhp_status info_prepare(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, const char *what,
                        const nhp_child **child, int *group)
{
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) {
        nhp_set_error(ctx, "%s: not available for a LogGaussianCoxProcess baseline", what);
        return NHP_ENOTIMPL;
    }
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "%s: not available on a column shard", what);
        return NHP_ENOTIMPL;
    }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    *child = ds->d_child;
    *group = ds->group;
    if ((flags & NHP_LL_RECURSIVE) && m->impulse_kind == NHP_IMPULSE_EXPONENTIAL) {
        if ((flags & NHP_LL_FULL_RECURSION) && !nhp_multi_trial(ds)) {      // (several trials: the window sum is that recursion)
            nhp_set_error(ctx, "%s: the O(M*N) recursion forms no second derivatives (NHP_LL_FULL_RECURSION)", what);
            return NHP_ENOTIMPL;
        }
        const nhp_child *cut = nullptr;
        int g = 0;
        if (ds->M > 0) {
            NHP_TRY(nhp_recursive_window(ctx, ds, m, &cut, &g, 1e9, true));
            if (!cut) {
                nhp_set_error(ctx, "%s: the recursive objective has no usable truncated window for these parameters "
                                   "(no decay bound, or more than 8192 parents per window); use the windowed form", what);
                return NHP_ENOTIMPL;
            }
            *child = cut;
            *group = g;
        }
    }
    return NHP_OK;
}

// pass A on the exact records: λ_i of every child (-> d_lambda, by event index) and the log-likelihood (-> ctx->d_results[0])
nhp_status info_pass_a(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_child *child, int group,
                       double *d_lambda)
{
    const bool cut = child != ds->d_child;
    // (a child list of the caller's keeps the launch on the 16-byte records: no pair list, no slices)
    NHP_TRY(nhp_launch_event_intensity_as(ctx, ds, m, cut ? child : ds->d_child_w, group, cut ? 0 : 1, d_lambda));
    return nhp_launch_finalize(ctx, nhp_make_args(ds, m), ds->n_items, ctx->d_results);
}

}   // namespace

extern "C" nhp_status nhp_cont_information(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                           const int32_t *columns, int32_t n_columns, int32_t tile_nodes, int32_t on_device,
                                           double *ll, double *blocks)
{
    if (!ctx || !ds || !m || !blocks) return NHP_EINVAL;
    const nhp_child *child = nullptr;
    int group = 0;
    NHP_TRY(info_prepare(ctx, ds, m, flags, "observed_information", &child, &group));
    const int N = ds->N;
    const bool expo = m->impulse_kind == NHP_IMPULSE_EXPONENTIAL;
    const int KK = expo ? 2 : 3;
    std::vector<int32_t> colmap((size_t)N, -1);
    if (!columns) {
        n_columns = N;
        for (int c = 0; c < N; ++c) colmap[c] = c;
    } else {
        if (n_columns <= 0) { nhp_set_error(ctx, "observed_information: n_columns must be positive"); return NHP_EINVAL; }
        for (int i = 0; i < n_columns; ++i) {
            const int32_t c = columns[i];
            if (c < 0 || c >= N || colmap[c] >= 0) {
                nhp_set_error(ctx, "observed_information: column %d (0-based, entry %d) is outside [0, %d) or repeated", c, i, N);
                return NHP_EINVAL;
            }
            colmap[c] = i;
        }
    }
    if (tile_nodes < 0 || tile_nodes > N) {
        nhp_set_error(ctx, "observed_information: tile_nodes = %d must lie in [0, %d] (0: automatic)", tile_nodes, N);
        return NHP_EINVAL;
    }
    const size_t budget = 160 * 1024;
    int tn = tile_nodes;
    if (tn == 0) {                                               // the whole block when it fits, else the largest run that does
        tn = N;
        while (tn > 1 && info_lds_bytes(N, expo, tn) > budget) --tn;
    }
    const size_t lds = info_lds_bytes(N, expo, tn);
    if (lds > budget) {
        nhp_set_error(ctx, "observed_information: n_nodes = %d with tile_nodes = %d needs %zu bytes of LDS, over the 160 KiB budget", N, tn, lds);
        return NHP_ENOTIMPL;
    }
    const int nt = (N + tn - 1) / tn;
    const size_t D = 1 + (size_t)KK * N, nblk = (size_t)n_columns, bytes = 8 * nblk * D * D;
    const size_t M = (size_t)(ds->M > 0 ? ds->M : 1);
    const size_t off_map = 8 * M;
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, off_map + 4 * (size_t)N + 16));
    double *d_blocks = blocks;
    if (!on_device && hipMalloc((void **)&d_blocks, bytes) != hipSuccess) {
        (void)hipGetLastError();
        nhp_set_error(ctx, "observed_information: out of device memory for %zu blocks of %zu x %zu (%zu bytes)", nblk, D, D, bytes);
        return NHP_ENOMEM;
    }
    double *d_lambda = (double *)ctx->d_scratch;
    int32_t *d_map = (int32_t *)((unsigned char *)ctx->d_scratch + off_map);
    hipStream_t st = ctx->main();
    nhp_status rc = NHP_OK;
    auto run = [&]() -> nhp_status {
        NHP_HIP(ctx, hipMemcpyAsync(d_map, colmap.data(), 4 * (size_t)N, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemsetAsync(d_blocks, 0, bytes, st));
        if (ds->M > 0) NHP_TRY(info_pass_a(ctx, ds, m, child, group, d_lambda));
        else NHP_TRY(nhp_launch_windowed(ctx, ds, m, ctx->d_results));   // no event: the integral alone, zero blocks
        nhp_cont_args a = nhp_make_args(ds, m);
        a.child = child;
        const dim3 grid((unsigned)ds->n_items, (unsigned)(nt * (nt + 1) / 2)), block(64 * INFO_WAVES);
        const double *lam = d_lambda;
        const int32_t *map = d_map;
        if (ds->M > 0 && expo) {
            if (lds > 64 * 1024)
                (void)hipFuncSetAttribute((const void *)k_info_blocks<NHP_IMPULSE_EXPONENTIAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL((k_info_blocks<NHP_IMPULSE_EXPONENTIAL>), grid, block, lds, st, a, lam, map, tn, d_blocks);
        } else if (ds->M > 0) {
            if (lds > 64 * 1024)
                (void)hipFuncSetAttribute((const void *)k_info_blocks<NHP_IMPULSE_LOGITNORMAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL((k_info_blocks<NHP_IMPULSE_LOGITNORMAL>), grid, block, lds, st, a, lam, map, tn, d_blocks);
        }
        NHP_HIP(ctx, hipGetLastError());
        const unsigned mb = (unsigned)std::min<size_t>(4096, (nblk * D * D + 255) / 256);
        hipLaunchKernelGGL(k_info_mirror, dim3(mb), dim3(256), 0, st, d_blocks, D, nblk);
        NHP_HIP(ctx, hipGetLastError());
        if (!on_device) NHP_TRY(nhp_download(ctx, blocks, d_blocks, bytes));
        double l = 0.0;
        NHP_TRY(nhp_ctx_fetch(ctx, 0, 1, &l));                   // (synchronises: the colmap vector may go)
        if (ll) *ll = l;
        return NHP_OK;
    };
    rc = run();
    if (!on_device) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(d_blocks);
    }
    return rc;
}

extern "C" nhp_status nhp_cont_hessian_vec(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                           int32_t on_device, const double *v, double *out, int64_t len)
{
    if (!ctx || !ds || !m || !v || !out) return NHP_EINVAL;
    const nhp_child *child = nullptr;
    int group = 0;
    NHP_TRY(info_prepare(ctx, ds, m, flags, "hessian_vector_product", &child, &group));
    const size_t P = nhp_layout(m).P;
    if ((size_t)len != P) {
        nhp_set_error(ctx, "Parameter vector length does not match model parameter length.");
        return NHP_EINVAL;
    }
    const bool expo = m->impulse_kind == NHP_IMPULSE_EXPONENTIAL;
    const size_t lds = hvp_lds_bytes(ds->N, expo);
    if (lds > 160 * 1024) {
        nhp_set_error(ctx, "hessian_vector_product: n_nodes = %d exceeds the 160 KiB LDS budget", ds->N);
        return NHP_ENOTIMPL;
    }
    const size_t M = (size_t)(ds->M > 0 ? ds->M : 1);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (M + 2 * P)));
    double *d_lambda = (double *)ctx->d_scratch, *d_v = d_lambda + M, *d_out = d_v + P;
    hipStream_t st = ctx->main();
    const double *dv = v;
    if (on_device) d_out = out;
    else {
        NHP_HIP(ctx, hipMemcpyAsync(d_v, v, 8 * P, hipMemcpyHostToDevice, st));
        dv = d_v;
    }
    NHP_HIP(ctx, hipMemsetAsync(d_out, 0, 8 * P, st));
    if (ds->M > 0) {                                             // (no event: no curvature, H·v = 0)
        NHP_TRY(info_pass_a(ctx, ds, m, child, group, d_lambda));
        nhp_cont_args a = nhp_make_args(ds, m);
        a.child = child;
        const dim3 grid((unsigned)ds->n_items);
        if (expo) launch_hvp<NHP_IMPULSE_EXPONENTIAL>(group, grid, lds, st, a, d_lambda, dv, d_out);
        else launch_hvp<NHP_IMPULSE_LOGITNORMAL>(group, grid, lds, st, a, d_lambda, dv, d_out);
        NHP_HIP(ctx, hipGetLastError());
    }
    if (!on_device) return nhp_download(ctx, out, d_out, 8 * P);
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}
