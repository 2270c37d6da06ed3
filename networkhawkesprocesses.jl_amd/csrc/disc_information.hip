// Observed and Fisher information of the discrete log-likelihood in mle!'s parameters x = [λ0 (N); vec(η)], η = W∘θ
// (params / params! src/discrete.jl:174-201; the reference has no counterpart), and information-vector products.
//
// The intensity is linear in x:  λ[t,c] = dt·x_tᵀ z_c,  x_t = [1; Ŝ[t,·,·]] (D = 1 + N·B),  z_c = [λ0[c]; η[·,c,·]].  So the
// log-likelihood is concave, minus its Hessian is block diagonal by child node c, and a block is a weighted Gram matrix of
// the convolution that already sits on the device:
//     observed  J_c = dt²·Σ_t (s[t,c]/λ[t,c]²)·x_t x_tᵀ        Fisher  I_c = dt²·Σ_t (1/λ[t,c])·x_t x_tᵀ
// Row 0 of a block is λ0[c], row 1 + k, k = p + b·N (d_conv's column order), is η[p,c,b].
//
// Pass A: λ from the intensity launch of disc.hip, then the weights w[t,c] of the selected columns (k_dinfo_weights) and,
// for the observed kind, each column's list of the 16-bin chunks that hold an event (k_dinfo_chunks: a bin without an event
// has weight exactly 0, so a chunk without one adds nothing and is never loaded).
// k_dinfo_gram: C_c = Xᵀ·diag(w_c)·X on the fp64 matrix cores, X = [1, Ŝ] as T x D with the ones column made in the
// staging (so the λ0 border of a block is one more row and column of the same tiles).  Batched over (column, tile pair
// ta >= tb, T-slab); both operands are k-contiguous (k = t); the B-side tile is multiplied by w as it is staged.  The slab
// partials go to a workspace and k_dinfo_finish sums them in slab order, applies dt² and writes the entry and its mirror
// image: no atomics, so a block has the same bits on every call, and is exactly symmetric.
#include <algorithm>

#include "nhp_internal.h"

typedef double v4d __attribute__((ext_vector_type(4)));

#define DI_MAXF 6                       // 16-row fragments per tile side, at most: tile_rows <= 96
#define DI_NCH 2                        // 16-bin chunks per staged tile
#define DI_BK (16 * DI_NCH)             // bins per staged tile
#define DI_LD (DI_BK + 2)               // row stride of an LDS image: 16 rows x 2 k hit 32 distinct bank pairs
#define DI_UNITS ((DI_MAXF * (DI_MAXF / 2) + 3) / 4)   // fragment pairs a wave owns, at most
#define DI_EPT (16 * DI_MAXF * DI_BK / 256)        // staged elements per thread and operand, at most

namespace {

struct dinfo_args {
    const double *conv;       // Ŝ [T x N·B], t fastest
    const double *w;          // [n_columns][T] weights of the selected columns
    const int32_t *list;      // [n_columns][nchunk]: slab z's chunks from entry z·slab_chunks on; null: every chunk (Fisher)
    const int32_t *cnt;       // [n_columns][nslab] entries of each slab's list
    double *part;             // [nslab][n_columns][npairs][tr·tr] slab partials, tile-local, row fastest
    int64_t T;
    int D, tr, nchunk, nslab, slab_chunks, ncols, npairs;
};

__device__ __forceinline__ void dinfo_pair(int q, int *ta, int *tb)
{
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= q) ++a;
    *ta = a; *tb = q - a * (a + 1) / 2;
}

// w[j][t] for the selected columns: s/λ² (exactly 0 where s = 0) or 1/λ
__global__ __launch_bounds__(256) void k_dinfo_weights(const double *__restrict__ lam, const double *__restrict__ dataT, int64_t T,
                                                       const int32_t *__restrict__ cols, int kind, double *__restrict__ w)
{
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t i = (size_t)t + (size_t)T * cols[blockIdx.y];
    const double l = lam[i], s = dataT[i];
    w[(size_t)t + (size_t)T * blockIdx.y] = kind == 0 ? (s == 0.0 ? 0.0 : s / (l * l)) : 1.0 / l;
}

// The chunk list of (column j, slab z): the 16-bin chunks of the slab that hold an event, ascending -- an order fixed by the
// data.  One wave per (j, z): 64 chunks a round, ballot + prefix count.
__global__ __launch_bounds__(64) void k_dinfo_chunks(const double *__restrict__ dataT, int64_t T, const int32_t *__restrict__ cols,
                                                     int nchunk, int nslab, int slab_chunks, int32_t *__restrict__ list,
                                                     int32_t *__restrict__ cnt)
{
    const int j = blockIdx.x, z = blockIdx.y, lane = threadIdx.x;
    const double *s = dataT + (size_t)T * cols[j];
    const int c0 = z * slab_chunks, c1 = min(nchunk, c0 + slab_chunks);
    int32_t *out = list + (size_t)j * nchunk + c0;
    int n = 0;
    for (int base = c0; base < c1; base += 64) {
        const int ch = base + lane;
        bool any = false;
        if (ch < c1) {
            const int64_t t0 = (int64_t)ch * 16, t1 = t0 + 16 < T ? t0 + 16 : T;
            for (int64_t t = t0; t < t1; ++t) any = any || s[t] != 0.0;
        }
        const unsigned long long m = __ballot(any);
        const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (any) out[pos] = ch;
        n += __popcll(m);
    }
    if (lane == 0) cnt[(size_t)j * nslab + z] = n;
}

// One workgroup = (column j, tile pair (ta, tb), slab z): the tr x tr tile  Σ_t X[t, ta·tr + r]·w[t]·X[t, tb·tr + c]  over
// the slab's chunks.  4 waves; the 16 x 16 fragments of the tile that hold a row and a column of the block are paired
// along the column (one A fragment serves both) and the pairs dealt to the waves in turn, so any tile height that is a
// multiple of 16 keeps the four waves within one pair of each other.  Fragment layout of v_mfma_f64_16x16x4_f64: A[m = lane&15]
// [k = lane>>4], B[k = lane>>4][n = lane&15], C[row = (lane>>4) + 4·reg][col = lane&15].
__global__ __launch_bounds__(256, 2) void k_dinfo_gram(dinfo_args g)          // 2 waves/SIMD: <= 256 VGPR+AGPR
{
    extern __shared__ __align__(16) double dsm[];
    const int tr = g.tr;
    double *As = dsm, *Bs = dsm + (size_t)tr * DI_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kk = lane >> 4;
    const int j = blockIdx.x, q = blockIdx.y, z = blockIdx.z;
    int ta, tb;
    dinfo_pair(q, &ta, &tb);
    const int ra0 = ta * tr, rb0 = tb * tr;
    const int rows_a = min(tr, g.D - ra0), rows_b = min(tr, g.D - rb0);
    const int fa = (rows_a + 15) / 16, fb = (rows_b + 15) / 16, nbp = (fb + 1) / 2, units = fa * nbp;
    const int64_t T = g.T;
    const int c0 = z * g.slab_chunks;
    const int n = g.list ? g.cnt[(size_t)j * g.nslab + z] : min(g.slab_chunks, g.nchunk - c0);
    const int32_t *lst = g.list ? g.list + (size_t)j * g.nchunk + c0 : nullptr;
    const double *wj = g.w + (size_t)j * (size_t)T;

    v4d acc[DI_UNITS][2];
#pragma unroll
    for (int u = 0; u < DI_UNITS; ++u) acc[u][0] = acc[u][1] = (v4d){0.0, 0.0, 0.0, 0.0};

    // staging: element e of a thread is (row = tid/32 + 8e, chunk tid/16 % 2 of the tile, bin tid % 16): at fixed e a wave
    // loads two rows x two chunks of 128 contiguous bytes and writes 2 x 32 consecutive doubles of the image
    const int bin = tid & 15, chs = (tid >> 4) & (DI_NCH - 1), row0 = tid >> 5;
    double sa[DI_EPT], sb[DI_EPT], wv = 0.0;
    auto load = [&](int it) {
        const int ent = it * DI_NCH + chs;
        bool ok = ent < n;
        const int chunk = ok ? (lst ? lst[ent] : c0 + ent) : 0;
        const int64_t t = (int64_t)chunk * 16 + bin;
        ok = ok && t < T;
        wv = ok ? wj[t] : 0.0;
#pragma unroll
        for (int e = 0; e < DI_EPT; ++e) {
            const int row = row0 + 8 * e;
            if (row < tr) {                                       // (rows past the block's last are staged as zeros)
                const int da = ra0 + row, db = rb0 + row;
                sa[e] = ok && row < rows_a ? (da == 0 ? 1.0 : g.conv[(size_t)(da - 1) * (size_t)T + (size_t)t]) : 0.0;
                sb[e] = ok && row < rows_b ? (db == 0 ? 1.0 : g.conv[(size_t)(db - 1) * (size_t)T + (size_t)t]) : 0.0;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int e = 0; e < DI_EPT; ++e) {
            const int row = row0 + 8 * e;
            if (row < tr) {
                As[row * DI_LD + chs * 16 + bin] = sa[e];
                Bs[row * DI_LD + chs * 16 + bin] = sb[e] * wv;
            }
        }
    };

    const int nst = (n + DI_NCH - 1) / DI_NCH;
    if (nst > 0) load(0);
    for (int it = 0; it < nst; ++it) {
        __syncthreads();                                          // the tile before this one has been read by all
        store();
        __syncthreads();
        if (it + 1 < nst) load(it + 1);                           // in flight under the MFMAs
#pragma unroll 1
        for (int ks = 0; ks < DI_BK / 4; ++ks) {
#pragma unroll
            for (int u = 0; u < DI_UNITS; ++u) {
                const int unit = wave + 4 * u;
                if (unit < units) {
                    const int i = unit / nbp, jp = unit - i * nbp;
                    const double a = As[(i * 16 + r16) * DI_LD + ks * 4 + kk];
                    const double b0 = Bs[(jp * 32 + r16) * DI_LD + ks * 4 + kk];
                    acc[u][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[u][0], 0, 0, 0);
                    if (2 * jp + 1 < fb) {
                        const double b1 = Bs[(jp * 32 + 16 + r16) * DI_LD + ks * 4 + kk];
                        acc[u][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[u][1], 0, 0, 0);
                    }
                }
            }
        }
    }

    double *out = g.part + (((size_t)z * g.ncols + j) * g.npairs + q) * (size_t)tr * tr;
#pragma unroll
    for (int u = 0; u < DI_UNITS; ++u) {
        const int unit = wave + 4 * u;
        if (unit < units) {
            const int i = unit / nbp, jp = unit - i * nbp;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (2 * jp + h < fb) {
                    const int col = (2 * jp + h) * 16 + r16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[(size_t)(i * 16 + kk + 4 * r) + (size_t)col * tr] = acc[u][h][r];
                }
            }
        }
    }
}

// blocks[j][dr + D·dc] = blocks[j][dc + D·dr] = dt²·Σ_z part[z][j][q][·]  for dr >= dc: the slabs in order, then the mirror image
__global__ __launch_bounds__(256) void k_dinfo_finish(dinfo_args g, double dt2, double *__restrict__ blocks)
{
#pragma clang fp contract(off)
    const int tr = g.tr, j = blockIdx.x / g.npairs, q = blockIdx.x % g.npairs;
    const int e = blockIdx.y * 256 + threadIdx.x;
    if (e >= tr * tr) return;
    int ta, tb;
    dinfo_pair(q, &ta, &tb);
    const int dr = ta * tr + e % tr, dc = tb * tr + e / tr;
    if (dr >= g.D || dc >= g.D || dr < dc) return;
    const size_t stride = (size_t)g.ncols * g.npairs * tr * tr;
    const double *p = g.part + ((size_t)j * g.npairs + q) * (size_t)tr * tr + e;
    double v = 0.0;
    for (int z = 0; z < g.nslab; ++z) v += p[(size_t)z * stride];
    v *= dt2;
    double *b = blocks + (size_t)j * g.D * g.D;
    b[(size_t)dr + (size_t)g.D * dc] = v;
    b[(size_t)dc + (size_t)g.D * dr] = v;
}

// ---- information-vector product: out = dt·[Σ_t r; Ŝᵀr],  r = w∘u,  u = dt·X·v ----
// v in mle!'s order -> the bump table's layout: E[k + c·K] = v_η[p,c,b]·dt (k = p + b·N), base[c] = v_λ0[c]·dt
__global__ __launch_bounds__(256) void k_dinfo_stage_v(int N, int B, double dt, const double *__restrict__ v, double *__restrict__ E,
                                                       double *__restrict__ base)
{
#pragma clang fp contract(off)
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NN * B) {
        const size_t b = i / NN, pc = i % NN, p = pc % N, c = pc / N;
        E[p + b * N + c * K] = v[N + i] * dt;
    }
    if (i < (size_t)N) base[i] = v[i] * dt;
}

// u <- w(λ, s)·u, every column
__global__ __launch_bounds__(256) void k_dinfo_r(const double *__restrict__ lam, const double *__restrict__ dataT, size_t n, int kind,
                                                 double *__restrict__ u)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double l = lam[i], s = dataT[i];
    const double w = kind == 0 ? (s == 0.0 ? 0.0 : s / (l * l)) : 1.0 / l;
    u[i] = w * u[i];
}

// Σ_t r[t, c]: one workgroup per column, fixed-order block reduction
__global__ __launch_bounds__(256) void k_dinfo_colsum(const double *__restrict__ r, int64_t T, double *__restrict__ out)
{
    __shared__ double red[NHP_WAVES];
    const double *col = r + (size_t)blockIdx.x * (size_t)T;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) s += col[t];
    s = nhp_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_dinfo_hv_finish(int N, int B, int splits, double dt, const double *__restrict__ slabs,
                                                         const double *__restrict__ colsum, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t NN = (size_t)N * N, K = (size_t)N * B;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NN * B) {
        const size_t b = i / NN, pc = i % NN, p = pc % N, c = pc / N, k = p + b * N;
        double g = 0.0;
        for (int z = 0; z < splits; ++z) g += slabs[(size_t)z * K * N + k + c * K];      // fixed order
        out[N + i] = dt * g;
    }
    if (i < (size_t)N) out[i] = dt * colsum[i];
}

bool dinfo_is_device(const void *p)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

nhp_status dinfo_check(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W, const double *theta,
                       double dt, int32_t kind, const char *what)
{
    if (!lambda0) {
        if (ds->d_baseT) { nhp_set_error(ctx, "%s: the LGCP baseline is not covered (homogeneous baseline only)", what); return NHP_ENOTIMPL; }
        nhp_set_error(ctx, "%s: lambda0 is NULL", what);
        return NHP_EINVAL;
    }
    if (!W || !theta) return NHP_EINVAL;
    if (kind != 0 && kind != 1) { nhp_set_error(ctx, "%s: kind = %d must be 0 (observed) or 1 (Fisher)", what, kind); return NHP_EINVAL; }
    if (!(dt > 0.0)) { nhp_set_error(ctx, "%s: dt must be positive", what); return NHP_EDOMAIN; }
    if (!ds->d_conv) { nhp_set_error(ctx, "convolve(process, data) must run before %s", what); return NHP_EINVAL; }
    return NHP_OK;
}

size_t align8(size_t bytes) { return (bytes + 7) / 8; }          // in doubles

}   // namespace

// LDS of one k_dinfo_gram workgroup: the A and the B image of a tile
static size_t dinfo_lds_bytes(int tr) { return 8 * 2 * (size_t)tr * DI_LD; }

extern "C" nhp_status nhp_disc_information(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W,
                                           const double *theta, double dt, int32_t kind, const int32_t *columns, int32_t n_columns,
                                           int32_t tile_rows, int32_t slab_bins, double *ll, double *blocks)
{
    if (!ctx || !ds || !blocks) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(dinfo_check(ctx, ds, lambda0, W, theta, dt, kind, "disc_information"));
    const int N = ds->N, B = ds->B;
    const int64_t T = ds->T;
    const int D = 1 + N * B;
    std::vector<int32_t> cols;
    if (!columns) {
        n_columns = N;
        for (int c = 0; c < N; ++c) cols.push_back(c);
    } else {
        if (n_columns <= 0) { nhp_set_error(ctx, "disc_information: n_columns must be positive"); return NHP_EINVAL; }
        std::vector<char> seen((size_t)N, 0);
        for (int i = 0; i < n_columns; ++i) {
            const int32_t c = columns[i];
            if (c < 0 || c >= N || seen[c]) {
                nhp_set_error(ctx, "disc_information: column %d (0-based, entry %d) is outside [0, %d) or repeated", c, i, N);
                return NHP_EDOMAIN;
            }
            seen[c] = 1;
            cols.push_back(c);
        }
    }
    if (tile_rows < 0 || tile_rows % 16 != 0 || tile_rows > 16 * DI_MAXF) {
        nhp_set_error(ctx, "disc_information: tile_rows = %d must be a multiple of 16 in [0, %d] (0: automatic)", tile_rows, 16 * DI_MAXF);
        return NHP_EINVAL;
    }
    if (slab_bins < 0) { nhp_set_error(ctx, "disc_information: slab_bins = %d must not be negative (0: automatic)", slab_bins); return NHP_EINVAL; }
    // tiles: as few as 96 rows allow, then the smallest multiple of 16 that covers the block with that many
    int tr = tile_rows;
    if (tr == 0) {
        const int nt0 = (D + 16 * DI_MAXF - 1) / (16 * DI_MAXF);
        tr = ((D + nt0 - 1) / nt0 + 15) / 16 * 16;
    }
    const int nt = (D + tr - 1) / tr, npairs = nt * (nt + 1) / 2;
    const int nchunk = (int)((T + 15) / 16);
    // slabs: whole 16-bin chunks.  Automatic: enough of them that the launch has four workgroups per CU, none shorter than
    // 64 chunks (the finish kernel reads every slab's partial of every entry once)
    int slab_chunks;
    if (slab_bins > 0) slab_chunks = (slab_bins + 15) / 16;
    else {
        const int64_t wg = (int64_t)n_columns * npairs;
        const int64_t want = std::max<int64_t>(1, (4 * (int64_t)ctx->cu_count + wg - 1) / wg);
        slab_chunks = (int)std::max<int64_t>(64, (nchunk + want - 1) / want);
    }
    slab_chunks = std::min(slab_chunks, std::max(nchunk, 1));
    const int nslab = (nchunk + slab_chunks - 1) / slab_chunks;
    if ((int64_t)npairs > 65535 || nslab > 65535) {
        nhp_set_error(ctx, "disc_information: %d tile pairs x %d slabs exceed the launch grid; use larger tile_rows / slab_bins", npairs, nslab);
        return NHP_ENOTIMPL;
    }
    const bool on_device = dinfo_is_device(blocks);
    const size_t nblk = (size_t)n_columns, bytes = 8 * nblk * D * D;
    const size_t ws_bytes = 8 * (size_t)nslab * nblk * npairs * tr * tr;
    // scratch behind the bump table: λ [T x N] | w [n_columns x T] | columns | chunk lists | their counts
    const size_t TN = (size_t)T * N;
    const size_t n_w = nblk * (size_t)T, n_cols = align8(4 * nblk), n_list = kind == 0 ? align8(4 * nblk * nchunk) : 0,
                 n_cnt = kind == 0 ? align8(4 * nblk * nslab) : 0;
    double *E, *base, *x;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, nullptr, dt, &E, &base, TN + n_w + n_cols + n_list + n_cnt, &x));
    double *dlam = x, *dw = dlam + TN;
    int32_t *dcols = (int32_t *)(dw + n_w), *dlist = (int32_t *)((double *)dcols + n_cols), *dcnt = (int32_t *)((double *)dlist + n_list);
    double *d_ws = nullptr, *d_blocks = blocks;
    if (hipMalloc((void **)&d_ws, ws_bytes) != hipSuccess) {
        (void)hipGetLastError();
        nhp_set_error(ctx, "disc_information: out of device memory for the split-T workspace of %d slabs x %zu columns x %d tile pairs of %d x %d (%zu bytes)",
                      nslab, nblk, npairs, tr, tr, ws_bytes);
        return NHP_ENOMEM;
    }
    if (!on_device && hipMalloc((void **)&d_blocks, bytes) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d_ws);
        nhp_set_error(ctx, "disc_information: out of device memory for %zu blocks of %d x %d (%zu bytes)", nblk, D, D, bytes);
        return NHP_ENOMEM;
    }
    hipStream_t st = ctx->main();
    auto run = [&]() -> nhp_status {
        NHP_HIP(ctx, hipMemcpyAsync(dcols, cols.data(), 4 * nblk, hipMemcpyHostToDevice, st));
        NHP_TRY(nhp_disc_launch_loglik(ctx, ds, E, base));
        NHP_TRY(nhp_disc_launch_intensity(ctx, ds, E, base, false, dlam));
        hipLaunchKernelGGL(k_dinfo_weights, dim3((unsigned)((T + 255) / 256), (unsigned)n_columns), dim3(256), 0, st, dlam, ds->d_dataT, T,
                           dcols, (int)kind, dw);
        if (kind == 0)
            hipLaunchKernelGGL(k_dinfo_chunks, dim3((unsigned)n_columns, (unsigned)nslab), dim3(64), 0, st, ds->d_dataT, T, dcols, nchunk,
                               nslab, slab_chunks, dlist, dcnt);
        NHP_HIP(ctx, hipGetLastError());
        dinfo_args g{};
        g.conv = ds->d_conv; g.w = dw; g.list = kind == 0 ? dlist : nullptr; g.cnt = kind == 0 ? dcnt : nullptr; g.part = d_ws;
        g.T = T; g.D = D; g.tr = tr; g.nchunk = nchunk; g.nslab = nslab; g.slab_chunks = slab_chunks; g.ncols = n_columns; g.npairs = npairs;
        const size_t lds = dinfo_lds_bytes(tr);
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)k_dinfo_gram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_dinfo_gram, dim3((unsigned)n_columns, (unsigned)npairs, (unsigned)nslab), dim3(256), lds, st, g);
        NHP_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_dinfo_finish, dim3((unsigned)(n_columns * npairs), (unsigned)((tr * tr + 255) / 256)), dim3(256), 0, st, g,
                           dt * dt, d_blocks);
        NHP_HIP(ctx, hipGetLastError());
        if (!on_device) NHP_TRY(nhp_download(ctx, blocks, d_blocks, bytes));
        double l = 0.0;
        NHP_TRY(nhp_ctx_fetch(ctx, 0, 1, &l));                   // (synchronises: the column vector may go)
        if (ll) *ll = l;
        return NHP_OK;
    };
    const nhp_status rc = run();
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_ws);
    if (!on_device) (void)hipFree(d_blocks);
    return rc;
}

extern "C" nhp_status nhp_disc_hessian_vec(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W,
                                           const double *theta, double dt, int32_t kind, const double *v, double *out)
{
    if (!ctx || !ds || !v || !out) return NHP_EINVAL;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(dinfo_check(ctx, ds, lambda0, W, theta, dt, kind, "disc_hessian_vec"));
    const size_t N = (size_t)ds->N, B = (size_t)ds->B, K = N * B, T = (size_t)ds->T, TN = T * N, P = N + N * N * B;
    int splits = 1, k_chunk = 0;
    nhp_disc_gtr_plan(ctx, ds, &splits, &k_chunk);
    // scratch behind the bump table: λ | u, then r [T x N] | E_v [K x N] | base_v [N] | slabs | column sums | v | out
    double *E, *base, *x;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, nullptr, dt, &E, &base, 2 * TN + K * N + N + (size_t)splits * K * N + N + 2 * P, &x));
    double *dlam = x, *du = dlam + TN, *Ev = du + TN, *basev = Ev + K * N, *dslab = basev + N, *dcs = dslab + (size_t)splits * K * N,
           *d_v = dcs + N, *d_out = d_v + P;
    hipStream_t st = ctx->main();
    const bool v_dev = dinfo_is_device(v), out_dev = dinfo_is_device(out);
    const double *dv = v;
    if (!v_dev) {
        NHP_HIP(ctx, hipMemcpyAsync(d_v, v, 8 * P, hipMemcpyHostToDevice, st));
        dv = d_v;
    }
    if (out_dev) d_out = out;
    NHP_TRY(nhp_disc_launch_intensity(ctx, ds, E, base, false, dlam));
    hipLaunchKernelGGL(k_dinfo_stage_v, dim3((unsigned)((N * N * B + 255) / 256)), dim3(256), 0, st, (int)N, (int)B, dt, dv, Ev, basev);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(nhp_disc_launch_intensity(ctx, ds, Ev, basev, false, du));
    hipLaunchKernelGGL(k_dinfo_r, dim3((unsigned)((TN + 255) / 256)), dim3(256), 0, st, dlam, ds->d_dataT, TN, (int)kind, du);
    hipLaunchKernelGGL(k_dinfo_colsum, dim3((unsigned)N), dim3(256), 0, st, du, (int64_t)T, dcs);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(nhp_disc_launch_gtr(ctx, ds, du, splits, k_chunk, dslab));
    hipLaunchKernelGGL(k_dinfo_hv_finish, dim3((unsigned)((N * N * B + 255) / 256)), dim3(256), 0, st, (int)N, (int)B, splits, dt, dslab, dcs,
                       d_out);
    NHP_HIP(ctx, hipGetLastError());
    if (!out_dev) return nhp_download(ctx, out, d_out, 8 * P);
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}
