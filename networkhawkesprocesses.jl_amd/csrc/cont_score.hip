// Scoring a continuous chain on the device (include/nhp.h: nhp_cont_score_*, nhp_cont_model_attach_score).
// The time axis is cut at edges b_0 < ... < b_K; cell (k, c) is node c on [b_k, b_{k+1}) and its log-likelihood under a draw is
//     ℓ_{k,c} = Σ_{events m of c, b_k <= t_m < b_{k+1}} log λ_c(t_m) − (Λ_c(b_{k+1}) − Λ_c(b_k)),
// the density of the block given the past, with λ what nhp_cont_event_intensity evaluates and Λ the compensator of
// nhp_cont_compensator (cont_compensator.hip: strict window, cut exponential, logit-normal mass W·Δtmax, mask A).  The running
// statistics over the kept draws are those of the discrete scorer (disc_score.hip, nhp_score.h): per cell a log-sum-exp and
// Welford's mean and M2 of ℓ, and the same three scalars for Σ ℓ.  A draw is scored in five launches on the main stream:
//   λ[M]             the windowed per-event intensity (nhp_launch_event_intensity), time order
//   k_cscore_tables  W·A, V = W·A·H(Δtmax), θ | μ and √τ ROW-major, so that lanes across the child column read coalesced
//   k_cscore_block   ΔΛ of every (block, column) formed directly, not as a difference of two cumulative values: one workgroup
//                    per (block, tile of 256 columns, part of the block's events).  The events from the first with
//                    t_i > b_k − Δtmax to the last before b_{k+1} go through LDS 256 at a time; per event and column one
//                    gather -- V for an event inside the block whose window ends inside it (these first, eight loads in
//                    flight), else W·A·(H(d2) − H(d1)) with d1 = max(b_k − t_i, 0), d2 = min(b_{k+1} − t_i, Δtmax):
//                    e^{−θ d1}·(−expm1(−θ (d2 − d1))) or a difference of two Φ taken in the tail where both are small.  CDF
//                    work only for events within Δtmax of an edge.
//   k_cont_score     the K x N cells: two binary searches in the node's bucket give the cell's events, Σ nhp_log λ in index
//                    order, the parts of ΔΛ in part order + λ0_c (b_{k+1} − b_k), then the plane update; a partial of Σ ℓ
//                    per workgroup
//   k_score_fold     the joint scalars (nhp_score.h)
// No atomics, no host read, every sum in one fixed order: two runs give the same bits.  Δtmax = ∞ has no saturated part:
// every earlier event is walked, as the windowed routes do.
#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_score.h"
#include <algorithm>
#include <cmath>
#include <vector>

#define CSCORE_COLS 256      // columns per workgroup of k_cscore_block
#define CSCORE_STAGE 256     // events staged through LDS at a time

struct nhp_cont_score {
    nhp_ctx *ctx = nullptr;
    const nhp_cont_dataset *ds = nullptr;      // not owned: must outlive the scorer
    int64_t K = 0;                             // blocks
    int32_t N = 0;
    int64_t count = 0;                         // kept draws
    unsigned bx = 1;                           // workgroups per node column in k_cont_score
    unsigned nsplit = 1;                       // parts a block's events are dealt to in k_cscore_block
    // ONE allocation: lse | mean | M2 [K·N each, k fastest] | partials [bx·N] | joint [8] | col [4N] | tot [16] | edges [K + 1]
    double *d_planes = nullptr, *d_partials = nullptr, *d_joint = nullptr, *d_col = nullptr, *d_tot = nullptr, *d_edges = nullptr;
};

// ---- the row-major tables: WAt[p·N + c] = W·A, Vt = W·A·H(Δtmax), P1t = θ | μ, P2t = √τ (logit-normal; else untouched) ---------
__global__ __launch_bounds__(256) void k_cscore_tables(nhp_cont_args a, double *__restrict__ WAt, double *__restrict__ Vt,
                                                       double *__restrict__ P1t, double *__restrict__ P2t)
{
    __shared__ double tw[32][33], tv[32][33], t1[32][33], t2[32][33];
    const int N = a.N, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const bool ln = a.impulse_kind == NHP_IMPULSE_LOGITNORMAL;
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + tx, c = c0 + r;
        if (p < N && c < N) {
            const size_t k = (size_t)p + (size_t)c * N;
            double w = a.W[k];
            if (a.A) w = a.A[k] * w;
            double v = 0.0;
            if (w != 0.0) {                                               // (the masses of k_comp_tables)
                if (!ln) v = a.dt_max < INFINITY ? w * -expm1(-(a.p1[k] * a.dt_max)) : w;
                else v = w * a.dt_max;
            }
            tw[r][tx] = w; tv[r][tx] = v; t1[r][tx] = a.p1[k];
            if (ln) t2[r][tx] = __builtin_sqrt(a.p2[k]);
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        if (p < N && c < N) {
            const size_t k = (size_t)p * N + c;
            WAt[k] = tw[tx][r]; Vt[k] = tv[tx][r]; P1t[k] = t1[tx][r];
            if (ln) P2t[k] = t2[tx][r];
        }
    }
}

// H(d2) − H(d1) for 0 <= d1 < d2 <= Δtmax, d1 < Δtmax; first = (d1 == 0), last = (d2 == Δtmax) are the same for every column
template <int IMP>
__device__ __forceinline__ double cscore_dH(double p1, double p2, double d1, double d2, double dt_max, bool first, bool last)
{
#pragma clang fp contract(off)
    if (IMP == NHP_IMPULSE_EXPONENTIAL) {
        const double tail = -expm1(-(p1 * (d2 - d1)));
        return first ? tail : exp(-(p1 * d1)) * tail;
    }
    // Φ(z2) − Φ(z1), z = √τ (logit(d / Δtmax) − μ) as comp_H forms it; z1 = −∞ at d1 = 0, z2 = +∞ at d2 = Δtmax.  Both
    // tails are taken on the side where they are small: 0.5 s (erfc(s z1 / √2) − erfc(s z2 / √2)), s = +1 when z1 > 0.
    double z1 = -INFINITY, z2 = INFINITY;
    if (!first) { const double x = d1 / dt_max; z1 = p2 * (log(x / (1.0 - x)) - p1); }
    if (!last) { const double x = d2 / dt_max; z2 = p2 * (log(x / (1.0 - x)) - p1); }
    const double s = z1 > 0.0 ? 0.7071067811865476 : -0.7071067811865476;
    const double h = 0.5 * (erfc(s * z1) - erfc(s * z2));
    return dt_max * (z1 > 0.0 ? h : -h);
}

// first index in [0, M) with times[i] >= x (strict = false) or > x (strict = true)
__device__ __forceinline__ int64_t cscore_bound(const double *__restrict__ times, int64_t M, double x, bool strict)
{
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const double t = times[mid];
        if (strict ? t > x : t >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// grid (K, ceil(N / CSCORE_COLS), nsplit): dLp[(s·N + c)·K + k] = part s of Σ_i W A (H(min(b_{k+1} − t_i, Δtmax)) − H(max(b_k − t_i, 0)))
template <int IMP>
__global__ __launch_bounds__(CSCORE_COLS) void k_cscore_block(const nhp_event *__restrict__ ev, const double *__restrict__ times, int64_t M, int N,
                                                              double dt_max, const double *__restrict__ edges, const double *__restrict__ WAt,
                                                              const double *__restrict__ Vt, const double *__restrict__ P1t,
                                                              const double *__restrict__ P2t, double *__restrict__ dLp, int64_t K)
{
#pragma clang fp contract(off)
    __shared__ double s_t[CSCORE_STAGE];
    __shared__ int32_t s_n[CSCORE_STAGE];
    __shared__ double s_sat[CSCORE_STAGE];         // 1 for an event that gives its saturated mass, else 0
    const int64_t k = blockIdx.x;
    const double b0 = edges[k], b1 = edges[k + 1];
    // the events that reach into the block: t_i > b_k − Δtmax (all of them for Δtmax = ∞) and t_i < b_{k+1}
    const int64_t lo = cscore_bound(times, M, b0 - dt_max, true), hi = cscore_bound(times, M, b1, false);
    const int64_t len = hi - lo, per = (len + gridDim.z - 1) / gridDim.z;
    const int64_t i0 = lo + (int64_t)blockIdx.z * per, i1 = i0 + per < hi ? i0 + per : hi;
    const int c = blockIdx.y * CSCORE_COLS + threadIdx.x;
    const bool active = c < N;
    double acc = 0.0;
    for (int64_t base = i0; base < i1; base += CSCORE_STAGE) {
        __syncthreads();
        const int64_t i = base + threadIdx.x;
        if (i < i1) {
            const nhp_event e = ev[i];
            const double d1r = b0 - e.t, d2r = b1 - e.t;
            s_t[threadIdx.x] = e.t; s_n[threadIdx.x] = e.node;
            // inside the block and the window ends inside it: the saturated mass
            s_sat[threadIdx.x] = d2r > 0.0 && d1r <= 0.0 && !(d2r < dt_max) ? 1.0 : 0.0;
        }
        __syncthreads();
        const int cnt = (int)(i1 - base < CSCORE_STAGE ? i1 - base : CSCORE_STAGE);
        if (!active) continue;
        // the saturated events first: a gather per event, loaded whether used or not (every row is a valid one) and selected
        // afterwards, so that eight loads are in flight; then the few events within Δtmax of an edge
#pragma unroll 8
        for (int e = 0; e < cnt; ++e) {
            const double v = Vt[(size_t)s_n[e] * N + c];
            acc += s_sat[e] != 0.0 ? v : 0.0;
        }
        for (int e = 0; e < cnt; ++e) {
            const double t = s_t[e], d1r = b0 - t, d2r = b1 - t;          // (the same for every lane)
            if (s_sat[e] != 0.0 || !(d2r > 0.0) || !(d1r < dt_max)) continue;
            const size_t row = (size_t)s_n[e] * N + c;
            const bool first = d1r <= 0.0, last = !(d2r < dt_max);
            const double w = WAt[row];
            if (w != 0.0)
                acc += w * cscore_dH<IMP>(P1t[row], IMP == NHP_IMPULSE_LOGITNORMAL ? P2t[row] : 0.0, first ? 0.0 : d1r, last ? dt_max : d2r,
                                          dt_max, first, last);
        }
    }
    if (active) dLp[((size_t)blockIdx.z * N + c) * (size_t)K + k] = acc;
}

// first bucket position in [kb, ke) whose child has t >= x
__device__ __forceinline__ int cscore_child_bound(const nhp_child *__restrict__ child, int kb, int ke, double x)
{
    int lo = kb, hi = ke;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (child[mid].t >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- the pass over the cells --------------------------------------------------------------------------------------------
// grid (bx, N): column c's blocks are dealt to bx workgroups, 256 at a time.  `n` = the kept count including this draw.
__global__ __launch_bounds__(256) void k_cont_score(const nhp_child *__restrict__ child, const int32_t *__restrict__ boff,
                                                    const double *__restrict__ lam, const double *__restrict__ edges,
                                                    const double *__restrict__ lambda0, const double *__restrict__ dLp, int nsplit, int64_t K,
                                                    int64_t KN, double *__restrict__ planes, double n, double *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const size_t c = blockIdx.y, N = gridDim.y;
    const int kb = boff[c], ke = boff[c + 1];
    double *plse = planes + c * (size_t)K, *pmean = plse + KN, *pm2 = pmean + KN;
    const bool first = n == 1.0;
    const double l0 = lambda0[c];
    double acc = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < K; k += (int64_t)gridDim.x * 256) {
        const double b0 = edges[k], b1 = edges[k + 1];
        const int j0 = cscore_child_bound(child, kb, ke, b0), j1 = cscore_child_bound(child, j0, ke, b1);
        double sl = 0.0;
        for (int j = j0; j < j1; ++j) sl += nhp_log(lam[child[j].idx]);
        double dl = 0.0;
        for (int s = 0; s < nsplit; ++s) dl += dLp[((size_t)s * N + c) * (size_t)K + k];
        dl += l0 * (b1 - b0);
        const double ell = sl - dl;
        acc += ell;
        if (first) {
            plse[k] = ell; pmean[k] = ell; pm2[k] = 0.0;
        } else {
            const double mean = pmean[k], d = ell - mean, mean1 = mean + d / n;
            plse[k] = score_lse(plse[k], ell);
            pmean[k] = mean1;
            pm2[k] = pm2[k] + d * (ell - mean1);
        }
    }
    acc = nhp_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x + (size_t)gridDim.x * blockIdx.y] = acc;
}

// ---- fetch ------------------------------------------------------------------------------------------------------------------
// One workgroup per node column, blocks in a fixed order; the two passes of k_disc_score_finalize (no data-only constant here)
template <bool SPREAD>
__global__ __launch_bounds__(256) void k_cont_score_finalize(const double *__restrict__ planes, int64_t K, int64_t KN, double logS, double Sm1,
                                                             double *__restrict__ col, const double *__restrict__ tot,
                                                             double *__restrict__ pointwise)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const size_t c = blockIdx.x, N = gridDim.x;
    const double *plse = planes + c * (size_t)K, *pm2 = plse + 2 * KN;
    const double mean = SPREAD ? tot[3] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t k = threadIdx.x; k < K; k += 256) {
        const double lppd = plse[k] - logS, p = pm2[k] / Sm1, e = lppd - p;
        if (SPREAD) {
            const double d = e - mean;
            a0 += d * d;
        } else {
            if (pointwise) pointwise[c * (size_t)K + k] = e;
            a0 += lppd; a1 += p; a2 += e;
        }
    }
    a0 = nhp_block_sum(a0, red);
    if (SPREAD) {
        if (threadIdx.x == 0) col[3 * N + c] = a0;
        return;
    }
    a1 = nhp_block_sum(a1, red);
    a2 = nhp_block_sum(a2, red);
    if (threadIdx.x == 0) { col[c] = a0; col[N + c] = a1; col[2 * N + c] = a2; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
static nhp_status cscore_check(nhp_ctx *ctx, const nhp_cont_score *sc)
{
    if (!ctx || !sc) return NHP_EINVAL;
    if (sc->ctx != ctx) { nhp_set_error(ctx, "scorer belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    return NHP_OK;
}

static nhp_status cscore_pair_check(nhp_ctx *ctx, const nhp_cont_score *sc, const nhp_cont_model *m)
{
    NHP_TRY(cscore_check(ctx, sc));
    NHP_TRY(nhp_check_pair(ctx, sc->ds, m));
    if (m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) {
        nhp_set_error(ctx, "cont_score: the model has an LGCP baseline; scoring is built for a homogeneous baseline (the draws of the "
                           "baseline's grid values are not scored)");
        return NHP_ENOTIMPL;
    }
    const size_t lds = 192 + (m->impulse_kind == NHP_IMPULSE_EXPONENTIAL ? 16 : 24) * (size_t)sc->N + 512;     // the per-event intensity's columns
    if (lds > 160 * 1024) { nhp_set_error(ctx, "cont_score: n_nodes = %d exceeds the 160 KiB LDS column budget", sc->N); return NHP_ENOTIMPL; }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_score_create(nhp_ctx *ctx, const nhp_cont_dataset *ds, const double *edges, int64_t n_edges, nhp_cont_score **out)
{
    if (!ctx || !ds || !edges || !out) return NHP_EINVAL;
    *out = nullptr;
    if (ds->ctx != ctx) { nhp_set_error(ctx, "dataset belongs to another ctx"); return NHP_EINVAL; }
    if (n_edges < 2) { nhp_set_error(ctx, "cont_score_create: %lld edges; a block needs two", (long long)n_edges); return NHP_EINVAL; }
    for (int64_t k = 0; k < n_edges; ++k) {
        if (!std::isfinite(edges[k]) || edges[k] < 0.0 || edges[k] > ds->duration) {
            nhp_set_error(ctx, "cont_score_create: edge %lld = %g is not inside [0, duration = %g]", (long long)k, edges[k], ds->duration);
            return NHP_EINVAL;
        }
        if (k > 0 && !(edges[k] > edges[k - 1])) {
            nhp_set_error(ctx, "cont_score_create: edges must increase strictly (edge %lld = %g after %g)", (long long)k, edges[k], edges[k - 1]);
            return NHP_EINVAL;
        }
    }
    NHP_ONE_RECORDING(ctx, ds, "cont_score_create", "a block of the stacked clock would straddle trials");
    NHP_WHOLE_DATASET(ctx, ds, "cont_score_create");
    if (ds->N > 65535) { nhp_set_error(ctx, "cont_score_create: N = %d is above 65535 node columns", ds->N); return NHP_ENOTIMPL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_cont_score *sc = new nhp_cont_score;
    const int64_t K = n_edges - 1;
    sc->ctx = ctx; sc->ds = ds; sc->K = K; sc->N = ds->N;
    const size_t N = (size_t)ds->N, KN = (size_t)K * N, ncol = (N + CSCORE_COLS - 1) / CSCORE_COLS;
    sc->bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((K + 255) / 256, std::max<int64_t>(1, 4096 / (int64_t)N)));
    // enough workgroups to fill the device where the blocks are few and long, never parts of fewer than 256 events on average
    const int64_t by_grid = 8192 / (K * (int64_t)ncol), by_len = ds->M / K / 256;
    sc->nsplit = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, std::min(by_grid, by_len)));
    const size_t np = (size_t)sc->bx * N, total = 3 * KN + np + 8 + 4 * N + 16 + (size_t)n_edges;
    if (hipMalloc((void **)&sc->d_planes, sizeof(double) * total) != hipSuccess) {
        (void)hipGetLastError();
        delete sc;
        nhp_set_error(ctx, "out of device memory (score planes: %zu bytes)", sizeof(double) * total);
        return NHP_ENOMEM;
    }
    sc->d_partials = sc->d_planes + 3 * KN; sc->d_joint = sc->d_partials + np; sc->d_col = sc->d_joint + 8;
    sc->d_tot = sc->d_col + 4 * N; sc->d_edges = sc->d_tot + 16;
    hipStream_t st = ctx->main();
    hipError_t e = hipMemsetAsync(sc->d_partials, 0, sizeof(double) * (total - 3 * KN), st);
    if (e == hipSuccess) e = hipMemcpyAsync(sc->d_edges, edges, sizeof(double) * (size_t)n_edges, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                    // `edges` is the caller's
    if (e != hipSuccess) { (void)hipFree(sc->d_planes); delete sc; NHP_HIP(ctx, e); }
    *out = sc;
    return NHP_OK;
}

extern "C" void nhp_cont_score_destroy(nhp_cont_score *sc)
{
    if (!sc) return;
    if (sc->ctx) { (void)hipSetDevice(sc->ctx->device); (void)hipStreamSynchronize(sc->ctx->main()); }
    (void)hipFree(sc->d_planes);
    delete sc;
}

extern "C" nhp_status nhp_cont_score_reset(nhp_ctx *ctx, nhp_cont_score *sc)
{
    NHP_TRY(cscore_check(ctx, sc));
    sc->count = 0;                     // the first draw after this overwrites the planes and the joint scalars
    return NHP_OK;
}

// doubles of context scratch one accumulate stages: λ [M] | W·A, V, θ | μ (, √τ) row-major [N²] each | the parts of ΔΛ [nsplit·K·N]
static size_t cscore_scratch(const nhp_cont_score *sc, const nhp_cont_model *m)
{
    const size_t N = (size_t)sc->N, M = (size_t)std::max<int64_t>(sc->ds->M, 1);
    return M + (m->impulse_kind == NHP_IMPULSE_LOGITNORMAL ? 4 : 3) * N * N + (size_t)sc->nsplit * (size_t)sc->K * N;
}

nhp_status nhp_cont_score_reserve(nhp_ctx *ctx, const nhp_cont_score *sc, const nhp_cont_model *m)
{
    NHP_TRY(cscore_pair_check(ctx, sc, m));
    return nhp_ctx_reserve_scratch(ctx, 8 * cscore_scratch(sc, m));
}

extern "C" nhp_status nhp_cont_score_accumulate(nhp_ctx *ctx, nhp_cont_score *sc, const nhp_cont_model *m)
{
    NHP_TRY(cscore_pair_check(ctx, sc, m));
    const nhp_cont_dataset *ds = sc->ds;
    const bool ln = m->impulse_kind == NHP_IMPULSE_LOGITNORMAL;
    const size_t N = (size_t)sc->N, NN = N * N, M = (size_t)std::max<int64_t>(ds->M, 1);
    const int64_t K = sc->K, KN = K * (int64_t)N;
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * cscore_scratch(sc, m)));
    double *lam = (double *)ctx->d_scratch, *WAt = lam + M, *Vt = WAt + NN, *P1t = Vt + NN, *P2t = P1t + NN, *dLp = P1t + (ln ? 2 : 1) * NN;
    if (ds->M > 0) NHP_TRY(nhp_launch_event_intensity(ctx, ds, m, lam));       // (joins the lanes: everything below is on main)
    else ctx->join_lanes();
    const nhp_cont_args a = nhp_make_args(ds, m);
    hipStream_t st = ctx->main();
    const unsigned nt = (unsigned)((N + 31) / 32), ncol = (unsigned)((N + CSCORE_COLS - 1) / CSCORE_COLS);
    hipLaunchKernelGGL(k_cscore_tables, dim3(nt, nt), dim3(256), 0, st, a, WAt, Vt, P1t, P2t);
    const dim3 grid((unsigned)K, ncol, sc->nsplit);
    if (ln)
        hipLaunchKernelGGL(k_cscore_block<NHP_IMPULSE_LOGITNORMAL>, grid, dim3(CSCORE_COLS), 0, st, (const nhp_event *)ds->d_ev, (const double *)ds->d_times,
                           ds->M, (int)N, ds->dt_max, (const double *)sc->d_edges, (const double *)WAt, (const double *)Vt, (const double *)P1t,
                           (const double *)P2t, dLp, K);
    else
        hipLaunchKernelGGL(k_cscore_block<NHP_IMPULSE_EXPONENTIAL>, grid, dim3(CSCORE_COLS), 0, st, (const nhp_event *)ds->d_ev, (const double *)ds->d_times,
                           ds->M, (int)N, ds->dt_max, (const double *)sc->d_edges, (const double *)WAt, (const double *)Vt, (const double *)P1t,
                           (const double *)P2t, dLp, K);
    const double n = (double)(sc->count + 1);
    hipLaunchKernelGGL(k_cont_score, dim3(sc->bx, (unsigned)N), dim3(256), 0, st, (const nhp_child *)ds->d_child, (const int32_t *)ds->d_boff,
                       (const double *)lam, (const double *)sc->d_edges, (const double *)m->d_lambda0, (const double *)dLp, (int)sc->nsplit, K, KN,
                       sc->d_planes, n, sc->d_partials);
    hipLaunchKernelGGL(k_score_fold, dim3(1), dim3(256), 0, st, (const double *)sc->d_partials, (int64_t)sc->bx * (int64_t)N, n, sc->d_joint);
    NHP_HIP(ctx, hipGetLastError());
    ++sc->count;
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_score_fetch(nhp_ctx *ctx, const nhp_cont_score *sc, double *summary, double *per_node, double *pointwise)
{
    NHP_TRY(cscore_check(ctx, sc));
    if (!summary || !per_node) return NHP_EINVAL;
    if (sc->count < 1) { nhp_set_error(ctx, "cont_score_fetch: nothing accumulated"); return NHP_EINVAL; }
    const int64_t K = sc->K, N = sc->N, KN = K * N;
    double *d_pw = nullptr;
    if (pointwise) {
        NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (size_t)KN));
        d_pw = (double *)ctx->d_scratch;
    }
    const double S = (double)sc->count, logS = std::log(S), cells = (double)KN;
    hipStream_t st = ctx->main();
    hipLaunchKernelGGL(k_cont_score_finalize<false>, dim3((unsigned)N), dim3(256), 0, st, (const double *)sc->d_planes, K, KN, logS, S - 1.0, sc->d_col,
                       (const double *)sc->d_tot, d_pw);
    hipLaunchKernelGGL(k_score_total<0>, dim3(1), dim3(256), 0, st, (const double *)sc->d_col, (int)N, cells, S, logS, (const double *)sc->d_joint,
                       sc->d_tot);
    hipLaunchKernelGGL(k_cont_score_finalize<true>, dim3((unsigned)N), dim3(256), 0, st, (const double *)sc->d_planes, K, KN, logS, S - 1.0, sc->d_col,
                       (const double *)sc->d_tot, (double *)nullptr);
    hipLaunchKernelGGL(k_score_total<1>, dim3(1), dim3(256), 0, st, (const double *)sc->d_col, (int)N, cells, S, logS, (const double *)sc->d_joint,
                       sc->d_tot);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(nhp_download(ctx, summary, sc->d_tot + 4, 10 * sizeof(double)));
    NHP_TRY(nhp_download(ctx, per_node, sc->d_col, 3 * sizeof(double) * (size_t)N));
    if (pointwise) NHP_TRY(nhp_download(ctx, pointwise, d_pw, sizeof(double) * (size_t)KN));
    return NHP_OK;
}

// the running planes as they stand: what the invariants of the definitions are checked on
extern "C" nhp_status nhp_cont_score_fetch_planes(nhp_ctx *ctx, const nhp_cont_score *sc, double *lse, double *mean, double *m2)
{
    NHP_TRY(cscore_check(ctx, sc));
    if (sc->count < 1) { nhp_set_error(ctx, "cont_score_fetch_planes: nothing accumulated"); return NHP_EINVAL; }
    const size_t KN = (size_t)sc->K * (size_t)sc->N;
    if (lse) NHP_TRY(nhp_download(ctx, lse, sc->d_planes, sizeof(double) * KN));
    if (mean) NHP_TRY(nhp_download(ctx, mean, sc->d_planes + KN, sizeof(double) * KN));
    if (m2) NHP_TRY(nhp_download(ctx, m2, sc->d_planes + 2 * KN, sizeof(double) * KN));
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_attach_score(nhp_ctx *ctx, nhp_cont_model *m, nhp_cont_score *sc, int64_t every)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    if (!sc) {                                                   // detach
        for (int k = 0; k < 2; ++k) { m->score[k] = nullptr; m->score_every[k] = 1; m->score_kept[k] = 0; }
        return NHP_OK;
    }
    NHP_TRY(cscore_pair_check(ctx, sc, m));
    if (every < 1) { nhp_set_error(ctx, "attach_score: every must be >= 1"); return NHP_EINVAL; }
    int slot = -1;
    for (int k = 1; k >= 0; --k) if (!m->score[k]) slot = k;
    for (int k = 0; k < 2; ++k) if (m->score[k] == sc) slot = k;
    if (slot < 0) { nhp_set_error(ctx, "attach_score: a model takes at most two scorers"); return NHP_EINVAL; }
    m->score[slot] = sc; m->score_every[slot] = every; m->score_kept[slot] = 0;
    return NHP_OK;
}
