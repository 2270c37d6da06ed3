// Scoring a discrete chain on the device (include/nhp.h: nhp_disc_score_*, nhp_disc_model_attach_score).
// Bin t of node c is Poisson(λ[t,c]) given the past, so the log-likelihood of a draw is a sum over cells and both scores a
// Bayesian fit is compared by -- the predictive log-likelihood of held-out bins, log mean_s p(D | θ_s), and WAIC -- are
// running statistics of the per-cell ℓ = xlogy(s, λ) − λ over the kept draws.  They are kept the way the chain's moments
// are: on the device, streaming, in the pass that keeps a step.  Per scored cell three doubles -- a running log-sum-exp of ℓ
// and Welford's mean and M2 of ℓ -- and for the draw's total over the scored cells the same three as scalars.  A draw is
// scored in four launches on the main stream: the bump table from the model's block, the fp64 GEMM on the scored rows of Ŝ
// with its plain epilogue, k_disc_score over the cells, k_score_fold (nhp_score.h) over the workgroup partials.  No atomics, every
// sum in one fixed order: two runs give the same bits.  The data-only loggamma(s + 1) shifts ℓ by a constant per cell: it
// leaves the variance alone and moves the log-sum-exp by itself, so it is left out of the pass and restored at fetch.
#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_score.h"
#include <algorithm>
#include <cmath>

struct nhp_disc_score {
    nhp_ctx *ctx = nullptr;
    const nhp_disc_dataset *ds = nullptr;      // not owned: must outlive the scorer
    int64_t t0 = 0, R = 0;                     // bins [t0, t0 + R)
    int32_t N = 0;
    int64_t count = 0;                         // kept draws
    unsigned bx = 1;                           // workgroups per node column in k_disc_score
    // ONE allocation: lse | mean | M2 [R·N each, t fastest] | partials [bx·N] | lgcol [N] | joint [8] | col [4N] | tot [16]
    double *d_planes = nullptr, *d_partials = nullptr, *d_lgcol = nullptr, *d_joint = nullptr, *d_col = nullptr, *d_tot = nullptr;
};
// joint: 0 lse, 1 mean, 2 M2 of the draw's total over the scored cells, 3 the latest total, 4 Σ loggamma(s + 1) of the range

// ---- Σ_t loggamma(s + 1) per node over the scored bins (once, at create) --------------------------------------------------
__global__ __launch_bounds__(256) void k_disc_score_lgamma(const double *__restrict__ data, int64_t T, int64_t R, double *__restrict__ lgcol)
{
    __shared__ double red[NHP_WAVES];
    const double *s = data + (size_t)blockIdx.x * (size_t)T;
    double lg = 0.0;
    for (int64_t r = threadIdx.x; r < R; r += 256) {
        const double v = s[r];
        if (v > 1.0) lg += lgamma(v + 1.0);
    }
    lg = nhp_block_sum(lg, red);
    if (threadIdx.x == 0) lgcol[blockIdx.x] = lg;
}

__global__ __launch_bounds__(256) void k_disc_score_lgamma_total(const double *__restrict__ lgcol, int N, double *__restrict__ joint)
{
    __shared__ double red[NHP_WAVES];
    const double s = score_sum(lgcol, N, red);
    if (threadIdx.x == 0) joint[4] = s;
}

// ---- the pass over the cells --------------------------------------------------------------------------------------------
// grid (bx, N): column c's rows are dealt to bx workgroups, 256 at a time.  Per cell 8 bytes of λ, 8 of the count, and a read
// and a write of the three planes: 64 bytes (40 for the first draw, which only writes).  `n` = the kept count including this
// draw, as a double.
__global__ __launch_bounds__(256) void k_disc_score(const double *__restrict__ lam, const double *__restrict__ data, int64_t T, int64_t R,
                                                    int64_t RN, double *__restrict__ planes, double n, double *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const size_t c = blockIdx.y;
    const double *l = lam + c * (size_t)R, *s = data + c * (size_t)T;
    double *plse = planes + c * (size_t)R, *pmean = plse + RN, *pm2 = pmean + RN;
    const bool first = n == 1.0;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += (int64_t)gridDim.x * 256) {
        const double lamv = l[r], sv = s[r];
        const double ell = (sv == 0.0 ? 0.0 : sv * nhp_log(lamv)) - lamv;        // the arithmetic of nhp_disc_loglik
        acc += ell;
        if (first) {
            plse[r] = ell; pmean[r] = ell; pm2[r] = 0.0;
        } else {
            const double mean = pmean[r], d = ell - mean, mean1 = mean + d / n;
            plse[r] = score_lse(plse[r], ell);
            pmean[r] = mean1;
            pm2[r] = pm2[r] + d * (ell - mean1);
        }
    }
    acc = nhp_block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x + (size_t)gridDim.x * blockIdx.y] = acc;
}

// ---- fetch ------------------------------------------------------------------------------------------------------------------
// One workgroup per node column, rows in a fixed order.  SPREAD = false: elpd_i (-> pointwise when asked) and the column's
// Σ lppd_i, Σ p_i, Σ elpd_i -> col[c], col[N + c], col[2N + c].  SPREAD = true: Σ (elpd_i − mean elpd)² -> col[3N + c], the
// mean read from tot[3] (two passes: the sum of squares alone would cancel).
template <bool SPREAD>
__global__ __launch_bounds__(256) void k_disc_score_finalize(const double *__restrict__ planes, const double *__restrict__ data, int64_t T,
                                                             int64_t R, int64_t RN, double logS, double Sm1, double *__restrict__ col,
                                                             const double *__restrict__ tot, double *__restrict__ pointwise)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const size_t c = blockIdx.x, N = gridDim.x;
    const double *plse = planes + c * (size_t)R, *pm2 = plse + 2 * RN, *s = data + c * (size_t)T;
    const double mean = SPREAD ? tot[3] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t r = threadIdx.x; r < R; r += 256) {
        const double sv = s[r], lg = sv > 1.0 ? lgamma(sv + 1.0) : 0.0;
        const double lppd = (plse[r] - logS) - lg, p = pm2[r] / Sm1, e = lppd - p;
        if (SPREAD) {
            const double d = e - mean;
            a0 += d * d;
        } else {
            if (pointwise) pointwise[c * (size_t)R + r] = e;
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
static nhp_status score_check(nhp_ctx *ctx, const nhp_disc_score *sc)
{
    if (!ctx || !sc) return NHP_EINVAL;
    if (sc->ctx != ctx) { nhp_set_error(ctx, "scorer belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    return NHP_OK;
}

static nhp_status score_pair_check(nhp_ctx *ctx, const nhp_disc_score *sc, const nhp_disc_model *m)
{
    NHP_TRY(score_check(ctx, sc));
    if (!m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    if (sc->ds->N != m->N || sc->ds->B != m->B) {
        nhp_set_error(ctx, "the model (N = %d, B = %d) does not match the dataset (N = %d, B = %d)", m->N, m->B, sc->ds->N, sc->ds->B);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_score_create(nhp_ctx *ctx, const nhp_disc_dataset *ds, int64_t t0, int64_t t1, nhp_disc_score **out)
{
    if (!ctx || !ds || !out) return NHP_EINVAL;
    *out = nullptr;
    if (ds->ctx != ctx) { nhp_set_error(ctx, "dataset belongs to another ctx"); return NHP_EINVAL; }
    if (!ds->d_conv) { nhp_set_error(ctx, "disc_score_create: convolve(process, data) must run before a scorer is made"); return NHP_EINVAL; }
    if (!(0 <= t0 && t0 < t1 && t1 <= ds->T)) {
        nhp_set_error(ctx, "disc_score_create: bins [%lld, %lld) must satisfy 0 <= t0 < t1 <= T = %lld", (long long)t0, (long long)t1, (long long)ds->T);
        return NHP_EINVAL;
    }
    if (ds->d_baseT) {
        nhp_set_error(ctx, "disc_score_create: the dataset has an LGCP baseline; scoring is built for a homogeneous baseline (the "
                           "draws of the baseline's grid values are not part of nhp_disc_model)");
        return NHP_ENOTIMPL;
    }
    if (ds->N > 65535) { nhp_set_error(ctx, "disc_score_create: N = %d is above 65535 node columns", ds->N); return NHP_ENOTIMPL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_disc_score *sc = new nhp_disc_score;
    sc->ctx = ctx; sc->ds = ds; sc->t0 = t0; sc->R = t1 - t0; sc->N = ds->N;
    const size_t N = (size_t)ds->N, RN = (size_t)sc->R * N;
    sc->bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((sc->R + 255) / 256, std::max<int64_t>(1, 4096 / (int64_t)N)));
    const size_t np = (size_t)sc->bx * N, total = 3 * RN + np + N + 8 + 4 * N + 16;
    if (hipMalloc((void **)&sc->d_planes, sizeof(double) * total) != hipSuccess) {
        (void)hipGetLastError();
        delete sc;
        nhp_set_error(ctx, "out of device memory (score planes: %zu bytes)", sizeof(double) * total);
        return NHP_ENOMEM;
    }
    sc->d_partials = sc->d_planes + 3 * RN; sc->d_lgcol = sc->d_partials + np; sc->d_joint = sc->d_lgcol + N;
    sc->d_col = sc->d_joint + 8; sc->d_tot = sc->d_col + 4 * N;
    hipStream_t st = ctx->main();
    hipError_t e = hipMemsetAsync(sc->d_partials, 0, sizeof(double) * (total - 3 * RN), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_disc_score_lgamma, dim3((unsigned)N), dim3(256), 0, st, (const double *)(ds->d_dataT + t0), ds->T, sc->R, sc->d_lgcol);
        hipLaunchKernelGGL(k_disc_score_lgamma_total, dim3(1), dim3(256), 0, st, (const double *)sc->d_lgcol, (int)N, sc->d_joint);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { (void)hipFree(sc->d_planes); delete sc; NHP_HIP(ctx, e); }
    *out = sc;
    return NHP_OK;
}

extern "C" void nhp_disc_score_destroy(nhp_disc_score *sc)
{
    if (!sc) return;
    if (sc->ctx) { (void)hipSetDevice(sc->ctx->device); (void)hipStreamSynchronize(sc->ctx->main()); }
    (void)hipFree(sc->d_planes);
    delete sc;
}

extern "C" nhp_status nhp_disc_score_reset(nhp_ctx *ctx, nhp_disc_score *sc)
{
    NHP_TRY(score_check(ctx, sc));
    sc->count = 0;                     // the first draw after this overwrites the planes and the joint scalars
    return NHP_OK;
}

// what nhp_disc_stage_bump reserves for this scorer's accumulate: its own block plus λ of the scored rows
nhp_status nhp_disc_score_reserve(nhp_ctx *ctx, const nhp_disc_score *sc)
{
    NHP_TRY(score_check(ctx, sc));
    const size_t N = (size_t)sc->ds->N, NN = N * N, B = (size_t)sc->ds->B, K = N * B;
    return nhp_ctx_reserve_scratch(ctx, 8 * (K * N + N + N + NN + NN * B + NN + (size_t)sc->R * N));
}

extern "C" nhp_status nhp_disc_score_accumulate(nhp_ctx *ctx, nhp_disc_score *sc, const nhp_disc_model *m)
{
    NHP_TRY(score_pair_check(ctx, sc, m));
    const nhp_disc_dataset *ds = sc->ds;
    const int64_t R = sc->R, RN = R * sc->N;
    double *E, *base, *dlam;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, m->d_lambda0, m->d_W, m->d_theta, m->has_A ? m->d_A : nullptr, m->dt, &E, &base, (size_t)RN, &dlam, 0, true));
    NHP_TRY(nhp_disc_launch_intensity_rows(ctx, ds, E, base, sc->t0, R, dlam));
    const double n = (double)(sc->count + 1);
    hipStream_t st = ctx->main();
    hipLaunchKernelGGL(k_disc_score, dim3(sc->bx, (unsigned)sc->N), dim3(256), 0, st, (const double *)dlam, (const double *)(ds->d_dataT + sc->t0),
                       ds->T, R, RN, sc->d_planes, n, sc->d_partials);
    hipLaunchKernelGGL(k_score_fold, dim3(1), dim3(256), 0, st, (const double *)sc->d_partials, (int64_t)sc->bx * sc->N, n, sc->d_joint);
    NHP_HIP(ctx, hipGetLastError());
    ++sc->count;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_score_fetch(nhp_ctx *ctx, const nhp_disc_score *sc, double *summary, double *per_node, double *pointwise)
{
    NHP_TRY(score_check(ctx, sc));
    if (!summary || !per_node) return NHP_EINVAL;
    if (sc->count < 1) { nhp_set_error(ctx, "disc_score_fetch: nothing accumulated"); return NHP_EINVAL; }
    const nhp_disc_dataset *ds = sc->ds;
    const int64_t R = sc->R, N = sc->N, RN = R * N;
    double *d_pw = nullptr;
    if (pointwise) {
        NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (size_t)RN));
        d_pw = (double *)ctx->d_scratch;
    }
    const double S = (double)sc->count, logS = std::log(S), cells = (double)RN;
    const double *data = ds->d_dataT + sc->t0;
    hipStream_t st = ctx->main();
    hipLaunchKernelGGL(k_disc_score_finalize<false>, dim3((unsigned)N), dim3(256), 0, st, (const double *)sc->d_planes, data, ds->T, R, RN, logS,
                       S - 1.0, sc->d_col, (const double *)sc->d_tot, d_pw);
    hipLaunchKernelGGL(k_score_total<0>, dim3(1), dim3(256), 0, st, (const double *)sc->d_col, (int)N, cells, S, logS,
                       (const double *)sc->d_joint, sc->d_tot);
    hipLaunchKernelGGL(k_disc_score_finalize<true>, dim3((unsigned)N), dim3(256), 0, st, (const double *)sc->d_planes, data, ds->T, R, RN, logS,
                       S - 1.0, sc->d_col, (const double *)sc->d_tot, (double *)nullptr);
    hipLaunchKernelGGL(k_score_total<1>, dim3(1), dim3(256), 0, st, (const double *)sc->d_col, (int)N, cells, S, logS,
                       (const double *)sc->d_joint, sc->d_tot);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(nhp_download(ctx, summary, sc->d_tot + 4, 10 * sizeof(double)));
    NHP_TRY(nhp_download(ctx, per_node, sc->d_col, 3 * sizeof(double) * (size_t)N));
    if (pointwise) NHP_TRY(nhp_download(ctx, pointwise, d_pw, sizeof(double) * (size_t)RN));
    return NHP_OK;
}

// the running planes as they stand (loggamma not restored): what the invariants of the definitions are checked on
extern "C" nhp_status nhp_disc_score_fetch_planes(nhp_ctx *ctx, const nhp_disc_score *sc, double *lse, double *mean, double *m2)
{
    NHP_TRY(score_check(ctx, sc));
    if (sc->count < 1) { nhp_set_error(ctx, "disc_score_fetch_planes: nothing accumulated"); return NHP_EINVAL; }
    const size_t RN = (size_t)sc->R * (size_t)sc->N;
    if (lse) NHP_TRY(nhp_download(ctx, lse, sc->d_planes, sizeof(double) * RN));
    if (mean) NHP_TRY(nhp_download(ctx, mean, sc->d_planes + RN, sizeof(double) * RN));
    if (m2) NHP_TRY(nhp_download(ctx, m2, sc->d_planes + 2 * RN, sizeof(double) * RN));
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_attach_score(nhp_ctx *ctx, nhp_disc_model *m, nhp_disc_score *sc, int64_t every)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    if (!sc) {                                                   // detach
        for (int k = 0; k < 2; ++k) { m->score[k] = nullptr; m->score_every[k] = 1; m->score_kept[k] = 0; }
        return NHP_OK;
    }
    NHP_TRY(score_pair_check(ctx, sc, m));
    if (every < 1) { nhp_set_error(ctx, "attach_score: every must be >= 1"); return NHP_EINVAL; }
    int slot = -1;
    for (int k = 1; k >= 0; --k) if (!m->score[k]) slot = k;
    for (int k = 0; k < 2; ++k) if (m->score[k] == sc) slot = k;
    if (slot < 0) { nhp_set_error(ctx, "attach_score: a model takes at most two scorers"); return NHP_EINVAL; }
    m->score[slot] = sc; m->score_every[slot] = every; m->score_kept[slot] = 0;
    return NHP_OK;
}
