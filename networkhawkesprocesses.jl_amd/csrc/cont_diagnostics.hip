// Streaming convergence diagnostics of a device-resident chain (include/nhp.h: nhp_cont_model_diagnostics_*).
// A chain at the sizes this library is built for keeps no samples, only Σx and Σx² (cont_sampler.hip: k_moments); effective
// sample size, Monte-Carlo standard error and split R-hat need three more running planes (batch sum, Σ and Σ² of the batch
// means) and two snapshots of the sums.  k_diag_accumulate makes the moments' pass and these updates in ONE launch per kept
// step -- same expressions and bits for Σx, Σx² -- and the finalize kernels turn the planes into per-entry values and one
// summary per parameter group, once per chain.  The planes, the snapshots and the finalize serve the discrete chain too
// (nhp_diag.h; disc_chain.hip brings its own accumulate kernel, since its source of x differs).
#include "nhp_diag.h"
#include <algorithm>
#include <math.h>

// every expression below is the one include/nhp.h writes down, operation by operation (the tests hold it to a numpy
// restatement): no contraction.  The one fused multiply-add is explicit: Σx² += x·x, as the moments kernel compiles it.
#pragma clang fp contract(off)

// ---- the fused accumulate ----------------------------------------------------------------------------------------------
// Streaming: per entry one read of x and a read + write of Σx, Σx², B (7 planes; 11 on a batch boundary, which adds SB and
// QB), nothing reused; at most 2048 workgroups stride over the entries.  Accesses stay at 8 bytes per lane: the planes of
// the sums start at multiples of len and the A seam sits at P, so with an odd len or P no pairing of entries is 16-byte
// aligned in every plane, and where it is (P and len even) a 16-byte variant measured the same within the spread of the
// runs -- the kernel moves its plane count at the rate k_moments moves its own.
template <bool BOUNDARY>
__global__ __launch_bounds__(256) void k_diag_accumulate(const double *__restrict__ params, int64_t P, const double *__restrict__ A,
                                                         int64_t len, double *__restrict__ mom, double *__restrict__ bat, double b,
                                                         double *__restrict__ rho, double *__restrict__ rd)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        const double x = i < P ? params[i] : A[i - P];
        double s1 = mom[i], s2 = mom[len + i], B = bat[i], SB = 0.0, QB = 0.0;
        if (BOUNDARY) { SB = bat[len + i]; QB = bat[2 * len + i]; }
        diag_update<BOUNDARY>(x, s1, s2, B, SB, QB, b);
        mom[i] = s1; mom[len + i] = s2; bat[i] = B;
        if (BOUNDARY) { bat[len + i] = SB; bat[2 * len + i] = QB; }
    }
    if (rho && blockIdx.x == 0 && threadIdx.x == 0) diag_rho<BOUNDARY>(rho, rd, b);
}

// ---- planes and snapshots: shared by the two models (nhp_diag.h) -------------------------------------------------------
void nhp_diag_release(nhp_diag_state **pd)
{
    if (!*pd) return;
    (void)hipFree((*pd)->d_bat);
    delete *pd;
    *pd = nullptr;
}

void nhp_diag_free(nhp_cont_model *m) { nhp_diag_release(&m->diag); }

static int64_t diag_model_len(const nhp_cont_model *m)
{
    return (int64_t)nhp_layout(m).P + (m->has_A ? (int64_t)m->N * m->N : 0);
}

// (re)allocate the planes for `len` entries; on failure diagnostics are off and the moments untouched
static nhp_status diag_fit(nhp_ctx *ctx, nhp_diag_state **pd, int64_t len)
{
    nhp_diag_state *d = *pd;
    if (d->d_bat && d->len == len) return NHP_OK;
    if (d->d_bat) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); (void)hipFree(d->d_bat); d->d_bat = nullptr; }
    d->len = len;
    const size_t n = (3 + 2 * (size_t)d->nsnap) * (size_t)len + 8;
    if (hipMalloc((void **)&d->d_bat, sizeof(double) * n) != hipSuccess) {
        (void)hipGetLastError();
        nhp_diag_release(pd);
        nhp_set_error(ctx, "out of device memory (convergence diagnostics): diagnostics are off, the moments are kept");
        return NHP_ENOMEM;
    }
    d->d_snap = d->d_bat + 3 * (size_t)len;
    d->d_rho = d->d_snap + (size_t)d->nsnap * 2 * (size_t)len;
    return NHP_OK;
}

nhp_status nhp_diag_zero(nhp_ctx *ctx, nhp_diag_state **pd, int64_t len)
{
    NHP_TRY(diag_fit(ctx, pd, len));
    nhp_diag_state *d = *pd;
    const size_t n = (3 + 2 * (size_t)d->nsnap) * (size_t)d->len + 8;
    NHP_HIP(ctx, hipMemsetAsync(d->d_bat, 0, sizeof(double) * n, ctx->main()));
    d->count = 0;
    return NHP_OK;
}

nhp_status nhp_diag_advance(nhp_ctx *ctx, nhp_diag_state *d, const nhp_diag_sums &s)
{
    const int64_t len = d->len;
    hipStream_t st = ctx->main();
    ++d->count;
    // the halves of split R-hat: (Σx, Σx²) as they stand after h and after n_planned − h kept steps, device to device
    for (int k = 0; k < d->nsnap; ++k) {
        if (d->count != (k == 0 ? d->h : d->planned - d->h)) continue;
        NHP_HIP(ctx, hipMemcpyAsync(d->d_snap + (size_t)k * 2 * (size_t)len, s.d_mom, sizeof(double) * 2 * (size_t)len,
                                    hipMemcpyDeviceToDevice, st));
        if (s.d_rho) NHP_HIP(ctx, hipMemcpyAsync(d->d_rho + 3 + 2 * k, s.d_rho + 1, 2 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return NHP_OK;
}

nhp_status nhp_diag_configure(nhp_ctx *ctx, nhp_diag_state **pd, int64_t len, int64_t batch_len, int64_t n_planned)
{
    if (batch_len == 0 && n_planned == 0) {
        if (*pd) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); nhp_diag_release(pd); }
        return NHP_OK;
    }
    if (batch_len < 1 || n_planned < 0) { nhp_set_error(ctx, "diagnostics: batch_len must be >= 1 and n_planned >= 0 (0, 0 turns them off)"); return NHP_EINVAL; }
    const int64_t h = n_planned / 2;
    const int nsnap = h < 2 ? 0 : (n_planned % 2 == 0 ? 1 : 2);
    if (*pd && (*pd)->nsnap != nsnap) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); nhp_diag_release(pd); }
    if (!*pd) *pd = new nhp_diag_state;
    nhp_diag_state *d = *pd;
    d->b = batch_len; d->planned = n_planned; d->h = h; d->nsnap = nsnap;
    return nhp_diag_zero(ctx, pd, len);
}

// ---- the continuous model's share --------------------------------------------------------------------------------------
nhp_status nhp_diag_reset(nhp_ctx *ctx, nhp_cont_model *m)
{
    return nhp_diag_zero(ctx, &m->diag, m->mom_len > 0 ? m->mom_len : diag_model_len(m));
}

nhp_status nhp_diag_accumulate(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_diag_state *d = m->diag;
    if (d->len != m->mom_len) { nhp_set_error(ctx, "diagnostics: the model's sums changed their length (nhp_cont_model_moments_reset)"); return NHP_EINVAL; }
    const int64_t len = d->len, P = (int64_t)nhp_layout(m).P;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((len + 255) / 256, 2048));
    const double *A = m->has_A ? m->d_A : nullptr;
    hipLaunchKernelGGL(nhp_diag_boundary(d) ? k_diag_accumulate<true> : k_diag_accumulate<false>, dim3(blocks), dim3(256), 0, ctx->main(),
                       (const double *)m->d_params, P, A, len, m->d_mom, d->d_bat, (double)d->b, m->d_rho, d->d_rho);
    NHP_HIP(ctx, hipGetLastError());
    return nhp_diag_advance(ctx, d, nhp_diag_sums{m->d_mom, m->mom_len, m->mom_count, m->d_rho});
}

extern "C" nhp_status nhp_cont_model_diagnostics_configure(nhp_ctx *ctx, nhp_cont_model *m, int64_t batch_len, int64_t n_planned)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    if ((batch_len != 0 || n_planned != 0) && batch_len >= 1 && n_planned >= 0 && m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) {
        nhp_set_error(ctx, "diagnostics: homogeneous baseline only");
        return NHP_ENOTIMPL;
    }
    return nhp_diag_configure(ctx, &m->diag, m->mom_len > 0 ? m->mom_len : diag_model_len(m), batch_len, n_planned);
}

// ---- finalize: per-entry values and one summary per group, once per chain ----------------------------------------------
struct diag_consts {
    double n, a, b, h;          // kept steps, whole batches, batch length, half length (as doubles)
    int split;                  // n = n_planned and h >= 2: split R-hat is defined
    double ess_below, rhat_above;
};
struct diag_value { double ess, mcse, rhat; bool undefined; };

__host__ __device__ __forceinline__ double diag_pos(double v) { return v > 0.0 ? v : 0.0; }

__device__ __forceinline__ diag_value diag_entry(const diag_consts &k, double S1, double S2, double SB, double QB, double A1, double A2,
                                                 double B1, double B2)
{
    const double nan = __builtin_nan("");
    diag_value v;
    const double s2 = diag_pos(S2 - S1 * S1 / k.n) / (k.n - 1.0);
    const double sbm = k.a >= 2.0 ? k.b * diag_pos(QB - SB * SB / k.a) / (k.a - 1.0) : nan;
    v.mcse = sqrt(sbm / k.n);
    v.ess = s2 == 0.0 ? nan : k.n * s2 / sbm;
    v.rhat = nan;
    if (k.split) {
        const double m1 = A1 / k.h, v1 = diag_pos(A2 - A1 * A1 / k.h) / (k.h - 1.0);
        const double c1 = S1 - B1, c2 = S2 - B2;
        const double m2 = c1 / k.h, v2 = diag_pos(c2 - c1 * c1 / k.h) / (k.h - 1.0);
        const double W = (v1 + v2) / 2.0, dm = m1 - m2;
        if (W != 0.0) v.rhat = sqrt((k.h - 1.0) / k.h + dm * dm / (2.0 * W));
    }
    v.undefined = s2 == 0.0;
    return v;
}

// what a thread, a workgroup and then a group know: extremes with their entry (index −1 and value NaN: none yet) and
// counts, every number a double that holds an integer or a copy of an entry's value -- merging is exact in any order, and
// the order is fixed anyway
struct diag_part { double undefined, min_ess, min_at, max_rhat, max_at, below, above, max_mcse; };
#define NHP_DIAG_PART 8

__device__ __forceinline__ diag_part diag_part_empty()
{
    const double nan = __builtin_nan("");
    return diag_part{0.0, nan, -1.0, nan, -1.0, 0.0, 0.0, nan};
}

__device__ __forceinline__ void diag_part_add(diag_part &p, const diag_consts &k, const diag_value &v, double at)
{
    if (v.undefined) { p.undefined += 1.0; return; }
    if (v.ess == v.ess) {
        if (p.min_at < 0.0 || v.ess < p.min_ess || (v.ess == p.min_ess && at < p.min_at)) { p.min_ess = v.ess; p.min_at = at; }
        if (v.ess < k.ess_below) p.below += 1.0;
    }
    if (v.rhat == v.rhat) {
        if (p.max_at < 0.0 || v.rhat > p.max_rhat || (v.rhat == p.max_rhat && at < p.max_at)) { p.max_rhat = v.rhat; p.max_at = at; }
        if (v.rhat > k.rhat_above) p.above += 1.0;
    }
    if (v.mcse == v.mcse && !(p.max_mcse >= v.mcse)) p.max_mcse = v.mcse;
}

__device__ __forceinline__ void diag_part_merge(diag_part &p, const diag_part &o)
{
    p.undefined += o.undefined; p.below += o.below; p.above += o.above;
    if (o.min_at >= 0.0 && (p.min_at < 0.0 || o.min_ess < p.min_ess || (o.min_ess == p.min_ess && o.min_at < p.min_at))) { p.min_ess = o.min_ess; p.min_at = o.min_at; }
    if (o.max_at >= 0.0 && (p.max_at < 0.0 || o.max_rhat > p.max_rhat || (o.max_rhat == p.max_rhat && o.max_at < p.max_at))) { p.max_rhat = o.max_rhat; p.max_at = o.max_at; }
    if (o.max_mcse == o.max_mcse && !(p.max_mcse >= o.max_mcse)) p.max_mcse = o.max_mcse;
}

// grid (nb, 5): workgroup (x, g) takes entries x·256 + t, + nb·256, ... of group g; its partial goes to parts[g·nb + x]
__global__ __launch_bounds__(256) void k_diag_entries(nhp_diag_groups G, diag_consts k, int64_t len, const double *__restrict__ mom,
                                                      const double *__restrict__ bat, const double *__restrict__ snapA,
                                                      const double *__restrict__ snapB, double *__restrict__ ess, double *__restrict__ mcse,
                                                      double *__restrict__ rhat, diag_part *__restrict__ parts)
{
    __shared__ diag_part sh[256];
    const int g = blockIdx.y;
    const int64_t first = G.start[g], n = G.end[g] - first;
    diag_part p = diag_part_empty();
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t i = first + e;
        double A1 = 0.0, A2 = 0.0, B1 = 0.0, B2 = 0.0;
        if (k.split) { A1 = snapA[i]; A2 = snapA[len + i]; B1 = snapB[i]; B2 = snapB[len + i]; }
        const diag_value v = diag_entry(k, mom[i], mom[len + i], bat[len + i], bat[2 * len + i], A1, A2, B1, B2);
        if (ess) ess[i] = v.ess;
        if (mcse) mcse[i] = v.mcse;
        if (rhat) rhat[i] = v.rhat;
        diag_part_add(p, k, v, (double)e);
    }
    sh[threadIdx.x] = p;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { diag_part q = sh[threadIdx.x]; diag_part_merge(q, sh[threadIdx.x + s]); sh[threadIdx.x] = q; }
        __syncthreads();
    }
    if (threadIdx.x == 0) parts[(size_t)g * gridDim.x + blockIdx.x] = sh[0];
}

// one workgroup: thread g < 5 merges its group's partials by index; thread 5 is ρ's single entry (snap_b: where its second
// snapshot sits in rd -- 5, or 3 when one snapshot serves both halves)
__global__ __launch_bounds__(64) void k_diag_summary(nhp_diag_groups G, diag_consts k, int nb, const diag_part *__restrict__ parts,
                                                     const double *__restrict__ rho, const double *__restrict__ rd, int snap_b,
                                                     double *__restrict__ summary)
{
    const int g = threadIdx.x;
    if (g >= NHP_DIAG_GROUPS) return;
    diag_part p = diag_part_empty();
    double entries = 0.0;
    if (g < NHP_DIAG_GROUPS - 1) {
        entries = (double)(G.end[g] - G.start[g]);
        for (int x = 0; x < nb; ++x) diag_part_merge(p, parts[(size_t)g * nb + x]);
    } else if (rho) {
        entries = 1.0;
        diag_part_add(p, k, diag_entry(k, rho[1], rho[2], rd[1], rd[2], rd[3], rd[4], rd[snap_b], rd[snap_b + 1]), 0.0);
    }
    double *s = summary + g * NHP_DIAG_FIELDS;
    s[0] = entries; s[1] = p.undefined; s[2] = p.min_ess; s[3] = p.min_at; s[4] = p.max_rhat; s[5] = p.max_at;
    s[6] = p.below; s[7] = p.above; s[8] = p.max_mcse;
}

nhp_status nhp_diag_finalize(nhp_ctx *ctx, const nhp_diag_state *d, const nhp_diag_sums &sums, const nhp_diag_groups &G, int nb,
                             bool with_rho, double ess_below, double rhat_above, double *summary, double *ess, double *mcse,
                             double *rhat, int64_t len)
{
    if (!d) { nhp_set_error(ctx, "diagnostics: nothing configured (nhp_cont_model_diagnostics_configure / nhp_disc_model_diagnostics_configure)"); return NHP_EINVAL; }
    if (!sums.d_mom || sums.count < 1) { nhp_set_error(ctx, "diagnostics: nothing accumulated"); return NHP_EINVAL; }
    if (d->count != sums.count) {
        nhp_set_error(ctx, "diagnostics: configured after %lld of the sums' %lld steps (configure before the first kept step, or reset the moments)",
                      (long long)(sums.count - d->count), (long long)sums.count);
        return NHP_EINVAL;
    }
    if (len != sums.len || len != d->len) { nhp_set_error(ctx, "Parameter vector length does not match model parameter length."); return NHP_ESHAPE; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    diag_consts k;
    k.n = (double)d->count; k.a = (double)(d->count / d->b); k.b = (double)d->b; k.h = (double)d->h;
    k.split = d->count == d->planned && d->nsnap > 0 ? 1 : 0;
    k.ess_below = ess_below; k.rhat_above = rhat_above;
    // scratch: summary [GROUPS·FIELDS] | partials [5·nb] | ess, mcse, rhat [len] each as asked for
    const size_t head = NHP_DIAG_GROUPS * NHP_DIAG_FIELDS + (size_t)(NHP_DIAG_GROUPS - 1) * nb * NHP_DIAG_PART;
    const int planes = (ess ? 1 : 0) + (mcse ? 1 : 0) + (rhat ? 1 : 0);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, sizeof(double) * (head + (size_t)planes * (size_t)len)));
    double *d_summary = (double *)ctx->d_scratch;
    diag_part *d_parts = (diag_part *)(d_summary + NHP_DIAG_GROUPS * NHP_DIAG_FIELDS);
    double *next = d_summary + head;
    double *d_ess = nullptr, *d_mcse = nullptr, *d_rhat = nullptr;
    if (ess) { d_ess = next; next += len; }
    if (mcse) { d_mcse = next; next += len; }
    if (rhat) { d_rhat = next; next += len; }
    const double *snapA = d->nsnap > 0 ? d->d_snap : nullptr;
    const double *snapB = d->nsnap > 1 ? d->d_snap + 2 * (size_t)len : snapA;
    hipStream_t st = ctx->main();
    hipLaunchKernelGGL(k_diag_entries, dim3(nb, NHP_DIAG_GROUPS - 1), dim3(256), 0, st, G, k, len, (const double *)sums.d_mom,
                       (const double *)d->d_bat, snapA, snapB, d_ess, d_mcse, d_rhat, d_parts);
    NHP_HIP(ctx, hipGetLastError());
    const double *rho = with_rho ? sums.d_rho : nullptr;
    hipLaunchKernelGGL(k_diag_summary, dim3(1), dim3(64), 0, st, G, k, nb, (const diag_part *)d_parts, rho, (const double *)d->d_rho,
                       d->nsnap > 1 ? 5 : 3, d_summary);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(nhp_download(ctx, summary, d_summary, sizeof(double) * NHP_DIAG_GROUPS * NHP_DIAG_FIELDS));
    if (ess) NHP_TRY(nhp_download(ctx, ess, d_ess, sizeof(double) * (size_t)len));
    if (mcse) NHP_TRY(nhp_download(ctx, mcse, d_mcse, sizeof(double) * (size_t)len));
    if (rhat) NHP_TRY(nhp_download(ctx, rhat, d_rhat, sizeof(double) * (size_t)len));
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_model_diagnostics_fetch(nhp_ctx *ctx, const nhp_cont_model *m, double ess_below, double rhat_above,
                                                       double *summary, double *ess, double *mcse, double *rhat, int64_t len)
{
    if (!ctx || !m || !summary) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    const nhp_layout L(m);
    const int64_t NN = (int64_t)m->N * m->N;
    nhp_diag_groups G;                  // λ0 | θ or μ | τ | W | vec(A), one after the other
    const int64_t cut[NHP_DIAG_GROUPS] = {0, (int64_t)L.p1, (int64_t)L.p2, (int64_t)L.W, (int64_t)L.P, m->mom_len};
    for (int g = 0; g < NHP_DIAG_GROUPS - 1; ++g) { G.start[g] = cut[g]; G.end[g] = cut[g + 1]; }
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((std::max<int64_t>(NN, m->N) + 255) / 256, 256));
    return nhp_diag_finalize(ctx, m->diag, nhp_diag_sums{m->d_mom, m->mom_len, m->mom_count, m->d_rho}, G, nb,
                             m->d_rho && !m->sbm && !m->latent, ess_below, rhat_above, summary, ess, mcse, rhat, len);
}
