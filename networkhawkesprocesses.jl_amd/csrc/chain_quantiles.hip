// Streaming quantiles of a device-resident chain (include/nhp.h: nhp_cont_model_quantiles_*, nhp_disc_model_quantiles_*;
// DESIGN 3.28).  A chain at the sizes this library is built for keeps no samples, and the moments and diagnostics say how
// the chain moved, not where the posterior lies: a credible interval of a skewed Gamma or of a spike-and-slab weight needs
// quantiles.  The extended P² algorithm keeps K = 2m + 3 markers per entry (heights and positions) and moves them with every
// value it sees; k_quant_update does that for every entry once per fed step, as a launch of its own AFTER the accumulate
// pass, whose kernels and bits stay as they are.
#include "nhp_quant.h"
#include <algorithm>
#include <math.h>

// every expression is the one include/nhp.h writes down, operation by operation (the tests hold the kernel to a numpy
// restatement bit for bit): no contraction
#pragma clang fp contract(off)

// ---- the update -----------------------------------------------------------------------------------------------------------
// Streaming: per entry one read of x (two for a product) and a read + write of K heights and K − 2 positions in planes
// [K][S] fp64 and [K − 2][S] int32, S = P + 1 -- 8 and 4 bytes per lane, coalesced, nothing reused; at most 2048 workgroups
// stride over the entries, as the accumulate kernels do.  n, the values seen so far, is the host's counter: the warm-up
// (n < K) is a uniform branch.  The scalar ρ's state is entry P, fed by one lane.
template <int M, class SRC>
__global__ __launch_bounds__(256) void k_quant_update(SRC src, int64_t P, double *__restrict__ q, int32_t *__restrict__ pos, int64_t S,
                                                      int32_t n, nhp_quant_probs D, const double *__restrict__ rho)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256)
        quant_feed<M>(src(i), q, pos, S, i, n, D);
    if (rho && blockIdx.x == 0 && threadIdx.x == 0) quant_feed<M>(rho[0], q, pos, S, P, n, D);
}

template <class SRC>
static nhp_status quant_launch(nhp_ctx *ctx, nhp_quant_state *s, const SRC &src, const double *rho)
{
    if (s->count >= INT32_MAX) { nhp_set_error(ctx, "quantiles: the positions are int32 and have run out"); return NHP_EINVAL; }
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((s->P + 255) / 256, 2048));
    const int64_t S = s->P + 1;
    const int32_t n = (int32_t)s->count;
    hipStream_t st = ctx->main();
    switch (s->m) {
    case 1: hipLaunchKernelGGL((k_quant_update<1, SRC>), dim3(blocks), dim3(256), 0, st, src, s->P, s->d_q, s->d_pos, S, n, s->d, rho); break;
    case 2: hipLaunchKernelGGL((k_quant_update<2, SRC>), dim3(blocks), dim3(256), 0, st, src, s->P, s->d_q, s->d_pos, S, n, s->d, rho); break;
    case 3: hipLaunchKernelGGL((k_quant_update<3, SRC>), dim3(blocks), dim3(256), 0, st, src, s->P, s->d_q, s->d_pos, S, n, s->d, rho); break;
    default: hipLaunchKernelGGL((k_quant_update<4, SRC>), dim3(blocks), dim3(256), 0, st, src, s->P, s->d_q, s->d_pos, S, n, s->d, rho); break;
    }
    NHP_HIP(ctx, hipGetLastError());
    ++s->count;
    return NHP_OK;
}

// ---- the planes -------------------------------------------------------------------------------------------------------------
void nhp_quant_release(nhp_quant_state **ps)
{
    if (!*ps) return;
    (void)hipFree((*ps)->d_q);
    delete *ps;
    *ps = nullptr;
}

static size_t quant_bytes(const nhp_quant_state *s)
{
    const size_t K = 2 * (size_t)s->m + 3, S = (size_t)s->P + 1;
    return K * S * sizeof(double) + (K - 2) * S * sizeof(int32_t);
}

// fit the planes to (len, P) and zero them and the counters; on failure quantiles are off, everything else untouched
static nhp_status quant_zero(nhp_ctx *ctx, nhp_quant_state **ps, int64_t len, int64_t P)
{
    nhp_quant_state *s = *ps;
    if (s->d_q && s->P != P) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); (void)hipFree(s->d_q); s->d_q = nullptr; }
    s->len = len; s->P = P;
    if (!s->d_q) {
        if (hipMalloc((void **)&s->d_q, quant_bytes(s)) != hipSuccess) {
            (void)hipGetLastError();
            s->d_q = nullptr;
            nhp_quant_release(ps);
            nhp_set_error(ctx, "out of device memory (streaming quantiles): quantiles are off, the moments and diagnostics are kept");
            return NHP_ENOMEM;
        }
        s->d_pos = reinterpret_cast<int32_t *>(s->d_q + (2 * (size_t)s->m + 3) * ((size_t)P + 1));
    }
    NHP_HIP(ctx, hipMemsetAsync(s->d_q, 0, quant_bytes(s), ctx->main()));
    s->count = 0; s->kept = 0;
    return NHP_OK;
}

static nhp_status quant_configure(nhp_ctx *ctx, nhp_quant_state **ps, int64_t len, int64_t P, const double *probs, int32_t m, int32_t every,
                                  int32_t effective)
{
    if (m == 0) {
        if (*ps) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); nhp_quant_release(ps); }
        return NHP_OK;
    }
    if (m < 0 || m > NHP_QUANT_MAX || !probs) { nhp_set_error(ctx, "quantiles: between 1 and %d probabilities (0 turns them off)", NHP_QUANT_MAX); return NHP_EINVAL; }
    if (every < 1) { nhp_set_error(ctx, "quantiles: every must be >= 1"); return NHP_EINVAL; }
    for (int j = 0; j < m; ++j)
        if (!(probs[j] > (j ? probs[j - 1] : 0.0) && probs[j] < 1.0)) {
            nhp_set_error(ctx, "quantiles: the probabilities must increase strictly inside (0, 1)");
            return NHP_EINVAL;
        }
    if (*ps) { NHP_HIP(ctx, hipStreamSynchronize(ctx->main())); nhp_quant_release(ps); }      // another m: other planes
    nhp_quant_state *s = *ps = new nhp_quant_state;
    s->m = m; s->every = every; s->effective = effective ? 1 : 0;
    // d_{2j} = p_j, d_{2j+1} = (p_j + p_{j+1})/2 with p_0 = 0, p_{m+1} = 1
    for (int j = 0; j <= m; ++j) {
        const double lo = j ? probs[j - 1] : 0.0, hi = j < m ? probs[j] : 1.0;
        s->d.d[2 * j] = lo;
        s->d.d[2 * j + 1] = (lo + hi) / 2.0;
        if (j < m) s->probs[j] = probs[j];
    }
    s->d.d[2 * m + 2] = 1.0;
    for (int i = 2 * m + 3; i < NHP_QUANT_KMAX; ++i) s->d.d[i] = 0.0;
    return quant_zero(ctx, ps, len, P);
}

// values [m][len], min, max [len], rho [m + 2]: rows of the height planes as they stand; NaN where there is no state
static nhp_status quant_fetch(nhp_ctx *ctx, const nhp_quant_state *s, bool with_rho, double *values, double *mn, double *mx, double *rho,
                              int64_t len, int64_t *count)
{
    if (!s) { nhp_set_error(ctx, "quantiles: nothing configured (nhp_cont_model_quantiles_configure / nhp_disc_model_quantiles_configure)"); return NHP_EINVAL; }
    if (len != s->len) { nhp_set_error(ctx, "Parameter vector length does not match model parameter length."); return NHP_ESHAPE; }
    const double nan = __builtin_nan("");
    const int K = 2 * s->m + 3;
    const size_t S = (size_t)s->P + 1, P = (size_t)s->P;
    const int64_t n = s->count;
    *count = n;
    // (row of the planes, destination, its ρ slot): the estimates need n >= K, the extremes n >= 1
    for (int j = 0; j < s->m + 2; ++j) {
        double *dst = j < s->m ? values + (size_t)j * (size_t)len : (j == s->m ? mn : mx);
        const bool defined = j < s->m ? n >= K : n >= 1;
        const int64_t row = j < s->m ? 2 * (j + 1) : (j == s->m ? 0 : std::min<int64_t>(n, K) - 1);
        if (rho) rho[j] = nan;
        if (dst) std::fill(dst, dst + len, nan);
        if (!defined) continue;
        if (dst) NHP_TRY(nhp_download(ctx, dst, s->d_q + (size_t)row * S, sizeof(double) * P));
        if (rho && with_rho) NHP_TRY(nhp_download(ctx, rho + j, s->d_q + (size_t)row * S + P, sizeof(double)));
    }
    return NHP_OK;
}

// ---- the continuous model ----------------------------------------------------------------------------------------------------
static nhp_status cont_check(nhp_ctx *ctx, const nhp_cont_model *m)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    return NHP_OK;
}

static int64_t cont_sums_len(const nhp_cont_model *m)
{
    return (int64_t)nhp_layout(m).P + (m->has_A ? (int64_t)m->N * m->N : 0);
}

static bool cont_scalar_rho(const nhp_cont_model *m) { return m->d_rho && !m->sbm && !m->latent; }

nhp_status nhp_quant_reset(nhp_ctx *ctx, nhp_cont_model *m)
{
    return quant_zero(ctx, &m->quant, cont_sums_len(m), (int64_t)nhp_layout(m).P);
}

extern "C" nhp_status nhp_cont_model_quantiles_configure(nhp_ctx *ctx, nhp_cont_model *m, const double *probs, int32_t n_probs, int32_t every,
                                                         int32_t effective_weights)
{
    NHP_TRY(cont_check(ctx, m));
    if (n_probs != 0 && m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) { nhp_set_error(ctx, "quantiles: homogeneous baseline only"); return NHP_ENOTIMPL; }
    return quant_configure(ctx, &m->quant, cont_sums_len(m), (int64_t)nhp_layout(m).P, probs, n_probs, every, effective_weights);
}

extern "C" nhp_status nhp_cont_model_quantiles_accumulate(nhp_ctx *ctx, nhp_cont_model *m)
{
    NHP_TRY(cont_check(ctx, m));
    nhp_quant_state *s = m->quant;
    if (!s) { nhp_set_error(ctx, "quantiles: nothing configured (nhp_cont_model_quantiles_configure)"); return NHP_EINVAL; }
    const nhp_layout L(m);
    if (s->P != (int64_t)L.P || s->len != cont_sums_len(m)) { nhp_set_error(ctx, "quantiles: the model's entries changed (nhp_cont_model_moments_reset)"); return NHP_EINVAL; }
    const quant_src_cont src{m->d_params, s->effective && m->has_A ? m->d_A : nullptr, (int64_t)L.W};
    return quant_launch(ctx, s, src, cont_scalar_rho(m) ? m->d_rho : nullptr);
}

nhp_status nhp_quant_kept_step(nhp_ctx *ctx, nhp_cont_model *m)
{
    nhp_quant_state *s = m->quant;
    const bool feed = s->kept % s->every == 0;
    ++s->kept;
    return feed ? nhp_cont_model_quantiles_accumulate(ctx, m) : NHP_OK;
}

extern "C" nhp_status nhp_cont_model_quantiles_fetch(nhp_ctx *ctx, const nhp_cont_model *m, double *values, double *mn, double *mx, double *rho,
                                                     int64_t len, int64_t *count)
{
    NHP_TRY(cont_check(ctx, m));
    if (!values || !count) return NHP_EINVAL;
    return quant_fetch(ctx, m->quant, cont_scalar_rho(m), values, mn, mx, rho, len, count);
}

// ---- the discrete model --------------------------------------------------------------------------------------------------------
static nhp_status disc_check(nhp_ctx *ctx, const nhp_disc_model *m)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    return NHP_OK;
}

// entries with a state, and the sums' length: the block without vec(A) | [λ0; vec(W∘θ)]
static int64_t disc_entries(const nhp_disc_model *m)
{
    const int64_t N = m->N, NN = N * N;
    return m->has_A ? N + NN + NN * m->B : N + NN * m->B;
}

static int64_t disc_sums_len(const nhp_disc_model *m) { return disc_entries(m) + (m->has_A ? (int64_t)m->N * m->N : 0); }

nhp_status nhp_quant_reset(nhp_ctx *ctx, nhp_disc_model *m) { return quant_zero(ctx, &m->quant, disc_sums_len(m), disc_entries(m)); }

extern "C" nhp_status nhp_disc_model_quantiles_configure(nhp_ctx *ctx, nhp_disc_model *m, const double *probs, int32_t n_probs, int32_t every,
                                                         int32_t effective_weights)
{
    NHP_TRY(disc_check(ctx, m));
    return quant_configure(ctx, &m->quant, disc_sums_len(m), disc_entries(m), probs, n_probs, every, effective_weights);
}

extern "C" nhp_status nhp_disc_model_quantiles_accumulate(nhp_ctx *ctx, nhp_disc_model *m)
{
    NHP_TRY(disc_check(ctx, m));
    nhp_quant_state *s = m->quant;
    if (!s) { nhp_set_error(ctx, "quantiles: nothing configured (nhp_disc_model_quantiles_configure)"); return NHP_EINVAL; }
    const int64_t N = m->N, NN = N * N;
    if (m->has_A) {
        const quant_src_disc_block src{m->d_block, s->effective ? m->d_A : nullptr, N, NN};
        return quant_launch(ctx, s, src, m->rho_set ? m->d_rho : nullptr);
    }
    const quant_src_disc_product src{m->d_block, N, NN, s->P < ((int64_t)1 << 32)};
    return quant_launch(ctx, s, src, nullptr);
}

nhp_status nhp_quant_kept_step(nhp_ctx *ctx, nhp_disc_model *m)
{
    nhp_quant_state *s = m->quant;
    const bool feed = s->kept % s->every == 0;
    ++s->kept;
    return feed ? nhp_disc_model_quantiles_accumulate(ctx, m) : NHP_OK;
}

extern "C" nhp_status nhp_disc_model_quantiles_fetch(nhp_ctx *ctx, const nhp_disc_model *m, double *values, double *mn, double *mx, double *rho,
                                                     int64_t len, int64_t *count)
{
    NHP_TRY(disc_check(ctx, m));
    if (!values || !count) return NHP_EINVAL;
    return quant_fetch(ctx, m->quant, m->has_A && m->rho_set, values, mn, mx, rho, len, count);
}
