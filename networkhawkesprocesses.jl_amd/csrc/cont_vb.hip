// Mean-field variational inference for the continuous standard Hawkes process (homogeneous baseline, the full-mass
// likelihood of cont_em.hip), with the whole iteration on the device.
//
// Model and priors are em!'s: with the branching z, log p(events, z | λ0, W, ħ) = Σ_i [z_i0 log λ0[c_i] + Σ_j z_ij (log W[n_j,c_i] +
// log ħ(Δt_ij))] - T Σ λ0 - Σ_p cnt_p Σ_c W[p,c], λ0 ~ Gamma(α0, β0), W ~ Gamma(κ, ν), θ ~ Gamma(a, b) | (μ, τ) ~ NormalGamma(μμ, κμ, a, b).
// One factor per entry, conjugate in the expected branching statistics bg, EM, S1, S2 of nhp_cont_em_stats:
//   λ0[c]  ~ Gamma(α' = α0 + bg[c], β' = β0 + T)            W[p,c] ~ Gamma(κ' = κ + EM, ν' = ν + cnt_p)
//   θ[p,c] ~ Gamma(a' = a + EM, b' = b + S1)
//   (μ,τ)[p,c] ~ NormalGamma(m', k', a', b'), centred at the surrogate's μ = c (D1 = Σ r (z - c), S2 = Σ r (z - c)², d0 = μμ - c):
//     k' = κμ + EM, m' = c + (D1 + κμ d0)/k', a' = a + EM/2, b' = b + ½[S2 + κμ d0² - k'(m' - c)²]      (the prior at EM = 0)
// The surrogate trick: q(z) needs E_q[log λ0], E_q[log W + log ħ(Δt)] per pair, and the latter is log(W̃ ħ_θ̃(Δt)) of an ordinary
// parameter vector x̃ (params! order),
//   λ̃0 = exp(ψ(α') - log β'),   θ̃ = a'/b',  W̃ = exp(ψ(κ') - log ν' + ψ(a') - log a')
//                               μ̃ = m', τ̃ = a'/b',  W̃ = exp(ψ(κ') - log ν' + ½(ψ(a') - log a') - 1/(2k'))
// so the E-step is em!'s (nhp_em_estep: the fused log-likelihood + gradient launch by whichever route nhp_grad_enqueue picks)
// evaluated at x̃: its responsibilities are the variational ones, and its Σ_i log λ̃_i = ll(x̃) + T Σ λ̃0 + Σ_p cnt_p Σ_c W̃ is the
// log-normaliser of q(z).  x̃ is not clamped to any box.  The ELBO of a state q with q(z) optimal for it:
//   L = Σ_i log λ̃_i - T Σ α'/β' - Σ_p cnt_p Σ_c κ'/ν' - KL_λ0 - KL_W - KL_imp
//   KL(Gamma(a₁,b₁)‖Gamma(a₀,b₀)) = (a₁-a₀)ψ(a₁) - lnΓ(a₁) + lnΓ(a₀) + a₀(log b₁ - log b₀) + a₁(b₀-b₁)/b₁
//   normal-gamma: the Gamma KL of (a',b') + ½[κμ/k' - 1 + log(k'/κμ) + κμ (a'/b')(m' - μμ)²]
//
// Per iteration the new HIP is ONE O(P) pass (k_vb_update): it reads x̃_k and the gradient at it, recovers the statistics
// with cont_em.hip's identities (nothing is divided by W̃), writes the factor planes S (shape-like: α', a' | m', a', κ') and R
// (rate-like: β', b' | k', b', ν') in params! order, the next surrogate x̃_{k+1} into the OTHER buffer, and per-workgroup
// partial sums of five pieces of the new state: the part of ll(x̃_{k+1}) to undo (T λ̃0 + cnt_p W̃), E_q[compensator], KL_λ0,
// KL_W, KL_imp.  k_vb_elbo (one workgroup) adds the partials and forms L.  No atomics: a thread adds its entries in index
// order, a wave adds with DPP, a workgroup its four waves in order, k_vb_elbo the VB_BLK partials with a fixed thread stride and
// the same block sum.  The statistics' own order is the E-step's (cont_em.hip: fixed on the slices route and in the
// recursion, LDS atomics on the two-pass windowed route).
#include <algorithm>
#include <cmath>

#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_vb.h"

namespace {

constexpr int VB_PIECES = 5;         // fix = T Σ λ̃0 + Σ cnt_p W̃, then E_q[compensator], KL_λ0, KL_W, KL_imp
constexpr int VB_OUT = 6;            // k_vb_elbo: Σ log λ̃, the four pieces, L

// (vb_args, vb_acc, vb_baseline, vb_pair, vb_kl_gamma, vb_write, VB_BLK: nhp_vb.h, shared with cont_netvb.hip)

// part[piece·VB_BLK + blockIdx.x] = this workgroup's share of each piece
__device__ __forceinline__ void vb_store(const vb_acc &s, double *__restrict__ part)
{
    __shared__ double red[4];
    const double v[VB_PIECES] = {s.fix, s.comp, s.kl0, s.klw, s.kli};
#pragma unroll
    for (int j = 0; j < VB_PIECES; ++j) {
        const double t = nhp_block_sum_n<4>(v[j], red);
        if (threadIdx.x == 0) part[j * VB_BLK + blockIdx.x] = t;
    }
}

// iteration 0: an ordinary parameter vector used as if it were a surrogate; only the part of its ll to undo has a meaning
__global__ __launch_bounds__(256) void k_vb_start(vb_args a, const double *__restrict__ xin, double *__restrict__ x, double *__restrict__ part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    vb_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { const double v = xin[i]; x[i] = v; s.fix += a.T * v; continue; }
        const size_t k = i - N;
        const double w = xin[L.W + k];
        vb_write(a, L, x, k, w, xin[L.p1 + k], a.impulse != NHP_IMPULSE_EXPONENTIAL ? xin[L.p2 + k] : 0.0);
        s.fix += (a.cnt ? a.cnt[k % N] : 0.0) * w;
    }
    vb_store(s, part);
}

// the surrogate and the pieces of a given state (S, R): the start of nhp_cont_vb_step and of a resumed run
__global__ __launch_bounds__(256) void k_vb_surrogate(vb_args a, const double *__restrict__ S, const double *__restrict__ R,
                                                      double *__restrict__ x, double *__restrict__ part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    vb_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { x[i] = vb_baseline(a, S[i], R[i], s); continue; }
        const size_t k = i - N;
        const bool ln = a.impulse != NHP_IMPULSE_EXPONENTIAL;
        const size_t sh = ln ? L.p2 + k : L.p1 + k;                  // where the impulse's Gamma factor sits
        double w, p1, p2;
        vb_pair(a, a.cnt ? a.cnt[k % N] : 0.0, S[L.W + k], R[L.W + k], ln ? S[L.p1 + k] : 0.0, ln ? R[L.p1 + k] : 1.0, S[sh], R[sh], s, w, p1, p2);
        vb_write(a, L, x, k, w, p1, p2);
    }
    vb_store(s, part);
}

// the coordinate-ascent update: factors (S, R) from the surrogate x and the gradient g at it, their surrogate xn, their pieces
__global__ __launch_bounds__(256) void k_vb_update(vb_args a, const double *__restrict__ x, const double *__restrict__ g,
                                                   double *__restrict__ S, double *__restrict__ R, double *__restrict__ xn,
                                                   double *__restrict__ part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    const nhp_gibbs_priors &q = a.pr;
    vb_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) {
            const double al = q.alpha0 + x[i] * (g[i] + a.T), be = q.beta0 + a.T;
            S[i] = al; R[i] = be;
            xn[i] = vb_baseline(a, al, be, s);
            continue;
        }
        const size_t k = i - N;
        const double cp = a.cnt ? a.cnt[k % N] : 0.0;
        const double EM = x[L.W + k] * (g[L.W + k] + cp);
        const double ka = q.kappa + EM, nu = q.nu + cp;
        double m = 0.0, kk = 1.0, sa, sb;
        if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
            sa = q.a + EM;
            sb = q.b + (EM / x[L.p1 + k] - g[L.p1 + k]);
            S[L.p1 + k] = sa; R[L.p1 + k] = sb;
        } else {
            const double c = x[L.p1 + k], tau = x[L.p2 + k];
            const double D1 = g[L.p1 + k] / tau, S2 = EM / tau - 2.0 * g[L.p2 + k], d0 = q.mu_mu - c;
            kk = q.kappa_mu + EM;
            const double dm = (D1 + q.kappa_mu * d0) / kk;
            m = c + dm;
            sa = q.a + 0.5 * EM;
            sb = q.b + 0.5 * ((S2 + q.kappa_mu * (d0 * d0)) - kk * (dm * dm));
            S[L.p1 + k] = m; R[L.p1 + k] = kk;
            S[L.p2 + k] = sa; R[L.p2 + k] = sb;
        }
        S[L.W + k] = ka; R[L.W + k] = nu;
        double w, p1, p2;
        vb_pair(a, cp, ka, nu, m, kk, sa, sb, s, w, p1, p2);
        vb_write(a, L, xn, k, w, p1, p2);
    }
    vb_store(s, part);
}

// out = [Σ_i log λ̃_i = ll + fix, E_q[compensator], KL_λ0, KL_W, KL_imp, L]: the partial sums in one fixed order
__global__ __launch_bounds__(256) void k_vb_elbo(const double *__restrict__ ll, const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[VB_PIECES];
    for (int j = 0; j < VB_PIECES; ++j) {
        double v = 0.0;
        for (int b = threadIdx.x; b < VB_BLK; b += 256) v += part[j * VB_BLK + b];
        v = nhp_block_sum_n<4>(v, red);
        if (threadIdx.x == 0) tot[j] = v;
    }
    if (threadIdx.x == 0) {
        const double sl = *ll + tot[0];
        out[0] = sl;
        for (int j = 1; j < VB_PIECES; ++j) out[j] = tot[j];
        out[5] = (((sl - tot[1]) - tot[2]) - tot[3]) - tot[4];
    }
}

// the posterior means in params! order: α'/β', a'/b' | m', a'/b', κ'/ν'
__global__ __launch_bounds__(256) void k_vb_mean(vb_args a, const double *__restrict__ S, const double *__restrict__ R, double *__restrict__ x)
{
    const nhp_layout L = vb_layout(a);
    const bool ln = a.impulse != NHP_IMPULSE_EXPONENTIAL;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < L.P; i += (size_t)gridDim.x * 256)
        x[i] = (ln && i >= L.p1 && i < L.p2) ? S[i] : S[i] / R[i];
}

nhp_status vb_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const char *what)
{
    NHP_TRY(nhp_em_check(ctx, ds, m, what));
    const bool ln = m->impulse_kind != NHP_IMPULSE_EXPONENTIAL;
    if (!vb_positive(pr->alpha0) || !vb_positive(pr->beta0) || !vb_positive(pr->kappa) || !vb_positive(pr->nu) || !vb_positive(pr->a) ||
        !vb_positive(pr->b) || (ln && (!vb_positive(pr->kappa_mu) || !std::isfinite(pr->mu_mu)))) {
        nhp_set_error(ctx, "%s: every prior hyper-parameter but the mean μμ must be positive and finite", what);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

struct vb_state { double *x, *S, *R, *part; };                       // a state, its surrogate and its pieces

}   // namespace

extern "C" nhp_status nhp_cont_vb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                       const nhp_gibbs_priors *priors, double *S, double *R, int64_t len, int32_t output_on_device,
                                       double *stats)
{
    if (!ctx || !ds || !m || !priors || !S || !R || !stats) return NHP_EINVAL;
    NHP_TRY(vb_check(ctx, ds, m, priors, "update!"));
    const size_t P = nhp_layout(m).P;
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const bool from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME);

    // the surrogate stepped from and the one stepped to, each with its pieces; the planes of a host caller; the sums
    const size_t np = (size_t)VB_PIECES * VB_BLK;
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * (4 * P + 2 * np + 2 * VB_OUT), "variational state"));
    double *d_x = (double *)ctx->d_mle, *d_xn = d_x + P, *d_S = d_xn + P, *d_R = d_S + P;
    double *d_p0 = d_R + P, *d_p1 = d_p0 + np, *d_out = d_p1 + np;
    if (output_on_device) { d_S = S; d_R = R; }
    const vb_args a = vb_make_args(ds, m, priors);
    const dim3 grid(VB_BLK), block(256);
    if (from_model) {
        hipLaunchKernelGGL(k_vb_start, grid, block, 0, st, a, (const double *)m->d_params, d_x, d_p0);
    } else {
        if (!output_on_device) {
            NHP_HIP(ctx, hipMemcpyAsync(d_S, S, 8 * P, hipMemcpyHostToDevice, st));
            NHP_HIP(ctx, hipMemcpyAsync(d_R, R, 8 * P, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(k_vb_surrogate, grid, block, 0, st, a, (const double *)d_S, (const double *)d_R, d_x, d_p0);
    }
    NHP_HIP(ctx, hipGetLastError());
    double *d_grad = nullptr;
    nhp_cont_model mm = *m;                                           // (the E-step bumps the version of what it evaluates)
    NHP_TRY(nhp_em_estep(ctx, ds, &mm, flags, d_x, (int64_t)P, &d_grad));
    hipLaunchKernelGGL(k_vb_elbo, dim3(1), block, 0, st, (const double *)ctx->d_results, (const double *)d_p0, d_out);
    hipLaunchKernelGGL(k_vb_update, grid, block, 0, st, a, (const double *)d_x, (const double *)d_grad, d_S, d_R, d_xn, d_p1);
    hipLaunchKernelGGL(k_vb_elbo, dim3(1), block, 0, st, (const double *)ctx->d_results, (const double *)d_p1, d_out + VB_OUT);
    NHP_HIP(ctx, hipGetLastError());
    double h[2 * VB_OUT];
    NHP_TRY(nhp_download(ctx, h, d_out, sizeof h));
    if (!output_on_device) {
        NHP_TRY(nhp_download(ctx, S, d_S, 8 * P));
        NHP_TRY(nhp_download(ctx, R, d_R, 8 * P));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    if (!std::isfinite(h[0])) {
        nhp_set_error(ctx, "update!: the intensity of some event is not positive and finite");
        return NHP_EDOMAIN;
    }
    stats[0] = h[0];
    for (int j = 1; j < VB_PIECES; ++j) { stats[j] = from_model ? 0.0 : h[j]; stats[4 + j] = h[VB_OUT + j]; }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_vb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                      const nhp_gibbs_priors *priors, double f_abstol, int32_t max_steps, double *x, double *S, double *R,
                                      int64_t len, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !x || !S || !R || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    NHP_TRY(vb_check(ctx, ds, m, priors, "vb!"));
    const bool resume = (flags & NHP_VB_RESUME) != 0;
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME);
    if (max_steps < (resume ? 0 : 1)) {
        nhp_set_error(ctx, "vb!: max_steps = %d (a run from a guess needs at least one step to have a state)", max_steps);
        return NHP_EDOMAIN;
    }
    const size_t P = nhp_layout(m).P;
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    nhp_em_host hs;
    if (hipHostMalloc((void **)&hs.h, 8 * VB_OUT) != hipSuccess) { hs.h = nullptr; nhp_set_error(ctx, "out of pinned memory"); return NHP_ENOMEM; }
    NHP_HIP(ctx, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));

    // two states (surrogate, planes, pieces): an update writes the other one only, so nothing is lost when the rule says stop
    const size_t np = (size_t)VB_PIECES * VB_BLK, stride = 3 * P + np;
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * (2 * stride + VB_OUT), "variational state"));
    double *base = (double *)ctx->d_mle, *d_out = base + 2 * stride;
    vb_state cur{base, base + P, base + 2 * P, base + 3 * P}, nxt{base + stride, base + stride + P, base + stride + 2 * P, base + stride + 3 * P};
    const vb_args a = vb_make_args(ds, m, priors);
    const dim3 grid(VB_BLK), block(256);

    if (resume) {
        NHP_HIP(ctx, hipMemcpyAsync(cur.S, S, 8 * P, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.R, R, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vb_surrogate, grid, block, 0, st, a, (const double *)cur.S, (const double *)cur.R, cur.x, cur.part);
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(nxt.x, x, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vb_start, grid, block, 0, st, a, (const double *)nxt.x, cur.x, cur.part);
    }
    NHP_HIP(ctx, hipGetLastError());

    const double nan = std::nan("");
    double L = nan, L_prev = nan;
    bool has_state = resume, converged = false;
    int k = 0;
    for (;; ++k) {
        // E-step at x̃_k and the ELBO of state k; the update is enqueued behind the scalars' copy, so it runs while the host looks
        // at the stopping rule
        double *d_grad = nullptr;
        NHP_TRY(nhp_em_estep(ctx, ds, m, flags, cur.x, (int64_t)P, &d_grad));
        hipLaunchKernelGGL(k_vb_elbo, dim3(1), block, 0, st, (const double *)ctx->d_results, (const double *)cur.part, d_out);
        NHP_HIP(ctx, hipGetLastError());
        NHP_HIP(ctx, hipMemcpyAsync(hs.h, d_out, 8 * VB_OUT, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipEventRecord(hs.ev, st));
        if (k < max_steps) {
            hipLaunchKernelGGL(k_vb_update, grid, block, 0, st, a, (const double *)cur.x, (const double *)d_grad, nxt.S, nxt.R, nxt.x, nxt.part);
            NHP_HIP(ctx, hipGetLastError());
        }
        NHP_HIP(ctx, hipEventSynchronize(hs.ev));
        if (!std::isfinite(hs.h[0])) {
            NHP_HIP(ctx, hipStreamSynchronize(st));
            nhp_set_error(ctx, "vb!: the intensity of some event is not positive and finite (iteration %d)", k);
            return NHP_EDOMAIN;
        }
        L_prev = L; L = has_state ? hs.h[5] : nan;
        if (trace) trace[k] = L;
        if (has_state && std::fabs(L - L_prev) < f_abstol) { converged = true; break; }     // (false while L_prev is NaN)
        if (k == max_steps) break;
        std::swap(cur, nxt);
        has_state = true;
    }
    // the state, and its means into x and the model's own block
    hipLaunchKernelGGL(k_vb_mean, grid, block, 0, st, a, (const double *)cur.S, (const double *)cur.R, nxt.x);
    NHP_HIP(ctx, hipGetLastError());
    ++m->version;
    NHP_HIP(ctx, hipMemcpyAsync(m->d_params, nxt.x, 8 * P, hipMemcpyDeviceToDevice, st));
    NHP_TRY(nhp_download(ctx, x, nxt.x, 8 * P));
    NHP_TRY(nhp_download(ctx, S, cur.S, 8 * P));
    NHP_TRY(nhp_download(ctx, R, cur.R, 8 * P));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *elbo = L; *steps_out = k; *converged_out = converged ? 1 : 0;
    return NHP_OK;
}
