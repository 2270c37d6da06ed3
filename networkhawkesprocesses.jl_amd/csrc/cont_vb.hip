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
//
// The host side is nhp_vb_drive.h's: vb_step_drive and vb_run_drive, which the network fits of cont_netvb.hip run through as
// well.  This file supplies its kernels, its argument checks and vb_fit, the struct that tells the drivers what a state of
// the standard fit is; the update kernel's conjugate lines, the start kernel's body and the sums are nhp_vb.h's.
#include "nhp_vb_drive.h"

namespace {

// (the kernels' shared pieces -- vb_args, vb_acc, vb_baseline, vb_pair, vb_update_*, vb_start_body, vb_store, vb_sum_parts, VB_BLK --
// are nhp_vb.h's, shared with cont_netvb.hip; VB_PIECES, VB_OUT and the state's sizing are nhp_cnetvb.h's, host-only)

__device__ __forceinline__ void vb_store_acc(const vb_acc &s, double *__restrict__ part)
{
    vb_store<VB_PIECES>({s.fix, s.comp, s.kl0, s.klw, s.kli}, part);
}

// iteration 0: an ordinary parameter vector used as if it were a surrogate
__global__ __launch_bounds__(256) void k_vb_start(vb_args a, const double *__restrict__ xin, double *__restrict__ x, double *__restrict__ part)
{
    vb_start_body<VB_PIECES>(a, xin, x, part);
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
    vb_store_acc(s, part);
}

// the coordinate-ascent update: factors (S, R) from the surrogate x and the gradient g at it, their surrogate xn, their pieces
__global__ __launch_bounds__(256) void k_vb_update(vb_args a, const double *__restrict__ x, const double *__restrict__ g,
                                                   double *__restrict__ S, double *__restrict__ R, double *__restrict__ xn,
                                                   double *__restrict__ part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    vb_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { vb_update_baseline(a, x, g, i, S, R, xn, s); continue; }
        const size_t k = i - N;
        const double cp = a.cnt ? a.cnt[k % N] : 0.0;
        const double EM = vb_link_em(L, x, g, k, cp);
        const double ka = a.pr.kappa + EM, nu = a.pr.nu + cp;
        double m, kk, sa, sb;
        vb_update_impulse(a, L, x, g, k, EM, S, R, m, kk, sa, sb);
        S[L.W + k] = ka; R[L.W + k] = nu;
        double w, p1, p2;
        vb_pair(a, cp, ka, nu, m, kk, sa, sb, s, w, p1, p2);
        vb_write(a, L, xn, k, w, p1, p2);
    }
    vb_store_acc(s, part);
}

// out = [Σ_i log λ̃_i = ll + fix, E_q[compensator], KL_λ0, KL_W, KL_imp, L]: the partial sums in one fixed order
__global__ __launch_bounds__(256) void k_vb_elbo(const double *__restrict__ ll, const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[VB_PIECES];
    vb_sum_parts<VB_PIECES>(part, tot, red);
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
    return vb_check_priors(ctx, m, pr, what);
}

// the standard fit for the drivers of nhp_vb_drive.h: S, R the caller's planes (host, or device for a step in place)
struct vb_fit {
    static constexpr int OUT = VB_OUT, L_SLOT = 5, STAT_PIECES = 4, PLANES = 2;
    static constexpr bool UNMASK = false;
    struct state { double *x, *S, *R, *part; };                      // a state, its surrogate and its pieces
    nhp_ctx *ctx;
    vb_args a;
    size_t P;
    double *S, *R;

    size_t reserve_doubles() const { return cvb_reserve_doubles(P, VB_BLK); }
    void carve(vb_bump &b, state &s) const { s.x = b.take(P); s.S = b.take(P); s.R = b.take(P); s.part = b.take((size_t)VB_PIECES * VB_BLK); }
    void carve_shared(vb_bump &) const {}
    // a step updates one pair of planes in place: the caller's own when they are on the device
    void place_step(state &cur, state &nxt, bool on_device) const
    {
        if (on_device) { cur.S = S; cur.R = R; }
        nxt.S = cur.S; nxt.R = cur.R;
    }
    void planes(const state &s, vb_plane *pl) const { pl[0] = {S, s.S, P, false}; pl[1] = {R, s.R, P, false}; }
    void start(hipStream_t st, const double *xin, const state &s) const
    {
        hipLaunchKernelGGL(k_vb_start, dim3(VB_BLK), dim3(256), 0, st, a, xin, s.x, s.part);
    }
    void surrogate(hipStream_t st, const state &s) const
    {
        hipLaunchKernelGGL(k_vb_surrogate, dim3(VB_BLK), dim3(256), 0, st, a, (const double *)s.S, (const double *)s.R, s.x, s.part);
    }
    void elbo(hipStream_t st, const state &s, bool, double *out) const
    {
        hipLaunchKernelGGL(k_vb_elbo, dim3(1), dim3(256), 0, st, (const double *)ctx->d_results, (const double *)s.part, out);
    }
    nhp_status update(nhp_ctx *, hipStream_t st, const state &cur, const state &nxt, const double *g, int) const
    {
        hipLaunchKernelGGL(k_vb_update, dim3(VB_BLK), dim3(256), 0, st, a, (const double *)cur.x, g, nxt.S, nxt.R, nxt.x, nxt.part);
        return NHP_OK;
    }
    void mean(hipStream_t st, const state &s, double *x, nhp_cont_model *) const
    {
        hipLaunchKernelGGL(k_vb_mean, dim3(VB_BLK), dim3(256), 0, st, a, (const double *)s.S, (const double *)s.R, x);
    }
    void stats(const double *h, bool from_model, double *out) const { vb_fill_stats(h, OUT, STAT_PIECES, from_model, out); }
};

}   // namespace

extern "C" nhp_status nhp_cont_vb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                       const nhp_gibbs_priors *priors, double *S, double *R, int64_t len, int32_t output_on_device,
                                       double *stats)
{
    if (!ctx || !ds || !m || !priors || !S || !R || !stats) return NHP_EINVAL;
    NHP_TRY(vb_check(ctx, ds, m, priors, "update!"));
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    vb_fit f{ctx, vb_make_args(ds, m, priors), nhp_layout(m).P, S, R};
    return vb_step_drive(ctx, ds, m, flags & ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME), f, (flags & NHP_VB_FROM_MODEL) != 0,
                         output_on_device != 0, stats);
}

extern "C" nhp_status nhp_cont_vb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                      const nhp_gibbs_priors *priors, double f_abstol, int32_t max_steps, double *x, double *S, double *R,
                                      int64_t len, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !x || !S || !R || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    NHP_TRY(vb_check(ctx, ds, m, priors, "vb!"));
    const bool resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(vb_run_args(ctx, m, resume, max_steps, len));
    vb_fit f{ctx, vb_make_args(ds, m, priors), nhp_layout(m).P, S, R};
    return vb_run_drive(ctx, ds, m, flags & ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME), f, resume, f_abstol, max_steps, x, elbo, steps_out,
                        converged_out, trace);
}
