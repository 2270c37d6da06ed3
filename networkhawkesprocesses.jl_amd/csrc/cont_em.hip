// Expectation-maximisation for the continuous standard Hawkes process: expected branching statistics (E-step) and the
// closed-form M-step, with the whole iteration on the device.
//
// The reference's objective charges each event the full mass Σ_c W[n_i,c] whatever θ is (src/continuous.jl:247), so
//   ll = -T Σ λ0 - Σ_p cnt_p Σ_c W[p,c] + Σ_i log λ_i,        λ_i = λ0[c_i] + Σ_j W[n_j,c_i] ħ_{n_j,c_i}(t_i - t_j),
// and Jensen's bound on Σ log λ_i with the responsibilities r_ij = W ħ / λ_i, r_i0 = λ0 / λ_i separates by coordinate:
//   bg[c]   = Σ_{i on c} r_i0                       λ0[c]  = bg[c] / T
//   EM[p,c] = Σ r_ij  (parent node p, child node c)  W[p,c] = EM / cnt_p
//   exponential:  S1 = ES = Σ r_ij Δt_ij             θ = EM / ES
//   logit-normal: S1 = EZ = Σ r_ij z_ij              μ = EZ / EM            z = logit(Δt / Δtmax)
//                 S2 = Σ r_ij (z_ij - μ_old)²         τ = EM / Σ r (z - μ)²  with the new (clamped) μ
// S2 is the second moment CENTRED at the model's current μ, not the raw Σ r z²: the raw moment loses EM·μ² to cancellation,
// the centred one is what the M-step needs, Σ r (z - μ_new)² = S2 - 2δ·D1 + δ²·EM with δ = μ_new - μ_old, D1 = EZ - μ_old·EM.
// Every step is a minorise-maximise step on the box [lower, upper]^P for the objective nhp_cont_loglik evaluates (plus the
// log prior with `priors`: the Gamma / normal-gamma modes of the same bound), so the objective never decreases.
//
// E-step: the accumulators the gradient kernels hold before scaling ARE these statistics (Σ g·ħ, Σ g·∂ħ per (p, c)), so the
// E-step is the fused log-likelihood + gradient launch (nhp_grad_enqueue: the slices route, the two-pass windowed route or
// the wave-partitioned recursion, whichever the flags and the dataset select) followed by an O(P) pass that recovers them
// from the gradient with multiplications by the parameters and divisions by θ | τ only -- nothing is divided by W, so a
// weight on the lower bound keeps its statistics:
//   bg = λ0·(g_λ0 + T)    EM = W·(g_W + cnt_p)    ES = EM/θ - g_θ    D1 = g_μ/τ    EZ = EM·μ + D1    S2 = EM/τ - 2 g_τ
// The summation order is the gradient's: fixed on the one-launch slices route where an item owns its node and in the
// recursion; the two-pass windowed route adds with LDS atomics, so its statistics are not bit-equal from run to run.
// M-step: one O(P) kernel reading the old vector and the gradient, writing the new vector into the OTHER buffer (the two
// are swapped, never updated in place) together with the partial sums of the new vector's log prior.
#include <algorithm>
#include <cmath>

#include "nhp_internal.h"
#include "nhp_math.h"

namespace {

constexpr int EM_BLK = 1024;         // workgroups of the O(P) passes = partial sums of the log prior behind each vector (four
                                     // per CU: the pass is three streams and a few fp64 divisions per coordinate)

struct em_args {
    int N, impulse, use_prior;
    double T, lo, hi;
    const double *cnt;               // [N] events per node (null: an empty dataset)
    nhp_gibbs_priors pr;
    double c_l0, c_w, c_imp;         // parameter-free terms of the Gamma log densities: shape·log(rate) - lgamma(shape)
};

struct em_pair { double EM, S1, S2, D1; };

// of the vectors x and g (the baseline is homogeneous: em_check)
__device__ __forceinline__ nhp_layout em_layout(const em_args &a) { return nhp_layout(a.N, 0, NHP_BASELINE_HOMOGENEOUS, a.impulse); }

__device__ __forceinline__ double em_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the maximiser of num·log(v) - den·v on [lo, hi]: flat keeps `old`; no mass -> lo; no charge -> hi
__device__ __forceinline__ double em_ratio(double num, double den, double old, double lo, double hi)
{
    if (num == 0.0 && den == 0.0) return old;
    if (!(num > 0.0)) return lo;
    if (!(den > 0.0)) return hi;
    return em_clamp(num / den, lo, hi);
}

__device__ __forceinline__ em_pair em_pair_stats(const em_args &a, const double *__restrict__ x, const double *__restrict__ g, size_t k)
{
    const nhp_layout L = em_layout(a);
    const double cp = a.cnt ? a.cnt[k % (size_t)a.N] : 0.0;
    em_pair s;
    s.EM = x[L.W + k] * (g[L.W + k] + cp);
    if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
        s.S1 = s.EM / x[L.p1 + k] - g[L.p1 + k];
        s.S2 = 0.0; s.D1 = 0.0;
    } else {
        const double mu = x[L.p1 + k], tau = x[L.p2 + k];
        s.D1 = g[L.p1 + k] / tau;
        s.S1 = s.EM * mu + s.D1;
        s.S2 = s.EM / tau - 2.0 * g[L.p2 + k];
    }
    return s;
}

// the statistics at x from the gradient at x
__global__ __launch_bounds__(256) void k_em_stats(em_args a, const double *__restrict__ x, const double *__restrict__ g,
                                                  double *__restrict__ bg, double *__restrict__ EM, double *__restrict__ S1,
                                                  double *__restrict__ S2)
{
    const size_t N = (size_t)a.N, NN = N * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { bg[i] = x[i] * (g[i] + a.T); continue; }
        const size_t k = i - N;
        const em_pair s = em_pair_stats(a, x, g, k);
        EM[k] = s.EM; S1[k] = s.S1;
        if (S2) S2[k] = s.S2;
    }
}

__device__ __forceinline__ double em_gamma_logpdf(double v, double c, double shape, double rate)
{
    return c + (shape - 1.0) * log(v) - rate * v;
}

// part[blockIdx.x] = this block's share of logprior(x) (inference.py::logprior; zero without priors)
__device__ __forceinline__ void em_store_prior(double lp, double *__restrict__ part)
{
    __shared__ double red[4];
    lp = nhp_block_sum_n<4>(lp, red);
    if (threadIdx.x == 0) part[blockIdx.x] = lp;
}

__device__ __forceinline__ double em_prior_pair(const em_args &a, double w, double p1, double p2)
{
    const nhp_gibbs_priors &q = a.pr;
    double lp = em_gamma_logpdf(w, a.c_w, q.kappa, q.nu);
    if (a.impulse == NHP_IMPULSE_EXPONENTIAL) return lp + em_gamma_logpdf(p1, a.c_imp, q.a, q.b);
    const double prec = q.kappa_mu * p2, d = p1 - q.mu_mu;
    return lp + em_gamma_logpdf(p2, a.c_imp, q.a, q.b) + (0.5 * log(prec / 6.283185307179586) - 0.5 * prec * (d * d));
}

// x = clamp(x_in) and the partial sums of its log prior: the start of a run
__global__ __launch_bounds__(256) void k_em_start(em_args a, const double *__restrict__ xin, double *__restrict__ x, double *__restrict__ part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = em_layout(a);
    double lp = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) {
            const double v = em_clamp(xin[i], a.lo, a.hi);
            x[i] = v;
            if (a.use_prior) lp += em_gamma_logpdf(v, a.c_l0, a.pr.alpha0, a.pr.beta0);
            continue;
        }
        const size_t k = i - N;
        const double w = em_clamp(xin[L.W + k], a.lo, a.hi), p1 = em_clamp(xin[L.p1 + k], a.lo, a.hi);
        double p2 = 0.0;
        x[L.W + k] = w; x[L.p1 + k] = p1;
        if (a.impulse != NHP_IMPULSE_EXPONENTIAL) { p2 = em_clamp(xin[L.p2 + k], a.lo, a.hi); x[L.p2 + k] = p2; }
        if (a.use_prior) lp += em_prior_pair(a, w, p1, p2);
    }
    em_store_prior(lp, part);
}

// the objective at the iterate whose E-step has just run: log-likelihood + the log prior's partial sums in a fixed order
__global__ __launch_bounds__(256) void k_em_objective(const double *__restrict__ ll, const double *__restrict__ part, int use_prior,
                                                      double *__restrict__ out)
{
    __shared__ double red[4];
    double v = 0.0;
    if (use_prior)
        for (int b = threadIdx.x; b < EM_BLK; b += 256) v += part[b];
    v = nhp_block_sum_n<4>(v, red);
    if (threadIdx.x == 0) *out = *ll + v;
}

// M-step: xn <- the maximiser of the bound (plus the log prior) per coordinate from x and the gradient g at x; partn <- the
// partial sums of logprior(xn)
__global__ __launch_bounds__(256) void k_em_mstep(em_args a, const double *__restrict__ x, const double *__restrict__ g,
                                                  double *__restrict__ xn, double *__restrict__ partn)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = em_layout(a);
    const nhp_gibbs_priors &q = a.pr;
    double lp = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) {
            const double bg = x[i] * (g[i] + a.T);
            const double v = a.use_prior ? em_ratio(bg + q.alpha0 - 1.0, a.T + q.beta0, x[i], a.lo, a.hi)
                                         : em_ratio(bg, a.T, x[i], a.lo, a.hi);
            xn[i] = v;
            if (a.use_prior) lp += em_gamma_logpdf(v, a.c_l0, q.alpha0, q.beta0);
            continue;
        }
        const size_t k = i - N;
        const em_pair s = em_pair_stats(a, x, g, k);
        const double cp = a.cnt ? a.cnt[k % N] : 0.0;
        const double w = a.use_prior ? em_ratio(s.EM + q.kappa - 1.0, cp + q.nu, x[L.W + k], a.lo, a.hi)
                                     : em_ratio(s.EM, cp, x[L.W + k], a.lo, a.hi);
        double p1, p2 = 0.0;
        if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
            p1 = a.use_prior ? em_ratio(s.EM + q.a - 1.0, s.S1 + q.b, x[L.p1 + k], a.lo, a.hi)
                             : em_ratio(s.EM, s.S1, x[L.p1 + k], a.lo, a.hi);
        } else {
            const double mu0 = x[L.p1 + k];
            const double mnum = a.use_prior ? s.S1 + q.kappa_mu * q.mu_mu : s.S1, mden = a.use_prior ? s.EM + q.kappa_mu : s.EM;
            p1 = mden > 0.0 ? em_clamp(mnum / mden, a.lo, a.hi) : mu0;
            const double d = p1 - mu0;
            double V = s.S2 - 2.0 * d * s.D1 + (d * d) * s.EM;      // Σ r (z - μ_new)²
            V = V > 0.0 ? V : 0.0;
            if (a.use_prior) {
                const double dm = p1 - q.mu_mu;
                p2 = em_ratio(0.5 * s.EM + q.a - 0.5, 0.5 * V + q.b + 0.5 * q.kappa_mu * (dm * dm), x[L.p2 + k], a.lo, a.hi);
            } else {
                p2 = em_ratio(s.EM, V, x[L.p2 + k], a.lo, a.hi);
            }
            xn[L.p2 + k] = p2;
        }
        xn[L.p1 + k] = p1;
        xn[L.W + k] = w;
        if (a.use_prior) lp += em_prior_pair(a, w, p1, p2);
    }
    em_store_prior(lp, partn);
}

// an empty dataset: ll = -T Σ λ0, ∇ll = [-T; 0; 0] (one workgroup; g is zeroed before)
__global__ __launch_bounds__(256) void k_em_empty(int N, double T, const double *__restrict__ x, double *__restrict__ g, double *__restrict__ ll)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int c = threadIdx.x; c < N; c += 256) { g[c] = -T; s += x[c]; }
    s = nhp_block_sum_n<4>(s, red);
    if (threadIdx.x == 0) *ll = -T * s;
}

}   // namespace

// what em!, expected_statistics and the variational fit (cont_vb.hip) are built for
nhp_status nhp_em_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const char *what)
{
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) {
        nhp_set_error(ctx, "%s: the M-step of a LogGaussianCoxProcess baseline has no closed form", what);
        return NHP_ENOTIMPL;
    }
    if (m->has_A) {
        nhp_set_error(ctx, "%s is defined for ContinuousStandardHawkesProcess (a masked / network model is not implemented)", what);
        return NHP_ENOTIMPL;
    }
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "%s: not available on a column shard", what);
        return NHP_ENOTIMPL;
    }
    return NHP_OK;
}

namespace {

em_args em_make_args(const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, double lo, double hi)
{
    em_args a{};
    a.N = m->N; a.impulse = m->impulse_kind; a.use_prior = pr ? 1 : 0;
    a.T = ds->duration; a.lo = lo; a.hi = hi;
    a.cnt = ds->M > 0 ? ds->d_cnt : nullptr;
    if (pr) {
        a.pr = *pr;
        a.c_l0 = pr->alpha0 * std::log(pr->beta0) - std::lgamma(pr->alpha0);
        a.c_w = pr->kappa * std::log(pr->nu) - std::lgamma(pr->kappa);
        a.c_imp = pr->a * std::log(pr->b) - std::lgamma(pr->a);
    }
    return a;
}

}   // namespace

// E-step at the DEVICE vector d_x (through nhp_model_view, as nhp_cont_mle_run evaluates a trial):
// log-likelihood -> ctx->d_results[0], gradient -> *d_grad
nhp_status nhp_em_estep(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags, const double *d_x, int64_t P, double **d_grad)
{
    if (ds->M == 0) {
        NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * (2 + (size_t)P)));
        double *g = (double *)ctx->d_scratch + 2;
        NHP_HIP(ctx, hipMemsetAsync(g, 0, 8 * (size_t)P, ctx->main()));
        hipLaunchKernelGGL(k_em_empty, dim3(1), dim3(256), 0, ctx->main(), m->N, ds->duration, d_x, g, ctx->d_results);
        NHP_HIP(ctx, hipGetLastError());
        *d_grad = g;
        return NHP_OK;
    }
    ++m->version;
    nhp_cont_model view = nhp_model_view(m, d_x);
    const nhp_status rc = nhp_grad_enqueue(ctx, ds, &view, flags, P, d_grad);
    nhp_model_view_keep_bound(m, view);
    return rc;
}


extern "C" nhp_status nhp_cont_em_stats(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                        int32_t output_on_device, double *ll, double *bg, double *EM, double *S1, double *S2)
{
    if (!ctx || !ds || !m || !ll || !bg || !EM || !S1) return NHP_EINVAL;
    NHP_TRY(nhp_em_check(ctx, ds, m, "expected_statistics"));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    const size_t N = (size_t)m->N, NN = N * N;
    const int64_t P = (int64_t)nhp_layout(m).P;
    if (m->impulse_kind == NHP_IMPULSE_EXPONENTIAL) S2 = nullptr;
    // the statistics at the model's own block (staged here for a host caller)
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * (N + 3 * NN), "EM state"));
    const double *d_x = m->d_params;
    double *o_bg = (double *)ctx->d_mle, *o_EM = o_bg + N, *o_S1 = o_EM + NN, *o_S2 = S2 ? o_S1 + NN : nullptr;
    hipStream_t st = ctx->main();
    double *d_grad = nullptr;
    nhp_cont_model mm = *m;                                           // (the E-step bumps the version of what it evaluates)
    NHP_TRY(nhp_em_estep(ctx, ds, &mm, flags, d_x, P, &d_grad));
    if (output_on_device) { o_bg = bg; o_EM = EM; o_S1 = S1; o_S2 = S2; }
    const em_args a = em_make_args(ds, m, nullptr, 0.0, 0.0);
    const unsigned nblk = (unsigned)std::min<size_t>(2048, (N + NN + 255) / 256);
    hipLaunchKernelGGL(k_em_stats, dim3(nblk), dim3(256), 0, st, a, d_x, (const double *)d_grad, o_bg, o_EM, o_S1, o_S2);
    NHP_HIP(ctx, hipGetLastError());
    if (!output_on_device) {
        NHP_TRY(nhp_download(ctx, bg, o_bg, 8 * N));
        NHP_TRY(nhp_download(ctx, EM, o_EM, 8 * NN));
        NHP_TRY(nhp_download(ctx, S1, o_S1, 8 * NN));
        if (S2) NHP_TRY(nhp_download(ctx, S2, o_S2, 8 * NN));
    }
    NHP_TRY(nhp_ctx_fetch(ctx, 0, 1, ll));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    if (!std::isfinite(*ll)) {
        nhp_set_error(ctx, "expected_statistics: the intensity of some event is not positive and finite");
        return NHP_EDOMAIN;
    }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_em_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                      const nhp_gibbs_priors *priors, double lower, double upper, double f_abstol, int32_t max_steps,
                                      double *x, int64_t len, double *loss, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !x || !loss || !steps_out || !converged_out) return NHP_EINVAL;
    NHP_TRY(nhp_em_check(ctx, ds, m, "em!"));
    if (!(lower < upper) || max_steps < 0) return NHP_EDOMAIN;
    const size_t P = nhp_layout(m).P;
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    nhp_em_host hs;
    if (hipHostMalloc((void **)&hs.h, 8) != hipSuccess) { hs.h = nullptr; nhp_set_error(ctx, "out of pinned memory"); return NHP_ENOMEM; }
    NHP_HIP(ctx, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));

    // two vectors, each with the partial sums of its log prior behind it, and the objective's scalar
    const size_t stride = P + EM_BLK;
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * (2 * stride + 2), "EM state"));
    double *d_x = (double *)ctx->d_mle, *d_xn = d_x + stride, *d_f = d_xn + stride;
    const em_args a = em_make_args(ds, m, priors, lower, upper);
    const dim3 grid(EM_BLK), block(256);

    NHP_HIP(ctx, hipMemcpyAsync(d_xn, x, 8 * P, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_em_start, grid, block, 0, st, a, (const double *)d_xn, d_x, d_x + P);
    NHP_HIP(ctx, hipGetLastError());

    double f = 0.0, f_prev = 0.0;
    int k = 0;
    bool converged = false;
    for (;; ++k) {
        // E-step at x_k and its objective; the M-step is enqueued behind the scalar's copy, so it runs while the host looks at
        // the stopping rule (it writes the other vector only: nothing is lost when the rule says stop)
        double *d_grad = nullptr;
        NHP_TRY(nhp_em_estep(ctx, ds, m, flags, d_x, (int64_t)P, &d_grad));
        hipLaunchKernelGGL(k_em_objective, dim3(1), block, 0, st, (const double *)ctx->d_results, (const double *)(d_x + P), a.use_prior, d_f);
        NHP_HIP(ctx, hipGetLastError());
        NHP_HIP(ctx, hipMemcpyAsync(hs.h, d_f, 8, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipEventRecord(hs.ev, st));
        if (k < max_steps) {
            hipLaunchKernelGGL(k_em_mstep, grid, block, 0, st, a, (const double *)d_x, (const double *)d_grad, d_xn, d_xn + P);
            NHP_HIP(ctx, hipGetLastError());
        }
        NHP_HIP(ctx, hipEventSynchronize(hs.ev));
        f_prev = f; f = *hs.h;
        if (trace) trace[k] = f;
        if (!std::isfinite(f)) {
            NHP_HIP(ctx, hipStreamSynchronize(st));
            nhp_set_error(ctx, "em!: the intensity of some event is not positive and finite (iteration %d)", k);
            return NHP_EDOMAIN;
        }
        if (k > 0 && std::fabs(f - f_prev) < f_abstol) { converged = true; break; }     // the reference's callback rule
        if (k == max_steps) break;
        std::swap(d_x, d_xn);
    }
    // the model's own block takes the iterate
    ++m->version;
    NHP_HIP(ctx, hipMemcpyAsync(m->d_params, d_x, 8 * P, hipMemcpyDeviceToDevice, st));
    NHP_TRY(nhp_download(ctx, x, d_x, 8 * P));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *loss = -f; *steps_out = k; *converged_out = converged ? 1 : 0;
    return NHP_OK;
}
