// Host-only parts of the discrete VB / SVI entry points (disc_vb.hip): the argument checks that run before
// any launch -- the network's and the SVI schedule's -- and the sizing of the device scratch of both fits.  Plain C++ with no
// HIP in it, so that a stand-alone program can run it under the host sanitizers (tools/netvb_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

enum { NETVB_OK = 0, NETVB_EINVAL = 1, NETVB_ENOTIMPL = 2 };

struct netvb_priors {
    double alpha0, beta0, kappa0, nu0, kappa1, nu1, gamma;
    int32_t net_kind;                  // 0 DenseNetworkModel, 1 BernoulliNetworkModel
    double net_alpha, net_beta;        // Beta(α, β) prior of the Bernoulli network's ρ
};

// The checks of nhp_disc_netvb_run / nhp_disc_netsvi_run that read host memory alone.  `what` names the caller in the
// message.  Returns NETVB_OK, or a status with a message in msg[cap].
inline int netvb_check_args(const char *what, const netvb_priors &q, double dt, int64_t N, int64_t B, int32_t n_steps,
                            const double *alpha_v, const double *beta_v, const double *kappa_v0, const double *nu_v0,
                            const double *kappa_v1, const double *nu_v1, const double *gamma_v, const double *rho_v,
                            const double *net_alpha_v, const double *net_beta_v, char *msg, size_t cap)
{
    if (cap) msg[0] = 0;
    if (n_steps < 1) { snprintf(msg, cap, "%s: n_steps must be >= 1", what); return NETVB_EINVAL; }
    if (!(dt > 0.0)) { snprintf(msg, cap, "%s: dt must be positive", what); return NETVB_EINVAL; }
    if (N < 1 || B < 1) { snprintf(msg, cap, "%s: the dataset has no nodes or no basis", what); return NETVB_EINVAL; }
    if (q.net_kind != 0 && q.net_kind != 1) {
        snprintf(msg, cap, "%s: net_kind = %d is not built (0 dense, 1 Bernoulli; the block model has entry points of its own, nhp_disc_sbmvb_run / nhp_disc_sbmsvi_run)", what, (int)q.net_kind);
        return NETVB_ENOTIMPL;
    }
    if (!alpha_v || !beta_v || !kappa_v0 || !nu_v0 || !kappa_v1 || !nu_v1 || !gamma_v || !rho_v) {
        snprintf(msg, cap, "%s: a variational parameter array is NULL", what);
        return NETVB_EINVAL;
    }
    if (!(q.alpha0 > 0.0) || !(q.beta0 > 0.0) || !(q.gamma > 0.0)) { snprintf(msg, cap, "%s: the priors alpha0, beta0, gamma must be > 0", what); return NETVB_EINVAL; }
    if (!(q.kappa0 > 0.0) || !(q.nu0 > 0.0) || !(q.kappa1 > 0.0) || !(q.nu1 > 0.0) || !std::isfinite(q.kappa0 + q.nu0 + q.kappa1 + q.nu1)) {
        snprintf(msg, cap, "%s: the weight priors kappa0, nu0, kappa1, nu1 must be > 0 and finite", what);
        return NETVB_EINVAL;
    }
    const size_t n = (size_t)N, nn = n * n;
    for (size_t i = 0; i < n; ++i)
        if (!(alpha_v[i] > 0.0) || !(beta_v[i] > 0.0)) { snprintf(msg, cap, "%s: alpha_v[%zu], beta_v[%zu] must be > 0", what, i, i); return NETVB_EINVAL; }
    for (size_t i = 0; i < nn; ++i) {
        if (!(kappa_v0[i] > 0.0) || !(kappa_v1[i] > 0.0)) { snprintf(msg, cap, "%s: kappa_v0 / kappa_v1 at entry %zu must be > 0", what, i); return NETVB_EINVAL; }
        if (!(nu_v0[i] > 0.0) || !(nu_v1[i] > 0.0)) { snprintf(msg, cap, "%s: nu_v0 / nu_v1 at entry %zu must be > 0", what, i); return NETVB_EINVAL; }
    }
    for (size_t i = 0; i < nn * (size_t)B; ++i)
        if (!(gamma_v[i] > 0.0)) { snprintf(msg, cap, "%s: gamma_v at entry %zu must be > 0", what, i); return NETVB_EINVAL; }
    if (q.net_kind == 1) {
        if (!net_alpha_v || !net_beta_v) { snprintf(msg, cap, "%s: a Bernoulli network needs net_alpha_v and net_beta_v", what); return NETVB_EINVAL; }
        if (!(q.net_alpha > 0.0) || !(q.net_beta > 0.0) || !(*net_alpha_v > 0.0) || !(*net_beta_v > 0.0)) {
            snprintf(msg, cap, "%s: the network's alpha, beta and their variational values must be > 0", what);
            return NETVB_EINVAL;
        }
        for (size_t i = 0; i < nn; ++i)
            if (!(rho_v[i] >= 0.0 && rho_v[i] <= 1.0)) { snprintf(msg, cap, "%s: rho_v at entry %zu = %g is outside [0, 1]", what, i, rho_v[i]); return NETVB_EINVAL; }
    }
    return NETVB_OK;
}

// workgroups of the per-link kernels = partial sums of ρv the finish kernel leaves (one pair each)
inline size_t netvb_link_blocks(size_t N) { return (N * N + 255) / 256; }

// Doubles of device scratch the parameters of a network VB / SVI run take next to the dense step's buffers:
// κv0, νv0, κv1, νv1 (the dense step holds one pair), ρv, the network's (αv, βv) and the ρv partial pairs.
inline size_t netvb_param_doubles(size_t N, size_t B)
{
    const size_t NN = N * N;
    return N * B * N /* E */ + 3 * N /* e0, αv, βv */ + 5 * NN + NN * B + 2 + 2 * netvb_link_blocks(N);
}

// What a discrete variational run reserves (disc_vb.hip carves it with vb_bump and refuses to launch when the two disagree).
// rows: bins of the largest window (VB: T, SVI: Tb); row_blocks, splits: the column partials' and slabs' counts, at their
// caps for SVI; L > 0: the streamed mode with L lags.
struct disc_vb_dims {
    size_t N, B, rows, row_blocks, splits;
    bool svi;
    size_t L;
};
// the window's buffers: D (SVI: the block's counts), R, the column partials, the slabs, the streamed image and basis
inline size_t disc_vb_work_doubles(const disc_vb_dims &d)
{
    const size_t K = d.N * d.B;
    return (d.svi ? 2 : 1) * d.rows * d.N + d.row_blocks * d.N + d.splits * K * d.N + (d.L ? d.rows * K + d.L * d.B : 0);
}
// the dense fit: E, e0, αv, βv, κv, νv, γv and the window's buffers
inline size_t dense_vb_param_doubles(size_t N, size_t B) { return N * B * N + 3 * N + 2 * N * N + N * N * B; }
inline size_t dense_vb_reserve_doubles(const disc_vb_dims &d) { return dense_vb_param_doubles(d.N, d.B) + disc_vb_work_doubles(d); }
// the network fit; block_doubles: sbmvb_param_doubles (nhp_sbmvb.h) of a block network, 0 otherwise
inline size_t netvb_reserve_doubles(const disc_vb_dims &d, size_t block_doubles)
{
    return netvb_param_doubles(d.N, d.B) + disc_vb_work_doubles(d) + block_doubles;
}

// The schedule of an SVI run as its entry point receives it ...
struct svi_request {
    int64_t batch_bins;
    double delay, forgetting;
    uint64_t seed;
    int64_t step0;
    const int32_t *blocks;             // NULL: drawn from (seed, step)
    const double *phi;                 // non-NULL: the streamed mode, with n_lags x n_basis
    int32_t n_lags, n_basis;
};
// ... and what the checks derive: Tb bins per block, nb blocks
struct svi_schedule {
    svi_request rq;
    int64_t Tb;
    int32_t nb;
    bool streamed;
};

constexpr int DISC_CONV_CB = 8;        // basis columns per pass of the convolution kernels of disc.hip and disc_vb.hip (their CONV_CB)
inline size_t svi_window_lds_bytes(size_t L, size_t B) { return 8 * (256 + L + L * ((B + DISC_CONV_CB - 1) / DISC_CONV_CB * DISC_CONV_CB)); }

// The checks of every SVI entry point on its schedule and on the state of the dataset (T bins; has_*: a per-bin baseline,
// trials, a resident Ŝ).  Returns NETVB_OK and fills *out, or a status with a message in msg[cap].
inline int svi_check_schedule(const char *what, const svi_request &rq, int32_t n_steps, int64_t T, bool has_baseline, bool has_trials,
                              bool has_conv, svi_schedule *out, char *msg, size_t cap)
{
    if (cap) msg[0] = 0;
    if (n_steps < 1 || rq.step0 < 0) { snprintf(msg, cap, "%s: n_steps must be >= 1 and step0 >= 0", what); return NETVB_EINVAL; }
    if (!(rq.delay >= 0.0)) { snprintf(msg, cap, "%s: delay must be >= 0", what); return NETVB_EINVAL; }
    if (!(rq.forgetting > 0.5 && rq.forgetting <= 1.0)) { snprintf(msg, cap, "%s: forgetting must lie in (0.5, 1]", what); return NETVB_EINVAL; }
    // a convention of the interface (block starts on whole 16-element reduction chunks), not a need of the GEMM, which loads
    // single doubles at any lda; nothing is rounded silently
    if (rq.batch_bins < T && (rq.batch_bins < 16 || rq.batch_bins % 16 != 0)) {
        snprintf(msg, cap, "%s: batch_bins = %lld must be a multiple of 16 (>= 16), or >= the %lld bins of the data", what, (long long)rq.batch_bins, (long long)T);
        return NETVB_EINVAL;
    }
    out->rq = rq;
    out->Tb = rq.batch_bins < T ? rq.batch_bins : T;
    out->nb = (int32_t)((T + out->Tb - 1) / out->Tb);
    out->streamed = rq.phi != nullptr;
    if (rq.blocks)
        for (int32_t k = 0; k < n_steps; ++k)
            if (rq.blocks[k] < 0 || rq.blocks[k] >= out->nb) { snprintf(msg, cap, "%s: blocks[%d] = %d is outside [0, %d)", what, k, rq.blocks[k], out->nb); return NETVB_EINVAL; }
    if (has_baseline) { snprintf(msg, cap, "%s: defined for DiscreteHomogeneousProcess baselines only", what); return NETVB_ENOTIMPL; }
    if (out->streamed && has_trials) { snprintf(msg, cap, "%s: the streamed mode convolves across the boundaries of the dataset's trials; convolve the dataset and use the resident mode", what); return NETVB_ENOTIMPL; }
    if (out->streamed && (rq.n_lags < 1 || rq.n_basis < 1)) { snprintf(msg, cap, "%s: the streamed mode needs n_lags >= 1 and n_basis >= 1", what); return NETVB_EINVAL; }
    if (!out->streamed && !has_conv) { snprintf(msg, cap, "%s: convolve(process, data) must run first, or pass the basis for the streamed mode", what); return NETVB_EINVAL; }
    if (out->streamed && svi_window_lds_bytes((size_t)rq.n_lags, (size_t)rq.n_basis) > 64 * 1024) {
        snprintf(msg, cap, "%s: nlags * nbasis = %d * %d exceeds the LDS budget", what, rq.n_lags, rq.n_basis);
        return NETVB_ENOTIMPL;
    }
    return NETVB_OK;
}

// (κ1 log ν1 − lgamma κ1) − (κ0 log ν0 − lgamma κ0): the prior's share of the logit, once per run on the host
inline double netvb_prior_logit(const netvb_priors &q)
{
    return (q.kappa1 * std::log(q.nu1) - std::lgamma(q.kappa1)) - (q.kappa0 * std::log(q.nu0) - std::lgamma(q.kappa0));
}
