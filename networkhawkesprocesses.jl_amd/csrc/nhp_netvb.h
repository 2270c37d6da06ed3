// Host-only parts of the network VB / SVI entry points (disc.hip): the argument checks that run before any
// launch and the sizing of the device scratch.  Plain C++ with no HIP in it, so that a stand-alone program can run it
// under the host sanitizers (tools/netvb_host_check.cpp).
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

// (κ1 log ν1 − lgamma κ1) − (κ0 log ν0 − lgamma κ0): the prior's share of the logit, once per run on the host
inline double netvb_prior_logit(const netvb_priors &q)
{
    return (q.kappa1 * std::log(q.nu1) - std::lgamma(q.kappa1)) - (q.kappa0 * std::log(q.nu0) - std::lgamma(q.kappa0));
}
