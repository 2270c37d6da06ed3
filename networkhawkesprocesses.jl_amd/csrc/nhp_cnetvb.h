// Host-only parts of the continuous network variational fit (cont_netvb.hip): the argument checks that run
// before any launch and the sizing of the device state -- the standard fit's (cont_vb.hip) sizing too, so that it is checked
// where the network's is (the bump allocator of the shared drivers: nhp_vb_bump.h).  Plain C++ with no HIP in it, so that a stand-alone program can run
// it under the host sanitizers (tools/cnetvb_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "nhp_vb_bump.h"

enum { CNETVB_OK = 0, CNETVB_EINVAL = 1 };
constexpr int CNETVB_PIECES = 8;     // partial sums per workgroup: fix, E_q[comp], KL_λ0, KL_W, KL_imp, Σ entropy terms, Σρv, Σ(1-ρv)
constexpr int CNETVB_OUT = 8;        // k_cnetvb_elbo: Σ log λ̃, the five pieces, L, (spare)

inline bool cnetvb_positive(double v) { return v > 0.0 && std::isfinite(v); }

// net = [κ0, ν0, α, β]: the spike's Gamma and the Beta prior of ρ (α, β ignored for a dense network)
inline int cnetvb_check_net(const char *what, const double *net, bool dense, char *msg, size_t cap)
{
    if (cap) msg[0] = 0;
    if (!net) { snprintf(msg, cap, "%s: net (kappa0, nu0, alpha, beta) is NULL", what); return CNETVB_EINVAL; }
    if (!cnetvb_positive(net[0]) || !cnetvb_positive(net[1])) {
        snprintf(msg, cap, "%s: the spike's kappa0 = %g, nu0 = %g must be positive and finite", what, net[0], net[1]);
        return CNETVB_EINVAL;
    }
    if (!dense && (!cnetvb_positive(net[2]) || !cnetvb_positive(net[3]))) {
        snprintf(msg, cap, "%s: the network's alpha = %g, beta = %g must be positive and finite", what, net[2], net[3]);
        return CNETVB_EINVAL;
    }
    return CNETVB_OK;
}

// Q = [κv0 (N²); νv0 (N²); ρv (N²); αv; βv] in host memory.  The network's (αv, βv) are read in every mode of a Bernoulli
// network; with `state` (a step from a state, a resumed run) the three planes and the slab's (kv1, nv1: the W blocks of S
// and R, N² each) are read too.
inline int cnetvb_check_state(const char *what, size_t N, bool dense, bool state, const double *Q, const double *kv1, const double *nv1,
                              char *msg, size_t cap)
{
    if (cap) msg[0] = 0;
    const size_t NN = N * N;
    if (!Q) { snprintf(msg, cap, "%s: Q is NULL", what); return CNETVB_EINVAL; }
    if (!dense && (!cnetvb_positive(Q[3 * NN]) || !cnetvb_positive(Q[3 * NN + 1]))) {
        snprintf(msg, cap, "%s: the network's alpha_v = %g, beta_v = %g must be positive and finite", what, Q[3 * NN], Q[3 * NN + 1]);
        return CNETVB_EINVAL;
    }
    if (!state) return CNETVB_OK;
    for (size_t i = 0; i < NN; ++i) {
        if (!cnetvb_positive(Q[i]) || !cnetvb_positive(Q[NN + i]) || !cnetvb_positive(kv1[i]) || !cnetvb_positive(nv1[i])) {
            snprintf(msg, cap, "%s: kappa_v / nu_v at link %zu must be positive and finite", what, i);
            return CNETVB_EINVAL;
        }
        if (!dense && !(Q[2 * NN + i] >= 0.0 && Q[2 * NN + i] <= 1.0)) {
            snprintf(msg, cap, "%s: rho_v at link %zu = %g is outside [0, 1]", what, i, Q[2 * NN + i]);
            return CNETVB_EINVAL;
        }
    }
    return CNETVB_OK;
}

// Q = [κv0 (N²); νv0 (N²); ρv (N²)] with no network pair behind the planes (the block and the latent distance fits, whose network
// state travels in an array of its own): the table checks above, and ρv inside [0, 1]
inline int cnetvb_check_planes(const char *what, size_t N, bool state, const double *Q, const double *kv1, const double *nv1, char *msg, size_t cap)
{
    if (cnetvb_check_state(what, N, true, state, Q, kv1, nv1, msg, cap) != CNETVB_OK) return CNETVB_EINVAL;
    if (!state) return CNETVB_OK;
    const size_t NN = N * N;
    for (size_t i = 0; i < NN; ++i)
        if (!(Q[2 * NN + i] >= 0.0 && Q[2 * NN + i] <= 1.0)) {
            snprintf(msg, cap, "%s: rho_v at link %zu = %g is outside [0, 1]", what, i, Q[2 * NN + i]);
            return CNETVB_EINVAL;
        }
    return CNETVB_OK;
}

// (vb_bump, which the drivers carve with and compare against the *_reserve_doubles below: nhp_vb_bump.h)

// the standard fit (cont_vb.hip): a state is its surrogate, S, R (P each) and the partial sums of its pieces; a step or a run
// reserves two states and the scalars of two ELBO evaluations
constexpr int VB_PIECES = 5;         // fix = T Σ λ̃0 + Σ cnt_p W̃, then E_q[compensator], KL_λ0, KL_W, KL_imp
constexpr int VB_OUT = 6;            // k_vb_elbo: Σ log λ̃, the four pieces, L
inline size_t cvb_state_doubles(size_t P, size_t blocks) { return 3 * P + (size_t)VB_PIECES * blocks; }
inline size_t cvb_reserve_doubles(size_t P, size_t blocks) { return 2 * cvb_state_doubles(P, blocks) + 2 * VB_OUT; }

// doubles of one device state: surrogate, S, R (P each), Q with the network's [αv, βv, ψ(αv) - ψ(βv)] behind its planes, and
// the partial sums of its pieces
inline size_t cnetvb_q_doubles(size_t N) { return 3 * N * N + 3; }
inline size_t cnetvb_state_doubles(size_t P, size_t N, size_t blocks) { return 3 * P + cnetvb_q_doubles(N) + (size_t)CNETVB_PIECES * blocks; }
// ... and of what a step or a run reserves: two states and the scalars of two ELBO evaluations
inline size_t cnetvb_reserve_doubles(size_t P, size_t N, size_t blocks) { return 2 * cnetvb_state_doubles(P, N, blocks) + 2 * CNETVB_OUT; }

// (κ1 log ν1 − lgamma κ1) − (κ0 log ν0 − lgamma κ0): the prior's share of the logit, once per call on the host
inline double cnetvb_prior_logit(double kappa0, double nu0, double kappa1, double nu1)
{
    return (kappa1 * std::log(nu1) - std::lgamma(kappa1)) - (kappa0 * std::log(nu0) - std::lgamma(kappa0));
}

// lnΓ(α + β) − lnΓ(α) − lnΓ(β): the prior's constant in KL(Beta(αv, βv) ‖ Beta(α, β))
inline double cnetvb_beta_const(double alpha, double beta) { return std::lgamma(alpha + beta) - std::lgamma(alpha) - std::lgamma(beta); }
