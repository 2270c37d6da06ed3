// Host-only parts of the continuous LATENT-DISTANCE-network variational fit (cont_netvb.hip): the argument checks
// that run before any launch, the ladder of step sizes and the sizing of the device state, on top of the Bernoulli fit's
// (nhp_cnetvb.h).  Plain C++ with no HIP in it, so that a stand-alone program can run it under the host sanitizers
// (tools/clatvb_host_check.cpp).
#pragma once
#include <cmath>

#include "nhp_cnetvb.h"

enum { CLATVB_OK = 0, CLATVB_EINVAL = 1 };
constexpr int CLATVB_MAX_DIMS = 8;                                // D in 1..8 (LatentDistanceNetworkModel.MAX_DIMS)
constexpr int CLATVB_MAX_ASCENT = 64;                             // ascent_steps J in 0..64
constexpr int CLATVB_RUNGS = 8;                                   // step sizes tried per ascent iteration
constexpr int CLATVB_SLOTS = CLATVB_RUNGS + 1;                    // ... and the current point (t = 0) behind them
constexpr int CLATVB_NET_PIECES = 4;                              // Σ entropy of ρv, links, ln p(zv), ln p(bv)
constexpr int CLATVB_OUT = 8 + CLATVB_NET_PIECES + CLATVB_MAX_ASCENT;   // k_clatvb_elbo: k_cnetvb_elbo's eight, the pieces, the rungs taken
constexpr int CLATVB_STATS_FIXED = 11 + 2 * CLATVB_NET_PIECES;    // nhp_cont_latvb_step: the Bernoulli step's eleven, pieces before, after; then J rungs
constexpr int CLATVB_SC = 2 + CLATVB_SLOTS;                       // device scalars of an iteration: t taken, its rung, F at every slot

// Z = [vec zv (N x D column-major: z_n[d] at n + N·d); bv]
inline size_t clatvb_z_doubles(size_t N, size_t D) { return N * D + 1; }

// t[r] = τ·4^(1-r), r = 0..7, τ = 1/(N + 1/σ²), and t[8] = 0 (the current point): powers of four are exact, so every rung is τ
// with another exponent
inline void clatvb_ladder(int64_t N, double sigma, double *t)
{
    const double tau = 1.0 / ((double)N + 1.0 / (sigma * sigma));
    for (int r = 0; r < CLATVB_RUNGS; ++r) t[r] = std::ldexp(tau, 2 * (1 - r));
    t[CLATVB_RUNGS] = 0.0;
}

// net = [κ0, ν0] (the spike's Gamma), lat = [σ, μb, σb], D, J = ascent_steps and the state Z.  `dense`: the caller set
// NHP_VB_DENSE_NETWORK, which has no meaning here.  `Z_on_device`: Z is a device pointer, so its entries cannot be read here.
inline int clatvb_check_args(const char *what, int64_t N, const double *net, const double *lat, int32_t D, int32_t J, bool dense, const double *Z,
                             char *msg, size_t cap, bool Z_on_device = false)
{
    if (cap) msg[0] = 0;
    if (dense) { snprintf(msg, cap, "%s: NHP_VB_DENSE_NETWORK has no meaning for a latent distance network", what); return CLATVB_EINVAL; }
    if (!net || !lat) { snprintf(msg, cap, "%s: net (kappa0, nu0) or lat (sigma, mu_b, sigma_b) is NULL", what); return CLATVB_EINVAL; }
    if (cnetvb_check_net(what, net, true, msg, cap) != CNETVB_OK) return CLATVB_EINVAL;
    if (D < 1 || D > CLATVB_MAX_DIMS) {                            // before Z is read: its length needs D
        snprintf(msg, cap, "%s: n_dims = %d must lie in 1..%d", what, (int)D, CLATVB_MAX_DIMS);
        return CLATVB_EINVAL;
    }
    if (J < 0 || J > CLATVB_MAX_ASCENT) {
        snprintf(msg, cap, "%s: ascent_steps = %d must lie in 0..%d", what, (int)J, CLATVB_MAX_ASCENT);
        return CLATVB_EINVAL;
    }
    if (!cnetvb_positive(lat[0]) || !cnetvb_positive(lat[2]) || !std::isfinite(lat[1])) {
        snprintf(msg, cap, "%s: the network's sigma = %g, sigma_b = %g must be positive and finite, mu_b = %g finite", what, lat[0], lat[2], lat[1]);
        return CLATVB_EINVAL;
    }
    if (!Z) { snprintf(msg, cap, "%s: Z (z_v, b_v) is NULL", what); return CLATVB_EINVAL; }
    if (Z_on_device) return CLATVB_OK;
    const size_t n = clatvb_z_doubles(N > 0 ? (size_t)N : 0, (size_t)D);
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(Z[i])) {
            snprintf(msg, cap, "%s: %s = %g is not finite", what, i + 1 < n ? "a position of z_v" : "b_v", Z[i]);
            return CLATVB_EINVAL;
        }
    return CLATVB_OK;
}

// Q = [κv0 (N²); νv0 (N²); ρv (N²)] in host memory, read where a state is (a step from a state, a resumed run) together with
// the slab's (kv1, nv1): cnetvb_check_planes
inline int clatvb_check_state(const char *what, size_t N, bool state, const double *Q, const double *kv1, const double *nv1, char *msg, size_t cap)
{
    return cnetvb_check_planes(what, N, state, Q, kv1, nv1, msg, cap) == CNETVB_OK ? CLATVB_OK : CLATVB_EINVAL;
}

// doubles of one device state: surrogate, S, R (P each), Q's three planes, Z, the per-node link sums at its own (zv, bv) and the
// partial sums of its pieces
inline size_t clatvb_state_doubles(size_t P, size_t N, size_t D, size_t blocks)
{
    return 3 * P + 3 * N * N + clatvb_z_doubles(N, D) + N + (size_t)CNETVB_PIECES * blocks;
}
// what both states share: C = ρv + ρvᵀ [N²], G = ∇F [N·D + 1], the per-node halves of ∂F/∂b [N], the per-node sums of every slot
// [N·9], the iteration's scalars and the rungs taken [64]
inline size_t clatvb_scratch_doubles(size_t N, size_t D)
{
    return N * N + clatvb_z_doubles(N, D) + N + N * (size_t)CLATVB_SLOTS + (size_t)CLATVB_SC + (size_t)CLATVB_MAX_ASCENT;
}
// ... and what a step or a run reserves: two states, the scratch and the scalars of two ELBO evaluations
inline size_t clatvb_reserve_doubles(size_t P, size_t N, size_t D, size_t blocks)
{
    return 2 * clatvb_state_doubles(P, N, D, blocks) + clatvb_scratch_doubles(N, D) + 2 * CLATVB_OUT;
}
// nhp_latent_expected_loglik: ρ, C, Z, G, the halves, one slot per node, the scalars and out [N·D + 2]
inline size_t clatvb_loglik_doubles(size_t N, size_t D)
{
    return 2 * N * N + 2 * clatvb_z_doubles(N, D) + 2 * N + (size_t)CLATVB_SC + clatvb_z_doubles(N, D) + 1;
}
