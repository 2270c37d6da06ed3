// Host-only parts of the continuous BLOCK-network variational fit (cont_netvb.hip): the argument checks that
// run before any launch and the sizing of the device state, on top of the Bernoulli fit's (nhp_cnetvb.h) and the block
// model's (nhp_sbmvb.h).  Plain C++ with no HIP in it, so that a stand-alone program can run it under the host sanitizers
// (tools/csbmvb_host_check.cpp).
#pragma once
#include <vector>

#include "nhp_cnetvb.h"
#include "nhp_sbmvb.h"

enum { CSBMVB_OK = 0, CSBMVB_EINVAL = 1, CSBMVB_ENOTIMPL = 2 };
constexpr int CSBMVB_NET_PIECES = 5;                              // Σ entropy of ρv, links, labels, KL_Dir, Σ KL_Beta
constexpr int CSBMVB_OUT = 8 + CSBMVB_NET_PIECES;                 // k_csbmvb_elbo: k_cnetvb_elbo's eight, then the network pieces
constexpr int CSBMVB_STATS = 11 + 2 * CSBMVB_NET_PIECES;          // nhp_cont_sbmvb_step: the Bernoulli step's eleven, pieces before, after

// B = [vec αv; vec βv; γv; vec mv], column-major: StochasticBlockNetworkModel.variational_params()
inline size_t csbmvb_b_doubles(size_t N, size_t K) { return 2 * K * K + K + N * K; }
// T = [T1; T0; Σ_n m]: Σ_pc ω ρv, Σ_pc ω (1 - ρv) and the label masses of a state at its own m
inline size_t csbmvb_t_doubles(size_t K) { return 2 * K * K + K; }

// net = [κ0, ν0] (the spike's Gamma), sbm = [α, β, γ], the schedule and the block state B.  `dense`: the caller set
// NHP_VB_DENSE_NETWORK, which has no meaning here.  `B_on_device`: B is a device pointer, so its entries cannot be read here;
// every other check (K, the schedule, the priors, the sweep's LDS need) is the same one, run on a stand-in state of the same
// shape that passes the entry checks.
inline int csbmvb_check_args(const char *what, int64_t N, const double *net, const double *sbm, int32_t K, int32_t labels_every, int64_t step0,
                             bool dense, const double *B, char *msg, size_t cap, bool B_on_device = false)
{
    if (cap) msg[0] = 0;
    if (dense) { snprintf(msg, cap, "%s: NHP_VB_DENSE_NETWORK has no meaning for a block network", what); return CSBMVB_EINVAL; }
    if (!net || !sbm) { snprintf(msg, cap, "%s: net (kappa0, nu0) or sbm (alpha, beta, gamma) is NULL", what); return CSBMVB_EINVAL; }
    if (cnetvb_check_net(what, net, true, msg, cap) != CNETVB_OK) return CSBMVB_EINVAL;
    if (step0 < 0) { snprintf(msg, cap, "%s: step0 = %lld must be >= 0", what, (long long)step0); return CSBMVB_EINVAL; }
    if (K < 1 || K > SBMVB_MAX_BLOCKS) {                          // before B is carved: its offsets need K
        snprintf(msg, cap, "%s: n_blocks = %d must lie in 1..%d", what, (int)K, (int)SBMVB_MAX_BLOCKS);
        return CSBMVB_EINVAL;
    }
    if (!B) { snprintf(msg, cap, "%s: B (alpha_v, beta_v, gamma_v, m) is NULL", what); return CSBMVB_EINVAL; }
    const size_t KK = (size_t)K * (size_t)K;
    std::vector<double> stand_in;
    if (B_on_device) {                                             // tables of ones, every node in block 0
        const size_t n = N > 0 ? (size_t)N : 0;
        stand_in.assign(csbmvb_b_doubles(n, (size_t)K), 1.0);
        for (size_t i = n; i < n * (size_t)K; ++i) stand_in[2 * KK + (size_t)K + i] = 0.0;
        B = stand_in.data();
    }
    const int rc = sbmvb_check_args(what, N, K, sbm[0], sbm[1], sbm[2], labels_every, B + 2 * KK + (size_t)K, B, B + KK, B + 2 * KK, msg, cap);
    return rc == NETVB_OK ? CSBMVB_OK : rc == NETVB_ENOTIMPL ? CSBMVB_ENOTIMPL : CSBMVB_EINVAL;
}

// Q = [κv0 (N²); νv0 (N²); ρv (N²)] in host memory, read where a state is (a step from a state, a resumed run) together with
// the slab's (kv1, nv1): cnetvb_check_planes
inline int csbmvb_check_state(const char *what, size_t N, bool state, const double *Q, const double *kv1, const double *nv1, char *msg, size_t cap)
{
    return cnetvb_check_planes(what, N, state, Q, kv1, nv1, msg, cap) == CNETVB_OK ? CSBMVB_OK : CSBMVB_EINVAL;
}

// doubles of one device state: surrogate, S, R (P each), Q's three planes, B, T and the partial sums of its pieces
inline size_t csbmvb_state_doubles(size_t P, size_t N, size_t K, size_t blocks)
{
    return 3 * P + 3 * N * N + csbmvb_b_doubles(N, K) + csbmvb_t_doubles(K) + (size_t)CNETVB_PIECES * blocks;
}
// what both states share: D [K²], E1, E0, E1ᵀ, E0ᵀ [4K²], Eπ [K], m·D, U1, U0 [N·K each]
inline size_t csbmvb_scratch_doubles(size_t N, size_t K) { return 5 * K * K + K + 3 * N * K; }
// ... and what a step or a run reserves: two states, the scratch and the scalars of two ELBO evaluations
inline size_t csbmvb_reserve_doubles(size_t P, size_t N, size_t K, size_t blocks)
{
    return 2 * csbmvb_state_doubles(P, N, K, blocks) + csbmvb_scratch_doubles(N, K) + 2 * CSBMVB_OUT;
}

// lnΓ(Kγ) − K lnΓ(γ): the prior's constant in KL(Dir(γv) ‖ Dir(γ·1_K))
inline double csbmvb_dir_const(double gamma, int32_t K) { return std::lgamma((double)K * gamma) - (double)K * std::lgamma(gamma); }
