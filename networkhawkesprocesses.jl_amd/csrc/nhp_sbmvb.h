// Host-only parts of the block-model VB / SVI entry points (disc_vb.hip): the argument checks that run before
// any launch, the LDS need of the label sweep and the sizing of the device scratch.  Plain C++ with no HIP in it, so that
// a stand-alone program can run it under the host sanitizers (tools/sbmvb_host_check.cpp).
#pragma once
#include "nhp_netvb.h"

enum { SBMVB_MAX_BLOCKS = 64, SBMVB_THREADS = 256, SBMVB_WAVES = 4, SBMVB_LDS_LIMIT = 160 * 1024 };

// the sweep deals its 256 threads as (block l, node group g) with l below the next power of two of K
inline size_t sbmvb_pow2(size_t K)
{
    size_t p = 1;
    while (p < K) p <<= 1;
    return p;
}

// Bytes of LDS k_sbmvb_sweep asks for: m [N·K], row n and column n of ρv [2·N], the four sums of each wave
// [4 waves · 4 · Kp] and their totals [4 · Kp]
inline size_t sbmvb_sweep_lds_bytes(size_t N, size_t K)
{
    const size_t Kp = sbmvb_pow2(K);
    return 8 * (N * K + 2 * N + (size_t)SBMVB_WAVES * 4 * Kp + 4 * Kp);
}

// E1, E0 and their transposes: the sweep copies them to LDS too when they fit next to the above (an optimisation, not a need:
// above the limit they stay in global memory and the limit itself is sbmvb_sweep_lds_bytes)
inline size_t sbmvb_sweep_table_bytes(size_t K) { return 8 * 4 * K * K; }

// Doubles of device scratch the block model's state takes after netvb_param_doubles: the state (m, αv, βv, γv), its hats
// (a second copy: SVI blends into the state, VB leaves it unused), the expectation tables D, E1, E0, E1ᵀ, E0ᵀ, Eπ,
// m·D, U1, U0 and (SVI) ρ̂v
inline size_t sbmvb_state_doubles(size_t N, size_t K) { return N * K + 2 * K * K + K; }
inline size_t sbmvb_param_doubles(size_t N, size_t K, bool svi)
{
    return 2 * sbmvb_state_doubles(N, K) + 5 * K * K + K + 3 * N * K + (svi ? N * N : 0);
}

// The checks of nhp_disc_sbmvb_run / nhp_disc_sbmsvi_run on the block model's own arguments (the process's go through
// netvb_check_args).  Returns NETVB_OK, or a status with a message in msg[cap].
inline int sbmvb_check_args(const char *what, int64_t N, int32_t K, double alpha, double beta, double gamma, int32_t labels_every,
                            const double *m, const double *alpha_v, const double *beta_v, const double *gamma_v, char *msg, size_t cap)
{
    if (cap) msg[0] = 0;
    if (N < 1) { snprintf(msg, cap, "%s: the dataset has no nodes", what); return NETVB_EINVAL; }
    if (K < 1 || K > SBMVB_MAX_BLOCKS) { snprintf(msg, cap, "%s: n_blocks = %d must lie in 1..%d", what, (int)K, (int)SBMVB_MAX_BLOCKS); return NETVB_EINVAL; }
    if (labels_every < 1) { snprintf(msg, cap, "%s: labels_every = %d must be positive", what, (int)labels_every); return NETVB_EINVAL; }
    if (!m || !alpha_v || !beta_v || !gamma_v) { snprintf(msg, cap, "%s: a block-model array (m, alpha_v, beta_v, gamma_v_net) is NULL", what); return NETVB_EINVAL; }
    if (!(alpha > 0.0) || !(beta > 0.0) || !(gamma > 0.0) || !std::isfinite(alpha + beta + gamma)) {
        snprintf(msg, cap, "%s: the block model's priors alpha, beta, gamma must be > 0 and finite", what);
        return NETVB_EINVAL;
    }
    const size_t n = (size_t)N, k = (size_t)K;
    for (size_t i = 0; i < k * k; ++i)
        if (!(alpha_v[i] > 0.0) || !(beta_v[i] > 0.0) || !std::isfinite(alpha_v[i] + beta_v[i])) {
            snprintf(msg, cap, "%s: the block model's alpha_v, beta_v at entry %zu must be > 0 and finite", what, i);
            return NETVB_EINVAL;
        }
    for (size_t i = 0; i < k; ++i)
        if (!(gamma_v[i] > 0.0) || !std::isfinite(gamma_v[i])) { snprintf(msg, cap, "%s: gamma_v_net[%zu] must be > 0 and finite", what, i); return NETVB_EINVAL; }
    for (size_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (size_t j = 0; j < k; ++j) {
            const double v = m[i + j * n];
            if (!(v >= 0.0)) { snprintf(msg, cap, "%s: m[%zu, %zu] = %g is negative or not a number", what, i, j, v); return NETVB_EINVAL; }
            s += v;
        }
        if (!(std::fabs(s - 1.0) <= 1e-12)) { snprintf(msg, cap, "%s: row %zu of m sums to %.17g, not to 1 within 1e-12", what, i, s); return NETVB_EINVAL; }
    }
    const size_t lds = sbmvb_sweep_lds_bytes(n, k);
    if (lds > (size_t)SBMVB_LDS_LIMIT) {
        snprintf(msg, cap, "%s: the label sweep keeps m in LDS and needs %zu bytes for N = %zu, K = %zu; a CU has %d", what, lds, n, k, (int)SBMVB_LDS_LIMIT);
        return NETVB_ENOTIMPL;
    }
    return NETVB_OK;
}
