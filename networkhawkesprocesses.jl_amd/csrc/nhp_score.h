// What the two chain scorers share (disc_score.hip, cont_score.hip): one more value into a running
// log-sum-exp, a workgroup's sum in one fixed order, the fold of a draw's workgroup partials into the joint scalars and the
// two stages over the nodes at fetch.  Included by both translation units; every kernel here is instantiated in each.
#pragma once
#include "nhp_internal.h"

// one more value into a running log-sum-exp
__device__ __forceinline__ double score_lse(double a, double b)
{
    const double d = a == b ? 0.0 : fabs(a - b);               // (equal infinities: no NaN)
    return fmax(a, b) + log1p(exp(-d));
}

// Σ over `n` values at x (stride 1), one workgroup, one fixed order; valid in thread 0
__device__ __forceinline__ double score_sum(const double *__restrict__ x, int64_t n, double *red)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += x[i];
    return nhp_block_sum(s, red);
}

// the draw's total over the scored cells, and the joint scalars (one workgroup).  joint: 0 lse, 1 mean, 2 M2 of the draw's
// total, 3 the latest total, 4 a data-only constant taken off the total (the discrete scorer's Σ loggamma(s + 1); else 0)
static __global__ __launch_bounds__(256) void k_score_fold(const double *__restrict__ partials, int64_t np, double n, double *__restrict__ joint)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    const double s = score_sum(partials, np, red);
    if (threadIdx.x != 0) return;
    const double tot = s - joint[4];
    if (n == 1.0) {
        joint[0] = tot; joint[1] = tot; joint[2] = 0.0;
    } else {
        const double mean = joint[1], d = tot - mean, mean1 = mean + d / n;
        joint[0] = score_lse(joint[0], tot);
        joint[1] = mean1;
        joint[2] = joint[2] + d * (tot - mean1);
    }
    joint[3] = tot;
}

// over the nodes, one workgroup.  STAGE 0: tot[0..2] = Σ_c of the three column sums, tot[3] = mean elpd_i.  STAGE 1: the
// summary (tot[4..13], the order of nhp_disc_score_fetch / nhp_cont_score_fetch).
template <int STAGE>
static __global__ __launch_bounds__(256) void k_score_total(const double *__restrict__ col, int N, double cells, double S, double logS,
                                                            const double *__restrict__ joint, double *__restrict__ tot)
{
#pragma clang fp contract(off)
    __shared__ double red[NHP_WAVES];
    if (STAGE == 0) {
        const double lppd = score_sum(col, N, red), p = score_sum(col + N, N, red), e = score_sum(col + 2 * (size_t)N, N, red);
        if (threadIdx.x == 0) { tot[0] = lppd; tot[1] = p; tot[2] = e; tot[3] = e / cells; }
    } else {
        const double ss = score_sum(col + 3 * (size_t)N, N, red);
        if (threadIdx.x == 0) {
            double *o = tot + 4;
            o[0] = S; o[1] = cells; o[2] = tot[0]; o[3] = tot[1]; o[4] = tot[2]; o[5] = -2.0 * tot[2];
            o[6] = sqrt(cells * (ss / (cells - 1.0)));
            o[7] = joint[0] - logS; o[8] = joint[1]; o[9] = sqrt(joint[2] / (S - 1.0));
        }
    }
}
