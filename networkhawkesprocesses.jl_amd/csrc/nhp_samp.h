// The categorical weights of one event's parent assignment, shared by the parent sampler (cont_sampler.hip) and the
// most-likely-parent walk (cont_cascades.hip): A·W·ħ(t_i - t_j) for a parent j of the look-back window, λ0_c(t_i) for the
// baseline.  Every weight is evaluated with the fixed operation sequence of nhp_math.h (nothing contracted), so both
// translation units -- and the CPU checker -- produce the same bits.
#pragma once
#include "nhp_internal.h"
#include "nhp_math.h"

struct samp_col {                  // staged column c of the parameter tables
    const double2 *col;            // exp: {rate, a*w};  logit-normal: {mu, sqrt(tau)}
    const double *colw;            // logit-normal: a*w
};

template <int IMP>
__device__ __forceinline__ double samp_weight(const nhp_cont_args &a, const samp_col &sc, double t, int j)
{
#pragma clang fp contract(off)
    const nhp_event e = a.ev[j];                  // one 16-byte load: (t_j, n_j)
    const double dt = t - e.t;
    const int p = e.node;
    const double2 q = sc.col[p];
    if (IMP == NHP_IMPULSE_EXPONENTIAL) return q.y * nhp_pdf_exponential(q.x, dt);
    return sc.colw[p] * nhp_pdf_logitnormal(q.x, q.y, a.inv_dtmax, dt);
}

// Weight k of a child through the logit-normal pair cache (lq, nd already point at the child's first pair): the logarithm and
// the division of the pdf were taken when the cache was built, with the same operations -- the same bits.
__device__ __forceinline__ double samp_weight_cached(const samp_col &sc, const double2 d, const int p)
{
#pragma clang fp contract(off)
    const double2 q = sc.col[p];
    return sc.colw[p] * nhp_pdf_logitnormal_cached(q.x, q.y, d);
}

__device__ __forceinline__ double samp_baseline(const nhp_cont_args &a, int c, double t)
{
#pragma clang fp contract(off)
    if (a.baseline_kind == NHP_BASELINE_HOMOGENEOUS) return a.lambda0[c];
    const double *x = a.grid;
    const double *y = a.lambda0 + (size_t)c * a.grid_n;
    int lo = 0, hi = a.grid_n - 1;
    if (!(t < x[hi])) return y[hi];
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (t >= x[mid]) lo = mid; else hi = mid;
    }
    return (y[lo + 1] * (t - x[lo]) + y[lo] * (x[lo + 1] - t)) / (x[lo + 1] - x[lo]);
}
