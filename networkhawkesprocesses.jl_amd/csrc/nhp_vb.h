// Device pieces the continuous variational fits share (cont_vb.hip: the standard process; cont_netvb.hip: the network
// process): the launch arguments, one baseline factor and one link's factors with their surrogates and ELBO pieces.
#pragma once
#include <cmath>

#include "nhp_internal.h"
#include "nhp_math.h"

constexpr int VB_BLK = 1024;         // workgroups of the O(P) passes = partial sums per piece (four per CU, as cont_em.hip)

struct vb_args {
    int N, impulse;
    double T;
    const double *cnt;               // [N] events per node (null: an empty dataset)
    nhp_gibbs_priors pr;
    double lg_alpha0, lg_kappa, lg_a;               // lnΓ of the prior shapes and the logarithms of the prior rates, once on the host
    double log_beta0, log_nu, log_b, log_kmu;
};

struct vb_acc { double fix = 0.0, comp = 0.0, kl0 = 0.0, klw = 0.0, kli = 0.0; };

__device__ __forceinline__ nhp_layout vb_layout(const vb_args &a) { return nhp_layout(a.N, 0, NHP_BASELINE_HOMOGENEOUS, a.impulse); }

// KL(Gamma(a1, b1) ‖ Gamma(a0, b0)) with ψ(a1), lnΓ(a1) and log b1 at hand
__device__ __forceinline__ double vb_kl_gamma(double a1, double b1, double psi1, double lg1, double logb1, double a0, double b0, double lg0,
                                              double logb0)
{
    return (a1 - a0) * psi1 - lg1 + lg0 + a0 * (logb1 - logb0) + a1 * (b0 - b1) / b1;
}

// one baseline factor Gamma(al, be): its surrogate λ̃0, and its pieces into s
__device__ __forceinline__ double vb_baseline(const vb_args &a, double al, double be, vb_acc &s)
{
    double psi, lg;
    nhp_digamma_lgamma(al, psi, lg);
    const double lb = nhp_log(be);
    const double lam = nhp_exp(psi - lb);
    s.fix += a.T * lam;
    s.comp += a.T * (al / be);
    s.kl0 += vb_kl_gamma(al, be, psi, lg, lb, a.pr.alpha0, a.pr.beta0, a.lg_alpha0, a.log_beta0);
    return lam;
}

// one link's factors -- W ~ Gamma(ka, nu), impulse Gamma(sa, sb) | NormalGamma(m, kk, sa, sb) -- : its surrogates (w, p1, p2)
// and its pieces into s; cp = cnt of the parent node
__device__ __forceinline__ void vb_pair(const vb_args &a, double cp, double ka, double nu, double m, double kk, double sa, double sb,
                                        vb_acc &s, double &w, double &p1, double &p2)
{
    const nhp_gibbs_priors &q = a.pr;
    double psik, lgk, psia, lga;
    nhp_digamma_lgamma(ka, psik, lgk);
    nhp_digamma_lgamma(sa, psia, lga);
    const double lnu = nhp_log(nu), lsb = nhp_log(sb);
    const double ela = psia - nhp_log(sa), prec = sa / sb;
    double kl = vb_kl_gamma(sa, sb, psia, lga, lsb, q.a, q.b, a.lg_a, a.log_b);
    if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
        w = nhp_exp((psik - lnu) + ela);
        p1 = prec; p2 = 0.0;
    } else {
        w = nhp_exp((psik - lnu) + (0.5 * ela - 0.5 / kk));
        p1 = m; p2 = prec;
        const double dm = m - q.mu_mu;
        kl += 0.5 * ((q.kappa_mu / kk - 1.0) + (nhp_log(kk) - a.log_kmu) + q.kappa_mu * prec * (dm * dm));
    }
    s.fix += cp * w;
    s.comp += cp * (ka / nu);
    s.klw += vb_kl_gamma(ka, nu, psik, lgk, lnu, q.kappa, q.nu, a.lg_kappa, a.log_nu);
    s.kli += kl;
}

__device__ __forceinline__ void vb_write(const vb_args &a, const nhp_layout &L, double *__restrict__ x, size_t k, double w, double p1, double p2)
{
    x[L.W + k] = w; x[L.p1 + k] = p1;
    if (a.impulse != NHP_IMPULSE_EXPONENTIAL) x[L.p2 + k] = p2;
}

inline bool vb_positive(double v) { return v > 0.0 && std::isfinite(v); }

inline vb_args vb_make_args(const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr)
{
    vb_args a{};
    a.N = m->N; a.impulse = m->impulse_kind;
    a.T = ds->duration;
    a.cnt = ds->M > 0 ? ds->d_cnt : nullptr;
    a.pr = *pr;
    a.lg_alpha0 = std::lgamma(pr->alpha0); a.lg_kappa = std::lgamma(pr->kappa); a.lg_a = std::lgamma(pr->a);
    a.log_beta0 = std::log(pr->beta0); a.log_nu = std::log(pr->nu); a.log_b = std::log(pr->b);
    a.log_kmu = m->impulse_kind != NHP_IMPULSE_EXPONENTIAL ? std::log(pr->kappa_mu) : 0.0;
    return a;
}
