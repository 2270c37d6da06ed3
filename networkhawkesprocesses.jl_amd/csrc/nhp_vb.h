// Device pieces the continuous variational fits share (cont_vb.hip: the standard process; cont_netvb.hip: the network
// process under a dense, Bernoulli or block network): the launch arguments, one baseline factor and one link's factors with
// their surrogates and ELBO pieces, the conjugate update of both, the start kernel's body, the store and the fixed-order sum
// of the partial sums, and the hyper-parameter check.  The host drivers all six entry points run through: nhp_vb_drive.h.
#pragma once
#include <cmath>

#include "nhp_cnetvb.h"
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

// part[piece·VB_BLK + blockIdx.x] = this workgroup's share of each piece
template <int PIECES>
__device__ __forceinline__ void vb_store(const double (&v)[PIECES], double *__restrict__ part)
{
    __shared__ double red[4];
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
        const double t = nhp_block_sum_n<4>(v[j], red);
        if (threadIdx.x == 0) part[j * VB_BLK + blockIdx.x] = t;
    }
}

// tot[piece] = the VB_BLK partial sums of each piece in one fixed order: the opening of every ELBO kernel (one workgroup of 256)
template <int PIECES>
__device__ __forceinline__ void vb_sum_parts(const double *__restrict__ part, double *tot, double *red)
{
    for (int j = 0; j < PIECES; ++j) {
        double v = 0.0;
        for (int b = threadIdx.x; b < VB_BLK; b += 256) v += part[j * VB_BLK + b];
        v = nhp_block_sum_n<4>(v, red);
        if (threadIdx.x == 0) tot[j] = v;
    }
}

// iteration 0 (k_vb_start, k_cnetvb_start): an ordinary parameter vector used as if it were a surrogate; only the part of its
// ll to undo has a meaning, the other PIECES - 1 are stored as zeros
template <int PIECES>
__device__ __forceinline__ void vb_start_body(const vb_args &a, const double *xin, double *x, double *part)
{
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    double v[PIECES] = {};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { const double l = xin[i]; x[i] = l; v[0] += a.T * l; continue; }
        const size_t k = i - N;
        const double w = xin[L.W + k];
        vb_write(a, L, x, k, w, xin[L.p1 + k], a.impulse != NHP_IMPULSE_EXPONENTIAL ? xin[L.p2 + k] : 0.0);
        v[0] += (a.cnt ? a.cnt[k % N] : 0.0) * w;
    }
    vb_store<PIECES>(v, part);
}

// The conjugate update every fit shares, from the surrogate x and the gradient g at it (cont_em.hip's identities; nothing is
// divided by W̃).  Baseline entry i: Gamma(α0 + bg, β0 + T) into S, R, its surrogate into xn, its pieces into s.
__device__ __forceinline__ void vb_update_baseline(const vb_args &a, const double *x, const double *g, size_t i,
                                                   double *S, double *R, double *xn, vb_acc &s)
{
    const double al = a.pr.alpha0 + x[i] * (g[i] + a.T), be = a.pr.beta0 + a.T;
    S[i] = al; R[i] = be;
    xn[i] = vb_baseline(a, al, be, s);
}
// Link k with cp events of its parent: EM = x·(g + cp) of its weight ...
__device__ __forceinline__ double vb_link_em(const nhp_layout &L, const double *x, const double *g, size_t k, double cp)
{
    return x[L.W + k] * (g[L.W + k] + cp);
}
// ... and the impulse's factor (m, kk, sa, sb) from it, written into its planes of S, R.  The weight's factor(s) are the caller's,
// formed from EM BEFORE this call: a product fuses with a sum of its own basic block only, and the bits of the weight's shape
// depend on that.  No contraction pragma: the callers' default holds, as before these lines were shared.
__device__ __forceinline__ void vb_update_impulse(const vb_args &a, const nhp_layout &L, const double *x, const double *g,
                                                  size_t k, double EM, double *S, double *R, double &m, double &kk,
                                                  double &sa, double &sb)
{
    const nhp_gibbs_priors &q = a.pr;
    m = 0.0; kk = 1.0;
    if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
        sa = q.a + EM;
        sb = q.b + (EM / x[L.p1 + k] - g[L.p1 + k]);
        S[L.p1 + k] = sa; R[L.p1 + k] = sb;
    } else {
        const double c = x[L.p1 + k], tau = x[L.p2 + k];
        const double D1 = g[L.p1 + k] / tau, S2 = EM / tau - 2.0 * g[L.p2 + k], d0 = q.mu_mu - c;
        kk = q.kappa_mu + EM;
        const double dm = (D1 + q.kappa_mu * d0) / kk;
        m = c + dm;
        sa = q.a + 0.5 * EM;
        sb = q.b + 0.5 * ((S2 + q.kappa_mu * (d0 * d0)) - kk * (dm * dm));
        S[L.p1 + k] = m; R[L.p1 + k] = kk;
        S[L.p2 + k] = sa; R[L.p2 + k] = sb;
    }
}

inline bool vb_positive(double v) { return v > 0.0 && std::isfinite(v); }

// the hyper-parameters of every continuous variational entry point (κμ and μμ are read for logit-normal impulses only)
inline nhp_status vb_check_priors(nhp_ctx *ctx, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const char *what)
{
    const bool ln = m->impulse_kind != NHP_IMPULSE_EXPONENTIAL;
    if (!vb_positive(pr->alpha0) || !vb_positive(pr->beta0) || !vb_positive(pr->kappa) || !vb_positive(pr->nu) || !vb_positive(pr->a) ||
        !vb_positive(pr->b) || (ln && (!vb_positive(pr->kappa_mu) || !std::isfinite(pr->mu_mu)))) {
        nhp_set_error(ctx, "%s: every prior hyper-parameter but the mean μμ must be positive and finite", what);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

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
