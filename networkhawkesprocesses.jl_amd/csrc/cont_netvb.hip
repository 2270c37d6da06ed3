// Mean-field variational inference for the continuous NETWORK Hawkes process (spike-and-slab weights under a dense or
// Bernoulli network), with the whole iteration on the device.  The definition is in include/nhp.h (nhp_cont_netvb_run).
//
// The likelihood is cont_vb.hip's full-mass one; the network acts through the prior of W alone: A[p,c] ~ Bernoulli(ρ),
// W[p,c] | A = a ~ Gamma(κ_a, ν_a) (a = 0 the spike, a = 1 the slab), ρ ~ Beta(α, β).  Factors: q(A = 1) = ρv,
// q(W | A = a) = Gamma(κv_a, νv_a), q(ρ) = Beta(αv, βv); λ0 and the impulses as in cont_vb.hip.  So the surrogate differs in
//   E log W = (1 - ρv)(ψ(κv0) - log νv0) + ρv (ψ(κv1) - log νv1)
// only (two products and a sum, contraction off: ρv = 1 gives the slab's term exactly, hence cont_vb.hip's bits), the
// E-step is em!'s at x̃ on a view of the model WITHOUT its adjacency matrix, and one O(P) pass (k_cnetvb_update) makes
//   κv_a = κ_a + EM, νv_a = ν_a + cnt_p,    logit ρv = [ψ(αv) - ψ(βv)]_old + prior + [lnΓκv1 - lnΓκv0] - [κv1 log νv1 - κv0 log νv0]
// in the cancellation-free form of nhp_math.h (netvb_logit), the next surrogate, and per-workgroup partial sums of eight
// pieces: cont_vb.hip's five, Σ[ρv log ρv + (1-ρv) log(1-ρv)], Σρv, Σ(1-ρv).  k_cnetvb_elbo (one workgroup) adds them in a fixed
// order, forms the state's (αv, βv) = (α + Σρv, β + Σ(1-ρv)), finishes KL_net and L, and leaves ψ(αv) - ψ(βv) behind the pair
// for the next update.  No atomics.  lnΓ: the pass has lnΓ(κv0), lnΓ(κv1) from nhp_digamma_lgamma for KL_W, so below 16 the
// logit's lnΓ difference is their difference (no library lgamma, no scratch) and from 16 on the Stirling form.
#include <algorithm>
#include <cmath>

#include "nhp_cnetvb.h"
#include "nhp_csbmvb.h"
#include "nhp_internal.h"
#include "nhp_math.h"
#include "nhp_sbmvb_dev.h"
#include "nhp_vb.h"

namespace {

struct cn_args {
    vb_args v;                       // pr.kappa, pr.nu (and lg_kappa, log_nu): the slab's
    double k0, n0, lg_k0, log_n0;    // the spike's Gamma, lnΓ(κ0), log ν0
    double dk, dn, prior;            // κ1 - κ0, ν1 - ν0, the prior's share of the logit
    double alpha, beta, beta_const;  // Beta prior of ρ and lnΓ(α+β) - lnΓα - lnΓβ
    int dense;
};

struct cn_acc : vb_acc { double ent = 0.0, sr = 0.0, s1r = 0.0; };

// a state on the device: surrogate, planes, Q = [κv0; νv0; ρv; αv, βv, ψ(αv) - ψ(βv)], partial sums
struct cn_state { double *x, *S, *R, *Q, *part; };

__device__ __forceinline__ void cn_store(const cn_acc &s, double *__restrict__ part)
{
    __shared__ double red[4];
    const double v[CNETVB_PIECES] = {s.fix, s.comp, s.kl0, s.klw, s.kli, s.ent, s.sr, s.s1r};
#pragma unroll
    for (int j = 0; j < CNETVB_PIECES; ++j) {
        const double t = nhp_block_sum_n<4>(v[j], red);
        if (threadIdx.x == 0) part[j * VB_BLK + blockIdx.x] = t;
    }
}

// lnΓ(κv1) - lnΓ(κv0) with both values at hand: their difference below 16, inside Stirling's formula from there on
// (nhp_math.h's netvb_lgamma_diff with the library lgamma replaced; cn_logit below is its netvb_logit: keep them in step)
__device__ __forceinline__ double cn_lgamma_diff(double kv0, double dk, double kv1, double lg0, double lg1)
{
    if (kv0 < 16.0 || kv1 < 16.0) return lg1 - lg0;
    return ((kv0 - 0.5) * log1p(dk / kv0) + dk * nhp_log(kv1) - dk) + (netvb_stirling_tail(kv1) - netvb_stirling_tail(kv0));
}

// netvb_logit with the lnΓ difference, log1p(dn/νv0) and log νv1 at hand; r0·e0 + r1·e1 as two products and a sum, so that
// r1 = 1 (r0 = 0) gives e1 exactly
__device__ __forceinline__ double cn_logit(double net_prior, double lgd, double kv0, double l1p, double dk, double ln1)
{
#pragma clang fp contract(off)
    return (net_prior + lgd) - (kv0 * l1p + dk * ln1);
}
__device__ __forceinline__ double cn_mix(double r0, double e0, double r1, double e1)
{
#pragma clang fp contract(off)
    return r0 * e0 + r1 * e1;
}

// ψ, lnΓ of a link's two weight shapes and the logarithms of its two rates: what the logit and the pieces share
struct cn_tab { double psi0, lg0, psi1, lg1, ln0, ln1; };
__device__ __forceinline__ cn_tab cn_tables(double kv0, double nv0, double kv1, double nv1)
{
    cn_tab t;
    nhp_digamma_lgamma(kv0, t.psi0, t.lg0);
    nhp_digamma_lgamma(kv1, t.psi1, t.lg1);
    t.ln0 = nhp_log(nv0); t.ln1 = nhp_log(nv1);
    return t;
}

// q(A = 1) from the new (kv, nv) and `net` = ψ(αv) - ψ(βv) of the state stepped from
__device__ __forceinline__ double cn_rho(const cn_args &A, double net, double kv0, double nv0, double kv1, const cn_tab &t)
{
    return netvb_sigmoid(cn_logit(net + A.prior, cn_lgamma_diff(kv0, A.dk, kv1, t.lg0, t.lg1), kv0, log1p(A.dn / nv0), A.dk, t.ln1));
}

// One link's factors -- spike Gamma(kv0, nv0), slab Gamma(kv1, nv1), q(A = 1) = rho, the impulse's as vb_pair -- : its
// surrogates and its pieces into s.  One function for the state a caller gave (k_cnetvb_surrogate) and the state an update
// made (k_cnetvb_update), not contracted, so that a state's pieces do not depend on which kernel added them up.
__device__ __forceinline__ void cn_link(const cn_args &A, double cp, double kv0, double nv0, double kv1, double nv1, const cn_tab &t, double rho,
                                        double m, double kk, double sa, double sb, cn_acc &s, double &w, double &p1, double &p2)
{
#pragma clang fp contract(off)
    const vb_args &a = A.v;
    const nhp_gibbs_priors &q = a.pr;
    double psia, lga;
    nhp_digamma_lgamma(sa, psia, lga);
    const double lsb = nhp_log(sb);
    const double r1 = rho, r0 = 1.0 - rho;
    const double elw = cn_mix(r0, t.psi0 - t.ln0, r1, t.psi1 - t.ln1);
    const double ela = psia - nhp_log(sa), prec = sa / sb;
    double kl = vb_kl_gamma(sa, sb, psia, lga, lsb, q.a, q.b, a.lg_a, a.log_b);
    if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
        w = nhp_exp(elw + ela);
        p1 = prec; p2 = 0.0;
    } else {
        w = nhp_exp(elw + (0.5 * ela - 0.5 / kk));
        p1 = m; p2 = prec;
        const double dm = m - q.mu_mu;
        kl += 0.5 * ((q.kappa_mu / kk - 1.0) + (nhp_log(kk) - a.log_kmu) + q.kappa_mu * prec * (dm * dm));
    }
    s.fix += cp * w;
    s.comp += cp * (r0 * (kv0 / nv0) + r1 * (kv1 / nv1));
    const double kl0 = vb_kl_gamma(kv0, nv0, t.psi0, t.lg0, t.ln0, A.k0, A.n0, A.lg_k0, A.log_n0);
    const double kl1 = vb_kl_gamma(kv1, nv1, t.psi1, t.lg1, t.ln1, q.kappa, q.nu, a.lg_kappa, a.log_nu);
    s.klw += r0 * kl0 + r1 * kl1;
    s.kli += kl;
    if (!A.dense) {
        s.ent += (r1 > 0.0 ? r1 * nhp_log(r1) : 0.0) + (r0 > 0.0 ? r0 * nhp_log(r0) : 0.0);
        s.sr += r1; s.s1r += r0;
    }
}

// iteration 0: an ordinary parameter vector used as if it were a surrogate; only the part of its ll to undo has a meaning
__global__ __launch_bounds__(256) void k_cnetvb_start(cn_args A, const double *__restrict__ xin, double *__restrict__ x, double *__restrict__ part)
{
    const vb_args &a = A.v;
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    cn_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { const double v = xin[i]; x[i] = v; s.fix += a.T * v; continue; }
        const size_t k = i - N;
        const double w = xin[L.W + k];
        vb_write(a, L, x, k, w, xin[L.p1 + k], a.impulse != NHP_IMPULSE_EXPONENTIAL ? xin[L.p2 + k] : 0.0);
        s.fix += (a.cnt ? a.cnt[k % N] : 0.0) * w;
    }
    cn_store(s, part);
}

// the surrogate and the pieces of a given state (S, R, Q): the start of nhp_cont_netvb_step and of a resumed run
__global__ __launch_bounds__(256) void k_cnetvb_surrogate(cn_args A, const double *__restrict__ S, const double *__restrict__ R,
                                                          double *__restrict__ Q, double *__restrict__ x, double *__restrict__ part)
{
    const vb_args &a = A.v;
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    cn_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { x[i] = vb_baseline(a, S[i], R[i], s); continue; }
        const size_t k = i - N;
        const bool ln = a.impulse != NHP_IMPULSE_EXPONENTIAL;
        const size_t sh = ln ? L.p2 + k : L.p1 + k;                  // where the impulse's Gamma factor sits
        double rho = 1.0;
        if (A.dense) Q[2 * NN + k] = 1.0; else rho = Q[2 * NN + k];
        const double kv0 = Q[k], nv0 = Q[NN + k], kv1 = S[L.W + k], nv1 = R[L.W + k];
        double w, p1, p2;
        cn_link(A, a.cnt ? a.cnt[k % N] : 0.0, kv0, nv0, kv1, nv1, cn_tables(kv0, nv0, kv1, nv1), rho, ln ? S[L.p1 + k] : 0.0,
                ln ? R[L.p1 + k] : 1.0, S[sh], R[sh], s, w, p1, p2);
        vb_write(a, L, x, k, w, p1, p2);
    }
    cn_store(s, part);
}

// the coordinate-ascent update: factors (S, R, Q) from the surrogate x, the gradient g at it and the network scalars `old`
// = [αv, βv, ψ(αv) - ψ(βv)] of the state stepped from; their surrogate xn, their pieces
__global__ __launch_bounds__(256) void k_cnetvb_update(cn_args A, const double *__restrict__ x, const double *__restrict__ g,
                                                       const double *__restrict__ old, double *__restrict__ S, double *__restrict__ R,
                                                       double *__restrict__ Q, double *__restrict__ xn, double *__restrict__ part)
{
    const vb_args &a = A.v;
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    const nhp_gibbs_priors &q = a.pr;
    const double net = A.dense ? 0.0 : old[2];                       // (a dense network: no kernel writes the slot, no link reads it)
    if (A.dense && blockIdx.x == 0 && threadIdx.x < 2) Q[3 * NN + threadIdx.x] = old[threadIdx.x];     // (a dense network's pass through)
    cn_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) {
            const double al = q.alpha0 + x[i] * (g[i] + a.T), be = q.beta0 + a.T;
            S[i] = al; R[i] = be;
            xn[i] = vb_baseline(a, al, be, s);
            continue;
        }
        const size_t k = i - N;
        const double cp = a.cnt ? a.cnt[k % N] : 0.0;
        const double EM = x[L.W + k] * (g[L.W + k] + cp);
        const double kv1 = q.kappa + EM, nv1 = q.nu + cp, kv0 = A.k0 + EM, nv0 = A.n0 + cp;
        double m = 0.0, kk = 1.0, sa, sb;
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
        S[L.W + k] = kv1; R[L.W + k] = nv1;
        const cn_tab t = cn_tables(kv0, nv0, kv1, nv1);
        const double rho = A.dense ? 1.0 : cn_rho(A, net, kv0, nv0, kv1, t);
        double w, p1, p2;
        cn_link(A, cp, kv0, nv0, kv1, nv1, t, rho, m, kk, sa, sb, s, w, p1, p2);
        Q[k] = kv0; Q[NN + k] = nv0; Q[2 * NN + k] = rho;
        vb_write(a, L, xn, k, w, p1, p2);
    }
    cn_store(s, part);
}

// out = [Σ_i log λ̃_i = ll + fix, E_q[compensator], KL_λ0, KL_W, KL_imp, KL_net, L, 0]: the partial sums in one fixed order.
// net = the state's [αv, βv, ψ(αv) - ψ(βv)]: with form_new the pair is made here from the sums of ρv (the state came out of
// k_cnetvb_update), otherwise it is the caller's; the third is written in both cases.  A dense network: KL_net = 0, net untouched.
__global__ __launch_bounds__(256) void k_cnetvb_elbo(cn_args A, int form_new, const double *__restrict__ ll, const double *__restrict__ part,
                                                     double *__restrict__ net, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[CNETVB_PIECES];
    for (int j = 0; j < CNETVB_PIECES; ++j) {
        double v = 0.0;
        for (int b = threadIdx.x; b < VB_BLK; b += 256) v += part[j * VB_BLK + b];
        v = nhp_block_sum_n<4>(v, red);
        if (threadIdx.x == 0) tot[j] = v;
    }
    if (threadIdx.x == 0) {
        const double sl = *ll + tot[0];
        double klnet = 0.0;
        if (!A.dense) {
            const double av = form_new ? A.alpha + tot[6] : net[0], bv = form_new ? A.beta + tot[7] : net[1];
            double pa, la, pb, lb, ps, ls;
            nhp_digamma_lgamma(av, pa, la);
            nhp_digamma_lgamma(bv, pb, lb);
            nhp_digamma_lgamma(av + bv, ps, ls);
            const double ea = pa - ps, eb = pb - ps;                 // E log ρ, E log(1 - ρ)
            const double klbeta = (((ls - la) - lb) - A.beta_const) + ((av - A.alpha) * ea + (bv - A.beta) * eb);
            klnet = ((tot[5] - tot[6] * ea) - tot[7] * eb) + klbeta;
            net[0] = av; net[1] = bv; net[2] = pa - pb;
        }
        out[0] = sl;
        for (int j = 1; j < 5; ++j) out[j] = tot[j];
        out[5] = klnet;
        out[6] = ((((sl - tot[1]) - tot[2]) - tot[3]) - tot[4]) - klnet;
        out[7] = 0.0;
    }
}

// the posterior means in params! order (α'/β', a'/b' | m', a'/b', κv1/νv1) and the adjacency matrix A = (ρv > ½)
__global__ __launch_bounds__(256) void k_cnetvb_mean(vb_args a, const double *__restrict__ S, const double *__restrict__ R,
                                                     const double *__restrict__ rho, double *__restrict__ x, double *__restrict__ Adj)
{
    const nhp_layout L = vb_layout(a);
    const bool ln = a.impulse != NHP_IMPULSE_EXPONENTIAL;
    const size_t NN = (size_t)a.N * (size_t)a.N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < L.P; i += (size_t)gridDim.x * 256) {
        x[i] = (ln && i >= L.p1 && i < L.p2) ? S[i] : S[i] / R[i];
        if (i < NN) Adj[i] = rho[i] > 0.5 ? 1.0 : 0.0;
    }
}

// the refusals and argument errors of both entry points, before any launch
nhp_status cn_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const double *net, bool dense,
                    const char *what, bool block = false)
{
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (m->baseline_kind != NHP_BASELINE_HOMOGENEOUS) {
        nhp_set_error(ctx, "%s: the update of a LogGaussianCoxProcess baseline has no closed form", what);
        return NHP_ENOTIMPL;
    }
    if (!m->has_A || !m->d_A) {
        nhp_set_error(ctx, "%s (network) is defined for ContinuousNetworkHawkesProcess: the model has no adjacency matrix (nhp_cont_vb_run fits the standard process)", what);
        return NHP_ENOTIMPL;
    }
    if (block && m->latent) {
        nhp_set_error(ctx, "%s: a latent distance network is attached to the model (the block-network fit needs none)", what);
        return NHP_ENOTIMPL;
    }
    if (!block && (m->sbm || m->latent)) {
        nhp_set_error(ctx, "%s: a block or latent distance network is not implemented (dense and Bernoulli networks are)", what);
        return NHP_ENOTIMPL;
    }
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "%s: not available on a column shard", what);
        return NHP_ENOTIMPL;
    }
    const bool ln = m->impulse_kind != NHP_IMPULSE_EXPONENTIAL;
    if (!vb_positive(pr->alpha0) || !vb_positive(pr->beta0) || !vb_positive(pr->kappa) || !vb_positive(pr->nu) || !vb_positive(pr->a) ||
        !vb_positive(pr->b) || (ln && (!vb_positive(pr->kappa_mu) || !std::isfinite(pr->mu_mu)))) {
        nhp_set_error(ctx, "%s: every prior hyper-parameter but the mean μμ must be positive and finite", what);
        return NHP_EINVAL;
    }
    char msg[200];
    if (cnetvb_check_net(what, net, dense || block, msg, sizeof msg) != CNETVB_OK) { nhp_set_error(ctx, "%s", msg); return NHP_EINVAL; }
    return NHP_OK;
}

nhp_status cn_check_state(nhp_ctx *ctx, const nhp_cont_model *m, bool dense, bool state, const double *S, const double *R, const double *Q,
                          const char *what)
{
    const nhp_layout L(m);
    char msg[200];
    if (cnetvb_check_state(what, (size_t)m->N, dense, state, Q, S + L.W, R + L.W, msg, sizeof msg) != CNETVB_OK) {
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

cn_args cn_make_args(const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const double *net, bool dense)
{
    cn_args A{};
    A.v = vb_make_args(ds, m, pr);
    A.k0 = net[0]; A.n0 = net[1];
    A.lg_k0 = std::lgamma(net[0]); A.log_n0 = std::log(net[1]);
    A.dk = pr->kappa - net[0]; A.dn = pr->nu - net[1];
    A.prior = cnetvb_prior_logit(net[0], net[1], pr->kappa, pr->nu);
    A.dense = dense ? 1 : 0;
    if (!dense) { A.alpha = net[2]; A.beta = net[3]; A.beta_const = cnetvb_beta_const(net[2], net[3]); }
    return A;
}

void cn_carve(double *base, size_t P, size_t N, cn_state &cur, cn_state &nxt, double **d_out)
{
    const size_t stride = cnetvb_state_doubles(P, N, VB_BLK);
    cn_state *st[2] = {&cur, &nxt};
    for (int j = 0; j < 2; ++j) {
        double *p = base + j * stride;
        st[j]->x = p; st[j]->S = p + P; st[j]->R = p + 2 * P; st[j]->Q = p + 3 * P; st[j]->part = p + 3 * P + cnetvb_q_doubles(N);
    }
    *d_out = base + 2 * stride;
}

// the model as the E-step sees it: no adjacency matrix (the network acts through the prior of W alone)
nhp_cont_model cn_unmasked(const nhp_cont_model *m)
{
    nhp_cont_model v = *m;
    v.has_A = 0; v.d_A = nullptr;
    return v;
}

// ---- the block network (the definition is in include/nhp.h, nhp_cont_sbmvb_run) --------------------------------
// The Bernoulli fit with A[p,c] ~ Bernoulli(ρ[z_p, z_c]): the scalar ψ(αv) - ψ(βv) of the logit becomes the link's own
// net[p,c] = Σ_kl ω D (sbmvb_net), and the network's Beta becomes the block model's state B = [αv; βv; γv; m], updated by the
// kernels of nhp_sbmvb_dev.h -- the tables from the new ρv, then THE label sweep at the steps that have one.

struct cb_args {
    int N, K;
    double alpha, beta, gamma;       // the block model's priors
    double beta_const, dir_const;    // lnΓ(α+β) - lnΓα - lnΓβ and lnΓ(Kγ) - K lnΓγ
};

// a state on the device: cn_state's (Q = the three planes alone), B = [αv; βv; γv; m] and T = [T1; T0; Σ_n m] at its own m
struct cb_state { double *x, *S, *R, *Q, *B, *T, *part; };
// what both states share: D, the four tables, Eπ, m·D, U1, U0
struct cb_scratch { double *D, *tabs, *Epi, *mD, *U1, *U0; };

// k_cnetvb_update with the link's own network term in place of the scalar: factors (S, R, Q) from the surrogate x, the
// gradient g at it and blk = (m, m·D, D) of the state stepped from; their surrogate xn, their pieces.  Link k = p + c·N, p
// fastest: (m·D)[p,l] is coalesced per l, m[c,l] one address for (almost) the whole wave; the term is a running sum.
__global__ __launch_bounds__(256) void k_csbmvb_update(cn_args A, const double *__restrict__ x, const double *__restrict__ g, sbmvb_link blk,
                                                       double *__restrict__ S, double *__restrict__ R, double *__restrict__ Q,
                                                       double *__restrict__ xn, double *__restrict__ part)
{
    const vb_args &a = A.v;
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    const nhp_gibbs_priors &q = a.pr;
    cn_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) {
            const double al = q.alpha0 + x[i] * (g[i] + a.T), be = q.beta0 + a.T;
            S[i] = al; R[i] = be;
            xn[i] = vb_baseline(a, al, be, s);
            continue;
        }
        const size_t k = i - N, p = k % N, c = k / N;
        const double cp = a.cnt ? a.cnt[p] : 0.0;
        const double EM = x[L.W + k] * (g[L.W + k] + cp);
        const double kv1 = q.kappa + EM, nv1 = q.nu + cp, kv0 = A.k0 + EM, nv0 = A.n0 + cp;
        double m = 0.0, kk = 1.0, sa, sb;
        if (a.impulse == NHP_IMPULSE_EXPONENTIAL) {
            sa = q.a + EM;
            sb = q.b + (EM / x[L.p1 + k] - g[L.p1 + k]);
            S[L.p1 + k] = sa; R[L.p1 + k] = sb;
        } else {
            const double cc = x[L.p1 + k], tau = x[L.p2 + k];
            const double D1 = g[L.p1 + k] / tau, S2 = EM / tau - 2.0 * g[L.p2 + k], d0 = q.mu_mu - cc;
            kk = q.kappa_mu + EM;
            const double dm = (D1 + q.kappa_mu * d0) / kk;
            m = cc + dm;
            sa = q.a + 0.5 * EM;
            sb = q.b + 0.5 * ((S2 + q.kappa_mu * (d0 * d0)) - kk * (dm * dm));
            S[L.p1 + k] = m; R[L.p1 + k] = kk;
            S[L.p2 + k] = sa; R[L.p2 + k] = sb;
        }
        S[L.W + k] = kv1; R[L.W + k] = nv1;
        const cn_tab t = cn_tables(kv0, nv0, kv1, nv1);
        const double rho = cn_rho(A, sbmvb_net(blk, N, p, c), kv0, nv0, kv1, t);
        double w, p1, p2;
        cn_link(A, cp, kv0, nv0, kv1, nv1, t, rho, m, kk, sa, sb, s, w, p1, p2);
        Q[k] = kv0; Q[NN + k] = nv0; Q[2 * NN + k] = rho;
        vb_write(a, L, xn, k, w, p1, p2);
    }
    cn_store(s, part);
}

// out = k_cnetvb_elbo's eight, then [Σ entropy of ρv, links, labels, KL_Dir, Σ KL_Beta]: the partial sums in one fixed order and
// the network pieces of the state (B, T) -- T1, T0 taken at the state's OWN m --
//   links = Σ_kl (T1 E1 + T0 E0),  labels = Σ_nk m (Eπ - ln m)  (0·ln 0 = 0),  KL_net = Σ entropy - (links + labels - KL_Dir - Σ KL_Beta).
// Thread i adds the entries i, i + 256, ... in increasing order and nhp_block_sum_n joins the threads in its fixed order.
__global__ __launch_bounds__(256) void k_csbmvb_elbo(cb_args b, const double *__restrict__ ll, const double *__restrict__ part,
                                                     const double *__restrict__ B, const double *__restrict__ T, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[CNETVB_PIECES];
    __shared__ double epi[SBMVB_MAX_BLOCKS];
    for (int j = 0; j < CNETVB_PIECES; ++j) {
        double v = 0.0;
        for (int i = threadIdx.x; i < VB_BLK; i += 256) v += part[j * VB_BLK + i];
        v = nhp_block_sum_n<4>(v, red);
        if (threadIdx.x == 0) tot[j] = v;
    }
    const int K = b.K, KK = K * K;
    const size_t N = (size_t)b.N;
    const double *av = B, *bv = B + KK, *gv = B + 2 * KK, *m = B + 2 * KK + K;
    const double *T1 = T, *T0 = T + KK;
    double links = 0.0, klb = 0.0;
    for (int i = threadIdx.x; i < KK; i += 256) {
        double pa, la, pb, lb, ps, ls;
        nhp_digamma_lgamma(av[i], pa, la);
        nhp_digamma_lgamma(bv[i], pb, lb);
        nhp_digamma_lgamma(av[i] + bv[i], ps, ls);
        const double e1 = pa - ps, e0 = pb - ps;                     // E log ρ[k,l], E log(1 - ρ[k,l])
        links += T1[i] * e1 + T0[i] * e0;
        klb += (((ls - la) - lb) - b.beta_const) + ((av[i] - b.alpha) * e1 + (bv[i] - b.beta) * e0);
    }
    links = nhp_block_sum_n<4>(links, red);
    klb = nhp_block_sum_n<4>(klb, red);
    double gs = 0.0;
    for (int k = 0; k < K; ++k) gs += gv[k];
    if ((int)threadIdx.x < K) epi[threadIdx.x] = nhp_digamma(gv[threadIdx.x]) - nhp_digamma(gs);
    __syncthreads();
    double lab = 0.0;
    for (size_t i = threadIdx.x; i < N * (size_t)K; i += 256) {
        const double v = m[i];
        lab += v * epi[i / N] - (v > 0.0 ? v * nhp_log(v) : 0.0);
    }
    lab = nhp_block_sum_n<4>(lab, red);
    if (threadIdx.x == 0) {
        double pg, lgs, lsum = 0.0, dot = 0.0;
        nhp_digamma_lgamma(gs, pg, lgs);
        for (int k = 0; k < K; ++k) {
            double pk, lk;
            nhp_digamma_lgamma(gv[k], pk, lk);
            lsum += lk;
            dot += (gv[k] - b.gamma) * epi[k];
        }
        const double kldir = ((lgs - lsum) - b.dir_const) + dot;
        const double sl = *ll + tot[0];
        const double klnet = tot[5] - (((links + lab) - kldir) - klb);
        out[0] = sl;
        for (int j = 1; j < 5; ++j) out[j] = tot[j];
        out[5] = klnet;
        out[6] = ((((sl - tot[1]) - tot[2]) - tot[3]) - tot[4]) - klnet;
        out[7] = 0.0;
        out[8] = tot[5]; out[9] = links; out[10] = lab; out[11] = kldir; out[12] = klb;
    }
}

void cb_carve(double *base, size_t P, size_t N, size_t K, cb_state &cur, cb_state &nxt, cb_scratch &w, double **d_out)
{
    const size_t stride = csbmvb_state_doubles(P, N, K, VB_BLK), NN = N * N, KK = K * K, NK = N * K;
    cb_state *st[2] = {&cur, &nxt};
    for (int j = 0; j < 2; ++j) {
        double *p = base + j * stride;
        st[j]->x = p; p += P;
        st[j]->S = p; p += P;
        st[j]->R = p; p += P;
        st[j]->Q = p; p += 3 * NN;
        st[j]->B = p; p += csbmvb_b_doubles(N, K);
        st[j]->T = p; p += csbmvb_t_doubles(K);
        st[j]->part = p;
    }
    double *p = base + 2 * stride;
    w.D = p; p += KK;
    w.tabs = p; p += 4 * KK;
    w.Epi = p; p += K;
    w.mD = p; p += NK;
    w.U1 = p; p += NK;
    w.U0 = p; p += NK;
    *d_out = p;
}

// the checks of both block entry points before any launch: cn_check's, then the block model's own
nhp_status cb_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, const nhp_gibbs_priors *pr, const double *net,
                    const double *sbm, int32_t K, int32_t labels_every, int64_t step0, const double *B, bool B_on_host, const char *what)
{
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0;
    char msg[256];
    // (the flag and the pointers first: cn_check reads net)
    if (dense || !net || !sbm) {
        csbmvb_check_args(what, m ? m->N : 0, net, sbm, K, labels_every, step0, dense, nullptr, msg, sizeof msg);
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    NHP_TRY(cn_check(ctx, ds, m, pr, net, false, what, true));
    const int rc = csbmvb_check_args(what, m->N, net, sbm, K, labels_every, step0, false, B, msg, sizeof msg, !B_on_host);
    if (rc == CSBMVB_OK) return NHP_OK;
    nhp_set_error(ctx, "%s", msg);
    return rc == CSBMVB_ENOTIMPL ? NHP_ENOTIMPL : NHP_EINVAL;
}

nhp_status cb_check_state(nhp_ctx *ctx, const nhp_cont_model *m, bool state, const double *S, const double *R, const double *Q, const char *what)
{
    const nhp_layout L(m);
    char msg[200];
    if (csbmvb_check_state(what, (size_t)m->N, state, Q, S + L.W, R + L.W, msg, sizeof msg) != CSBMVB_OK) {
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

cb_args cb_make_args(const nhp_cont_model *m, const double *sbm, int32_t K)
{
    cb_args b{};
    b.N = m->N; b.K = K;
    b.alpha = sbm[0]; b.beta = sbm[1]; b.gamma = sbm[2];
    b.beta_const = cnetvb_beta_const(sbm[0], sbm[1]);
    b.dir_const = csbmvb_dir_const(sbm[2], K);
    return b;
}

// T = [T1; T0; Σ_n m] of state s at its own m (k_sbmvb_u, then the tables' reduction with zero priors); with `have_U` the link
// sums in w.U1, w.U0 are already those of (s's ρv, s's m)
void cb_own_sums(hipStream_t st, const cb_args &b, const cb_state &s, const cb_scratch &w, bool have_U)
{
    const size_t N = (size_t)b.N, K = (size_t)b.K, KK = K * K;
    const double *rho = s.Q + 2 * N * N, *m = s.B + 2 * KK + K;
    if (!have_U) hipLaunchKernelGGL(k_sbmvb_u, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, b.N, b.K, rho, m, w.U1, w.U0);
    hipLaunchKernelGGL(k_sbmvb_tables, dim3((unsigned)KK), dim3(256), 0, st, b.N, b.K, rho, m, (const double *)w.U1, (const double *)w.U0, 0.0, 0.0,
                       0.0, s.T, s.T + KK, s.T + 2 * KK);
}

// the update from `cur` (surrogate cur.x, gradient g) to `nxt`: steps 2-5 of the definition
nhp_status cb_update(nhp_ctx *ctx, hipStream_t st, const cn_args &A, const cb_args &b, const cb_state &cur, const cb_state &nxt, const cb_scratch &w,
                     const double *g, bool sweep)
{
    const size_t N = (size_t)b.N, K = (size_t)b.K, KK = K * K, NK = N * K, NN = N * N;
    const dim3 block(256), gk((unsigned)((KK + 255) / 256)), gnk((unsigned)((NK + 255) / 256));
    double *cm = cur.B + 2 * KK + K, *nm = nxt.B + 2 * KK + K, *nrho = nxt.Q + 2 * NN;
    // D from the OLD tables and m·D from the OLD m, then the O(P) pass
    hipLaunchKernelGGL(k_sbmvb_expect, gk, block, 0, st, b.K, (const double *)cur.B, (const double *)(cur.B + KK), (const double *)(cur.B + 2 * KK),
                       w.D, w.tabs, w.Epi);
    hipLaunchKernelGGL(k_sbmvb_md, gnk, block, 0, st, b.N, b.K, (const double *)cm, (const double *)w.D, w.mD);
    hipLaunchKernelGGL(k_csbmvb_update, dim3(VB_BLK), block, 0, st, A, (const double *)cur.x, g,
                       sbmvb_link{b.K, cm, w.mD, w.D, nullptr}, nxt.S, nxt.R, nxt.Q, nxt.x, nxt.part);
    // the tables from the NEW ρv and the current m
    hipLaunchKernelGGL(k_sbmvb_u, gnk, block, 0, st, b.N, b.K, (const double *)nrho, (const double *)cm, w.U1, w.U0);
    hipLaunchKernelGGL(k_sbmvb_tables, dim3((unsigned)KK), block, 0, st, b.N, b.K, (const double *)nrho, (const double *)cm, (const double *)w.U1,
                       (const double *)w.U0, b.alpha, b.beta, b.gamma, nxt.B, nxt.B + KK, nxt.B + 2 * KK);
    NHP_HIP(ctx, hipMemcpyAsync(nm, cm, 8 * NK, hipMemcpyDeviceToDevice, st));
    if (sweep) {
        hipLaunchKernelGGL(k_sbmvb_expect, gk, block, 0, st, b.K, (const double *)nxt.B, (const double *)(nxt.B + KK),
                           (const double *)(nxt.B + 2 * KK), w.D, w.tabs, w.Epi);
        sbmvb_bufs s{};
        s.tabs = w.tabs; s.Epi = w.Epi;
        NHP_TRY(sbmvb_launch_sweep(ctx, st, s, N, K, nrho, nm));
    }
    cb_own_sums(st, b, nxt, w, !sweep);                              // (no sweep: m is the one the link sums were taken at)
    NHP_HIP(ctx, hipGetLastError());
    return NHP_OK;
}

}   // namespace

extern "C" nhp_status nhp_cont_netvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                          const nhp_gibbs_priors *priors, const double *net, double *S, double *R, int64_t len, double *Q,
                                          int32_t output_on_device, double *stats)
{
    if (!ctx || !ds || !m || !priors || !net || !S || !R || !Q || !stats) return NHP_EINVAL;
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0, from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    NHP_TRY(cn_check(ctx, ds, m, priors, net, dense, "update!"));
    const size_t P = nhp_layout(m).P, N = (size_t)m->N, NN = N * N;
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    if (!output_on_device) NHP_TRY(cn_check_state(ctx, m, dense, !from_model, S, R, Q, "update!"));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME | NHP_VB_DENSE_NETWORK);

    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * cnetvb_reserve_doubles(P, N, VB_BLK), "variational state"));
    cn_state cur, nxt;
    double *d_out = nullptr;
    cn_carve((double *)ctx->d_mle, P, N, cur, nxt, &d_out);
    const cn_args A = cn_make_args(ds, m, priors, net, dense);
    const dim3 grid(VB_BLK), block(256);
    const hipMemcpyKind in = output_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    NHP_HIP(ctx, hipMemcpyAsync(cur.Q, Q, 8 * (3 * NN + 2), in, st));
    if (from_model) {
        hipLaunchKernelGGL(k_cnetvb_start, grid, block, 0, st, A, (const double *)m->d_params, cur.x, cur.part);
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(cur.S, S, 8 * P, in, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.R, R, 8 * P, in, st));
        hipLaunchKernelGGL(k_cnetvb_surrogate, grid, block, 0, st, A, (const double *)cur.S, (const double *)cur.R, cur.Q, cur.x, cur.part);
    }
    NHP_HIP(ctx, hipGetLastError());
    double *d_grad = nullptr;
    nhp_cont_model mm = cn_unmasked(m);                               // (the E-step bumps the version of what it evaluates)
    NHP_TRY(nhp_em_estep(ctx, ds, &mm, flags, cur.x, (int64_t)P, &d_grad));
    hipLaunchKernelGGL(k_cnetvb_elbo, dim3(1), block, 0, st, A, 0, (const double *)ctx->d_results, (const double *)cur.part, cur.Q + 3 * NN, d_out);
    hipLaunchKernelGGL(k_cnetvb_update, grid, block, 0, st, A, (const double *)cur.x, (const double *)d_grad, (const double *)(cur.Q + 3 * NN),
                       nxt.S, nxt.R, nxt.Q, nxt.x, nxt.part);
    hipLaunchKernelGGL(k_cnetvb_elbo, dim3(1), block, 0, st, A, 1, (const double *)ctx->d_results, (const double *)nxt.part, nxt.Q + 3 * NN,
                       d_out + CNETVB_OUT);
    NHP_HIP(ctx, hipGetLastError());
    double h[2 * CNETVB_OUT];
    NHP_TRY(nhp_download(ctx, h, d_out, sizeof h));
    if (!std::isfinite(h[0])) {
        NHP_HIP(ctx, hipStreamSynchronize(st));
        nhp_set_error(ctx, "update!: the intensity of some event is not positive and finite");
        return NHP_EDOMAIN;
    }
    if (output_on_device) {
        NHP_HIP(ctx, hipMemcpyAsync(S, nxt.S, 8 * P, hipMemcpyDeviceToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(R, nxt.R, 8 * P, hipMemcpyDeviceToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(Q, nxt.Q, 8 * (3 * NN + 2), hipMemcpyDeviceToDevice, st));
    } else {
        NHP_TRY(nhp_download(ctx, S, nxt.S, 8 * P));
        NHP_TRY(nhp_download(ctx, R, nxt.R, 8 * P));
        NHP_TRY(nhp_download(ctx, Q, nxt.Q, 8 * (3 * NN + 2)));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    stats[0] = h[0];
    for (int j = 1; j <= 5; ++j) { stats[j] = from_model ? 0.0 : h[j]; stats[5 + j] = h[CNETVB_OUT + j]; }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_netvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                         const nhp_gibbs_priors *priors, const double *net, double f_abstol, int32_t max_steps, double *x,
                                         double *S, double *R, int64_t len, double *Q, double *elbo, int32_t *steps_out,
                                         int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !net || !x || !S || !R || !Q || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0, resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(cn_check(ctx, ds, m, priors, net, dense, "vb!"));
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME | NHP_VB_DENSE_NETWORK);
    if (max_steps < (resume ? 0 : 1)) {
        nhp_set_error(ctx, "vb!: max_steps = %d (a run from a guess needs at least one step to have a state)", max_steps);
        return NHP_EDOMAIN;
    }
    const size_t P = nhp_layout(m).P, N = (size_t)m->N, NN = N * N;
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    NHP_TRY(cn_check_state(ctx, m, dense, resume, S, R, Q, "vb!"));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    nhp_em_host hs;
    if (hipHostMalloc((void **)&hs.h, 8 * CNETVB_OUT) != hipSuccess) { hs.h = nullptr; nhp_set_error(ctx, "out of pinned memory"); return NHP_ENOMEM; }
    NHP_HIP(ctx, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));

    // two states (surrogate, planes, Q, pieces): an update writes the other one only, so nothing is lost when the rule says stop
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * cnetvb_reserve_doubles(P, N, VB_BLK), "variational state"));
    cn_state cur, nxt;
    double *d_out = nullptr;
    cn_carve((double *)ctx->d_mle, P, N, cur, nxt, &d_out);
    const cn_args A = cn_make_args(ds, m, priors, net, dense);
    const dim3 grid(VB_BLK), block(256);

    NHP_HIP(ctx, hipMemcpyAsync(cur.Q, Q, 8 * (3 * NN + 2), hipMemcpyHostToDevice, st));     // (a guess: its αv, βv alone are read)
    if (resume) {
        NHP_HIP(ctx, hipMemcpyAsync(cur.S, S, 8 * P, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.R, R, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cnetvb_surrogate, grid, block, 0, st, A, (const double *)cur.S, (const double *)cur.R, cur.Q, cur.x, cur.part);
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(nxt.x, x, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cnetvb_start, grid, block, 0, st, A, (const double *)nxt.x, cur.x, cur.part);
    }
    NHP_HIP(ctx, hipGetLastError());

    const double nan = std::nan("");
    double L = nan, L_prev = nan;
    bool has_state = resume, converged = false, made_here = false;    // made_here: `cur` came out of k_cnetvb_update
    nhp_cont_model view = cn_unmasked(m);
    int k = 0;
    for (;; ++k) {
        // E-step at x̃_k and the ELBO of state k (which also completes the state's network scalars, read by the update); the
        // update is enqueued behind the scalars' copy, so it runs while the host looks at the stopping rule
        double *d_grad = nullptr;
        NHP_TRY(nhp_em_estep(ctx, ds, &view, flags, cur.x, (int64_t)P, &d_grad));
        hipLaunchKernelGGL(k_cnetvb_elbo, dim3(1), block, 0, st, A, made_here ? 1 : 0, (const double *)ctx->d_results, (const double *)cur.part,
                           cur.Q + 3 * NN, d_out);
        NHP_HIP(ctx, hipGetLastError());
        NHP_HIP(ctx, hipMemcpyAsync(hs.h, d_out, 8 * CNETVB_OUT, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipEventRecord(hs.ev, st));
        if (k < max_steps) {
            hipLaunchKernelGGL(k_cnetvb_update, grid, block, 0, st, A, (const double *)cur.x, (const double *)d_grad,
                               (const double *)(cur.Q + 3 * NN), nxt.S, nxt.R, nxt.Q, nxt.x, nxt.part);
            NHP_HIP(ctx, hipGetLastError());
        }
        NHP_HIP(ctx, hipEventSynchronize(hs.ev));
        if (!std::isfinite(hs.h[0])) {
            NHP_HIP(ctx, hipStreamSynchronize(st));
            nhp_set_error(ctx, "vb!: the intensity of some event is not positive and finite (iteration %d)", k);
            return NHP_EDOMAIN;
        }
        L_prev = L; L = has_state ? hs.h[6] : nan;
        if (trace) trace[k] = L;
        if (has_state && std::fabs(L - L_prev) < f_abstol) { converged = true; break; }     // (false while L_prev is NaN)
        if (k == max_steps) break;
        std::swap(cur, nxt);
        has_state = true; made_here = true;
    }
    m->version = view.version;
    nhp_model_view_keep_bound(m, view);
    // the state, and its means and A = (ρv > ½) into x and the model's own block
    hipLaunchKernelGGL(k_cnetvb_mean, grid, block, 0, st, A.v, (const double *)cur.S, (const double *)cur.R, (const double *)(cur.Q + 2 * NN),
                       nxt.x, m->d_A);
    NHP_HIP(ctx, hipGetLastError());
    ++m->version;
    NHP_HIP(ctx, hipMemcpyAsync(m->d_params, nxt.x, 8 * P, hipMemcpyDeviceToDevice, st));
    NHP_TRY(nhp_download(ctx, x, nxt.x, 8 * P));
    NHP_TRY(nhp_download(ctx, S, cur.S, 8 * P));
    NHP_TRY(nhp_download(ctx, R, cur.R, 8 * P));
    NHP_TRY(nhp_download(ctx, Q, cur.Q, 8 * (3 * NN + 2)));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *elbo = L; *steps_out = k; *converged_out = converged ? 1 : 0;
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_sbmvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                          const nhp_gibbs_priors *priors, const double *net, const double *sbm, int32_t n_blocks,
                                          int32_t labels_every, int64_t step0, double *S, double *R, int64_t len, double *Q, double *B,
                                          int32_t output_on_device, double *stats)
{
    if (!ctx || !ds || !m || !priors || !S || !R || !Q || !B || !stats) return NHP_EINVAL;
    const bool from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    NHP_TRY(cb_check(ctx, ds, m, flags, priors, net, sbm, n_blocks, labels_every, step0, B, !output_on_device, "update!"));
    const size_t P = nhp_layout(m).P, N = (size_t)m->N, NN = N * N, K = (size_t)n_blocks, nB = csbmvb_b_doubles(N, K);
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    if (!output_on_device) NHP_TRY(cb_check_state(ctx, m, !from_model, S, R, Q, "update!"));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME | NHP_VB_DENSE_NETWORK);

    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * csbmvb_reserve_doubles(P, N, K, VB_BLK), "variational state"));
    cb_state cur, nxt;
    cb_scratch w;
    double *d_out = nullptr;
    cb_carve((double *)ctx->d_mle, P, N, K, cur, nxt, w, &d_out);
    cn_args A = cn_make_args(ds, m, priors, net, true);              // (net = [κ0, ν0] alone: the Beta's slots stay 0 and unread)
    A.dense = 0;
    const cb_args b = cb_make_args(m, sbm, n_blocks);
    const dim3 grid(VB_BLK), block(256);
    const hipMemcpyKind in = output_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    NHP_HIP(ctx, hipMemcpyAsync(cur.B, B, 8 * nB, in, st));
    if (from_model) {
        hipLaunchKernelGGL(k_cnetvb_start, grid, block, 0, st, A, (const double *)m->d_params, cur.x, cur.part);
        NHP_HIP(ctx, hipMemsetAsync(cur.T, 0, 8 * csbmvb_t_doubles(K), st));     // (no state: of its evaluation Σ log λ̃ alone is used)
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(cur.Q, Q, 8 * 3 * NN, in, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.S, S, 8 * P, in, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.R, R, 8 * P, in, st));
        hipLaunchKernelGGL(k_cnetvb_surrogate, grid, block, 0, st, A, (const double *)cur.S, (const double *)cur.R, cur.Q, cur.x, cur.part);
        cb_own_sums(st, b, cur, w, false);
    }
    NHP_HIP(ctx, hipGetLastError());
    double *d_grad = nullptr;
    nhp_cont_model mm = cn_unmasked(m);                               // (the E-step bumps the version of what it evaluates)
    NHP_TRY(nhp_em_estep(ctx, ds, &mm, flags, cur.x, (int64_t)P, &d_grad));
    hipLaunchKernelGGL(k_csbmvb_elbo, dim3(1), block, 0, st, b, (const double *)ctx->d_results, (const double *)cur.part, (const double *)cur.B,
                       (const double *)cur.T, d_out);
    NHP_TRY(cb_update(ctx, st, A, b, cur, nxt, w, d_grad, (step0 + 1) % labels_every == 0));
    hipLaunchKernelGGL(k_csbmvb_elbo, dim3(1), block, 0, st, b, (const double *)ctx->d_results, (const double *)nxt.part, (const double *)nxt.B,
                       (const double *)nxt.T, d_out + CSBMVB_OUT);
    NHP_HIP(ctx, hipGetLastError());
    double h[2 * CSBMVB_OUT];
    NHP_TRY(nhp_download(ctx, h, d_out, sizeof h));
    if (!std::isfinite(h[0])) {
        NHP_HIP(ctx, hipStreamSynchronize(st));
        nhp_set_error(ctx, "update!: the intensity of some event is not positive and finite");
        return NHP_EDOMAIN;
    }
    if (output_on_device) {
        NHP_HIP(ctx, hipMemcpyAsync(S, nxt.S, 8 * P, hipMemcpyDeviceToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(R, nxt.R, 8 * P, hipMemcpyDeviceToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(Q, nxt.Q, 8 * 3 * NN, hipMemcpyDeviceToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(B, nxt.B, 8 * nB, hipMemcpyDeviceToDevice, st));
    } else {
        NHP_TRY(nhp_download(ctx, S, nxt.S, 8 * P));
        NHP_TRY(nhp_download(ctx, R, nxt.R, 8 * P));
        NHP_TRY(nhp_download(ctx, Q, nxt.Q, 8 * 3 * NN));
        NHP_TRY(nhp_download(ctx, B, nxt.B, 8 * nB));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    stats[0] = h[0];
    for (int j = 1; j <= 5; ++j) { stats[j] = from_model ? 0.0 : h[j]; stats[5 + j] = h[CSBMVB_OUT + j]; }
    for (int j = 0; j < CSBMVB_NET_PIECES; ++j) {
        stats[11 + j] = from_model ? 0.0 : h[8 + j];
        stats[11 + CSBMVB_NET_PIECES + j] = h[CSBMVB_OUT + 8 + j];
    }
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_sbmvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                         const nhp_gibbs_priors *priors, const double *net, const double *sbm, int32_t n_blocks,
                                         int32_t labels_every, int64_t step0, double f_abstol, int32_t max_steps, double *x, double *S, double *R,
                                         int64_t len, double *Q, double *B, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !x || !S || !R || !Q || !B || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    const bool resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(cb_check(ctx, ds, m, flags, priors, net, sbm, n_blocks, labels_every, step0, B, true, "vb!"));
    flags &= ~(int32_t)(NHP_VB_FROM_MODEL | NHP_VB_RESUME | NHP_VB_DENSE_NETWORK);
    if (max_steps < (resume ? 0 : 1)) {
        nhp_set_error(ctx, "vb!: max_steps = %d (a run from a guess needs at least one step to have a state)", max_steps);
        return NHP_EDOMAIN;
    }
    const size_t P = nhp_layout(m).P, N = (size_t)m->N, NN = N * N, K = (size_t)n_blocks, nB = csbmvb_b_doubles(N, K);
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    NHP_TRY(cb_check_state(ctx, m, resume, S, R, Q, "vb!"));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    nhp_em_host hs;
    if (hipHostMalloc((void **)&hs.h, 8 * CSBMVB_OUT) != hipSuccess) { hs.h = nullptr; nhp_set_error(ctx, "out of pinned memory"); return NHP_ENOMEM; }
    NHP_HIP(ctx, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));

    // two states (surrogate, planes, Q, B, T, pieces): an update writes the other one only -- the sweep works on the copy of m --
    // so nothing is lost when the rule says stop
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * csbmvb_reserve_doubles(P, N, K, VB_BLK), "variational state"));
    cb_state cur, nxt;
    cb_scratch w;
    double *d_out = nullptr;
    cb_carve((double *)ctx->d_mle, P, N, K, cur, nxt, w, &d_out);
    cn_args A = cn_make_args(ds, m, priors, net, true);
    A.dense = 0;
    const cb_args b = cb_make_args(m, sbm, n_blocks);
    const dim3 grid(VB_BLK), block(256);

    NHP_HIP(ctx, hipMemcpyAsync(cur.B, B, 8 * nB, hipMemcpyHostToDevice, st));
    if (resume) {
        NHP_HIP(ctx, hipMemcpyAsync(cur.Q, Q, 8 * 3 * NN, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.S, S, 8 * P, hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(cur.R, R, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cnetvb_surrogate, grid, block, 0, st, A, (const double *)cur.S, (const double *)cur.R, cur.Q, cur.x, cur.part);
        cb_own_sums(st, b, cur, w, false);
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(nxt.x, x, 8 * P, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cnetvb_start, grid, block, 0, st, A, (const double *)nxt.x, cur.x, cur.part);
        NHP_HIP(ctx, hipMemsetAsync(cur.T, 0, 8 * csbmvb_t_doubles(K), st));     // (a guess has no state: Σ log λ̃ alone is used)
    }
    NHP_HIP(ctx, hipGetLastError());

    const double nan = std::nan("");
    double L = nan, L_prev = nan;
    bool has_state = resume, converged = false;
    nhp_cont_model view = cn_unmasked(m);
    int k = 0;
    for (;; ++k) {
        // E-step at x̃_k and the ELBO of state k; the update is enqueued behind the scalars' copy, so it runs while the host looks
        // at the stopping rule
        double *d_grad = nullptr;
        NHP_TRY(nhp_em_estep(ctx, ds, &view, flags, cur.x, (int64_t)P, &d_grad));
        hipLaunchKernelGGL(k_csbmvb_elbo, dim3(1), block, 0, st, b, (const double *)ctx->d_results, (const double *)cur.part,
                           (const double *)cur.B, (const double *)cur.T, d_out);
        NHP_HIP(ctx, hipGetLastError());
        NHP_HIP(ctx, hipMemcpyAsync(hs.h, d_out, 8 * CSBMVB_OUT, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipEventRecord(hs.ev, st));
        if (k < max_steps) NHP_TRY(cb_update(ctx, st, A, b, cur, nxt, w, d_grad, (step0 + k + 1) % labels_every == 0));
        NHP_HIP(ctx, hipEventSynchronize(hs.ev));
        if (!std::isfinite(hs.h[0])) {
            NHP_HIP(ctx, hipStreamSynchronize(st));
            nhp_set_error(ctx, "vb!: the intensity of some event is not positive and finite (iteration %d)", k);
            return NHP_EDOMAIN;
        }
        L_prev = L; L = has_state ? hs.h[6] : nan;
        if (trace) trace[k] = L;
        if (has_state && std::fabs(L - L_prev) < f_abstol) { converged = true; break; }     // (false while L_prev is NaN)
        if (k == max_steps) break;
        std::swap(cur, nxt);
        has_state = true;
    }
    m->version = view.version;
    nhp_model_view_keep_bound(m, view);
    // the state, and its means and A = (ρv > ½) into x and the model's own block
    hipLaunchKernelGGL(k_cnetvb_mean, grid, block, 0, st, A.v, (const double *)cur.S, (const double *)cur.R, (const double *)(cur.Q + 2 * NN),
                       nxt.x, m->d_A);
    NHP_HIP(ctx, hipGetLastError());
    ++m->version;
    NHP_HIP(ctx, hipMemcpyAsync(m->d_params, nxt.x, 8 * P, hipMemcpyDeviceToDevice, st));
    NHP_TRY(nhp_download(ctx, x, nxt.x, 8 * P));
    NHP_TRY(nhp_download(ctx, S, cur.S, 8 * P));
    NHP_TRY(nhp_download(ctx, R, cur.R, 8 * P));
    NHP_TRY(nhp_download(ctx, Q, cur.Q, 8 * 3 * NN));
    NHP_TRY(nhp_download(ctx, B, cur.B, 8 * nB));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *elbo = L; *steps_out = k; *converged_out = converged ? 1 : 0;
    return NHP_OK;
}
