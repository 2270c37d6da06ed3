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
//
// The block network's fit (further down) is the same pass with the link's own network term: both update kernels are one body,
// cn_update_body<NET>.  The host side is nhp_vb_drive.h's step and run drivers, shared with cont_vb.hip; cn_fit and cb_fit tell
// them what a state of either network fit is, how it is carved and which kernels run.  The latent distance network's fit (last)
// is the third: cn_latent_net, cl_fit and the kernels of nhp_latvb_dev.h.
#include "nhp_csbmvb.h"
#include "nhp_latvb_dev.h"
#include "nhp_sbmvb_dev.h"
#include "nhp_vb_drive.h"

namespace {

struct cn_args {
    vb_args v;                       // pr.kappa, pr.nu (and lg_kappa, log_nu): the slab's
    double k0, n0, lg_k0, log_n0;    // the spike's Gamma, lnΓ(κ0), log ν0
    double dk, dn, prior;            // κ1 - κ0, ν1 - ν0, the prior's share of the logit
    double alpha, beta, beta_const;  // Beta prior of ρ and lnΓ(α+β) - lnΓα - lnΓβ
    int dense;
};

struct cn_acc : vb_acc { double ent = 0.0, sr = 0.0, s1r = 0.0; };

__device__ __forceinline__ void cn_store(const cn_acc &s, double *__restrict__ part)
{
    vb_store<CNETVB_PIECES>({s.fix, s.comp, s.kl0, s.klw, s.kli, s.ent, s.sr, s.s1r}, part);
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

// iteration 0: an ordinary parameter vector used as if it were a surrogate
__global__ __launch_bounds__(256) void k_cnetvb_start(cn_args A, const double *__restrict__ xin, double *__restrict__ x, double *__restrict__ part)
{
    vb_start_body<CNETVB_PIECES>(A.v, xin, x, part);
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

// Where a link's network term of the logit comes from.  A dense or Bernoulli network: the scalar ψ(αv) - ψ(βv) of the state
// stepped from, old = [αv, βv, ψ(αv) - ψ(βv)] (a dense network: no kernel writes the slot, no link reads it, and the pair passes
// through into the new Q).  A block network: the link's own net[p,c] = Σ_kl ω D (sbmvb_net) from blk = (m, m·D, D)
// of the state stepped from; link k = p + c·N, p fastest: (m·D)[p,l] is coalesced per l, m[c,l] one address for (almost) the
// whole wave; the term is a running sum.  This source has no dense branch.
struct cn_scalar_net {
    double net;
    __device__ __forceinline__ cn_scalar_net(const cn_args &A, const double *__restrict__ old, double *__restrict__ Q, size_t NN)
        : net(A.dense ? 0.0 : old[2])
    {
        if (A.dense && blockIdx.x == 0 && threadIdx.x < 2) Q[3 * NN + threadIdx.x] = old[threadIdx.x];
    }
    __device__ __forceinline__ double rho(const cn_args &A, size_t, size_t, size_t, double kv0, double nv0, double kv1, const cn_tab &t) const
    {
        return A.dense ? 1.0 : cn_rho(A, net, kv0, nv0, kv1, t);
    }
};
struct cn_block_net {
    sbmvb_link blk;
    __device__ __forceinline__ double rho(const cn_args &A, size_t N, size_t p, size_t c, double kv0, double nv0, double kv1, const cn_tab &t) const
    {
        return cn_rho(A, sbmvb_net(blk, N, p, c), kv0, nv0, kv1, t);
    }
};

// A latent distance network: the link's own η[p,c] = b - ‖z_p - z_c‖² at the (zv, bv) of the state stepped from
// -- a point estimate, so E_q[log s(η)] - E_q[log(1 - s(η))] is η itself.  No dense branch either.
struct cn_latent_net {
    latvb_link lat;
    __device__ __forceinline__ double rho(const cn_args &A, size_t N, size_t p, size_t c, double kv0, double nv0, double kv1, const cn_tab &t) const
    {
        return cn_rho(A, latvb_eta(lat, N, p, c), kv0, nv0, kv1, t);
    }
};

// the coordinate-ascent update of the network fits: factors (S, R, Q) from the surrogate x, the gradient g at it and the
// network term of `net`; their surrogate xn, their pieces
template <class NET>
__device__ __forceinline__ void cn_update_body(const cn_args &A, const double *__restrict__ x, const double *__restrict__ g, const NET &net,
                                               double *__restrict__ S, double *__restrict__ R, double *__restrict__ Q,
                                               double *__restrict__ xn, double *__restrict__ part)
{
    const vb_args &a = A.v;
    const size_t N = (size_t)a.N, NN = N * N;
    const nhp_layout L = vb_layout(a);
    cn_acc s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N + NN; i += (size_t)gridDim.x * 256) {
        if (i < N) { vb_update_baseline(a, x, g, i, S, R, xn, s); continue; }
        const size_t k = i - N, p = k % N, c = k / N;                // (c: the block network's alone)
        const double cp = a.cnt ? a.cnt[p] : 0.0;
        const double EM = vb_link_em(L, x, g, k, cp);
        const double kv1 = a.pr.kappa + EM, nv1 = a.pr.nu + cp, kv0 = A.k0 + EM, nv0 = A.n0 + cp;
        double m, kk, sa, sb;
        vb_update_impulse(a, L, x, g, k, EM, S, R, m, kk, sa, sb);
        S[L.W + k] = kv1; R[L.W + k] = nv1;
        const cn_tab t = cn_tables(kv0, nv0, kv1, nv1);
        const double rho = net.rho(A, N, p, c, kv0, nv0, kv1, t);
        double w, p1, p2;
        cn_link(A, cp, kv0, nv0, kv1, nv1, t, rho, m, kk, sa, sb, s, w, p1, p2);
        Q[k] = kv0; Q[NN + k] = nv0; Q[2 * NN + k] = rho;
        vb_write(a, L, xn, k, w, p1, p2);
    }
    cn_store(s, part);
}

__global__ __launch_bounds__(256) void k_cnetvb_update(cn_args A, const double *__restrict__ x, const double *__restrict__ g,
                                                       const double *__restrict__ old, double *__restrict__ S, double *__restrict__ R,
                                                       double *__restrict__ Q, double *__restrict__ xn, double *__restrict__ part)
{
    cn_update_body(A, x, g, cn_scalar_net(A, old, Q, (size_t)A.v.N * (size_t)A.v.N), S, R, Q, xn, part);
}
__global__ __launch_bounds__(256) void k_csbmvb_update(cn_args A, const double *__restrict__ x, const double *__restrict__ g, sbmvb_link blk,
                                                       double *__restrict__ S, double *__restrict__ R, double *__restrict__ Q,
                                                       double *__restrict__ xn, double *__restrict__ part)
{
    cn_update_body(A, x, g, cn_block_net{blk}, S, R, Q, xn, part);
}
__global__ __launch_bounds__(256) void k_clatvb_update(cn_args A, const double *__restrict__ x, const double *__restrict__ g, latvb_link lat,
                                                       double *__restrict__ S, double *__restrict__ R, double *__restrict__ Q,
                                                       double *__restrict__ xn, double *__restrict__ part)
{
    cn_update_body(A, x, g, cn_latent_net{lat}, S, R, Q, xn, part);
}

// out = [Σ_i log λ̃_i = ll + fix, E_q[compensator], KL_λ0, KL_W, KL_imp, KL_net, L, 0]: the partial sums in one fixed order.
// net = the state's [αv, βv, ψ(αv) - ψ(βv)]: with form_new the pair is made here from the sums of ρv (the state came out of
// k_cnetvb_update), otherwise it is the caller's; the third is written in both cases.  A dense network: KL_net = 0, net untouched.
__global__ __launch_bounds__(256) void k_cnetvb_elbo(cn_args A, int form_new, const double *__restrict__ ll, const double *__restrict__ part,
                                                     double *__restrict__ net, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[CNETVB_PIECES];
    vb_sum_parts<CNETVB_PIECES>(part, tot, red);
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
                    const char *what, bool block = false, bool latent = false)
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
    if (latent && m->sbm) {
        nhp_set_error(ctx, "%s: a block network is attached to the model (the latent-distance-network fit needs none)", what);
        return NHP_ENOTIMPL;
    }
    if (!block && !latent && (m->sbm || m->latent)) {
        nhp_set_error(ctx, "%s: a block or latent distance network is not implemented (dense and Bernoulli networks are)", what);
        return NHP_ENOTIMPL;
    }
    if (nhp_is_column_shard(ds)) {
        nhp_set_error(ctx, "%s: not available on a column shard", what);
        return NHP_ENOTIMPL;
    }
    NHP_TRY(vb_check_priors(ctx, m, pr, what));
    char msg[200];
    if (cnetvb_check_net(what, net, dense || block || latent, msg, sizeof msg) != CNETVB_OK) { nhp_set_error(ctx, "%s", msg); return NHP_EINVAL; }
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

// the dense / Bernoulli fit for the drivers of nhp_vb_drive.h: S, R, Q the caller's arrays
struct cn_fit {
    static constexpr int OUT = CNETVB_OUT, L_SLOT = 6, STAT_PIECES = 5, PLANES = 3;
    static constexpr bool UNMASK = true;
    // a state on the device: surrogate, planes, Q = [κv0; νv0; ρv; αv, βv, ψ(αv) - ψ(βv)], partial sums
    struct state { double *x, *S, *R, *Q, *part; };
    nhp_ctx *ctx;
    cn_args A;
    size_t P, N;
    double *S, *R, *Q;

    size_t reserve_doubles() const { return cnetvb_reserve_doubles(P, N, VB_BLK); }
    void carve(vb_bump &b, state &s) const
    {
        s.x = b.take(P); s.S = b.take(P); s.R = b.take(P); s.Q = b.take(cnetvb_q_doubles(N)); s.part = b.take((size_t)CNETVB_PIECES * VB_BLK);
    }
    void carve_shared(vb_bump &) const {}
    void place_step(state &, state &, bool) const {}
    // (Q: a guess's or the model's αv, βv are read without a state too; the third scalar behind them is the device's own)
    void planes(const state &s, vb_plane *pl) const { pl[0] = {S, s.S, P, false}; pl[1] = {R, s.R, P, false}; pl[2] = {Q, s.Q, 3 * N * N + 2, true}; }
    void start(hipStream_t st, const double *xin, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_start, dim3(VB_BLK), dim3(256), 0, st, A, xin, s.x, s.part);
    }
    void surrogate(hipStream_t st, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_surrogate, dim3(VB_BLK), dim3(256), 0, st, A, (const double *)s.S, (const double *)s.R, s.Q, s.x, s.part);
    }
    // (the ELBO kernel also completes the state's network scalars, read by the update)
    void elbo(hipStream_t st, const state &s, bool made_here, double *out) const
    {
        hipLaunchKernelGGL(k_cnetvb_elbo, dim3(1), dim3(256), 0, st, A, made_here ? 1 : 0, (const double *)ctx->d_results, (const double *)s.part,
                           s.Q + 3 * N * N, out);
    }
    nhp_status update(nhp_ctx *, hipStream_t st, const state &cur, const state &nxt, const double *g, int) const
    {
        hipLaunchKernelGGL(k_cnetvb_update, dim3(VB_BLK), dim3(256), 0, st, A, (const double *)cur.x, g, (const double *)(cur.Q + 3 * N * N), nxt.S,
                           nxt.R, nxt.Q, nxt.x, nxt.part);
        return NHP_OK;
    }
    void mean(hipStream_t st, const state &s, double *x, nhp_cont_model *m) const
    {
        hipLaunchKernelGGL(k_cnetvb_mean, dim3(VB_BLK), dim3(256), 0, st, A.v, (const double *)s.S, (const double *)s.R,
                           (const double *)(s.Q + 2 * N * N), x, m->d_A);
    }
    void stats(const double *h, bool from_model, double *out) const { vb_fill_stats(h, OUT, STAT_PIECES, from_model, out); }
};

// ---- the block network (the definition is in include/nhp.h, nhp_cont_sbmvb_run) --------------------------------
// The Bernoulli fit with A[p,c] ~ Bernoulli(ρ[z_p, z_c]): the scalar ψ(αv) - ψ(βv) of the logit becomes the link's own
// net[p,c] = Σ_kl ω D (sbmvb_net), and the network's Beta becomes the block model's state B = [αv; βv; γv; m], updated by the
// kernels of nhp_sbmvb_dev.h -- the tables from the new ρv, then THE label sweep at the steps that have one.

struct cb_args {
    int N, K;
    double alpha, beta, gamma;       // the block model's priors
    double beta_const, dir_const;    // lnΓ(α+β) - lnΓα - lnΓβ and lnΓ(Kγ) - K lnΓγ
};

// a state on the device: cn_fit::state's (Q = the three planes alone), B = [αv; βv; γv; m] and T = [T1; T0; Σ_n m] at its own m
struct cb_state { double *x, *S, *R, *Q, *B, *T, *part; };
// what both states share: D, the four tables, Eπ, m·D, U1, U0
struct cb_scratch { double *D, *tabs, *Epi, *mD, *U1, *U0; };

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
    vb_sum_parts<CNETVB_PIECES>(part, tot, red);
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

// the block fit for the drivers of nhp_vb_drive.h: S, R, Q, B the caller's arrays; update number k of a call is step
// step0 + k + 1 of the label sweep's schedule
struct cb_fit {
    static constexpr int OUT = CSBMVB_OUT, L_SLOT = 6, STAT_PIECES = 5, PLANES = 4;
    static constexpr bool UNMASK = true;
    using state = cb_state;
    nhp_ctx *ctx;
    cn_args A;
    cb_args b;
    size_t P, N, K;
    int32_t labels_every;
    int64_t step0;
    double *S, *R, *Q, *B;
    cb_scratch w;

    size_t reserve_doubles() const { return csbmvb_reserve_doubles(P, N, K, VB_BLK); }
    void carve(vb_bump &m, state &s) const
    {
        s.x = m.take(P); s.S = m.take(P); s.R = m.take(P); s.Q = m.take(3 * N * N);
        s.B = m.take(csbmvb_b_doubles(N, K)); s.T = m.take(csbmvb_t_doubles(K)); s.part = m.take((size_t)CNETVB_PIECES * VB_BLK);
    }
    void carve_shared(vb_bump &m)
    {
        w.D = m.take(K * K); w.tabs = m.take(4 * K * K); w.Epi = m.take(K); w.mD = m.take(N * K); w.U1 = m.take(N * K); w.U0 = m.take(N * K);
    }
    void place_step(state &, state &, bool) const {}
    void planes(const state &s, vb_plane *pl) const
    {
        pl[0] = {S, s.S, P, false}; pl[1] = {R, s.R, P, false}; pl[2] = {Q, s.Q, 3 * N * N, false}; pl[3] = {B, s.B, csbmvb_b_doubles(N, K), true};
    }
    void start(hipStream_t st, const double *xin, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_start, dim3(VB_BLK), dim3(256), 0, st, A, xin, s.x, s.part);
        (void)hipMemsetAsync(s.T, 0, 8 * csbmvb_t_doubles(K), st);    // (no state: of its evaluation Σ log λ̃ alone is used; errors: the driver's)
    }
    void surrogate(hipStream_t st, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_surrogate, dim3(VB_BLK), dim3(256), 0, st, A, (const double *)s.S, (const double *)s.R, s.Q, s.x, s.part);
        cb_own_sums(st, b, s, w, false);
    }
    void elbo(hipStream_t st, const state &s, bool, double *out) const
    {
        hipLaunchKernelGGL(k_csbmvb_elbo, dim3(1), dim3(256), 0, st, b, (const double *)ctx->d_results, (const double *)s.part, (const double *)s.B,
                           (const double *)s.T, out);
    }
    nhp_status update(nhp_ctx *c, hipStream_t st, const state &cur, const state &nxt, const double *g, int k) const
    {
        return cb_update(c, st, A, b, cur, nxt, w, g, (step0 + k + 1) % labels_every == 0);
    }
    void mean(hipStream_t st, const state &s, double *x, nhp_cont_model *m) const
    {
        hipLaunchKernelGGL(k_cnetvb_mean, dim3(VB_BLK), dim3(256), 0, st, A.v, (const double *)s.S, (const double *)s.R,
                           (const double *)(s.Q + 2 * N * N), x, m->d_A);
    }
    void stats(const double *h, bool from_model, double *out) const
    {
        vb_fill_stats(h, OUT, STAT_PIECES, from_model, out);
        for (int j = 0; j < CSBMVB_NET_PIECES; ++j) {
            out[11 + j] = from_model ? 0.0 : h[8 + j];
            out[11 + CSBMVB_NET_PIECES + j] = h[OUT + 8 + j];
        }
    }
};

cn_fit cn_make_fit(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const double *net, bool dense,
                   double *S, double *R, double *Q)
{
    return cn_fit{ctx, cn_make_args(ds, m, pr, net, dense), nhp_layout(m).P, (size_t)m->N, S, R, Q};
}

cb_fit cb_make_fit(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const double *net,
                   const double *sbm, int32_t K, int32_t labels_every, int64_t step0, double *S, double *R, double *Q, double *B)
{
    cn_args A = cn_make_args(ds, m, pr, net, true);                  // (net = [κ0, ν0] alone: the Beta's slots stay 0 and unread)
    A.dense = 0;
    return cb_fit{ctx, A, cb_make_args(m, sbm, K), nhp_layout(m).P, (size_t)m->N, (size_t)K, labels_every, step0, S, R, Q, B, cb_scratch{}};
}

// ---- the latent distance network (the definition is in include/nhp.h, nhp_cont_latvb_run) ------------------------
// The Bernoulli fit with A[p,c] ~ Bernoulli(s(η[p,c])), η = b - ‖z_p - z_c‖²: the scalar of the logit becomes the link's own η at
// the point estimate (zv, bv) of the state stepped from, and the network's Beta becomes Z = [vec zv; bv], moved by J iterations of
// the monotone ascent of nhp_latvb_dev.h at the new ρv.

struct cl_args {
    int N, D, J;
    latvb_prior pr;
    double lnz_const, lnb_const;     // the normalising constants of ln p(z) and ln p(b): -(N·D/2) ln(2πσ²), -½ ln(2πσb²)
    latvb_steps ladder, here;        // the rungs with the current point behind them; the current point alone
};

// a state on the device: cn_fit::state's (Q = the three planes alone), Z = [vec zv; bv] and lk = the per-node link sums at its own Z
struct cl_state { double *x, *S, *R, *Q, *Z, *lk, *part; };
// what both states share: C = ρv + ρvᵀ, G = ∇F, the per-node halves of ∂F/∂b, the per-node sums of every slot, the iteration's
// scalars and the rungs the latest update took
struct cl_scratch { double *C, *G, *hb, *lad, *sc, *rungs; };

// out = k_cnetvb_elbo's eight, then [Σ entropy of ρv, links, ln p(zv), ln p(bv)], then the J rungs the update that made the state
// took (-1: the point stayed; all -1 for a state the caller gave): the partial sums in one fixed order and the network pieces of
// the state at its OWN (zv, bv),
//   links = ½ Σ_n lk[n] = Σ_pc [ρv η - softplus(η)],  ln p(z) = -‖z‖²/(2σ²) - (N·D/2) ln(2πσ²),  ln p(b) = -(b - μb)²/(2σb²) - ½ ln(2πσb²),
//   KL_net = Σ entropy - (links + ln p(z) + ln p(b)).
// Thread i adds the entries i, i + 256, ... in increasing order and nhp_block_sum_n joins the threads in its fixed order.
__global__ __launch_bounds__(256) void k_clatvb_elbo(cl_args c, int made_here, const double *__restrict__ ll, const double *__restrict__ part,
                                                     const double *__restrict__ Z, const double *__restrict__ lk,
                                                     const double *__restrict__ rungs, double *__restrict__ out)
{
    __shared__ double red[4];
    __shared__ double tot[CNETVB_PIECES];
    vb_sum_parts<CNETVB_PIECES>(part, tot, red);
    const size_t ND = (size_t)c.N * c.D;
    double links = 0.0, zz = 0.0;
    for (int n = threadIdx.x; n < c.N; n += 256) links += lk[n];
    links = nhp_block_sum_n<4>(links, red);
    for (size_t i = threadIdx.x; i < ND; i += 256) zz += Z[i] * Z[i];
    zz = nhp_block_sum_n<4>(zz, red);
    if ((int)threadIdx.x < CLATVB_MAX_ASCENT)
        out[8 + CLATVB_NET_PIECES + threadIdx.x] = (made_here && (int)threadIdx.x < c.J) ? rungs[threadIdx.x] : -1.0;
    if (threadIdx.x == 0) {
        links *= 0.5;
        const double db = Z[ND] - c.pr.mu_b;
        const double lnz = c.lnz_const - 0.5 * c.pr.inv_s2 * zz, lnb = c.lnb_const - 0.5 * c.pr.inv_sb2 * (db * db);
        const double sl = *ll + tot[0];
        const double klnet = tot[5] - ((links + lnz) + lnb);
        out[0] = sl;
        for (int j = 1; j < 5; ++j) out[j] = tot[j];
        out[5] = klnet;
        out[6] = ((((sl - tot[1]) - tot[2]) - tot[3]) - tot[4]) - klnet;
        out[7] = 0.0;
        out[8] = tot[5]; out[9] = links; out[10] = lnz; out[11] = lnb;
    }
}

// the checks of the latent entry points before any launch: the flag and the pointers, cn_check's, then the latent model's own
nhp_status cl_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, const nhp_gibbs_priors *pr, const double *net,
                    const double *lat, int32_t D, int32_t J, const double *Z, bool Z_on_host, const char *what)
{
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0;
    char msg[256];
    // (the flag and the pointers first: cn_check reads net)
    if (dense || !net || !lat) {
        clatvb_check_args(what, m ? m->N : 0, net, lat, D, J, dense, nullptr, msg, sizeof msg);
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    NHP_TRY(cn_check(ctx, ds, m, pr, net, false, what, false, true));
    if (clatvb_check_args(what, m->N, net, lat, D, J, false, Z, msg, sizeof msg, !Z_on_host) == CLATVB_OK) return NHP_OK;
    nhp_set_error(ctx, "%s", msg);
    return NHP_EINVAL;
}

nhp_status cl_check_state(nhp_ctx *ctx, const nhp_cont_model *m, bool state, const double *S, const double *R, const double *Q, const char *what)
{
    const nhp_layout L(m);
    char msg[200];
    if (clatvb_check_state(what, (size_t)m->N, state, Q, S + L.W, R + L.W, msg, sizeof msg) != CLATVB_OK) {
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

cl_args cl_make_args(int32_t N, const double *lat, int32_t D, int32_t J)
{
    cl_args c{};
    c.N = N; c.D = D; c.J = J;
    c.pr = latvb_prior{1.0 / (lat[0] * lat[0]), lat[1], 1.0 / (lat[2] * lat[2])};
    const double two_pi = 6.283185307179586476925;
    c.lnz_const = -0.5 * (double)N * (double)D * std::log(two_pi * lat[0] * lat[0]);
    c.lnb_const = -0.5 * std::log(two_pi * lat[2] * lat[2]);
    c.ladder.n = CLATVB_SLOTS;
    clatvb_ladder(N, lat[0], c.ladder.t);
    c.here.n = 1;
    return c;
}

inline dim3 cl_tiles(size_t N) { const unsigned t = (unsigned)((N + LATVB_TILE - 1) / LATVB_TILE); return dim3(t, t); }

// lk of state s at its own (zv, bv): C from its ρv (unless `have_C`), then the ladder kernel at the point itself
void cl_own_sums(hipStream_t st, const cl_args &c, const cl_state &s, const cl_scratch &w, bool have_C)
{
    const size_t N = (size_t)c.N;
    if (!have_C) hipLaunchKernelGGL(k_latvb_sym, cl_tiles(N), dim3(256), 0, st, c.N, (const double *)(s.Q + 2 * N * N), w.C);
    hipLaunchKernelGGL(k_latvb_ladder, dim3((unsigned)N), dim3(256), 0, st, c.N, c.D, c.here, (const double *)w.C, (const double *)s.Z,
                       (const double *)nullptr, s.lk, 1);
}

// J iterations of the ascent of F at the ρv behind C, moving Z in place; rung j of w.rungs = the rung iteration j took
void cl_ascent(hipStream_t st, const cl_args &c, const cl_scratch &w, double *Z)
{
    const size_t N = (size_t)c.N, nz = clatvb_z_doubles(N, (size_t)c.D);
    for (int j = 0; j < c.J; ++j) {
        hipLaunchKernelGGL(k_latvb_grad, dim3((unsigned)N), dim3(256), 0, st, c.N, c.D, c.pr.inv_s2, (const double *)w.C, (const double *)Z, w.G, w.hb);
        hipLaunchKernelGGL(k_latvb_gb, dim3(1), dim3(256), 0, st, c.N, c.D, c.pr.mu_b, c.pr.inv_sb2, (const double *)Z, (const double *)w.hb, w.G);
        hipLaunchKernelGGL(k_latvb_ladder, dim3((unsigned)N), dim3(256), 0, st, c.N, c.D, c.ladder, (const double *)w.C, (const double *)Z,
                           (const double *)w.G, w.lad, CLATVB_SLOTS);
        hipLaunchKernelGGL(k_latvb_finish, dim3(1), dim3(256), 0, st, c.N, c.D, c.ladder, c.pr, (const double *)w.lad, CLATVB_SLOTS,
                           (const double *)Z, (const double *)w.G, w.sc, w.rungs + j);
        hipLaunchKernelGGL(k_latvb_apply, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, nz, (const double *)w.sc, (const double *)w.G, Z);
    }
}

// the latent fit for the drivers of nhp_vb_drive.h: S, R, Q, Z the caller's arrays
struct cl_fit {
    static constexpr int OUT = CLATVB_OUT, L_SLOT = 6, STAT_PIECES = 5, PLANES = 4;
    static constexpr bool UNMASK = true;
    using state = cl_state;
    nhp_ctx *ctx;
    cn_args A;
    cl_args c;
    size_t P, N, D;
    double *S, *R, *Q, *Z;
    cl_scratch w;

    size_t reserve_doubles() const { return clatvb_reserve_doubles(P, N, D, VB_BLK); }
    void carve(vb_bump &m, state &s) const
    {
        s.x = m.take(P); s.S = m.take(P); s.R = m.take(P); s.Q = m.take(3 * N * N);
        s.Z = m.take(clatvb_z_doubles(N, D)); s.lk = m.take(N); s.part = m.take((size_t)CNETVB_PIECES * VB_BLK);
    }
    void carve_shared(vb_bump &m)
    {
        w.C = m.take(N * N); w.G = m.take(clatvb_z_doubles(N, D)); w.hb = m.take(N); w.lad = m.take(N * (size_t)CLATVB_SLOTS);
        w.sc = m.take(CLATVB_SC); w.rungs = m.take(CLATVB_MAX_ASCENT);
    }
    void place_step(state &, state &, bool) const {}
    void planes(const state &s, vb_plane *pl) const
    {
        pl[0] = {S, s.S, P, false}; pl[1] = {R, s.R, P, false}; pl[2] = {Q, s.Q, 3 * N * N, false}; pl[3] = {Z, s.Z, clatvb_z_doubles(N, D), true};
    }
    void start(hipStream_t st, const double *xin, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_start, dim3(VB_BLK), dim3(256), 0, st, A, xin, s.x, s.part);
        (void)hipMemsetAsync(s.lk, 0, 8 * N, st);                     // (no state: of its evaluation Σ log λ̃ alone is used; errors: the driver's)
    }
    void surrogate(hipStream_t st, const state &s) const
    {
        hipLaunchKernelGGL(k_cnetvb_surrogate, dim3(VB_BLK), dim3(256), 0, st, A, (const double *)s.S, (const double *)s.R, s.Q, s.x, s.part);
        cl_own_sums(st, c, s, w, false);
    }
    void elbo(hipStream_t st, const state &s, bool made_here, double *out) const
    {
        hipLaunchKernelGGL(k_clatvb_elbo, dim3(1), dim3(256), 0, st, c, made_here ? 1 : 0, (const double *)ctx->d_results, (const double *)s.part,
                           (const double *)s.Z, (const double *)s.lk, (const double *)w.rungs, out);
    }
    // the O(P) pass with η from the OLD (zv, bv), C from the NEW ρv, the ascent on a copy of the old Z, the new state's own sums
    nhp_status update(nhp_ctx *cx, hipStream_t st, const state &cur, const state &nxt, const double *g, int) const
    {
        hipLaunchKernelGGL(k_clatvb_update, dim3(VB_BLK), dim3(256), 0, st, A, (const double *)cur.x, g, latvb_link{c.D, cur.Z}, nxt.S, nxt.R,
                           nxt.Q, nxt.x, nxt.part);
        hipLaunchKernelGGL(k_latvb_sym, cl_tiles(N), dim3(256), 0, st, c.N, (const double *)(nxt.Q + 2 * N * N), w.C);
        NHP_HIP(cx, hipMemcpyAsync(nxt.Z, cur.Z, 8 * clatvb_z_doubles(N, D), hipMemcpyDeviceToDevice, st));
        cl_ascent(st, c, w, nxt.Z);
        cl_own_sums(st, c, nxt, w, true);
        NHP_HIP(cx, hipGetLastError());
        return NHP_OK;
    }
    void mean(hipStream_t st, const state &s, double *x, nhp_cont_model *m) const
    {
        hipLaunchKernelGGL(k_cnetvb_mean, dim3(VB_BLK), dim3(256), 0, st, A.v, (const double *)s.S, (const double *)s.R,
                           (const double *)(s.Q + 2 * N * N), x, m->d_A);
    }
    void stats(const double *h, bool from_model, double *out) const
    {
        vb_fill_stats(h, OUT, STAT_PIECES, from_model, out);
        for (int j = 0; j < CLATVB_NET_PIECES; ++j) {
            out[11 + j] = from_model ? 0.0 : h[8 + j];
            out[11 + CLATVB_NET_PIECES + j] = h[OUT + 8 + j];
        }
        for (int j = 0; j < c.J; ++j) out[CLATVB_STATS_FIXED + j] = h[OUT + 8 + CLATVB_NET_PIECES + j];
    }
};

cl_fit cl_make_fit(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_gibbs_priors *pr, const double *net,
                   const double *lat, int32_t D, int32_t J, double *S, double *R, double *Q, double *Z)
{
    cn_args A = cn_make_args(ds, m, pr, net, true);                  // (net = [κ0, ν0] alone: the Beta's slots stay 0 and unread)
    A.dense = 0;
    return cl_fit{ctx, A, cl_make_args(m->N, lat, D, J), nhp_layout(m).P, (size_t)m->N, (size_t)D, S, R, Q, Z, cl_scratch{}};
}

constexpr int32_t CN_MODE_FLAGS = NHP_VB_FROM_MODEL | NHP_VB_RESUME | NHP_VB_DENSE_NETWORK;     // not the E-step's

}   // namespace

extern "C" nhp_status nhp_cont_netvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                          const nhp_gibbs_priors *priors, const double *net, double *S, double *R, int64_t len, double *Q,
                                          int32_t output_on_device, double *stats)
{
    if (!ctx || !ds || !m || !priors || !net || !S || !R || !Q || !stats) return NHP_EINVAL;
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0, from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    NHP_TRY(cn_check(ctx, ds, m, priors, net, dense, "update!"));
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    if (!output_on_device) NHP_TRY(cn_check_state(ctx, m, dense, !from_model, S, R, Q, "update!"));
    cn_fit f = cn_make_fit(ctx, ds, m, priors, net, dense, S, R, Q);
    return vb_step_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, from_model, output_on_device != 0, stats);
}

extern "C" nhp_status nhp_cont_netvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                         const nhp_gibbs_priors *priors, const double *net, double f_abstol, int32_t max_steps, double *x,
                                         double *S, double *R, int64_t len, double *Q, double *elbo, int32_t *steps_out,
                                         int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !net || !x || !S || !R || !Q || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    const bool dense = (flags & NHP_VB_DENSE_NETWORK) != 0, resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(cn_check(ctx, ds, m, priors, net, dense, "vb!"));
    NHP_TRY(vb_run_args(ctx, m, resume, max_steps, len));
    NHP_TRY(cn_check_state(ctx, m, dense, resume, S, R, Q, "vb!"));
    cn_fit f = cn_make_fit(ctx, ds, m, priors, net, dense, S, R, Q);
    return vb_run_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, resume, f_abstol, max_steps, x, elbo, steps_out, converged_out, trace);
}

extern "C" nhp_status nhp_cont_sbmvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                          const nhp_gibbs_priors *priors, const double *net, const double *sbm, int32_t n_blocks,
                                          int32_t labels_every, int64_t step0, double *S, double *R, int64_t len, double *Q, double *B,
                                          int32_t output_on_device, double *stats)
{
    if (!ctx || !ds || !m || !priors || !S || !R || !Q || !B || !stats) return NHP_EINVAL;
    const bool from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    NHP_TRY(cb_check(ctx, ds, m, flags, priors, net, sbm, n_blocks, labels_every, step0, B, !output_on_device, "update!"));
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    if (!output_on_device) NHP_TRY(cb_check_state(ctx, m, !from_model, S, R, Q, "update!"));
    cb_fit f = cb_make_fit(ctx, ds, m, priors, net, sbm, n_blocks, labels_every, step0, S, R, Q, B);
    return vb_step_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, from_model, output_on_device != 0, stats);
}

extern "C" nhp_status nhp_cont_sbmvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                         const nhp_gibbs_priors *priors, const double *net, const double *sbm, int32_t n_blocks,
                                         int32_t labels_every, int64_t step0, double f_abstol, int32_t max_steps, double *x, double *S, double *R,
                                         int64_t len, double *Q, double *B, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !x || !S || !R || !Q || !B || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    const bool resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(cb_check(ctx, ds, m, flags, priors, net, sbm, n_blocks, labels_every, step0, B, true, "vb!"));
    NHP_TRY(vb_run_args(ctx, m, resume, max_steps, len));
    NHP_TRY(cb_check_state(ctx, m, resume, S, R, Q, "vb!"));
    cb_fit f = cb_make_fit(ctx, ds, m, priors, net, sbm, n_blocks, labels_every, step0, S, R, Q, B);
    return vb_run_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, resume, f_abstol, max_steps, x, elbo, steps_out, converged_out, trace);
}


extern "C" nhp_status nhp_cont_latvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                          const nhp_gibbs_priors *priors, const double *net, const double *lat, int32_t n_dims,
                                          int32_t ascent_steps, double *S, double *R, int64_t len, double *Q, double *Z,
                                          int32_t output_on_device, double *stats)
{
    if (!ctx || !ds || !m || !priors || !S || !R || !Q || !stats) return NHP_EINVAL;     // (net, lat, Z: cl_check's, with a message)
    const bool from_model = (flags & NHP_VB_FROM_MODEL) != 0;
    NHP_TRY(cl_check(ctx, ds, m, flags, priors, net, lat, n_dims, ascent_steps, Z, !output_on_device, "update!"));
    NHP_TRY(nhp_layout_check(ctx, nhp_layout(m), len));
    if (!output_on_device) NHP_TRY(cl_check_state(ctx, m, !from_model, S, R, Q, "update!"));
    cl_fit f = cl_make_fit(ctx, ds, m, priors, net, lat, n_dims, ascent_steps, S, R, Q, Z);
    return vb_step_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, from_model, output_on_device != 0, stats);
}

extern "C" nhp_status nhp_cont_latvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags,
                                         const nhp_gibbs_priors *priors, const double *net, const double *lat, int32_t n_dims,
                                         int32_t ascent_steps, double f_abstol, int32_t max_steps, double *x, double *S, double *R, int64_t len,
                                         double *Q, double *Z, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    if (!ctx || !ds || !m || !priors || !x || !S || !R || !Q || !elbo || !steps_out || !converged_out) return NHP_EINVAL;
    const bool resume = (flags & NHP_VB_RESUME) != 0;
    NHP_TRY(cl_check(ctx, ds, m, flags, priors, net, lat, n_dims, ascent_steps, Z, true, "vb!"));
    NHP_TRY(vb_run_args(ctx, m, resume, max_steps, len));
    NHP_TRY(cl_check_state(ctx, m, resume, S, R, Q, "vb!"));
    cl_fit f = cl_make_fit(ctx, ds, m, priors, net, lat, n_dims, ascent_steps, S, R, Q, Z);
    return vb_run_drive(ctx, ds, m, flags & ~CN_MODE_FLAGS, f, resume, f_abstol, max_steps, x, elbo, steps_out, converged_out, trace);
}

extern "C" nhp_status nhp_latent_expected_loglik(nhp_ctx *ctx, const double *rho, int32_t N, int32_t D, const double *z, double b, const double *lat,
                                                 double *out)
{
    if (!ctx || !rho || !z || !lat || !out) return NHP_EINVAL;
    if (N < 1) { nhp_set_error(ctx, "latent_expected_loglik: n_nodes = %d must be positive", N); return NHP_EINVAL; }
    const double spike[2] = {1.0, 1.0};
    char msg[256];
    if (D >= 1 && D <= CLATVB_MAX_DIMS) {                            // (z, b) as a host Z for the shared check
        std::vector<double> Zh((size_t)N * D + 1);
        std::copy(z, z + (size_t)N * D, Zh.begin());
        Zh.back() = b;
        if (clatvb_check_args("latent_expected_loglik", N, spike, lat, D, 0, false, Zh.data(), msg, sizeof msg) != CLATVB_OK) {
            nhp_set_error(ctx, "%s", msg);
            return NHP_EINVAL;
        }
    } else {
        clatvb_check_args("latent_expected_loglik", N, spike, lat, D, 0, false, z, msg, sizeof msg);
        nhp_set_error(ctx, "%s", msg);
        return NHP_EINVAL;
    }
    const size_t n = (size_t)N, NN = n * n, nz = clatvb_z_doubles(n, (size_t)D);
    for (size_t i = 0; i < NN; ++i)
        if (!(rho[i] >= 0.0 && rho[i] <= 1.0)) {
            nhp_set_error(ctx, "latent_expected_loglik: rho at link %zu = %g is outside [0, 1]", i, rho[i]);
            return NHP_EINVAL;
        }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * clatvb_loglik_doubles(n, (size_t)D)));
    vb_bump mem((double *)ctx->d_scratch);
    double *d_rho = mem.take(NN), *C = mem.take(NN), *Z = mem.take(nz), *G = mem.take(nz), *hb = mem.take(n), *lk = mem.take(n);
    double *sc = mem.take(CLATVB_SC), *d_out = mem.take(nz + 1);
    hipStream_t st = ctx->main();
    const cl_args c = cl_make_args(N, lat, D, 0);
    NHP_HIP(ctx, hipMemcpyAsync(d_rho, rho, 8 * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(Z, z, 8 * (nz - 1), hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(Z + nz - 1, &b, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_latvb_sym, cl_tiles(n), dim3(256), 0, st, N, (const double *)d_rho, C);
    hipLaunchKernelGGL(k_latvb_grad, dim3((unsigned)n), dim3(256), 0, st, N, D, c.pr.inv_s2, (const double *)C, (const double *)Z, G, hb);
    hipLaunchKernelGGL(k_latvb_gb, dim3(1), dim3(256), 0, st, N, D, c.pr.mu_b, c.pr.inv_sb2, (const double *)Z, (const double *)hb, G);
    hipLaunchKernelGGL(k_latvb_ladder, dim3((unsigned)n), dim3(256), 0, st, N, D, c.here, (const double *)C, (const double *)Z, (const double *)nullptr,
                       lk, 1);
    hipLaunchKernelGGL(k_latvb_finish, dim3(1), dim3(256), 0, st, N, D, c.here, c.pr, (const double *)lk, 1, (const double *)Z, (const double *)nullptr, sc,
                       (double *)nullptr);
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipMemcpyAsync(d_out, sc + 2, 8, hipMemcpyDeviceToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_out + 1, G, 8 * nz, hipMemcpyDeviceToDevice, st));
    return nhp_download(ctx, out, d_out, 8 * (nz + 1));              // (waits for the stream: `b` is a stack value)
}
