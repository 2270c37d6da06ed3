// The discrete chain on the device (include/nhp.h: nhp_disc_model_*, nhp_disc_mcmc_run).  A discrete mcmc! step
// is two calls that already run on the GPU -- parents + conjugate draws, and for a network process the adjacency sweep -- but
// each of them used to take the whole model from the host and hand it back.  nhp_disc_model keeps λ0 | W | θ | A in ONE device
// block in the order nhp_disc_stage_bump lays its copies out, the two steps read and write it in place (disc_gibbs.hip:
// nhp_disc_gibbs_enqueue, nhp_disc_adjacency_enqueue: same launches, same bits), the network's ρ is drawn next to it with the
// continuous chain's kernel, and the running sums and convergence diagnostics of the kept steps stay there too.  What is new
// as a kernel is the accumulate pass over the block: params(process) of a standard process is [λ0; vec(W∘θ)], a product that
// exists nowhere in memory, so the pass forms it on the fly.
#include "nhp_diag.h"
#include "nhp_rho.h"
#include <algorithm>

// ---- ΣA on the device: an exact integer, one workgroup, one fixed order, no atomics --------------------------------------
// state[3] takes it as the double k_rho_draw reads, *links as the integer the next sweep's route is chosen from (8 bytes read
// back by the host: the one transfer of a step).  One workgroup walks N² doubles: 2 MB at N = 512 next to an 18 ms sweep.
__global__ __launch_bounds__(1024) void k_disc_links(const double *__restrict__ A, int64_t NN, long long *__restrict__ links,
                                                     double *__restrict__ state)
{
    __shared__ long long red[1024];
    long long s = 0;
    for (int64_t i = threadIdx.x; i < NN; i += 1024) s += A[i] != 0.0 ? 1 : 0;
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) { links[0] = red[0]; state[3] = (double)red[0]; }
}

// ---- the accumulate pass ------------------------------------------------------------------------------------------------
// Entry i of the sums is entry i of params(process) without the network's ρ:
//   network process:  the block itself, [λ0; vec(W); vec(θ); vec(A)];
//   standard process: [λ0; vec(W∘θ)], x = W[p,c]·θ[p,c,b] -- ONE rounded product (no contraction: numpy's product, bit for
//                     bit), because the mean of a product is not the product of the means.
// Streaming like k_diag_accumulate (cont_diagnostics.hip): per entry one read of x (two for a product: W's N² entries are
// re-read once per basis, out of L2) and a read + write of Σx, Σx² (and B; SB and QB on a batch boundary), 8 bytes per lane,
// at most 2048 workgroups striding over the entries -- the continuous kernel's measurement of 16-byte accesses (no gain:
// DESIGN 3.22) holds here for the same reason, the planes start at multiples of an odd len.
template <bool PRODUCT>
__device__ __forceinline__ double disc_entry(const double *__restrict__ block, int64_t N, int64_t NN, bool narrow, int64_t i)
{
#pragma clang fp contract(off)
    if (!PRODUCT || i < N) return block[i];
    const int64_t j = i - N;                                         // p + N·c + N²·b
    const int64_t pc = narrow ? (int64_t)((uint32_t)j % (uint32_t)NN) : j % NN;
    const double w = block[N + pc], t = block[N + NN + j];
    const double x = w * t;
    return x;
}

template <bool PRODUCT, bool BOUNDARY>
__global__ __launch_bounds__(256) void k_disc_accumulate(const double *__restrict__ block, int64_t N, int64_t NN, int64_t len,
                                                         double *__restrict__ mom, double *__restrict__ bat, double b,
                                                         double *__restrict__ rho, double *__restrict__ rd)
{
    const bool narrow = len < ((int64_t)1 << 32);                    // 32-bit remainder where the indices fit
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        const double x = disc_entry<PRODUCT>(block, N, NN, narrow, i);
        double s1 = mom[i], s2 = mom[len + i], B = bat[i], SB = 0.0, QB = 0.0;
        if (BOUNDARY) { SB = bat[len + i]; QB = bat[2 * len + i]; }
        diag_update<BOUNDARY>(x, s1, s2, B, SB, QB, b);
        mom[i] = s1; mom[len + i] = s2; bat[i] = B;
        if (BOUNDARY) { bat[len + i] = SB; bat[2 * len + i] = QB; }
    }
    if (rho && blockIdx.x == 0 && threadIdx.x == 0) diag_rho<BOUNDARY>(rho, rd, b);
}

// the sums alone (no diagnostics configured): the same two expressions, the same bits
template <bool PRODUCT>
__global__ __launch_bounds__(256) void k_disc_moments(const double *__restrict__ block, int64_t N, int64_t NN, int64_t len,
                                                      double *__restrict__ mom, double *__restrict__ rho)
{
#pragma clang fp contract(off)
    const bool narrow = len < ((int64_t)1 << 32);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (int64_t)gridDim.x * 256) {
        const double x = disc_entry<PRODUCT>(block, N, NN, narrow, i);
        mom[i] += x;
        mom[len + i] = __builtin_fma(x, x, mom[len + i]);
    }
    if (rho && blockIdx.x == 0 && threadIdx.x == 0) { const double r = rho[0]; rho[1] += r; rho[2] = __builtin_fma(r, r, rho[2]); }
}

// ---- the model ------------------------------------------------------------------------------------------------------------
static nhp_status disc_model_check(nhp_ctx *ctx, const nhp_disc_model *m)
{
    if (!ctx || !m) return NHP_EINVAL;
    if (m->ctx != ctx) { nhp_set_error(ctx, "model belongs to another ctx"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    return NHP_OK;
}

static nhp_status disc_pair_check(nhp_ctx *ctx, const nhp_disc_dataset *ds, const nhp_disc_model *m)
{
    if (!ds) return NHP_EINVAL;
    NHP_TRY(disc_model_check(ctx, m));
    if (ds->N != m->N || ds->B != m->B) {
        nhp_set_error(ctx, "the model (N = %d, B = %d) does not match the dataset (N = %d, B = %d)", m->N, m->B, ds->N, ds->B);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

static int64_t disc_block_len(const nhp_disc_model *m)
{
    const int64_t N = m->N, NN = N * N;
    return N + NN + NN * m->B + (m->has_A ? NN : 0);
}

// entries of the sums: the block for a network process, [λ0; vec(W∘θ)] for a standard one
static int64_t disc_sums_len(const nhp_disc_model *m)
{
    const int64_t N = m->N, NN = N * N;
    return m->has_A ? disc_block_len(m) : N + NN * m->B;
}

extern "C" nhp_status nhp_disc_model_create(nhp_ctx *ctx, int32_t N, int32_t B, int32_t has_A, double dt, nhp_disc_model **out)
{
    if (!ctx || !out) return NHP_EINVAL;
    *out = nullptr;
    if (N < 1 || B < 1 || !(dt > 0.0)) { nhp_set_error(ctx, "disc_model_create: N, B >= 1 and dt > 0"); return NHP_EINVAL; }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_disc_model *m = new nhp_disc_model;
    m->ctx = ctx; m->N = N; m->B = B; m->has_A = has_A ? 1 : 0; m->dt = dt;
    const size_t n = (size_t)disc_block_len(m), NN = (size_t)N * N;
    // the network's scalars and the integer link count sit behind the block: one allocation
    if (hipMalloc((void **)&m->d_block, sizeof(double) * (n + (m->has_A ? 6 : 0))) != hipSuccess) {
        (void)hipGetLastError();
        delete m;
        nhp_set_error(ctx, "out of device memory (discrete model)");
        return NHP_ENOMEM;
    }
    m->d_lambda0 = m->d_block; m->d_W = m->d_lambda0 + N; m->d_theta = m->d_W + NN;
    hipStream_t st = ctx->main();
    hipError_t e = hipMemsetAsync(m->d_block, 0, sizeof(double) * (n + (m->has_A ? 6 : 0)), st);
    if (m->has_A) {
        m->d_A = m->d_theta + NN * (size_t)B;
        m->d_rho = m->d_block + n;
        m->d_links = reinterpret_cast<long long *>(m->d_rho + 4);
    }
    if (e != hipSuccess) { (void)hipFree(m->d_block); delete m; NHP_HIP(ctx, e); }
    *out = m;
    return NHP_OK;
}

extern "C" void nhp_disc_model_destroy(nhp_disc_model *m)
{
    if (!m) return;
    if (m->ctx) { (void)hipSetDevice(m->ctx->device); (void)hipStreamSynchronize(m->ctx->main()); }
    nhp_diag_release(&m->diag);
    nhp_quant_release(&m->quant);
    (void)hipFree(m->d_mom);
    (void)hipFree(m->d_block);
    delete m;
}

extern "C" nhp_status nhp_disc_model_set(nhp_ctx *ctx, nhp_disc_model *m, const double *lambda0, const double *W, const double *theta,
                                         const double *A)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (A && !m->has_A) { nhp_set_error(ctx, "disc_model_set: the model has no adjacency matrix"); return NHP_EINVAL; }
    const size_t N = (size_t)m->N, NN = N * N;
    hipStream_t st = ctx->main();
    if (lambda0) NHP_HIP(ctx, hipMemcpyAsync(m->d_lambda0, lambda0, 8 * N, hipMemcpyHostToDevice, st));
    if (W) NHP_HIP(ctx, hipMemcpyAsync(m->d_W, W, 8 * NN, hipMemcpyHostToDevice, st));
    if (theta) NHP_HIP(ctx, hipMemcpyAsync(m->d_theta, theta, 8 * NN * (size_t)m->B, hipMemcpyHostToDevice, st));
    if (A) {
        NHP_HIP(ctx, hipMemcpyAsync(m->d_A, A, 8 * NN, hipMemcpyHostToDevice, st));
        int64_t links = 0;
        for (size_t i = 0; i < NN; ++i) links += A[i] != 0.0;            // what nhp_disc_resample_adjacency counts
        m->links = links; m->links_on_device = false;
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));                              // the sources are the caller's
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_get(nhp_ctx *ctx, const nhp_disc_model *m, double *lambda0, double *W, double *theta, double *A)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (A && !m->has_A) { nhp_set_error(ctx, "disc_model_get: the model has no adjacency matrix"); return NHP_EINVAL; }
    const size_t N = (size_t)m->N, NN = N * N;
    if (lambda0) NHP_TRY(nhp_download(ctx, lambda0, m->d_lambda0, 8 * N));
    if (W) NHP_TRY(nhp_download(ctx, W, m->d_W, 8 * NN));
    if (theta) NHP_TRY(nhp_download(ctx, theta, m->d_theta, 8 * NN * (size_t)m->B));
    if (A) NHP_TRY(nhp_download(ctx, A, m->d_A, 8 * NN));
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_set_rho(nhp_ctx *ctx, nhp_disc_model *m, double rho)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (!m->has_A) { nhp_set_error(ctx, "set_rho: the model has no adjacency matrix"); return NHP_EINVAL; }
    if (!(rho >= 0.0 && rho <= 1.0)) { nhp_set_error(ctx, "link probability must lie in [0, 1]"); return NHP_EDOMAIN; }
    NHP_HIP(ctx, hipMemcpyAsync(m->d_rho, &rho, sizeof(double), hipMemcpyHostToDevice, ctx->main()));
    NHP_HIP(ctx, hipStreamSynchronize(ctx->main()));          // `rho` is a stack value
    m->rho_set = true;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_get_rho(nhp_ctx *ctx, const nhp_disc_model *m, double *out)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (!out) return NHP_EINVAL;
    if (!m->rho_set) { nhp_set_error(ctx, "get_rho: the model has no device-side link probability (nhp_disc_model_set_rho)"); return NHP_EINVAL; }
    return nhp_download(ctx, out, m->d_rho, 3 * sizeof(double));
}

// ---- the two halves of a step --------------------------------------------------------------------------------------------
extern "C" nhp_status nhp_disc_model_gibbs_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *m, double alpha0, double beta0,
                                                double kappa, double nu, double gamma0, uint64_t seed, uint64_t step)
{
    NHP_TRY(disc_pair_check(ctx, ds, m));
    return nhp_disc_gibbs_enqueue(ctx, ds, m->d_lambda0, m->d_W, m->d_theta, m->d_A, m->dt, alpha0, beta0, kappa, nu, gamma0, seed, step);
}

extern "C" nhp_status nhp_disc_model_network_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *m, double alpha, double beta,
                                                  uint64_t seed, uint64_t step)
{
    NHP_TRY(disc_pair_check(ctx, ds, m));
    if (!m->has_A) { nhp_set_error(ctx, "network_step: the model has no adjacency matrix"); return NHP_EINVAL; }
    if (!m->rho_set) { nhp_set_error(ctx, "network_step: set the link probability first (nhp_disc_model_set_rho)"); return NHP_EINVAL; }
    const bool fixed = alpha == 0.0 && beta == 0.0;                                         // DenseNetworkModel: ρ stays
    if (!fixed && !(alpha > 0.0 && beta > 0.0)) { nhp_set_error(ctx, "network_step: the Beta prior needs alpha, beta > 0"); return NHP_EDOMAIN; }
    // the sweep picks its route to the initial λ from ΣA of the A it starts from (disc_gibbs.hip: lam_pass), as the host entry
    // does from its host copy: the previous sweep's count comes back here, 8 bytes, the step's one read
    if (m->links_on_device) {
        long long links = 0;
        NHP_TRY(nhp_download(ctx, &links, m->d_links, sizeof(links)));
        m->links = links; m->links_on_device = false;
    }
    const int64_t NN = (int64_t)m->N * m->N;
    NHP_TRY(nhp_disc_adjacency_enqueue(ctx, ds, m->d_lambda0, m->d_W, m->d_theta, m->d_A, m->dt, m->d_rho, seed, step, (size_t)m->links));
    hipLaunchKernelGGL(k_disc_links, dim3(1), dim3(1024), 0, ctx->main(), (const double *)m->d_A, NN, m->d_links, m->d_rho);
    NHP_HIP(ctx, hipGetLastError());
    m->links_on_device = true;
    if (!fixed) {
        hipLaunchKernelGGL(k_rho_draw, dim3(1), dim3(64), 0, ctx->main(), m->d_rho, alpha, beta, (double)NN, seed, step);
        NHP_HIP(ctx, hipGetLastError());
    }
    return NHP_OK;
}

// ---- running sums and diagnostics of the kept steps ----------------------------------------------------------------------
extern "C" nhp_status nhp_disc_model_moments_reset(nhp_ctx *ctx, nhp_disc_model *m)
{
    NHP_TRY(disc_model_check(ctx, m));
    const int64_t len = disc_sums_len(m);
    if (!m->d_mom) {
        if (hipMalloc((void **)&m->d_mom, sizeof(double) * 2 * (size_t)len) != hipSuccess) {
            (void)hipGetLastError();
            m->d_mom = nullptr;
            nhp_set_error(ctx, "out of device memory (sample moments)");
            return NHP_ENOMEM;
        }
        m->mom_len = len;
    }
    NHP_HIP(ctx, hipMemsetAsync(m->d_mom, 0, sizeof(double) * 2 * (size_t)len, ctx->main()));
    if (m->d_rho) NHP_HIP(ctx, hipMemsetAsync(m->d_rho + 1, 0, 2 * sizeof(double), ctx->main()));
    m->mom_count = 0;
    if (m->diag) NHP_TRY(nhp_diag_zero(ctx, &m->diag, len));
    if (m->quant) NHP_TRY(nhp_quant_reset(ctx, m));
    return NHP_OK;
}

template <bool PRODUCT>
static void disc_launch_accumulate(nhp_ctx *ctx, nhp_disc_model *m)
{
    const int64_t N = m->N, NN = N * N, len = m->mom_len;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((len + 255) / 256, 2048));
    hipStream_t st = ctx->main();
    const nhp_diag_state *d = m->diag;
    if (!d)
        hipLaunchKernelGGL(k_disc_moments<PRODUCT>, dim3(blocks), dim3(256), 0, st, (const double *)m->d_block, N, NN, len, m->d_mom, m->d_rho);
    else if (nhp_diag_boundary(d))
        hipLaunchKernelGGL((k_disc_accumulate<PRODUCT, true>), dim3(blocks), dim3(256), 0, st, (const double *)m->d_block, N, NN, len, m->d_mom,
                           d->d_bat, (double)d->b, m->d_rho, d->d_rho);
    else
        hipLaunchKernelGGL((k_disc_accumulate<PRODUCT, false>), dim3(blocks), dim3(256), 0, st, (const double *)m->d_block, N, NN, len, m->d_mom,
                           d->d_bat, (double)d->b, m->d_rho, d->d_rho);
}

extern "C" nhp_status nhp_disc_model_moments_accumulate(nhp_ctx *ctx, nhp_disc_model *m)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (!m->d_mom) NHP_TRY(nhp_disc_model_moments_reset(ctx, m));
    if (m->diag && m->diag->len != m->mom_len) { nhp_set_error(ctx, "diagnostics: the planes do not fit the model's sums"); return NHP_EINVAL; }
    if (m->has_A) disc_launch_accumulate<false>(ctx, m);
    else disc_launch_accumulate<true>(ctx, m);
    NHP_HIP(ctx, hipGetLastError());
    if (m->diag) NHP_TRY(nhp_diag_advance(ctx, m->diag, nhp_diag_sums{m->d_mom, m->mom_len, m->mom_count, m->d_rho}));
    ++m->mom_count;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_moments_fetch(nhp_ctx *ctx, const nhp_disc_model *m, double *sum, double *sumsq, int64_t len,
                                                   int64_t *count)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (!sum || !sumsq || !count) return NHP_EINVAL;
    if (!m->d_mom) { nhp_set_error(ctx, "moments: nothing accumulated"); return NHP_EINVAL; }
    if (len != m->mom_len) { nhp_set_error(ctx, "Parameter vector length does not match model parameter length."); return NHP_ESHAPE; }
    NHP_TRY(nhp_download(ctx, sum, m->d_mom, sizeof(double) * (size_t)len));
    NHP_TRY(nhp_download(ctx, sumsq, m->d_mom + len, sizeof(double) * (size_t)len));
    *count = m->mom_count;
    return NHP_OK;
}

extern "C" nhp_status nhp_disc_model_diagnostics_configure(nhp_ctx *ctx, nhp_disc_model *m, int64_t batch_len, int64_t n_planned)
{
    NHP_TRY(disc_model_check(ctx, m));
    return nhp_diag_configure(ctx, &m->diag, disc_sums_len(m), batch_len, n_planned);
}

extern "C" nhp_status nhp_disc_model_diagnostics_fetch(nhp_ctx *ctx, const nhp_disc_model *m, double ess_below, double rhat_above,
                                                       double *summary, double *ess, double *mcse, double *rhat, int64_t len)
{
    NHP_TRY(disc_model_check(ctx, m));
    if (!summary) return NHP_EINVAL;
    const int64_t N = m->N, NN = N * N, NNB = NN * m->B;
    nhp_diag_groups G{};                                  // every group empty until set
    G.end[0] = N;                                         // 0: λ0
    if (m->has_A) {                                       // the block: λ0 | W | θ | A
        G.start[3] = N; G.end[3] = N + NN;                // 3: W
        G.start[1] = N + NN; G.end[1] = N + NN + NNB;     // 1: θ
        G.start[4] = N + NN + NNB; G.end[4] = N + 2 * NN + NNB;
    } else {
        G.start[1] = N; G.end[1] = N + NNB;               // 1: W∘θ
    }
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((NNB + 255) / 256, 256));
    return nhp_diag_finalize(ctx, m->diag, nhp_diag_sums{m->d_mom, m->mom_len, m->mom_count, m->d_rho}, G, nb, m->has_A && m->rho_set,
                             ess_below, rhat_above, summary, ess, mcse, rhat, len);
}

// ---- the driver: the loop body of mcmc! (src/inference.jl:55-62) for a discrete process, device-resident end to end -------
extern "C" nhp_status nhp_disc_mcmc_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *m, double alpha0, double beta0,
                                        double kappa, double nu, double gamma0, double net_alpha, double net_beta, uint64_t seed,
                                        uint64_t step0, int64_t n_steps, int64_t burn)
{
    if (n_steps < 0) return NHP_EINVAL;
    NHP_TRY(disc_pair_check(ctx, ds, m));
    if (m->has_A && !m->rho_set) { nhp_set_error(ctx, "mcmc_run: set the network's link probability first (nhp_disc_model_set_rho)"); return NHP_EINVAL; }
    // attached scorers (nhp_disc_model_attach_score) see the kept steps: those the moments take, or with the moments off
    // (burn < 0) the steps from −(burn + 1) on.  Their scratch is reserved here, so that no step grows it under work in flight.
    const bool scoring = m->score[0] || m->score[1];
    const int64_t score_from = burn >= 0 ? burn : -(burn + 1);
    for (int j = 0; j < 2; ++j)
        if (m->score[j]) NHP_TRY(nhp_disc_score_reserve(ctx, m->score[j]));
    for (int64_t k = 0; k < n_steps; ++k) {
        const uint64_t step = step0 + (uint64_t)k;
        NHP_TRY(nhp_disc_model_gibbs_step(ctx, ds, m, alpha0, beta0, kappa, nu, gamma0, seed, step));
        if (m->has_A) NHP_TRY(nhp_disc_model_network_step(ctx, ds, m, net_alpha, net_beta, seed, step));
        if (burn >= 0 && (int64_t)step >= burn) {
            NHP_TRY(nhp_disc_model_moments_accumulate(ctx, m));
            if (m->quant) NHP_TRY(nhp_quant_kept_step(ctx, m));
        }
        if (scoring && (int64_t)step >= score_from)
            for (int j = 0; j < 2; ++j) {
                if (!m->score[j]) continue;
                if (m->score_kept[j] % m->score_every[j] == 0) NHP_TRY(nhp_disc_score_accumulate(ctx, m->score[j], m));
                ++m->score_kept[j];
            }
    }
    return nhp_ctx_synchronize(ctx);
}
