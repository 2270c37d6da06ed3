// disc_residuals(process, data): nhp_disc_residuals.
//
// Goodness of fit of a discrete Hawkes process on its count matrix.  Cell (t, c) is Poisson(μ[t,c]) with μ the intensity of
// nhp_disc_intensity (the EPI_INTENSITY GEMM, kept on the device here); one streaming pass over (μ, counts) makes of every
// cell its randomized probability integral transform (uniform under the model), its Pearson residual, and the per-node sums
// Σμ, Σs, χ², deviance and the histogram of the transforms; a two-level scan along t makes the cumulative compensator.
//
// Every fp64 sum has one fixed order (per-workgroup partials in the order of nhp_block_sum, joined chunk by chunk by a second
// kernel; the scan likewise), every integer sum goes through integer atomics: the same call gives the same bits.  The Poisson
// cdf of a cell is summed term by term from the saddle-point pmf, so lanes run as long as their cell needs (DESIGN 3.14 has
// what that costs); include/nhp.h has the arithmetic in full, tests/disc_residuals_ref.py restates it in numpy.
#include "nhp_sim.h"

#define RES_KEY 0x2545F4914F6CDD1Dull                 // Philox key family: step 0, element c + N·t, attempt 0
#define RES_BLOCK 256
#define RES_ITEMS 4                                   // cells per thread
#define RES_CHUNK (RES_BLOCK * RES_ITEMS)             // bins of one node per workgroup, in the residual pass and in the scan
#define RES_BINS_MAX 4096                             // histogram bins (the LDS counters of a workgroup)
#define RES_CELL_MAX 1048576.0                        // 2^20: the largest mean and the largest count (bounds the tail loops)
#define RES_TINY 0x1p-60                              // a tail stops at this fraction of its sum

struct res_scal {
    unsigned long long impossible;                    // cells with μ = 0 and s > 0
    int bad;                                          // 1: a mean negative or not finite, 2: a mean or a count above 2^20
    int pad;
};

// the Stirling error δ(s) = lgamma(s + 1) - (s + 1/2)·log s + s - log(2π)/2 for s = 1 .. 15, correctly rounded
static __device__ const double res_sferr[16] = {
    0.0, 0.081061466795327258, 0.041340695955409294, 0.027677925684998339, 0.020790672103765093, 0.016644691189821192,
    0.013876128823070748, 0.011896709945891770, 0.010411265261972096, 0.0092554621827127329, 0.0083305634333628713,
    0.0075736754879518408, 0.0069428401072095299, 0.0064089941880042071, 0.0059513701127588477, 0.0055547335519628014};

static __device__ __forceinline__ double res_stirlerr(double s)
{
#pragma clang fp contract(off)
    if (s < 16.0) return res_sferr[(int)s];
    const double s2 = s * s;
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) / s2) / s2) / s2) / s2) / s;
}

// D(s, μ) = s·log(s/μ) + μ - s for s > 0, μ > 0: by its series in x = (s - μ)/(s + μ) where the closed form cancels
static __device__ __forceinline__ double res_bd0(double s, double mu)
{
#pragma clang fp contract(off)
    const double d = s - mu, sm = s + mu;
    if (fabs(d) < 0.1 * sm) {
        const double x = d / sm, v = x * x;
        double q = 1.0 / 21.0;
        q = q * v + 1.0 / 19.0;
        q = q * v + 1.0 / 17.0;
        q = q * v + 1.0 / 15.0;
        q = q * v + 1.0 / 13.0;
        q = q * v + 1.0 / 11.0;
        q = q * v + 1.0 / 9.0;
        q = q * v + 1.0 / 7.0;
        q = q * v + 1.0 / 5.0;
        q = q * v + 1.0 / 3.0;
        q = q * v;
        return d * x + ((2.0 * s) * x) * q;
    }
    return s * nhp_log(s / mu) + mu - s;
}

// one cell with 0 < μ <= 2^20, 0 <= s <= 2^20: the transform, and D(s, μ) for the deviance
static __device__ double res_cell(double s, double mu, double v, double *dev)
{
#pragma clang fp contract(off)
    double ps, D;
    if (s == 0.0) {
        D = mu;
        ps = nhp_exp(-mu);
    } else {
        D = res_bd0(s, mu);
        ps = nhp_exp(-res_stirlerr(s) - D) / sqrt(6.283185307179586 * s);
    }
    *dev = D;
    double t = ps, acc = 0.0, k = s, pit;
    if (s <= mu) {                                    // F(s - 1): the terms below s, downward
        while (k > 0.0) {
            t = t * k / mu;
            acc = acc + t;
            k -= 1.0;
            if (!(t > RES_TINY * acc)) break;
        }
        pit = acc + v * ps;
    } else {                                          // 1 - F(s): the terms above s, upward (the rest is below t·r/(1 - r))
        for (;;) {
            k += 1.0;
            t = t * mu / k;
            acc = acc + t;
            if (!(t > RES_TINY * acc * (1.0 - mu / (k + 1.0)))) break;
        }
        pit = (1.0 - acc) - (1.0 - v) * ps;
    }
    return fmin(fmax(pit, 0.0), 1.0);
}

// the checks, before anything is released: lane i = t + T·c
static __global__ void __launch_bounds__(RES_BLOCK) k_disc_res_check(const double *__restrict__ lam, const double *__restrict__ data,
                                                                     int64_t n, res_scal *__restrict__ sc)
{
    const int64_t i = (int64_t)blockIdx.x * RES_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double mu = lam[i], s = data[i];
    int bad = 0;
    if (!(mu >= 0.0 && mu < INFINITY)) bad = 1;
    else if (mu > RES_CELL_MAX || s > RES_CELL_MAX) bad = 2;
    if (bad) atomicOr(&sc->bad, bad);
}

// Workgroup (c, j) takes the bins [j·RES_CHUNK, (j+1)·RES_CHUNK) of node c: thread x the bins t0 + x + RES_BLOCK·r, so a wave
// reads and writes 512 contiguous bytes.  part[(c·nch + j)·3 + {0, 1, 2}] = the chunk's Σμ, Σ(s-μ)²/μ, ΣD; observed, the
// histogram and sc->impossible receive integer atomics (the histogram through LDS counters first).
static __global__ void __launch_bounds__(RES_BLOCK) k_disc_residuals(const double *__restrict__ lam, const double *__restrict__ data,
                                                                     int64_t T, int32_t N, int32_t nch, uint64_t key, int32_t nbins,
                                                                     double *__restrict__ pit, double *__restrict__ pearson,
                                                                     double *__restrict__ part, unsigned long long *__restrict__ observed,
                                                                     unsigned long long *__restrict__ hist, res_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    __shared__ unsigned int bins[RES_BINS_MAX];
    __shared__ double red[NHP_WAVES];
    const int32_t c = (int32_t)(blockIdx.x / (unsigned)nch), j = (int32_t)(blockIdx.x % (unsigned)nch);
    for (int32_t b = threadIdx.x; b < nbins; b += RES_BLOCK) bins[b] = 0u;
    __syncthreads();
    const int64_t t0 = (int64_t)j * RES_CHUNK + threadIdx.x;
    const double fb = (double)nbins;
    double e_sum = 0.0, x_sum = 0.0, d_sum = 0.0;
    unsigned long long obs = 0ull, imp = 0ull;
    for (int r = 0; r < RES_ITEMS; ++r) {
        const int64_t t = t0 + (int64_t)RES_BLOCK * r;
        if (t >= T) break;
        const size_t i = (size_t)t + (size_t)T * (size_t)c;
        const double mu = lam[i], s = data[i];
        double ua, ub;
        philox_2u(key, 0, (uint64_t)c + (uint64_t)N * (uint64_t)t, 0, &ua, &ub);
        const double v = ua - 0x1p-53;
        double p, pe, chi, dev;
        if (mu == 0.0) {
            dev = 0.0;
            if (s == 0.0) { p = v; pe = 0.0; chi = 0.0; }
            else { p = 1.0; pe = INFINITY; chi = INFINITY; ++imp; }
        } else {
            const double d = s - mu;
            pe = d / sqrt(mu);
            chi = (d * d) / mu;
            p = res_cell(s, mu, v, &dev);
        }
        e_sum = e_sum + mu;
        x_sum = x_sum + chi;
        d_sum = d_sum + dev;
        obs += (unsigned long long)s;
        if (pit) pit[i] = p;
        if (pearson) pearson[i] = pe;
        const int32_t b = min((int32_t)(p * fb), nbins - 1);
        atomicAdd(&bins[b], 1u);
    }
    e_sum = nhp_block_sum(e_sum, red);
    x_sum = nhp_block_sum(x_sum, red);
    d_sum = nhp_block_sum(d_sum, red);
    if (threadIdx.x == 0) {
        double *o = part + (size_t)blockIdx.x * 3;
        o[0] = e_sum; o[1] = x_sum; o[2] = d_sum;
    }
    sim_wave_add(obs, observed + c);
    sim_wave_add(imp, &sc->impossible);
    __syncthreads();
    for (int32_t b = threadIdx.x; b < nbins; b += RES_BLOCK)
        if (bins[b]) atomicAdd(hist + ((size_t)c * nbins + b), (unsigned long long)bins[b]);
}

// the chunks of a node, j ascending: lane c
static __global__ void __launch_bounds__(RES_BLOCK) k_disc_res_join(const double *__restrict__ part, int32_t N, int32_t nch,
                                                                    double *__restrict__ expected, double *__restrict__ chi2,
                                                                    double *__restrict__ deviance)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * RES_BLOCK + threadIdx.x;
    if (c >= N) return;
    const double *p = part + (size_t)c * nch * 3;
    double e = 0.0, x = 0.0, d = 0.0;
    for (int32_t j = 0; j < nch; ++j) { e = e + p[3 * j]; x = x + p[3 * j + 1]; d = d + p[3 * j + 2]; }
    expected[c] = e;
    chi2[c] = x;
    deviance[c] = 2.0 * d;
}

// ---- the cumulative compensator: an inclusive scan along t per node, two levels ---------------------------------------------
// a thread's RES_ITEMS consecutive bins of chunk (c, j); beyond T: 0
static __device__ __forceinline__ double res_load_run(const double *__restrict__ lam, int64_t T, int32_t c, int64_t t0, double *v)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int r = 0; r < RES_ITEMS; ++r) {
        v[r] = t0 + r < T ? lam[(size_t)(t0 + r) + (size_t)T * (size_t)c] : 0.0;
        s = s + v[r];
    }
    return s;
}

static __global__ void __launch_bounds__(RES_BLOCK) k_disc_cum_sums(const double *__restrict__ lam, int64_t T, int32_t nch,
                                                                    double *__restrict__ csum)
{
    __shared__ double wsum[RES_BLOCK / 64];
    const int32_t c = (int32_t)(blockIdx.x / (unsigned)nch), j = (int32_t)(blockIdx.x % (unsigned)nch);
    double v[RES_ITEMS], tot;
    const double s = res_load_run(lam, T, c, (int64_t)j * RES_CHUNK + (int64_t)threadIdx.x * RES_ITEMS, v);
    (void)dd_block_exclusive<double>(s, wsum, &tot);
    if (threadIdx.x == 0) csum[blockIdx.x] = tot;
}

// the chunk sums of node c (lane c) in place, exclusive, j ascending
static __global__ void __launch_bounds__(RES_BLOCK) k_disc_cum_offsets(double *__restrict__ csum, int32_t N, int32_t nch)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * RES_BLOCK + threadIdx.x;
    if (c >= N) return;
    double *p = csum + (size_t)c * nch;
    double run = 0.0;
    for (int32_t j = 0; j < nch; ++j) { const double v = p[j]; p[j] = run; run = run + v; }
}

static __global__ void __launch_bounds__(RES_BLOCK) k_disc_cumulative(const double *__restrict__ lam, int64_t T, int32_t nch,
                                                                      const double *__restrict__ csum, double *__restrict__ cum)
{
#pragma clang fp contract(off)
    __shared__ double wsum[RES_BLOCK / 64];
    const int32_t c = (int32_t)(blockIdx.x / (unsigned)nch), j = (int32_t)(blockIdx.x % (unsigned)nch);
    const int64_t t0 = (int64_t)j * RES_CHUNK + (int64_t)threadIdx.x * RES_ITEMS;
    double v[RES_ITEMS], tot;
    const double s = res_load_run(lam, T, c, t0, v);
    double run = csum[blockIdx.x] + dd_block_exclusive<double>(s, wsum, &tot);
    for (int r = 0; r < RES_ITEMS; ++r) {
        run = run + v[r];
        if (t0 + r < T) cum[(size_t)(t0 + r) + (size_t)T * (size_t)c] = run;
    }
}


extern "C" nhp_status nhp_disc_residuals(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W,
                                         const double *theta, const double *A, double dt, uint64_t seed, int32_t nbins,
                                         int32_t output_on_device, double *pit, double *pearson, double *cumulative, double *expected,
                                         int64_t *observed, double *chi2, double *deviance, int64_t *histogram, int64_t *impossible,
                                         double *pass_ms)
{
    if (!ctx) return NHP_EINVAL;
    if (!ds || !W || !theta || !expected || !observed || !chi2 || !deviance || !histogram || !impossible) {
        nhp_set_error(ctx, "disc_residuals: null argument");
        return NHP_EINVAL;
    }
    if (nbins < 1 || nbins > RES_BINS_MAX) {
        nhp_set_error(ctx, "disc_residuals: nbins = %d outside [1, %d]", nbins, RES_BINS_MAX);
        return NHP_EINVAL;
    }
    *impossible = 0;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const int32_t N = ds->N;
    const int64_t T = ds->T, TN = T * N, nch64 = (T + RES_CHUNK - 1) / RES_CHUNK, NB = (int64_t)N * nbins;
    if (nch64 * N >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "disc_residuals: n_nodes * ceil(n_bins / %d) is not below 2^31 (one workgroup each)", RES_CHUNK);
        return NHP_ENOTIMPL;
    }
    const int32_t nch = (int32_t)nch64;
    const unsigned wgs = (unsigned)(nch64 * N);

    // ---- the intensity, kept on the device (behind the staged model in the ctx scratch)
    double *E, *base, *d_lam;
    NHP_TRY(nhp_disc_stage_bump(ctx, ds, lambda0, W, theta, A, dt, &E, &base, (size_t)TN, &d_lam));
    NHP_TRY(nhp_disc_launch_intensity(ctx, ds, E, base, lambda0 == nullptr, d_lam));

    // ---- scratch: the partial sums, and the outputs a host caller receives by copy
    dd_arena a1;
    a1.st = st;
    res_scal *d_sc = nullptr;
    double *d_part = nullptr, *d_csum = nullptr;
    double *o_pit = pit, *o_pe = pearson, *o_cum = cumulative, *o_exp = expected, *o_chi = chi2, *o_dev = deviance;
    int64_t *o_obs = observed, *o_hist = histogram;
    a1.ask(&d_sc, 1); a1.ask(&d_part, (int64_t)wgs * 3);
    if (cumulative) a1.ask(&d_csum, (int64_t)wgs);
    if (!output_on_device) {
        if (pit) a1.ask(&o_pit, TN);
        if (pearson) a1.ask(&o_pe, TN);
        if (cumulative) a1.ask(&o_cum, TN);
        a1.ask(&o_exp, N); a1.ask(&o_chi, N); a1.ask(&o_dev, N); a1.ask(&o_obs, N); a1.ask(&o_hist, NB);
    }
    if (a1.alloc() != hipSuccess) {
        (void)hipGetLastError();
        nhp_set_error(ctx, "disc_residuals: out of device memory (N = %d, T = %lld)", N, (long long)T);
        return NHP_ENOMEM;
    }
    sim_pinned<res_scal> pin;
    NHP_HIP(ctx, hipHostMalloc((void **)&pin.h, sizeof(res_scal), hipHostMallocDefault));

    // ---- the checks; readback 1
    NHP_HIP(ctx, hipMemsetAsync(d_sc, 0, sizeof(res_scal), st));
    k_disc_res_check<<<dd_grid(TN, RES_BLOCK), RES_BLOCK, 0, st>>>(d_lam, ds->d_dataT, TN, d_sc);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, pin.h, d_sc));
    if (pin.h->bad & 1) {
        nhp_set_error(ctx, "disc_residuals: the cell means must be finite and >= 0");
        return NHP_EDOMAIN;
    }
    if (pin.h->bad & 2) {
        nhp_set_error(ctx, "disc_residuals: a cell mean or a count above 2^20");
        return NHP_ENOTIMPL;
    }

    // ---- the pass, the join, the scan; readback 2
    NHP_HIP(ctx, hipMemsetAsync(o_obs, 0, sizeof(int64_t) * N, st));
    NHP_HIP(ctx, hipMemsetAsync(o_hist, 0, sizeof(int64_t) * NB, st));
    if (pass_ms) NHP_HIP(ctx, hipEventRecord(ctx->ev0, st));
    k_disc_residuals<<<wgs, RES_BLOCK, 0, st>>>(d_lam, ds->d_dataT, T, N, nch, seed ^ RES_KEY, nbins, o_pit, o_pe, d_part,
                                                (unsigned long long *)o_obs, (unsigned long long *)o_hist, d_sc);
    if (pass_ms) NHP_HIP(ctx, hipEventRecord(ctx->ev1, st));
    k_disc_res_join<<<dd_grid(N, RES_BLOCK), RES_BLOCK, 0, st>>>(d_part, N, nch, o_exp, o_chi, o_dev);
    if (cumulative) {
        k_disc_cum_sums<<<wgs, RES_BLOCK, 0, st>>>(d_lam, T, nch, d_csum);
        k_disc_cum_offsets<<<dd_grid(N, RES_BLOCK), RES_BLOCK, 0, st>>>(d_csum, N, nch);
        k_disc_cumulative<<<wgs, RES_BLOCK, 0, st>>>(d_lam, T, nch, d_csum, o_cum);
    }
    NHP_HIP(ctx, hipGetLastError());
    if (!output_on_device) {
        if (pit) NHP_TRY(nhp_download(ctx, pit, o_pit, sizeof(double) * TN));
        if (pearson) NHP_TRY(nhp_download(ctx, pearson, o_pe, sizeof(double) * TN));
        if (cumulative) NHP_TRY(nhp_download(ctx, cumulative, o_cum, sizeof(double) * TN));
        NHP_HIP(ctx, hipMemcpyAsync(expected, o_exp, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipMemcpyAsync(chi2, o_chi, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipMemcpyAsync(deviance, o_dev, sizeof(double) * N, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipMemcpyAsync(observed, o_obs, sizeof(int64_t) * N, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipMemcpyAsync(histogram, o_hist, sizeof(int64_t) * NB, hipMemcpyDeviceToHost, st));
    }
    NHP_TRY(sim_read(ctx, pin.h, d_sc));
    *impossible = (int64_t)pin.h->impossible;
    if (pass_ms) {
        float ms = 0.0f;
        NHP_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        *pass_ms = (double)ms;
    }
    return NHP_OK;
}
