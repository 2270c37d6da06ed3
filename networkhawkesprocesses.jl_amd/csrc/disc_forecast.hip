// disc_forecast(process, data, horizon): nhp_disc_forecast.
//
// S independent continuations of an observed count matrix s[p, 1..T0] over the bins T0+1 .. T0+H, conditional on the counts,
// under the law nhp_disc_simulate draws.  A continuation is the union of three independent parts: the children the observed
// events still have beyond T0 -- cell (c, T0+k) receives Poisson(carry[k,c]) of them, carry[k,c] = Σ_p Σ_{l>=k}
// s[p,T0+k-l]·h[p,c,l] --, new immigrants, Poisson(base[k,c]) per cell, and the descendants of both inside the H bins.
//
// Boundary state: the tables of nhp_dsim.h (lag CDF, link masses, row prefixes); the lagged history sums
// x[k,p,b] = Σ_{l>=k} s[p,T0+k-l]·φ[l,b]; carry[k,c] = dt·Σ_p Σ_b (W·A·θ)[p,c,b]·x[k,p,b]; the cell means base + carry; and
// the exact predictive mean μ_k = base_k + carry_k + Σ_l H_lᵀ μ_{k-l}, bin after bin (two small launches per bin).  Every sum
// runs in one fixed order in fp64 without contraction and without floating-point atomics.
//
// Ensemble: nhp_disc_simulate over S·H bins -- cell e = c + N·(k + H·r), bin k of replica r -- with the cell mean
// (base + carry)[k,c] and children that stay only inside their replica's H bins (k_dsim_children<true>).  All replicas share
// the arena and every launch; chunking, scans, block-partial run scalars, one readback per generation and the max_events guard
// are those of disc_simulate.hip.  The result leaves through integer atomics: totals[r,c], cell_sum[k,c], optionally
// paths[r,k,c].
//
// Random numbers: Philox4x32-10 of nhp_rng.h with three key families of its own; include/nhp.h has the scheme in full,
// tests/disc_forecast_ref.py restates it in numpy.
#include "nhp_dsim.h"

// Philox key families (XORed into the seed)
#define DFC_KEY_CELL 0xDA942042E4DD58B5ull            // carry-over + immigrants of a cell: step 0, element c + N·(k + H·r)
#define DFC_KEY_CHILD_COUNT 0xD1B54A32D192ED03ull     // children of an arena entry:        step = its generation, element = arena index
#define DFC_KEY_CHILD 0x8CB92BA72F3D8DD7ull           // node, basis, lag of a child:       step = its parent's generation, element = slot

#define DFC_CELL_CHECK 8                              // cell chunks between two looks at the event count (a blocking readback each)

// lagged history sums: lane i = k + K·(b + B·p) (k, b, p 0-based; forecast bin k+1), x[i] = Σ_l s[p, T0+(k+1)-l]·φ[l,b] over the
// lags l = k+1 .. L that reach an observed bin, l ascending.  tail [Tu*N] holds the last Tu bins, node fastest; the lanes of
// k = 0 read every count of the tail, which is where negative counts are flagged.
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_lagged(const int64_t *__restrict__ tail, int32_t Tu, const double *__restrict__ phi,
                                                                 int32_t N, int32_t B, int32_t L, int32_t K, int64_t n,
                                                                 double *__restrict__ x, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t k = (int32_t)(i % K);
    const int64_t pb = i / K;
    const int32_t b = (int32_t)(pb % B), p = (int32_t)(pb / B);
    double acc = 0.0;
    int bad = 0;
    for (int32_t l = k + 1; l <= L; ++l) {
        const int32_t j = Tu + k - l;                 // the tail's bin of T0 + (k+1) - l
        if (j < 0) break;
        const int64_t s = tail[(size_t)j * N + p];
        bad |= s < 0;
        acc = acc + (double)s * phi[(size_t)b * L + (l - 1)];
    }
    x[i] = acc;
    if (bad) atomicOr(&sc->bad, 4);
}

// carry[k,c] = dt·Σ_p Σ_b ((W[p,c]·A[p,c])·θ[p,c,b])·x[k,p,b], p ascending, b ascending inside: lane i = k + K·c, so a wave shares
// its one or two columns of θ (a broadcast read) and reads x along k
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_carry(const double *__restrict__ W, const double *__restrict__ A,
                                                                const double *__restrict__ theta, const double *__restrict__ x, double dt,
                                                                int32_t N, int32_t B, int32_t K, double *__restrict__ carry)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i >= (int64_t)K * N) return;
    const int32_t k = (int32_t)(i % K), c = (int32_t)(i / K);
    const size_t NN = (size_t)N * N;
    double acc = 0.0;
    for (int32_t p = 0; p < N; ++p) {
        const size_t q = (size_t)p + (size_t)c * N;
        const double w = A ? W[q] * A[q] : W[q];
        for (int32_t b = 0; b < B; ++b) acc = acc + (w * theta[q + NN * b]) * x[((size_t)p * B + b) * K + k];
    }
    carry[(size_t)k * N + c] = dt * acc;
}

// the cell means cm[k,c] = base[k,c] + carry[k,c] (carry is 0 from bin K on), with the checks: lane i = c + N·k
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_means(const double *__restrict__ lambda0, const double *__restrict__ base, double dt,
                                                                const double *__restrict__ carry, int32_t N, int64_t H, int64_t n,
                                                                double *__restrict__ cm, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t k = i / N;
    const int32_t c = (int32_t)(i - k * N);
    const double b = lambda0 ? lambda0[c] * dt : base[(size_t)c * H + k];
    const double mean = b + carry[i];
    const bool ok = b >= 0.0 && mean >= 0.0 && mean <= DSIM_CELL_MAX;
    if (!ok) atomicOr(&sc->bad, 2);
    cm[i] = ok ? mean : 0.0;
}

// the mean recursion, first launch of bin k (0-based, k >= 1): z[p,b] = Σ_{l=1..min(L,k)} φ[l,b]·μ[k-l,p], l ascending
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_conv(const double *__restrict__ phi, const double *__restrict__ mu, int32_t N,
                                                               int32_t B, int32_t L, int64_t k, double *__restrict__ z)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i >= (int64_t)N * B) return;
    const int32_t b = (int32_t)(i % B), p = (int32_t)(i / B);
    const int32_t top = (int32_t)min((int64_t)L, k);
    double acc = 0.0;
    for (int32_t l = 1; l <= top; ++l) acc = acc + phi[(size_t)b * L + (l - 1)] * mu[(size_t)(k - l) * N + p];
    z[i] = acc;
}

// second launch: μ[k,c] = cm[k,c] + dt·Σ_p Σ_b ((W·A)·θ)[p,c,b]·z[p,b], one wave per c: lane t adds its rows p = t, t + 64, ...
// (p ascending, b ascending inside: θ[·,c,b] is read along p), then the 64 partial sums meet in a fixed butterfly
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_mix(const double *__restrict__ W, const double *__restrict__ A,
                                                              const double *__restrict__ theta, const double *__restrict__ z,
                                                              const double *__restrict__ cm, double dt, int32_t N, int32_t B, int64_t k,
                                                              double *__restrict__ mu)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * (SIM_BLOCK / 64) + (threadIdx.x >> 6), t = threadIdx.x & 63;
    if (c >= N) return;                               // whole waves leave together
    const size_t NN = (size_t)N * N;
    double acc = 0.0;
    for (int32_t p = t; p < N; p += 64) {
        const size_t q = (size_t)p + (size_t)c * N;
        const double w = A ? W[q] * A[q] : W[q];
        for (int32_t b = 0; b < B; ++b) acc = acc + (w * theta[q + NN * b]) * z[(size_t)p * B + b];
    }
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    if (t == 0) mu[(size_t)k * N + c] = cm[(size_t)k * N + c] + dt * acc;
}

// carry-over children + immigrants of the cells e = e0 + j (e = c + N·(k + H·r)): one Poisson(cm[k,c]); i0 = e0 mod H·N
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_cells(const double *__restrict__ cm, uint64_t HN, uint64_t i0, int64_t e0, int64_t m,
                                                                uint64_t key, int32_t *__restrict__ kbuf, uint32_t *__restrict__ flag)
{
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint64_t q = i0 + (uint64_t)j;
    const uint64_t i = (q >> 32) == 0 && (HN >> 32) == 0 ? (uint64_t)((uint32_t)q % (uint32_t)HN) : q % HN;
    const int32_t k = (int32_t)sim_poisson(cm[i], key, 0, (uint64_t)(e0 + j));
    kbuf[j] = k;
    flag[j] = k > 0;
}

// the histograms: every entry's multiplicity into its replica's node total, its (bin, node) sum over the replicas, its cell
static __global__ void __launch_bounds__(SIM_BLOCK) k_dfc_hist(int64_t n, const int32_t *__restrict__ anode, const int32_t *__restrict__ abin,
                                                               const int32_t *__restrict__ ak, int32_t N, int32_t H, int64_t *__restrict__ totals,
                                                               int64_t *__restrict__ cell_sum, int64_t *__restrict__ paths)
{
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t g = abin[i], c = anode[i], r = g / H, k = g - r * H;
    const unsigned long long v = (unsigned long long)ak[i];
    atomicAdd((unsigned long long *)(totals + ((size_t)r * N + c)), v);
    atomicAdd((unsigned long long *)(cell_sum + ((size_t)k * N + c)), v);
    if (paths) atomicAdd((unsigned long long *)(paths + ((size_t)g * N + c)), v);
}


extern "C" nhp_status nhp_disc_forecast(nhp_ctx *ctx, const double *lambda0, const double *base, const double *W, const double *theta,
                                        const double *A, const double *phi, int32_t n_lags, int32_t n_basis, double dt, int32_t n_nodes,
                                        const int64_t *history, int64_t n_history_bins, int32_t history_on_device, int64_t horizon_bins,
                                        int64_t nsamples, uint64_t seed, int64_t max_events, int32_t output_on_device, int64_t *totals,
                                        int64_t *cell_sum, int64_t *paths, double *carry, double *expected, int64_t *n_events,
                                        int32_t *n_generations)
{
    if (!ctx) return NHP_EINVAL;
    if (!W || !theta || !phi || !history || !totals || !cell_sum || !n_events) {
        nhp_set_error(ctx, "disc_forecast: null argument");
        return NHP_EINVAL;
    }
    if ((lambda0 != nullptr) == (base != nullptr)) {
        nhp_set_error(ctx, "disc_forecast: exactly one of lambda0 [N] and base [H*N] must be given");
        return NHP_EINVAL;
    }
    if (n_nodes < 1 || n_lags < 1 || n_basis < 1 || n_history_bins < 1 || horizon_bins < 1 || nsamples < 1) {
        nhp_set_error(ctx, "disc_forecast: n_nodes, n_lags, n_basis, n_history_bins, horizon_bins and nsamples must be positive");
        return NHP_EINVAL;
    }
    if (max_events < 0 || max_events >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "disc_forecast: max_events = %lld outside [0, 2^31)", (long long)max_events);
        return NHP_EINVAL;
    }
    if (horizon_bins >= ((int64_t)1 << 31) || nsamples >= ((int64_t)1 << 31) || nsamples * horizon_bins >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "disc_forecast: nsamples * horizon_bins = %lld * %lld is not below 2^31 (bins are 32-bit in the arena)",
                      (long long)nsamples, (long long)horizon_bins);
        return NHP_ENOTIMPL;
    }
    if (nsamples * horizon_bins * n_nodes >= ((int64_t)1 << 56)) {
        nhp_set_error(ctx, "disc_forecast: nsamples * horizon_bins * n_nodes is not below 2^56 (int64 indexing of the paths in bytes)");
        return NHP_ENOTIMPL;
    }
    if (!(dt >= 0.0 && dt < INFINITY)) {
        nhp_set_error(ctx, "disc_forecast: dt must be non-negative and finite, got %g", dt);
        return NHP_EDOMAIN;
    }
    *n_events = 0;
    if (n_generations) *n_generations = 0;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const int32_t N = n_nodes, B = n_basis, L = n_lags;
    const int64_t H = horizon_bins, S = nsamples, HN = H * N, SN = S * N, NT = S * HN, NN = (int64_t)N * N;
    const int32_t K = (int32_t)std::min<int64_t>(L, H);                  // forecast bins the observed events still reach
    const int32_t Tu = (int32_t)std::min<int64_t>(L, n_history_bins);    // history bins that reach a forecast bin
    const int64_t *tail = history + (n_history_bins - Tu) * N;
    const int64_t cap = max_events;
    const int64_t CH = std::min(std::max(cap, SIM_CHUNK_MIN), SIM_CHUNK_MAX);
    sim_pinned<dsim_scal> pin;
    NHP_HIP(ctx, hipHostMalloc((void **)&pin.h, sizeof(dsim_scal), hipHostMallocDefault));
    dsim_scal *h = pin.h;

    // ---- scratch: the parameters and tables, the boundary state, the arena (max_events entries), one chunk of cells / child
    // slots, and the outputs a host caller receives by copy
    dd_arena a1;
    a1.st = st;
    double *d_W = nullptr, *d_th = nullptr, *d_A = nullptr, *d_phi = nullptr, *d_l0 = nullptr, *d_base = nullptr;
    double *d_V = nullptr, *d_G = nullptr, *d_R = nullptr, *d_mb = nullptr, *d_cdf = nullptr;
    double *d_x = nullptr, *d_cm = nullptr, *d_z = nullptr, *o_carry = carry, *o_mu = expected;
    int64_t *d_tail = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_tmp64 = nullptr;
    int64_t *o_tot = totals, *o_cell = cell_sum, *o_paths = paths;
    int32_t *d_anode = nullptr, *d_abin = nullptr, *d_ak = nullptr, *d_cn = nullptr, *d_cb = nullptr;
    uint32_t *d_keep = nullptr, *d_pos = nullptr, *d_tmp32 = nullptr;
    unsigned long long *d_pa = nullptr, *d_pb = nullptr;
    dsim_scal *d_sc = nullptr;
    a1.ask(&d_W, NN); a1.ask(&d_th, NN * B); a1.ask(&d_phi, (int64_t)L * B);
    if (A) a1.ask(&d_A, NN);
    if (lambda0) a1.ask(&d_l0, N); else a1.ask(&d_base, HN);
    if (!history_on_device) a1.ask(&d_tail, (int64_t)Tu * N);
    a1.ask(&d_V, NN); a1.ask(&d_G, NN); a1.ask(&d_R, N); a1.ask(&d_mb, B); a1.ask(&d_cdf, (int64_t)L * B);
    a1.ask(&d_x, (int64_t)K * N * B); a1.ask(&d_cm, HN);
    if (expected) a1.ask(&d_z, (int64_t)N * B);
    a1.ask(&d_tmp64, dd_grid(cap, DD_TILE));
    a1.ask(&d_anode, cap); a1.ask(&d_abin, cap); a1.ask(&d_ak, cap); a1.ask(&d_cnt, cap); a1.ask(&d_off, cap + 1);
    a1.ask(&d_cn, CH); a1.ask(&d_cb, CH); a1.ask(&d_keep, CH); a1.ask(&d_pos, CH + 1);
    a1.ask(&d_tmp32, dd_grid(CH, DD_TILE)); a1.ask(&d_pa, dd_grid(CH, SIM_BLOCK)); a1.ask(&d_pb, dd_grid(CH, SIM_BLOCK));
    a1.ask(&d_sc, 1);
    if (!output_on_device || !carry) a1.ask(&o_carry, HN);
    if (!output_on_device) {
        a1.ask(&o_tot, SN); a1.ask(&o_cell, HN);
        if (paths) a1.ask(&o_paths, NT);
        if (expected) a1.ask(&o_mu, HN);
    }
    if (a1.alloc() != hipSuccess) {
        (void)hipGetLastError();
        nhp_set_error(ctx, "disc_forecast: out of device memory (N = %d, H = %lld, S = %lld, max_events = %lld)", N, (long long)H,
                      (long long)S, (long long)cap);
        return NHP_ENOMEM;
    }
    NHP_HIP(ctx, hipMemcpyAsync(d_W, W, sizeof(double) * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_th, theta, sizeof(double) * NN * B, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_phi, phi, sizeof(double) * L * B, hipMemcpyHostToDevice, st));
    if (A) NHP_HIP(ctx, hipMemcpyAsync(d_A, A, sizeof(double) * NN, hipMemcpyHostToDevice, st));
    if (lambda0) NHP_HIP(ctx, hipMemcpyAsync(d_l0, lambda0, sizeof(double) * N, hipMemcpyHostToDevice, st));
    else NHP_HIP(ctx, hipMemcpyAsync(d_base, base, sizeof(double) * HN, hipMemcpyHostToDevice, st));
    if (!history_on_device) {
        NHP_HIP(ctx, hipMemcpyAsync(d_tail, tail, sizeof(int64_t) * Tu * N, hipMemcpyHostToDevice, st));
        tail = d_tail;
    }

    dsim_args a;
    a.G = d_G; a.R = d_R; a.theta = d_th; a.mb = d_mb; a.cdf = d_cdf; a.T = H; a.N = N; a.B = B; a.L = L;
    a.key_count = seed ^ DFC_KEY_CHILD_COUNT; a.key_child = seed ^ DFC_KEY_CHILD;

    // ---- boundary state: tables, lagged sums, carry, cell means, the exact mean; readback 1: the checks
    NHP_HIP(ctx, hipMemsetAsync(d_sc, 0, sizeof(dsim_scal), st));
    NHP_HIP(ctx, hipMemsetAsync(o_carry, 0, sizeof(double) * HN, st));
    NHP_HIP(ctx, hipMemsetAsync(o_tot, 0, sizeof(int64_t) * SN, st));
    NHP_HIP(ctx, hipMemsetAsync(o_cell, 0, sizeof(int64_t) * HN, st));
    if (o_paths) NHP_HIP(ctx, hipMemsetAsync(o_paths, 0, sizeof(int64_t) * NT, st));
    k_dsim_lags<<<dd_grid(B, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_phi, L, B, dt, d_cdf, d_mb, d_sc);
    k_dsim_mass<<<dd_grid(NN, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_W, d_A, d_th, d_mb, NN, B, d_V, d_sc);
    k_dsim_rows<<<dd_grid(N, SIM_ROWS), SIM_ROWS, 0, st>>>(d_V, N, d_G, d_R, d_sc);
    const int64_t nx = (int64_t)K * N * B;
    k_dfc_lagged<<<dd_grid(nx, SIM_BLOCK), SIM_BLOCK, 0, st>>>(tail, Tu, d_phi, N, B, L, K, nx, d_x, d_sc);
    k_dfc_carry<<<dd_grid((int64_t)K * N, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_W, d_A, d_th, d_x, dt, N, B, K, o_carry);
    k_dfc_means<<<dd_grid(HN, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_l0, d_base, dt, o_carry, N, H, HN, d_cm, d_sc);
    if (expected) {
        NHP_HIP(ctx, hipMemcpyAsync(o_mu, d_cm, sizeof(double) * N, hipMemcpyDeviceToDevice, st));       // bin 1: no forecast bin before it
        for (int64_t k = 1; k < H; ++k) {
            k_dfc_conv<<<dd_grid((int64_t)N * B, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_phi, o_mu, N, B, L, k, d_z);
            k_dfc_mix<<<dd_grid(N, SIM_BLOCK / 64), SIM_BLOCK, 0, st>>>(d_W, d_A, d_th, d_z, d_cm, dt, N, B, k, o_mu);
        }
    }
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 1) {
        nhp_set_error(ctx, "disc_forecast: W, W·A, θ and φ must be finite and >= 0, with row sums Σ_c W·A·Σ_b θ·m_b <= 2^32");
        return NHP_EDOMAIN;
    }
    if (h->bad & 4) {
        nhp_set_error(ctx, "disc_forecast: history counts must be non-negative");
        return NHP_EDOMAIN;
    }
    if (h->bad & 2) {
        nhp_set_error(ctx, "disc_forecast: baseline means per bin must be finite and >= 0, and base + carry at most 2^20 expected "
                           "events per cell");
        return NHP_EDOMAIN;
    }

    // ---- carry-over + immigrants, cell chunk by cell chunk; readback 2: {entries, events, the child slots of generation 0}
    int64_t chunks = 0;
    for (int64_t e0 = 0; e0 < NT; e0 += CH) {
        const int64_t mc = std::min<int64_t>(CH, NT - e0);
        const unsigned gr = dd_grid(mc, SIM_BLOCK);
        k_dfc_cells<<<gr, SIM_BLOCK, 0, st>>>(d_cm, (uint64_t)HN, (uint64_t)(e0 % HN), e0, mc, seed ^ DFC_KEY_CELL, d_cn, d_keep);
        dd_scan<uint32_t>(st, d_keep, d_pos, mc, d_tmp32);
        k_dsim_store_cells<<<gr, SIM_BLOCK, 0, st>>>(a, e0, mc, d_cn, d_keep, d_pos, d_sc, cap, d_anode, d_abin, d_ak, d_cnt, nullptr, d_pa,
                                                     d_pb);
        k_dsim_advance<<<1, SIM_BLOCK, 0, st>>>(d_sc, d_pos + mc, d_pa, d_pb, gr, 0);
        if (++chunks % DFC_CELL_CHECK == 0 && e0 + CH < NT) {          // an overflowing ensemble stops here, not after all its cells
            NHP_HIP(ctx, hipGetLastError());
            NHP_TRY(sim_read(ctx, h, d_sc));
            if ((int64_t)h->events > cap || h->fill > cap) return sim_exploded(ctx);
        }
    }
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if ((int64_t)h->events > cap || h->fill > cap) return sim_exploded(ctx);

    // ---- generations: parents [g0, g1) of generation gen with C child slots in all
    int64_t g0 = 0, g1 = h->fill, C = (int64_t)h->next;
    uint64_t gen = 0;
    int32_t filled = g1 > 0;                          // generations that hold an entry
    while (C > 0) {
        const int64_t np = g1 - g0;
        dd_scan<int64_t>(st, d_cnt, d_off, np, d_tmp64);
        k_dsim_clear_next<<<1, 1, 0, st>>>(d_sc);
        for (int64_t s0 = 0; s0 < C; s0 += CH) {
            const int64_t mc = std::min<int64_t>(CH, C - s0);
            const unsigned gr = dd_grid(mc, SIM_BLOCK);
            k_dsim_children<true><<<gr, SIM_BLOCK, 0, st>>>(a, gen, s0, mc, d_off, np, g0, d_anode, d_abin, d_cn, d_cb, d_keep);
            dd_scan<uint32_t>(st, d_keep, d_pos, mc, d_tmp32);
            k_dsim_keep<<<gr, SIM_BLOCK, 0, st>>>(a, gen + 1, mc, d_keep, d_pos, d_cn, d_cb, d_sc, g1, cap, d_anode, d_abin, d_ak, d_cnt,
                                                  d_pa, d_pb);
            k_dsim_advance<<<1, SIM_BLOCK, 0, st>>>(d_sc, d_pos + mc, d_pa, d_pb, gr, 1);
            NHP_HIP(ctx, hipGetLastError());
            if (s0 + CH < C) {                        // a generation of several chunks: stop as soon as it overflows
                NHP_TRY(sim_read(ctx, h, d_sc));
                if ((int64_t)h->events > cap) return sim_exploded(ctx);
            }
        }
        NHP_TRY(sim_read(ctx, h, d_sc));
        if ((int64_t)h->events > cap) return sim_exploded(ctx);
        g0 = g1; g1 = h->fill; C = (int64_t)h->next;
        filled += g1 > g0;
        ++gen;
    }

    // ---- the histograms
    if (g1 > 0) k_dfc_hist<<<dd_grid(g1, SIM_BLOCK), SIM_BLOCK, 0, st>>>(g1, d_anode, d_abin, d_ak, N, (int32_t)H, o_tot, o_cell, o_paths);
    NHP_HIP(ctx, hipGetLastError());
    if (!output_on_device) {
        NHP_HIP(ctx, hipMemcpyAsync(totals, o_tot, sizeof(int64_t) * SN, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipMemcpyAsync(cell_sum, o_cell, sizeof(int64_t) * HN, hipMemcpyDeviceToHost, st));
        if (paths) NHP_HIP(ctx, hipMemcpyAsync(paths, o_paths, sizeof(int64_t) * NT, hipMemcpyDeviceToHost, st));
        if (carry) NHP_HIP(ctx, hipMemcpyAsync(carry, o_carry, sizeof(double) * HN, hipMemcpyDeviceToHost, st));
        if (expected) NHP_HIP(ctx, hipMemcpyAsync(expected, o_mu, sizeof(double) * HN, hipMemcpyDeviceToHost, st));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *n_events = (int64_t)h->events;
    if (n_generations) *n_generations = filled;
    return NHP_OK;
}
