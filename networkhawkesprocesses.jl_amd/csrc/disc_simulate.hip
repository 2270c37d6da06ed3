// rand(process, steps) for discrete processes on the device: nhp_disc_simulate.
//
// The branching sampler of src/discrete.jl:20-38 -- every event in bin t of node p adds Poisson(h[p,c,l]) events to bin
// t + l of node c for every c and every lag l = 1..L, h[p,c,l] = W[p,c]·A[p,c]·dt·Σ_b θ[p,c,b]·φ[l,b] -- drawn in stages
// (Poisson superposition): an event has Poisson(R_p) children, R_p = Σ_c G[p,c], G[p,c] = W·A·Σ_b θ[p,c,b]·m_b,
// m_b = dt·Σ_l φ[l,b]; a child takes node c with probability G[p,c]/R_p, basis b with probability θ[p,c,b]·m_b / Σ_b' θ m,
// lag l with probability φ[l,b] / Σ_l' φ[l',b].  Children past the last bin are dropped with their descendants.
//
// Entries live in a generation-ordered arena (0-based node, 0-based bin, multiplicity).  Generation 0: one lane per cell
// (c, t) draws its Poisson(base[t,c]) immigrants; the occupied cells are compacted (scan of the flags) into the arena, one
// entry of multiplicity k per cell, which draws Poisson(k·R_c) children at once.  Then, as in cont_simulate.hip, generation by
// generation: the parents' child counts are scanned into child slots; the slots go through chunks of at most SIM_CHUNK_MAX;
// a slot finds its parent by binary search over the slots, its node by binary search over the parent's row of the prefix
// table, its basis from θ[p,c,·] on the fly and its lag by binary search over the basis' column of the lag CDF; survivors
// (bin + lag within the T bins) are compacted behind the fill counter, never at or past max_events, with multiplicity 1, and
// draw their own child counts there.  One readback per generation.  The result is a histogram: an integer atomicAdd of every
// entry's multiplicity into counts[c + N·t] -- integer sums, so the matrix does not depend on order or launch geometry.
//
// Random numbers: Philox4x32-10 of nhp_rng.h, key seed ^ family, counter (element, attempt, step); include/nhp.h has the
// scheme in full, tests/disc_simulate_ref.py restates it in numpy.
#include "nhp_dsim.h"

// Philox key families (XORed into the seed)
#define DSIM_KEY_IMM 0xA3B195354A39B70Dull            // immigrants of a cell:        step 0, element c + N·t
#define DSIM_KEY_CHILD_COUNT 0x1B03738712FAD5C9ull    // children of an arena entry:  step = its generation, element = arena index
#define DSIM_KEY_CHILD 0xC2B2AE3D27D4EB4Full          // node, basis, lag of a child: step = its parent's generation, element = slot

// immigrants of the cells e = e0 + j (e = c + N·t): Poisson(λ0_c·dt) or Poisson(base[t, c])
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_cells(const double *__restrict__ lambda0, const double *__restrict__ base, double dt,
                                                          int32_t N, int64_t T, int64_t e0, int64_t m, uint64_t seed,
                                                          int32_t *__restrict__ kbuf, uint32_t *__restrict__ flag,
                                                          dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t e = e0 + j, t = e / N;
    const int32_t c = (int32_t)(e - t * N);
    const double mean = lambda0 ? lambda0[c] * dt : base[(size_t)c * T + t];
    const bool ok = mean >= 0.0 && mean <= DSIM_CELL_MAX;
    if (!ok) atomicOr(&sc->bad, 2);
    const int32_t k = ok ? (int32_t)sim_poisson(mean, seed ^ DSIM_KEY_IMM, 0, (uint64_t)e) : 0;
    kbuf[j] = k;
    flag[j] = k > 0;
}

// the histogram: every entry's multiplicity into its cell
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_hist(int64_t n, const int32_t *__restrict__ anode, const int32_t *__restrict__ abin,
                                                         const int32_t *__restrict__ ak, int32_t N, int64_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (i < n) atomicAdd((unsigned long long *)(counts + ((size_t)abin[i] * N + anode[i])), (unsigned long long)ak[i]);
}


extern "C" nhp_status nhp_disc_simulate(nhp_ctx *ctx, const double *lambda0, const double *base, const double *W, const double *theta,
                                        const double *A, const double *phi, int32_t n_lags, int32_t n_basis, double dt, int32_t n_nodes,
                                        int64_t n_bins, uint64_t seed, int64_t max_events, int32_t output_on_device, int64_t *counts,
                                        int64_t *background, int64_t *n_events, int32_t *n_generations)
{
    if (!ctx) return NHP_EINVAL;
    if (!W || !theta || !phi || !counts || !n_events) { nhp_set_error(ctx, "disc_simulate: null argument"); return NHP_EINVAL; }
    if ((lambda0 != nullptr) == (base != nullptr)) {
        nhp_set_error(ctx, "disc_simulate: exactly one of lambda0 [N] and base [T*N] must be given");
        return NHP_EINVAL;
    }
    if (n_nodes < 1 || n_bins < 1 || n_lags < 1 || n_basis < 1) {
        nhp_set_error(ctx, "disc_simulate: n_nodes, n_bins, n_lags and n_basis must be positive");
        return NHP_EINVAL;
    }
    if (max_events < 0 || max_events >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "disc_simulate: max_events = %lld outside [0, 2^31)", (long long)max_events);
        return NHP_EINVAL;
    }
    if (n_bins >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "disc_simulate: n_bins = %lld is not below 2^31 (bins are 32-bit in the arena)", (long long)n_bins);
        return NHP_ENOTIMPL;
    }
    if ((int64_t)n_nodes * n_bins >= ((int64_t)1 << 56)) {
        nhp_set_error(ctx, "disc_simulate: n_nodes * n_bins is not below 2^56 (int64 indexing of the count matrix in bytes)");
        return NHP_ENOTIMPL;
    }
    if (!(dt >= 0.0 && dt < INFINITY)) {
        nhp_set_error(ctx, "disc_simulate: dt must be non-negative and finite, got %g", dt);
        return NHP_EDOMAIN;
    }
    *n_events = 0;
    if (n_generations) *n_generations = 0;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const int32_t N = n_nodes, B = n_basis, L = n_lags;
    const int64_t T = n_bins, NT = (int64_t)N * T, NN = (int64_t)N * N;
    const int64_t cap = max_events;
    const int64_t CH = std::min(std::max(cap, SIM_CHUNK_MIN), SIM_CHUNK_MAX);
    sim_pinned<dsim_scal> pin;
    NHP_HIP(ctx, hipHostMalloc((void **)&pin.h, sizeof(dsim_scal), hipHostMallocDefault));
    dsim_scal *h = pin.h;

    // ---- scratch: the parameters and tables, the arena (max_events entries), one chunk of cells / child slots, the outputs
    dd_arena a1;
    a1.st = st;
    double *d_W = nullptr, *d_th = nullptr, *d_A = nullptr, *d_phi = nullptr, *d_l0 = nullptr, *d_base = nullptr;
    double *d_V = nullptr, *d_G = nullptr, *d_R = nullptr, *d_mb = nullptr, *d_cdf = nullptr;
    int64_t *d_cnt = nullptr, *d_off = nullptr, *d_tmp64 = nullptr, *o_counts = counts, *o_bg = background;
    int32_t *d_anode = nullptr, *d_abin = nullptr, *d_ak = nullptr, *d_cn = nullptr, *d_cb = nullptr;
    uint32_t *d_keep = nullptr, *d_pos = nullptr, *d_tmp32 = nullptr;
    unsigned long long *d_pa = nullptr, *d_pb = nullptr;
    dsim_scal *d_sc = nullptr;
    a1.ask(&d_W, NN); a1.ask(&d_th, NN * B); a1.ask(&d_phi, (int64_t)L * B);
    if (A) a1.ask(&d_A, NN);
    if (lambda0) a1.ask(&d_l0, N); else a1.ask(&d_base, NT);
    a1.ask(&d_V, NN); a1.ask(&d_G, NN); a1.ask(&d_R, N); a1.ask(&d_mb, B); a1.ask(&d_cdf, (int64_t)L * B);
    a1.ask(&d_tmp64, dd_grid(cap, DD_TILE));
    a1.ask(&d_anode, cap); a1.ask(&d_abin, cap); a1.ask(&d_ak, cap); a1.ask(&d_cnt, cap); a1.ask(&d_off, cap + 1);
    a1.ask(&d_cn, CH); a1.ask(&d_cb, CH); a1.ask(&d_keep, CH); a1.ask(&d_pos, CH + 1);
    a1.ask(&d_tmp32, dd_grid(CH, DD_TILE)); a1.ask(&d_pa, dd_grid(CH, SIM_BLOCK)); a1.ask(&d_pb, dd_grid(CH, SIM_BLOCK));
    a1.ask(&d_sc, 1);
    if (!output_on_device) {
        a1.ask(&o_counts, NT);
        if (background) a1.ask(&o_bg, NT);
    }
    if (a1.alloc() != hipSuccess) {
        (void)hipGetLastError();
        nhp_set_error(ctx, "disc_simulate: out of device memory (N = %d, T = %lld, max_events = %lld)", N, (long long)T, (long long)cap);
        return NHP_ENOMEM;
    }
    NHP_HIP(ctx, hipMemcpyAsync(d_W, W, sizeof(double) * NN, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_th, theta, sizeof(double) * NN * B, hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(d_phi, phi, sizeof(double) * L * B, hipMemcpyHostToDevice, st));
    if (A) NHP_HIP(ctx, hipMemcpyAsync(d_A, A, sizeof(double) * NN, hipMemcpyHostToDevice, st));
    if (lambda0) NHP_HIP(ctx, hipMemcpyAsync(d_l0, lambda0, sizeof(double) * N, hipMemcpyHostToDevice, st));
    else NHP_HIP(ctx, hipMemcpyAsync(d_base, base, sizeof(double) * NT, hipMemcpyHostToDevice, st));

    dsim_args a;
    a.G = d_G; a.R = d_R; a.theta = d_th; a.mb = d_mb; a.cdf = d_cdf; a.T = T; a.N = N; a.B = B; a.L = L;
    a.key_count = seed ^ DSIM_KEY_CHILD_COUNT; a.key_child = seed ^ DSIM_KEY_CHILD;

    // ---- setup; readback 1: the parameter checks
    NHP_HIP(ctx, hipMemsetAsync(d_sc, 0, sizeof(dsim_scal), st));
    NHP_HIP(ctx, hipMemsetAsync(o_counts, 0, sizeof(int64_t) * NT, st));
    k_dsim_lags<<<dd_grid(B, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_phi, L, B, dt, d_cdf, d_mb, d_sc);
    k_dsim_mass<<<dd_grid(NN, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_W, d_A, d_th, d_mb, NN, B, d_V, d_sc);
    k_dsim_rows<<<dd_grid(N, SIM_ROWS), SIM_ROWS, 0, st>>>(d_V, N, d_G, d_R, d_sc);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 1) {
        nhp_set_error(ctx, "disc_simulate: W, W·A, θ and φ must be finite and >= 0, with row sums Σ_c W·A·Σ_b θ·m_b <= 2^32");
        return NHP_EDOMAIN;
    }

    // ---- immigrants, cell chunk by cell chunk; readback 2: {entries, events, the child slots of generation 0, baseline check}
    for (int64_t e0 = 0; e0 < NT; e0 += CH) {
        const int64_t mc = std::min<int64_t>(CH, NT - e0);
        const unsigned gr = dd_grid(mc, SIM_BLOCK);
        k_dsim_cells<<<gr, SIM_BLOCK, 0, st>>>(d_l0, d_base, dt, N, T, e0, mc, seed, d_cn, d_keep, d_sc);
        dd_scan<uint32_t>(st, d_keep, d_pos, mc, d_tmp32);
        k_dsim_store_cells<<<gr, SIM_BLOCK, 0, st>>>(a, e0, mc, d_cn, d_keep, d_pos, d_sc, cap, d_anode, d_abin, d_ak, d_cnt, o_bg, d_pa, d_pb);
        k_dsim_advance<<<1, SIM_BLOCK, 0, st>>>(d_sc, d_pos + mc, d_pa, d_pb, gr, 0);
    }
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 2) {
        nhp_set_error(ctx, "disc_simulate: baseline means per bin must be finite and >= 0 (at most 2^20 expected events per cell)");
        return NHP_EDOMAIN;
    }
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
            k_dsim_children<false><<<gr, SIM_BLOCK, 0, st>>>(a, gen, s0, mc, d_off, np, g0, d_anode, d_abin, d_cn, d_cb, d_keep);
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

    // ---- the histogram
    if (g1 > 0) k_dsim_hist<<<dd_grid(g1, SIM_BLOCK), SIM_BLOCK, 0, st>>>(g1, d_anode, d_abin, d_ak, N, o_counts);
    NHP_HIP(ctx, hipGetLastError());
    if (!output_on_device) {
        NHP_HIP(ctx, hipMemcpyAsync(counts, o_counts, sizeof(int64_t) * NT, hipMemcpyDeviceToHost, st));
        if (background) NHP_HIP(ctx, hipMemcpyAsync(background, o_bg, sizeof(int64_t) * NT, hipMemcpyDeviceToHost, st));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *n_events = (int64_t)h->events;
    if (n_generations) *n_generations = filled;
    return NHP_OK;
}
