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
#include "nhp_sim.h"

// Philox key families (XORed into the seed)
#define DSIM_KEY_IMM 0xA3B195354A39B70Dull            // immigrants of a cell:        step 0, element c + N·t
#define DSIM_KEY_CHILD_COUNT 0x1B03738712FAD5C9ull    // children of an arena entry:  step = its generation, element = arena index
#define DSIM_KEY_CHILD 0xC2B2AE3D27D4EB4Full          // node, basis, lag of a child: step = its parent's generation, element = slot

#define DSIM_CELL_MAX 1048576.0                       // 2^20 expected immigrants per cell at most

struct dsim_scal {
    long long fill;                  // arena entries so far (may pass max_events: nothing at or past it is written)
    unsigned long long next;         // child slots of the generation being stored
    unsigned long long events;       // events so far: Σ multiplicities, the entries that found no room included
    int bad;                         // 1: weights / basis parameters, 2: baseline
    int pad;
};

struct dsim_args {
    const double *G, *R;             // row-major inclusive prefix of G [N*N], row totals R_p [N]
    const double *theta, *mb, *cdf;  // θ [N*N*B] column-major; m_b [B]; inclusive prefix of φ[·,b] over the lags [L*B], lag fastest
    int64_t T;
    int32_t N, B, L;
    uint64_t seed;
};

// the lag CDF: one lane per basis b, a sequential running sum over the lags; m_b = dt·Σ_l φ[l,b]
__global__ void k_dsim_lags(const double *__restrict__ phi, int32_t L, int32_t B, double dt, double *__restrict__ cdf,
                            double *__restrict__ mb, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int32_t b = blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (b >= B) return;
    double run = 0.0;
    int bad = 0;
    for (int32_t l = 0; l < L; ++l) {
        const double v = phi[(size_t)b * L + l];
        bad |= !(v >= 0.0 && v < INFINITY);
        run = run + v;
        cdf[(size_t)b * L + l] = run;
    }
    mb[b] = run * dt;
    bad |= !(run < INFINITY);
    if (bad) atomicOr(&sc->bad, 1);
}

// the link masses V[p,c] = (W[p,c]·A[p,c])·Σ_b θ[p,c,b]·m_b (column-major, as W), one lane per link, with the parameter checks
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_mass(const double *__restrict__ W, const double *__restrict__ A,
                                                         const double *__restrict__ theta, const double *__restrict__ mb, int64_t NN,
                                                         int32_t B, double *__restrict__ V, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t q = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (q >= NN) return;
    const double w = A ? W[q] * A[q] : W[q];
    double s = 0.0;
    int bad = 0;
    for (int32_t b = 0; b < B; ++b) {
        const double th = theta[q + NN * b];
        bad |= !(th >= 0.0 && th < INFINITY);
        s = s + th * mb[b];
    }
    const double v = w * s;
    bad |= !(W[q] >= 0.0 && w >= 0.0 && v >= 0.0 && v < INFINITY);
    V[q] = v;
    if (bad) atomicOr(&sc->bad, 1);
}

// k_sim_rows of nhp_sim.h over the link masses: one lane per row p, a sequential running sum over c (so the table is
// monotone and a zero-mass entry equals the one before it exactly: it can never be chosen); column c of 64 rows is one
// coalesced read, the running sums leave row by row through an LDS tile
__global__ void __launch_bounds__(SIM_ROWS) k_dsim_rows(const double *__restrict__ V, int32_t N, double *__restrict__ G,
                                                        double *__restrict__ R, dsim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    __shared__ double tile[SIM_ROWS][SIM_ROWS + 1];
    const int32_t p0 = blockIdx.x * SIM_ROWS, tx = threadIdx.x, p = p0 + tx;
    double run = 0.0;
    for (int32_t c0 = 0; c0 < N; c0 += SIM_ROWS) {
        const int32_t nc = min(SIM_ROWS, N - c0);
        if (p < N) {
#pragma unroll 16
            for (int32_t k = 0; k < SIM_ROWS; ++k) {
                if (k < nc) {
                    run = run + V[(size_t)p + (size_t)(c0 + k) * N];
                    tile[tx][k] = run;
                }
            }
        }
        __syncthreads();
        for (int32_t r = 0; r < SIM_ROWS && p0 + r < N; ++r)
            if (tx < nc) G[(size_t)(p0 + r) * N + c0 + tx] = tile[r][tx];
        __syncthreads();
    }
    if (p < N) {
        R[p] = run;
        if (!(run <= 4294967296.0)) atomicOr(&sc->bad, 1);      // 2^32 children per event: the slot sums stay far inside int64
    }
}

// The run scalars are summed without atomics: a block leaves the sums of its lanes' a and b in pa[block], pb[block], and the
// one-block advance kernel behind it adds them up -- with an atomic per wave, the 16384 waves of a chunk queued on the two
// counters for 0.3 ms.  Block sums of a and b, valid in thread 0 (every thread of the block calls it):
static __device__ __forceinline__ void dsim_block_sums(unsigned long long &a, unsigned long long &b)
{
    __shared__ unsigned long long red[2][SIM_BLOCK / 64];
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < SIM_BLOCK / 64; ++w) { a += red[0][w]; b += red[1][w]; }
    }
}

// one block: fill += kept entries, next += Σ pa (child slots), events += Σ pb (cells: the multiplicities; children: one each)
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_advance(dsim_scal *__restrict__ sc, const uint32_t *__restrict__ kept,
                                                            const unsigned long long *__restrict__ pa,
                                                            const unsigned long long *__restrict__ pb, uint32_t nb, int children)
{
    unsigned long long a = 0, b = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += SIM_BLOCK) { a += pa[i]; b += pb[i]; }
    dsim_block_sums(a, b);
    if (threadIdx.x == 0) {
        sc->fill += *kept;
        sc->next += a;
        sc->events += children ? (unsigned long long)*kept : b;
    }
}

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

// the occupied cells of a chunk behind the fill counter (never at or past cap), with their child counts; background
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_store_cells(dsim_args a, int64_t e0, int64_t m, const int32_t *__restrict__ kbuf,
                                                                const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                                dsim_scal *__restrict__ sc, int64_t cap, int32_t *__restrict__ anode,
                                                                int32_t *__restrict__ abin, int32_t *__restrict__ ak,
                                                                int64_t *__restrict__ cnt, int64_t *__restrict__ background,
                                                                unsigned long long *__restrict__ pa, unsigned long long *__restrict__ pb)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0, evs = 0;
    if (j < m) {
        const int64_t e = e0 + j;
        const int32_t k = kbuf[j];
        if (background) background[e] = k;
        if (flag[j]) {
            evs = (unsigned long long)k;
            const int64_t dst = (int64_t)sc->fill + pos[j];
            if (dst < cap) {
                const int64_t t = e / a.N;
                const int32_t c = (int32_t)(e - t * a.N);
                anode[dst] = c; abin[dst] = (int32_t)t; ak[dst] = k;
                const double n = sim_poisson((double)k * a.R[c], a.seed ^ DSIM_KEY_CHILD_COUNT, 0, (uint64_t)dst);
                cnt[dst] = (int64_t)n;
                kids = (unsigned long long)n;
            }
        }
    }
    dsim_block_sums(kids, evs);
    if (threadIdx.x == 0) { pa[blockIdx.x] = kids; pb[blockIdx.x] = evs; }
}

// child slot s = s0 + j of the current generation: parent, node, basis, lag, bin, keep flag
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_children(dsim_args a, uint64_t gen, int64_t s0, int64_t m, const int64_t *__restrict__ off,
                                                             int64_t n_par, int64_t g0, const int32_t *__restrict__ anode,
                                                             const int32_t *__restrict__ abin, int32_t *__restrict__ cn,
                                                             int32_t *__restrict__ cb, uint32_t *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t s = s0 + j;
    int64_t lo = 0, hi = n_par;                       // last parent i with off[i] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= s) lo = mid; else hi = mid; }
    const int64_t par = g0 + lo;
    const int32_t p = anode[par], N = a.N, B = a.B, L = a.L;
    const uint64_t key = a.seed ^ DSIM_KEY_CHILD;
    double ua, ub, uc, unused;
    philox_2u(key, gen, (uint64_t)s, 0, &ua, &ub);
    philox_2u(key, gen, (uint64_t)s, 1, &uc, &unused);
    const double *row = a.G + (size_t)p * N;
    double x = sim_u01(ua) * a.R[p];
    int32_t l = 0, h = N;                             // node: first c with row[c] > x
    while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] > x) h = mid; else l = mid + 1; }
    if (l == N) {                                     // x rounded up to R_p: the first entry reaching it (a positive mass)
        l = 0; h = N - 1;
        while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] >= x) h = mid; else l = mid + 1; }
    }
    const int32_t c = l;
    const double *th = a.theta + (size_t)p + (size_t)c * N;
    const size_t NN = (size_t)N * N;
    double tot = 0.0;
    for (int32_t b = 0; b < B; ++b) tot = tot + th[NN * b] * a.mb[b];
    x = sim_u01(ub) * tot;
    int32_t bs = -1, bg = -1;                         // basis: first b with prefix[b] > x (if none, the first prefix[b] >= x)
    double run = 0.0;
    for (int32_t b = 0; b < B; ++b) {
        run = run + th[NN * b] * a.mb[b];
        if (bs < 0 && run > x) bs = b;
        if (bg < 0 && run >= x) bg = b;
    }
    if (bs < 0) bs = bg < 0 ? B - 1 : bg;
    const double *col = a.cdf + (size_t)bs * L;
    x = sim_u01(uc) * col[L - 1];
    l = 0; h = L;                                     // lag: first l with col[l] > x
    while (l < h) { const int32_t mid = (l + h) >> 1; if (col[mid] > x) h = mid; else l = mid + 1; }
    if (l == L) {
        l = 0; h = L - 1;
        while (l < h) { const int32_t mid = (l + h) >> 1; if (col[mid] >= x) h = mid; else l = mid + 1; }
    }
    const int64_t bin = (int64_t)abin[par] + l + 1;   // lags are 1..L
    cn[j] = c; cb[j] = (int32_t)min(bin, a.T);
    keep[j] = bin < a.T;
}

// survivors of a chunk behind the fill counter (never at or past cap), with their own child counts
__global__ void __launch_bounds__(SIM_BLOCK) k_dsim_keep(dsim_args a, uint64_t gen_next, int64_t m, const uint32_t *__restrict__ keep,
                                                         const uint32_t *__restrict__ pos, const int32_t *__restrict__ cn,
                                                         const int32_t *__restrict__ cb, dsim_scal *__restrict__ sc, int64_t g1, int64_t cap,
                                                         int32_t *__restrict__ anode, int32_t *__restrict__ abin, int32_t *__restrict__ ak,
                                                         int64_t *__restrict__ cnt, unsigned long long *__restrict__ pa,
                                                         unsigned long long *__restrict__ pb)
{
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (j < m && keep[j]) {
        const int64_t dst = (int64_t)sc->fill + pos[j];
        if (dst < cap) {
            const int32_t c = cn[j];
            anode[dst] = c; abin[dst] = cb[j]; ak[dst] = 1;
            const double n = sim_poisson(a.R[c], a.seed ^ DSIM_KEY_CHILD_COUNT, gen_next, (uint64_t)dst);
            cnt[dst - g1] = (int64_t)n;
            kids = (unsigned long long)n;
        }
    }
    unsigned long long none = 0;
    dsim_block_sums(kids, none);
    if (threadIdx.x == 0) { pa[blockIdx.x] = kids; pb[blockIdx.x] = 0; }
}

__global__ void k_dsim_clear_next(dsim_scal *__restrict__ sc) { sc->next = 0; }

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
    hipStream_t st = ctx->stream;
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
    a.G = d_G; a.R = d_R; a.theta = d_th; a.mb = d_mb; a.cdf = d_cdf; a.T = T; a.N = N; a.B = B; a.L = L; a.seed = seed;

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
            k_dsim_children<<<gr, SIM_BLOCK, 0, st>>>(a, gen, s0, mc, d_off, np, g0, d_anode, d_abin, d_cn, d_cb, d_keep);
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
