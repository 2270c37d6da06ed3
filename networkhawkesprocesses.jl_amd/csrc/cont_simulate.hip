// rand(process, duration) on the device: nhp_cont_simulate.
//
// Generation-wise branching in continuous time, the generative model of src/continuous.jl:16-48,131-142,335-348: Poisson
// immigrants per node (homogeneous: Poisson(λ0_c T) uniform positions; LGCP, src/baselines.jl:190-210: Poisson(trapezoid
// ∫λ_c) positions by rejection from the piecewise-linear λ_c), then generation by generation Poisson(R_p) children per
// event, R_p = Σ_c W[p,c]A[p,c] (the N Poisson(W[p,c]A[p,c]) draws of the reference merged by Poisson splitting), each
// child's node drawn from W[p,:]∘A[p,:] / R_p and its delay from the impulse response.  Children after T are dropped;
// their descendants would be later still, so the whole subtree goes with them (`truncate`, src/continuous.jl:39-48).
//
// Events live in a generation-ordered arena (time, 0-based node, arena index of the parent).  Per generation: the
// parents' child counts (drawn when the parents were stored) are scanned into child slots; the slots are processed in
// chunks of at most SIM_CHUNK_MAX (scratch stays O(max_events) however fast a process explodes); each slot finds its
// parent by binary search over the slots, its node by binary search over the parent's row of the prefix table, draws
// its delay, and survives if t <= T; survivors are compacted (scan of the keep flags) behind the arena's fill counter,
// never past max_events, and draw their own child counts there.  One readback per generation: {fill, next slot count}.
// At the end a stable LSD radix sort on the times' bit patterns (non-negative doubles order as unsigned integers),
// payload = arena index, gives the output order; ties keep arena order, so a parent precedes its children.
//
// Random numbers: Philox4x32-10 of nhp_rng.h, key seed ^ family, counter (element, attempt, step); include/nhp.h has
// the scheme in full, tests/test_simulate_gpu.py restates it in numpy.
#include <string.h>

#include "nhp_sim.h"

// Philox key families (XORed into the seed)
#define SIM_KEY_IMM_COUNT 0x9E3779B97F4A7C15ull       // immigrants per node:        step 0, element c
#define SIM_KEY_IMM_POS 0xBF58476D1CE4E5B9ull         // immigrant positions:        step 0, element k (node-major order)
#define SIM_KEY_CHILD_COUNT 0x94D049BB133111EBull     // children of an event:       step = its generation, element = arena index
#define SIM_KEY_CHILD 0xD6E8FEB86659FD93ull           // node and delay of a child:  step = its parent's generation, element = slot

struct sim_args {
    const double *G, *R;             // row-major inclusive prefix of W∘A [N*N], row totals R_p = G[p, N-1] [N]
    const double *p1, *p2;           // θ | μ, τ (column-major, the model's own)
    double T, dt_max;
    int32_t N, impulse_kind;
    uint64_t seed;
};

// the piecewise-linear intensity through (x, y) at x0 in [x[0], x[G-1]]  (src/utils/interpolation.jl:40-50)
static __device__ double sim_interp(const double *x, const double *y, int32_t G, double x0)
{
#pragma clang fp contract(off)
    if (x0 >= x[G - 1]) return y[G - 1];
    int32_t lo = 0, hi = G - 1;                       // last i < G-1 with x[i] <= x0
    while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if (x[mid] <= x0) lo = mid; else hi = mid; }
    return (y[lo + 1] * (x0 - x[lo]) + y[lo] * (x[lo + 1] - x0)) / (x[lo + 1] - x[lo]);
}


// immigrant counts per node: Poisson(λ0_c T) or Poisson(trapezoid ∫λ_c) (src/utils/interpolation.jl:53-63, same order
// of operations), and the LGCP's max λ_c for the rejection step
__global__ void k_sim_baseline(const double *__restrict__ lambda0, const double *__restrict__ gx, int32_t grid_n, int32_t N, double T,
                               uint64_t seed, int64_t *__restrict__ cnt0, double *__restrict__ ymax, sim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (c >= N) return;
    double mean, top = 0.0;
    bool ok = true;
    if (grid_n == 0) {
        ok = lambda0[c] >= 0.0;
        mean = lambda0[c] * T;
    } else {
        const double *y = lambda0 + (size_t)c * grid_n;
        double I = 0.0;
        for (int32_t i = 0; i < grid_n; ++i) {
            ok = ok && y[i] >= 0.0 && y[i] < INFINITY;
            top = fmax(top, y[i]);
            if (i + 1 < grid_n) I += 0.5 * (y[i] + y[i + 1]) * (gx[i + 1] - gx[i]);
        }
        mean = I;
    }
    ok = ok && mean <= 1099511627776.0;               // 2^40 immigrants per node at most (and not NaN)
    if (!ok) atomicOr(&sc->bad, 2);
    cnt0[c] = ok ? (int64_t)sim_poisson(mean, seed ^ SIM_KEY_IMM_COUNT, 0, (uint64_t)c) : 0;
    ymax[c] = top;
}

__global__ void k_sim_start(sim_scal *__restrict__ sc, const int64_t *__restrict__ n0)
{
    sc->fill = *n0;
    sc->next = 0;
}

// immigrant k of node c (k in [off0[c], off0[c+1])): position, arena entry, its child count
__global__ void __launch_bounds__(SIM_BLOCK) k_sim_immigrants(sim_args a, const double *__restrict__ lambda0, const double *__restrict__ gx,
                                                              int32_t grid_n, const int64_t *__restrict__ off0, int64_t n0,
                                                              const double *__restrict__ ymax, double *__restrict__ at,
                                                              int32_t *__restrict__ anode, int32_t *__restrict__ apar,
                                                              int64_t *__restrict__ cnt, sim_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (k < n0) {
        int32_t lo = 0, hi = a.N;                     // last c with off0[c] <= k
        while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if (off0[mid] <= k) lo = mid; else hi = mid; }
        const int32_t c = lo;
        const uint64_t key = a.seed ^ SIM_KEY_IMM_POS;
        double ua, ub, t;
        philox_2u(key, 0, (uint64_t)k, 0, &ua, &ub);
        t = sim_u01(ua) * a.T;
        if (grid_n) {                                 // accept (x, y) under λ_c, y uniform on (0, max λ_c]
            const double *y = lambda0 + (size_t)c * grid_n;
            for (uint32_t att = 1; !(ub * ymax[c] <= sim_interp(gx, y, grid_n, t)) && att < (1u << 24); ++att) {
                philox_2u(key, 0, (uint64_t)k, att, &ua, &ub);
                t = sim_u01(ua) * a.T;
            }
        }
        at[k] = t; anode[k] = c; apar[k] = -1;
        const double n = sim_poisson(a.R[c], a.seed ^ SIM_KEY_CHILD_COUNT, 0, (uint64_t)k);
        cnt[k] = (int64_t)n;
        kids = (unsigned long long)n;
    }
    sim_wave_add(kids, &sc->next);
}

// child slot s = s0 + j of the current generation: parent, node, delay, time, keep flag
__global__ void __launch_bounds__(SIM_BLOCK) k_sim_children(sim_args a, uint64_t gen, int64_t s0, int64_t m, const int64_t *__restrict__ off,
                                                            int64_t n_par, int64_t g0, const double *__restrict__ at,
                                                            const int32_t *__restrict__ anode, double *__restrict__ ct,
                                                            int32_t *__restrict__ cn, int32_t *__restrict__ cp, uint32_t *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t s = s0 + j;
    int64_t lo = 0, hi = n_par;                       // last parent i with off[i] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= s) lo = mid; else hi = mid; }
    const int64_t par = g0 + lo;
    const int32_t p = anode[par], N = a.N;
    const uint64_t key = a.seed ^ SIM_KEY_CHILD;
    double ua, ub;
    philox_2u(key, gen, (uint64_t)s, 0, &ua, &ub);
    const double *row = a.G + (size_t)p * N;
    const double x = sim_u01(ua) * a.R[p];
    int32_t l = 0, h = N;                             // first c with row[c] > x
    while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] > x) h = mid; else l = mid + 1; }
    if (l == N) {                                     // x rounded up to R_p: the first entry reaching it (a positive weight)
        l = 0; h = N - 1;
        while (l < h) { const int32_t mid = (l + h) >> 1; if (row[mid] >= x) h = mid; else l = mid + 1; }
    }
    const size_t q = (size_t)p + (size_t)l * N;
    double dt;
    if (a.impulse_kind == NHP_IMPULSE_EXPONENTIAL) {
        dt = -nhp_log(ub) / a.p1[q];                  // Exp(θ), not cut at Δtmax (src/impulses.jl:53-66)
    } else {
        double z, unused;
        philox_attempt(key, gen, (uint64_t)s, 1, &z, &unused);
        dt = a.dt_max / (1.0 + nhp_exp(-(a.p1[q] + z / sqrt(a.p2[q]))));      // Δtmax·logistic(μ + Z/√τ)  (:180-202)
    }
    const double t = at[par] + dt;
    ct[j] = t; cn[j] = l; cp[j] = (int32_t)par;
    keep[j] = t <= a.T;
}

// survivors of a chunk behind the fill counter (never at or past cap), with their own child counts
__global__ void __launch_bounds__(SIM_BLOCK) k_sim_keep(sim_args a, uint64_t gen_next, int64_t m, const uint32_t *__restrict__ keep,
                                                        const uint32_t *__restrict__ pos, const double *__restrict__ ct,
                                                        const int32_t *__restrict__ cn, const int32_t *__restrict__ cp,
                                                        sim_scal *__restrict__ sc, int64_t g1, int64_t cap, double *__restrict__ at,
                                                        int32_t *__restrict__ anode, int32_t *__restrict__ apar, int64_t *__restrict__ cnt)
{
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (j < m && keep[j]) {
        const int64_t dst = (int64_t)sc->fill + pos[j];
        if (dst < cap) {
            const int32_t c = cn[j];
            at[dst] = ct[j]; anode[dst] = c; apar[dst] = cp[j];
            const double n = sim_poisson(a.R[c], a.seed ^ SIM_KEY_CHILD_COUNT, gen_next, (uint64_t)dst);
            cnt[dst - g1] = (int64_t)n;
            kids = (unsigned long long)n;
        }
    }
    sim_wave_add(kids, &sc->next);
}

__global__ void k_sim_advance(sim_scal *__restrict__ sc, const uint32_t *__restrict__ kept) { sc->fill += *kept; }
__global__ void k_sim_clear_next(sim_scal *__restrict__ sc) { sc->next = 0; }

__global__ void k_sim_inverse(const int32_t *__restrict__ perm, int64_t n, int32_t *__restrict__ inv)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k < n) inv[perm[k]] = (int32_t)k;
}

// sorted order: times, 1-based nodes, 1-based parent positions (0 = immigrant)
__global__ void k_sim_gather(const int32_t *__restrict__ perm, const int32_t *__restrict__ inv, int64_t n, const double *__restrict__ at,
                             const int32_t *__restrict__ anode, const int32_t *__restrict__ apar, double *__restrict__ times,
                             int64_t *__restrict__ nodes, int64_t *__restrict__ parents)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int32_t i = perm[k];
    times[k] = at[i];
    nodes[k] = (int64_t)anode[i] + 1;
    if (parents) {
        const int32_t pa = apar[i];
        parents[k] = pa < 0 ? 0 : (int64_t)inv[pa] + 1;
    }
}


extern "C" nhp_status nhp_cont_simulate(nhp_ctx *ctx, const nhp_cont_model *m, double duration, uint64_t seed, int64_t max_events,
                                        int32_t output_on_device, double *times, int64_t *nodes, int64_t *parents, int64_t *n_events)
{
    if (!ctx) return NHP_EINVAL;
    if (!m || !times || !nodes || !n_events) { nhp_set_error(ctx, "simulate: null argument"); return NHP_EINVAL; }
    if (!(duration >= 0.0 && duration < INFINITY)) {
        nhp_set_error(ctx, "simulate: duration must be non-negative and finite, got %g", duration);
        return NHP_EDOMAIN;
    }
    if (max_events < 0 || max_events >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "simulate: max_events = %lld outside [0, 2^31)", (long long)max_events);
        return NHP_EINVAL;
    }
    if (m->baseline_kind == NHP_BASELINE_LGCP && duration != m->grid_end) {
        nhp_set_error(ctx, "Sample duration does not match process duration.");      // src/baselines.jl:191
        return NHP_EDOMAIN;
    }
    *n_events = 0;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const int32_t N = m->N;
    const int64_t cap = max_events;
    const int64_t CH = std::min(std::max(cap, SIM_CHUNK_MIN), SIM_CHUNK_MAX);
    sim_pinned<sim_scal> pin;
    NHP_HIP(ctx, hipHostMalloc((void **)&pin.h, sizeof(sim_scal), hipHostMallocDefault));
    sim_scal *h = pin.h;

    // ---- scratch: the prefix table, the arena (max_events entries), one chunk of child slots
    dd_arena a1;
    a1.st = st;
    double *d_G = nullptr, *d_R = nullptr, *d_ymax = nullptr, *d_at = nullptr, *d_ct = nullptr;
    int64_t *d_cnt0 = nullptr, *d_off0 = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_tmp64 = nullptr;
    int32_t *d_anode = nullptr, *d_apar = nullptr, *d_cn = nullptr, *d_cp = nullptr;
    uint32_t *d_keep = nullptr, *d_pos = nullptr, *d_tmp32 = nullptr;
    sim_scal *d_sc = nullptr;
    a1.ask(&d_G, (int64_t)N * N); a1.ask(&d_R, N); a1.ask(&d_ymax, N); a1.ask(&d_cnt0, N); a1.ask(&d_off0, (int64_t)N + 1);
    a1.ask(&d_tmp64, dd_grid(std::max<int64_t>(cap, N), DD_TILE));
    a1.ask(&d_at, cap); a1.ask(&d_anode, cap); a1.ask(&d_apar, cap); a1.ask(&d_cnt, cap); a1.ask(&d_off, cap + 1);
    a1.ask(&d_ct, CH); a1.ask(&d_cn, CH); a1.ask(&d_cp, CH); a1.ask(&d_keep, CH); a1.ask(&d_pos, CH + 1);
    a1.ask(&d_tmp32, dd_grid(CH, DD_TILE)); a1.ask(&d_sc, 1);
    NHP_HIP(ctx, a1.alloc());

    sim_args a;
    a.G = d_G; a.R = d_R; a.p1 = m->d_p1; a.p2 = m->d_p2; a.T = duration; a.dt_max = m->dt_max;
    a.N = N; a.impulse_kind = m->impulse_kind; a.seed = seed;

    // ---- setup and immigrant counts; readback 1: {immigrants, parameter checks}
    NHP_HIP(ctx, hipMemsetAsync(d_sc, 0, sizeof(sim_scal), st));
    k_sim_rows<<<dd_grid(N, SIM_ROWS), SIM_ROWS, 0, st>>>(m->d_W, m->has_A ? m->d_A : nullptr, m->d_p1, m->d_p2, N, m->impulse_kind,
                                                          d_G, d_R, d_sc);
    k_sim_baseline<<<dd_grid(N, SIM_BLOCK), SIM_BLOCK, 0, st>>>(m->d_lambda0, m->d_grid, m->grid_n, N, duration, seed, d_cnt0, d_ymax, d_sc);
    dd_scan<int64_t>(st, d_cnt0, d_off0, N, d_tmp64);
    k_sim_start<<<1, 1, 0, st>>>(d_sc, d_off0 + N);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 1) {
        nhp_set_error(ctx, "simulate: every W[p,c]·A[p,c] must be finite and >= 0 with row sums <= 2^32, and every link with weight "
                           "needs a finite positive θ (finite μ, positive τ)");
        return NHP_EDOMAIN;
    }
    if (h->bad & 2) {
        nhp_set_error(ctx, "simulate: baseline intensities must be finite and >= 0 (at most 2^40 expected events per node)");
        return NHP_EDOMAIN;
    }
    const int64_t n0 = h->fill;
    if (n0 > cap) return sim_exploded(ctx);

    // ---- immigrants; readback 2: the child slots of generation 0
    if (n0 > 0)
        k_sim_immigrants<<<dd_grid(n0, SIM_BLOCK), SIM_BLOCK, 0, st>>>(a, m->d_lambda0, m->d_grid, m->grid_n, d_off0, n0, d_ymax, d_at,
                                                                       d_anode, d_apar, d_cnt, d_sc);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));

    // ---- generations: parents [g0, g1) of generation gen with C child slots in all
    int64_t g0 = 0, g1 = n0, C = (int64_t)h->next;
    uint64_t gen = 0;
    while (C > 0) {
        const int64_t np = g1 - g0;
        dd_scan<int64_t>(st, d_cnt, d_off, np, d_tmp64);
        k_sim_clear_next<<<1, 1, 0, st>>>(d_sc);
        for (int64_t s0 = 0; s0 < C; s0 += CH) {
            const int64_t mc = std::min<int64_t>(CH, C - s0);
            const unsigned gr = dd_grid(mc, SIM_BLOCK);
            k_sim_children<<<gr, SIM_BLOCK, 0, st>>>(a, gen, s0, mc, d_off, np, g0, d_at, d_anode, d_ct, d_cn, d_cp, d_keep);
            dd_scan<uint32_t>(st, d_keep, d_pos, mc, d_tmp32);
            k_sim_keep<<<gr, SIM_BLOCK, 0, st>>>(a, gen + 1, mc, d_keep, d_pos, d_ct, d_cn, d_cp, d_sc, g1, cap, d_at, d_anode, d_apar,
                                                 d_cnt);
            k_sim_advance<<<1, 1, 0, st>>>(d_sc, d_pos + mc);
            NHP_HIP(ctx, hipGetLastError());
            if (s0 + CH < C) {                        // a generation of several chunks: stop as soon as it overflows
                NHP_TRY(sim_read(ctx, h, d_sc));
                if (h->fill > cap) return sim_exploded(ctx);
            }
        }
        NHP_TRY(sim_read(ctx, h, d_sc));
        if (h->fill > cap) return sim_exploded(ctx);
        g0 = g1; g1 = h->fill; C = (int64_t)h->next;
        ++gen;
    }
    const int64_t n = g1;

    // ---- sort by time (stable: ties keep arena order), gather the outputs
    if (n > 0) {
        dd_arena a2;
        a2.st = st;
        uint64_t *d_key = nullptr, *k_sorted = nullptr;
        int32_t *d_inv = nullptr, *perm = nullptr;
        double *o_t = times;
        int64_t *o_n = nodes, *o_p = parents;
        dd_sort_buf<uint64_t> sb;
        const int64_t ntn = dd_grid(n, DD_TILE);
        a2.ask(&d_key, n); a2.ask(&sb.k2, n); a2.ask(&sb.v1, n); a2.ask(&sb.v2, n);
        a2.ask(&sb.hist, (int64_t)DD_RADIX * ntn); a2.ask(&sb.offs, (int64_t)DD_RADIX * ntn + 1);
        a2.ask(&sb.tmp, dd_grid((int64_t)DD_RADIX * ntn, DD_TILE)); a2.ask(&d_inv, n);
        if (!output_on_device) {
            a2.ask(&o_t, n); a2.ask(&o_n, n);
            if (parents) a2.ask(&o_p, n);
        }
        NHP_HIP(ctx, a2.alloc());
        NHP_HIP(ctx, hipMemcpyAsync(d_key, d_at, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
        uint64_t tbits;
        memcpy(&tbits, &duration, sizeof tbits);       // every key is <= the bits of T
        dd_sort<uint64_t>(st, d_key, n, dd_bitlen(tbits), sb, &k_sorted, &perm);
        const unsigned gn = dd_grid(n, SIM_BLOCK);
        if (parents) k_sim_inverse<<<gn, SIM_BLOCK, 0, st>>>(perm, n, d_inv);
        k_sim_gather<<<gn, SIM_BLOCK, 0, st>>>(perm, d_inv, n, d_at, d_anode, d_apar, o_t, o_n, parents ? o_p : nullptr);
        NHP_HIP(ctx, hipGetLastError());
        if (!output_on_device) {
            NHP_HIP(ctx, hipMemcpyAsync(times, o_t, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            NHP_HIP(ctx, hipMemcpyAsync(nodes, o_n, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
            if (parents) NHP_HIP(ctx, hipMemcpyAsync(parents, o_p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
        }
        NHP_HIP(ctx, hipStreamSynchronize(st));
    }
    *n_events = n;
    return NHP_OK;
}
