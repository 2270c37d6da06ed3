// forecast(process, data, horizon): nhp_cont_forecast.
//
// S independent continuations on (T0, T0 + h] of the generative model nhp_cont_simulate samples (exponential delays not
// cut at Δtmax, W[p,c]·A[p,c] expected children per link for both impulse kinds), conditional on the observed events of the
// dataset (T0 = its duration).  One continuation is the union of three independent parts:
//   carry-over     the not-yet-realised direct children of the observed events,
//   new immigrants Poisson(λ0_c h) per node, uniform,
//   descendants    of both, by the generation loop of the simulator with the end time T0 + h.
// Exponential impulses are memoryless, so the observed events enter through the state G[p,c] = Σ_{j on p} e^{-θ[p,c](T0 - t_j)}
// alone (k_fc_state: one lane per (p, c), the node's events in time order, at most M·N exponentials once per call): the carry
// mass of a link is m[p,c] = W·A·G·(1 - e^{-θh}), node c gets Poisson(Σ_p m[p,c]) carry-over children, each picks its parent
// node from the column prefix of m and its delay from the exponential cut at h.  Logit-normal impulses have bounded support:
// the events with T0 - t_j < Δtmax are the parents of a generation before the first in every replica, draw Poisson(R_p)
// children exactly as any event does, and the children landing in (T0, T0 + h] stay (thinning: exact, no Φ⁻¹).
//
// All replicas share one arena (time, 0-based node, replica): [the logit-normal window events, once per replica | roots:
// immigrants and exponential carry-over children, replica by replica | generation by generation the surviving children in
// slot order].  The generation loop is the simulator's, every entry carrying its replica to its children.  At the end
// counts[r, c] is a histogram of the arena, and the paths are the arena sorted by time bits (minus the bits of T0: still a
// non-negative integer in time order, in fewer digits), then stably by replica.
//
// Random numbers: the Philox block of nhp_rng.h with the forecast's own key families; include/nhp.h has the scheme in full,
// tests/forecast_ref.py restates it in numpy.
#include <math.h>
#include <string.h>

#include <chrono>

#include "nhp_sim.h"

// Philox key families (XORed into the seed)
#define FC_KEY_IMM_COUNT 0xA0761D6478BD642Full        // immigrants of (replica r, node c):            step 0, element r·N + c
#define FC_KEY_CARRY_COUNT 0xE7037ED1A0B428DBull      // exponential carry-over children of (r, c):    step 0, element r·N + c
#define FC_KEY_ROOT 0x8EBC6AF09C88C6E3ull             // position / parent node and delay of root k:   step 0, element k
#define FC_KEY_CHILD_COUNT 0x589965CC75374CC3ull      // children of an arena entry:                   step = its generation, element = arena index
#define FC_KEY_CHILD 0x1D8E4E27C47D124Full            // node and delay of a child:                    step = its parent's generation, element = slot

struct fc_scal : sim_scal {         // fill counts arena entries; bad has one more bit, 4: a carry mass that is not finite
    long long w0;                    // logit-normal: the first event with T0 - t_j < Δtmax
};

struct fc_args {
    const double *G, *R;             // row-major inclusive prefix of W∘A [N*N], row totals [N]
    const double *p1, *p2;           // θ | μ, τ (column-major, the model's own)
    const double *CP, *carry;        // exponential: inclusive prefix over p of the carry masses, CP[p*N + c]; carry[c] = column totals
    double T0, Tend, h, dt_max;
    int32_t N, impulse_kind;
    uint64_t seed;
};

// T0 + d for a delay d in [0, h], inside (T0, Tend] also when d is lost to rounding
static __device__ __forceinline__ double fc_after(double T0, double d)
{
    const double t = T0 + d;
    return t > T0 ? t : nextafter(T0, INFINITY);
}

// the logit-normal delay CDF Φ(√τ (logit(d/Δtmax) - μ)), st = √τ
static __device__ double fc_cdf_ln(double mu, double st, double d, double dt_max)
{
#pragma clang fp contract(off)
    if (!(d > 0.0)) return 0.0;
    if (!(d < dt_max)) return 1.0;
    const double x = d / dt_max;
    return 0.5 * erfc(-0.7071067811865476 * (st * (log(x / (1.0 - x)) - mu)));
}

// ---- the boundary: exponential state and carry masses ---------------------------------------------------------------
// Workgroup = parent node p, lane = child node c: m[p,c] = W·A · Σ_k e^{-θ(T0 - t_k)} · (1 - e^{-θh}) over p's events in time
// order (one running fp64 sum per lane: the same bits every call), written row-major so that the column prefix below reads
// coalesced.  nhp_exp is exactly 0 below -708, so the sum starts at the first event that is not.
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_state(const nhp_child *__restrict__ child, const int32_t *__restrict__ boff,
                                                        const double *__restrict__ W, const double *__restrict__ A,
                                                        const double *__restrict__ theta, int32_t N, double T0, double h,
                                                        double *__restrict__ mT)
{
#pragma clang fp contract(off)
    const int32_t p = blockIdx.x, k0 = boff[p], k1 = boff[p + 1];
    for (int32_t c = threadIdx.x; c < N; c += SIM_BLOCK) {
        const size_t q = (size_t)p + (size_t)c * N;
        const double wa = A ? W[q] * A[q] : W[q];
        double m = 0.0;
        if (wa > 0.0) {
            const double th = theta[q];
            int32_t lo = k0, hi = k1;                 // first k with -θ(T0 - t_k) >= -708 (monotone in t_k)
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (-(th * (T0 - child[mid].t)) >= -708.0) hi = mid; else lo = mid + 1; }
            double g = 0.0;
            for (int32_t k = lo; k < k1; ++k) g = g + nhp_exp(-(th * (T0 - child[k].t)));
            m = wa * g * -expm1(-(th * h));
        }
        mT[(size_t)p * N + c] = m;
    }
}

// lane = child node c: the running sum over p in place, the column total = the expected carry-over of node c.  Eight rows
// are loaded ahead of the eight dependent additions (the sum itself stays sequential in p: it is the documented order).
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_colprefix(double *__restrict__ mT, int32_t N, double *__restrict__ carry,
                                                            fc_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (c >= N) return;
    double run = 0.0;
    for (int32_t p0 = 0; p0 < N; p0 += 8) {
        double v[8];
#pragma unroll
        for (int32_t k = 0; k < 8; ++k) v[k] = p0 + k < N ? mT[(size_t)(p0 + k) * N + c] : 0.0;
#pragma unroll
        for (int32_t k = 0; k < 8; ++k)
            if (p0 + k < N) { run = run + v[k]; mT[(size_t)(p0 + k) * N + c] = run; }
    }
    carry[c] = run;
    if (!(run <= 1099511627776.0)) atomicOr(&sc->bad, 4);        // 2^40 carry-over children per node at most (and not NaN)
}

// logit-normal: the first event inside the look-back window of T0
__global__ void k_fc_window(const double *__restrict__ times, int64_t M, double T0, double dt_max, fc_scal *__restrict__ sc)
{
    int64_t lo = 0, hi = M;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (T0 - times[mid] < dt_max) hi = mid; else lo = mid + 1; }
    sc->w0 = lo;
}

// logit-normal: carry[c] = Σ_j W·A·(F(Tend - t_j) - F(T0 - t_j)) over the window events in time order, lane = c
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_carry_ln(const double *__restrict__ times, const int32_t *__restrict__ nodes, int64_t w0,
                                                           int64_t M, const double *__restrict__ W, const double *__restrict__ A,
                                                           const double *__restrict__ mu, const double *__restrict__ tau, int32_t N,
                                                           double T0, double Tend, double dt_max, double *__restrict__ carry)
{
#pragma clang fp contract(off)
    const int32_t c = blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (c >= N) return;
    double run = 0.0;
    for (int64_t j = w0; j < M; ++j) {
        const size_t q = (size_t)nodes[j] + (size_t)c * N;
        const double wa = A ? W[q] * A[q] : W[q];
        if (wa > 0.0) {
            const double st = sqrt(tau[q]);
            run = run + wa * (fc_cdf_ln(mu[q], st, Tend - times[j], dt_max) - fc_cdf_ln(mu[q], st, T0 - times[j], dt_max));
        }
    }
    carry[c] = run;
}

// ---- generation 0 (logit-normal): the window events as parents, once per replica --------------------------------------
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_prologue(fc_args a, const double *__restrict__ times, const int32_t *__restrict__ nodes,
                                                           int64_t w0, int64_t wn, int64_t n_pro, double *__restrict__ at,
                                                           int32_t *__restrict__ anode, int32_t *__restrict__ arep,
                                                           int64_t *__restrict__ cnt, fc_scal *__restrict__ sc)
{
    const int64_t i = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (i < n_pro) {
        const int64_t r = i / wn, j = w0 + (i - r * wn);
        const int32_t p = nodes[j];
        at[i] = times[j]; anode[i] = p; arep[i] = (int32_t)r;
        const double n = sim_poisson(a.R[p], a.seed ^ FC_KEY_CHILD_COUNT, 0, (uint64_t)i);
        cnt[i] = (int64_t)n;
        kids = (unsigned long long)n;
    }
    sim_wave_add(kids, &sc->next);
}

// ---- roots: per (replica, node) the immigrant count and the exponential carry-over count -------------------------------
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_root_counts(fc_args a, const double *__restrict__ lambda0, int64_t SN,
                                                              int64_t *__restrict__ cnt0, fc_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (e >= SN) return;
    const int32_t c = (int32_t)(e % a.N);
    const double mean = lambda0[c] * a.h;
    const bool ok = lambda0[c] >= 0.0 && mean <= 1099511627776.0;      // 2^40 immigrants per node at most (and not NaN)
    if (!ok) atomicOr(&sc->bad, 2);
    cnt0[2 * e] = ok ? (int64_t)sim_poisson(mean, a.seed ^ FC_KEY_IMM_COUNT, 0, (uint64_t)e) : 0;
    cnt0[2 * e + 1] = a.carry ? (int64_t)sim_poisson(a.carry[c], a.seed ^ FC_KEY_CARRY_COUNT, 0, (uint64_t)e) : 0;
}

__global__ void k_fc_start(fc_scal *__restrict__ sc, const int64_t *__restrict__ n_roots, int64_t n_pro) { sc->fill = n_pro + *n_roots; }

// root k (k in [off0[2e + kind], off0[2e + kind + 1]), e = r·N + c, kind 0 immigrant, 1 carry-over child): arena entry
// n_pro + k and its child count
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_roots(fc_args a, const int64_t *__restrict__ off0, int64_t n2, int64_t n_roots,
                                                        int64_t n_pro, double *__restrict__ at, int32_t *__restrict__ anode,
                                                        int32_t *__restrict__ arep, int64_t *__restrict__ cnt, fc_scal *__restrict__ sc)
{
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (k < n_roots) {
        int64_t lo = 0, hi = n2;                      // last e2 with off0[e2] <= k
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off0[mid] <= k) lo = mid; else hi = mid; }
        const int64_t e = lo >> 1;
        const int32_t N = a.N, c = (int32_t)(e % N);
        double ua, ub, t;
        philox_2u(a.seed ^ FC_KEY_ROOT, 0, (uint64_t)k, 0, &ua, &ub);
        if (!(lo & 1)) {
            t = fc_after(a.T0, ua * a.h);
        } else {
            const double x = sim_u01(ua) * a.carry[c];
            int32_t l = 0, hh = N;                    // first p with CP[p, c] > x
            while (l < hh) { const int32_t mid = (l + hh) >> 1; if (a.CP[(size_t)mid * N + c] > x) hh = mid; else l = mid + 1; }
            if (l == N) {                             // x rounded up to the total: the first entry reaching it (a positive mass)
                l = 0; hh = N - 1;
                while (l < hh) { const int32_t mid = (l + hh) >> 1; if (a.CP[(size_t)mid * N + c] >= x) hh = mid; else l = mid + 1; }
            }
            const double th = a.p1[(size_t)l + (size_t)c * N];
            const double qh = -expm1(-(th * a.h));                    // the delay is Exp(θ) given <= h
            t = fc_after(a.T0, fmin(-log1p(-(ub * qh)) / th, a.h));
        }
        const int64_t i = n_pro + k;
        at[i] = t; anode[i] = c; arep[i] = (int32_t)(e / N);
        const double n = sim_poisson(a.R[c], a.seed ^ FC_KEY_CHILD_COUNT, 1, (uint64_t)i);
        cnt[k] = (int64_t)n;
        kids = (unsigned long long)n;
    }
    sim_wave_add(kids, &sc->next);
}

// ---- the generation loop of the simulator, every entry with its replica ------------------------------------------------
// child slot s = s0 + j of generation gen: parent, node, delay, time, keep flag
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_children(fc_args a, uint64_t gen, int64_t s0, int64_t m, const int64_t *__restrict__ off,
                                                           int64_t n_par, int64_t g0, const double *__restrict__ at,
                                                           const int32_t *__restrict__ anode, const int32_t *__restrict__ arep,
                                                           double *__restrict__ ct, int32_t *__restrict__ cn, int32_t *__restrict__ cr,
                                                           uint32_t *__restrict__ keep)
{
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t s = s0 + j;
    int64_t lo = 0, hi = n_par;                       // last parent i with off[i] <= s
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (off[mid] <= s) lo = mid; else hi = mid; }
    const int64_t par = g0 + lo;
    const int32_t p = anode[par], N = a.N;
    const uint64_t key = a.seed ^ FC_KEY_CHILD;
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
        dt = -nhp_log(ub) / a.p1[q];
    } else {
        double z, unused;
        philox_attempt(key, gen, (uint64_t)s, 1, &z, &unused);
        dt = a.dt_max / (1.0 + nhp_exp(-(a.p1[q] + z / sqrt(a.p2[q]))));
    }
    const double t = at[par] + dt;
    ct[j] = t; cn[j] = l; cr[j] = arep[par];
    keep[j] = t > a.T0 && t <= a.Tend;
}

// survivors of a chunk behind the fill counter (never at or past cap), with their own child counts
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_keep(fc_args a, uint64_t gen_next, int64_t m, const uint32_t *__restrict__ keep,
                                                       const uint32_t *__restrict__ pos, const double *__restrict__ ct,
                                                       const int32_t *__restrict__ cn, const int32_t *__restrict__ cr,
                                                       fc_scal *__restrict__ sc, int64_t g1, int64_t cap, double *__restrict__ at,
                                                       int32_t *__restrict__ anode, int32_t *__restrict__ arep, int64_t *__restrict__ cnt)
{
    const int64_t j = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    unsigned long long kids = 0;
    if (j < m && keep[j]) {
        const int64_t dst = (int64_t)sc->fill + pos[j];
        if (dst < cap) {
            const int32_t c = cn[j];
            at[dst] = ct[j]; anode[dst] = c; arep[dst] = cr[j];
            const double n = sim_poisson(a.R[c], a.seed ^ FC_KEY_CHILD_COUNT, gen_next, (uint64_t)dst);
            cnt[dst - g1] = (int64_t)n;
            kids = (unsigned long long)n;
        }
    }
    sim_wave_add(kids, &sc->next);
}

__global__ void k_fc_advance(fc_scal *__restrict__ sc, const uint32_t *__restrict__ kept) { sc->fill += *kept; }
__global__ void k_fc_clear_next(fc_scal *__restrict__ sc) { sc->next = 0; }

// ---- outputs -----------------------------------------------------------------------------------------------------------
// counts[r, c]: integer atomics, so the order of the additions does not show
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_count(const int32_t *__restrict__ anode, const int32_t *__restrict__ arep, int64_t n,
                                                        int32_t N, unsigned long long *__restrict__ counts)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k < n) atomicAdd(&counts[(size_t)arep[k] * N + anode[k]], 1ull);
}

// one wave per replica: the row sum of counts (integers: any order)
__global__ void __launch_bounds__(64) k_fc_replica_totals(const int64_t *__restrict__ counts, int32_t N, int64_t *__restrict__ tot)
{
    const int64_t r = blockIdx.x;
    long long s = 0;
    for (int32_t c = threadIdx.x; c < N; c += 64) s += counts[(size_t)r * N + c];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) tot[r] = s;
}

__global__ void __launch_bounds__(SIM_BLOCK) k_fc_time_keys(const double *__restrict__ at, int64_t n, uint64_t bits0, uint64_t *__restrict__ key)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k < n) key[k] = (uint64_t)__double_as_longlong(at[k]) - bits0;
}

__global__ void __launch_bounds__(SIM_BLOCK) k_fc_replica_keys(const int32_t *__restrict__ arep, const int32_t *__restrict__ perm, int64_t n,
                                                               uint32_t *__restrict__ key)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k < n) key[k] = (uint32_t)arep[perm[k]];
}

// output position k <- kept entry by_time[by_replica[k]]: times, 1-based nodes
__global__ void __launch_bounds__(SIM_BLOCK) k_fc_gather(const int32_t *__restrict__ by_time, const int32_t *__restrict__ by_replica, int64_t n,
                                                         const double *__restrict__ at, const int32_t *__restrict__ anode,
                                                         double *__restrict__ times, int64_t *__restrict__ nodes)
{
    const int64_t k = (int64_t)blockIdx.x * SIM_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int32_t i = by_time[by_replica[k]];
    times[k] = at[i];
    nodes[k] = (int64_t)anode[i] + 1;
}

static double fc_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" nhp_status nhp_cont_forecast(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double horizon, int32_t nsamples,
                                        uint64_t seed, int64_t max_events, int32_t output_on_device, double *carry, int64_t *counts,
                                        double *times, int64_t *nodes, int64_t *offsets, double *phase_ms)
{
    if (!ctx) return NHP_EINVAL;
    if (!ds || !m || !counts) { nhp_set_error(ctx, "forecast: null argument"); return NHP_EINVAL; }
    if ((times != nullptr) != (nodes != nullptr) || (times != nullptr) != (offsets != nullptr)) {
        nhp_set_error(ctx, "forecast: times, nodes and offsets are given together or not at all");
        return NHP_EINVAL;
    }
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (nsamples < 1) { nhp_set_error(ctx, "forecast: nsamples = %d must be at least 1", nsamples); return NHP_EINVAL; }
    if (max_events < 0 || max_events >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "forecast: max_events = %lld outside [0, 2^31)", (long long)max_events);
        return NHP_EINVAL;
    }
    if (!(horizon >= 0.0 && horizon < INFINITY)) {
        nhp_set_error(ctx, "forecast: horizon must be non-negative and finite, got %g", horizon);
        return NHP_EDOMAIN;
    }
    if (m->baseline_kind == NHP_BASELINE_LGCP) {
        nhp_set_error(ctx, "forecast: not available with a LogGaussianCoxProcess baseline (the grid ends where the data end)");
        return NHP_ENOTIMPL;
    }
    NHP_WHOLE_DATASET(ctx, ds, "forecast");
    NHP_ONE_RECORDING(ctx, ds, "forecast", "a forecast continues one recording: pass the trial to continue");
    const auto t_begin = std::chrono::steady_clock::now();
    const int32_t N = m->N;
    const int64_t S = nsamples, SN = S * N, cap = max_events, M = ds->M;
    const bool expo = m->impulse_kind == NHP_IMPULSE_EXPONENTIAL, paths = times != nullptr;
    const double T0 = ds->duration, Tend = T0 + horizon;
    if (SN >= ((int64_t)1 << 30)) {
        nhp_set_error(ctx, "forecast: nsamples x n_nodes = %lld must stay below 2^30 (the root counts are scanned as one array)", (long long)SN);
        return NHP_ENOTIMPL;
    }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    if (phase_ms) phase_ms[0] = phase_ms[1] = 0.0;

    // ---- results that leave through a staging copy when the caller's pointers are host memory
    dd_arena a0;
    a0.st = st;
    double *o_carry = nullptr;
    int64_t *o_counts = counts, *o_off = offsets;
    a0.ask(&o_carry, N);
    if (!output_on_device) {
        a0.ask(&o_counts, SN);
        if (paths) a0.ask(&o_off, S + 1);
    }
    NHP_HIP(ctx, a0.alloc());
    NHP_HIP(ctx, hipMemsetAsync(o_carry, 0, sizeof(double) * N, st));
    NHP_HIP(ctx, hipMemsetAsync(o_counts, 0, sizeof(int64_t) * SN, st));
    if (paths) NHP_HIP(ctx, hipMemsetAsync(o_off, 0, sizeof(int64_t) * (S + 1), st));
    auto finish = [&](int64_t n, const double *d_t, const int64_t *d_n) -> nhp_status {
        if (carry) NHP_HIP(ctx, hipMemcpyAsync(carry, o_carry, sizeof(double) * N, output_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        if (!output_on_device) {
            NHP_HIP(ctx, hipMemcpyAsync(counts, o_counts, sizeof(int64_t) * SN, hipMemcpyDeviceToHost, st));
            if (paths) NHP_HIP(ctx, hipMemcpyAsync(offsets, o_off, sizeof(int64_t) * (S + 1), hipMemcpyDeviceToHost, st));
            if (paths && n > 0) {
                NHP_HIP(ctx, hipMemcpyAsync(times, d_t, sizeof(double) * n, hipMemcpyDeviceToHost, st));
                NHP_HIP(ctx, hipMemcpyAsync(nodes, d_n, sizeof(int64_t) * n, hipMemcpyDeviceToHost, st));
            }
        }
        NHP_HIP(ctx, hipStreamSynchronize(st));
        return NHP_OK;
    };

    sim_pinned<fc_scal> pin;
    NHP_HIP(ctx, hipHostMalloc((void **)&pin.h, sizeof(fc_scal), hipHostMallocDefault));
    fc_scal *h = pin.h;

    // ---- the boundary state: prefix table and parameter checks, exponential carry masses | the logit-normal window
    dd_arena a1;
    a1.st = st;
    double *d_G = nullptr, *d_R = nullptr, *d_CP = nullptr;
    int64_t *d_chk = nullptr;
    fc_scal *d_sc = nullptr;
    a1.ask(&d_G, (int64_t)N * N); a1.ask(&d_R, N); a1.ask(&d_sc, 1); a1.ask(&d_chk, 2 * (int64_t)N);
    if (expo) a1.ask(&d_CP, (int64_t)N * N);
    NHP_HIP(ctx, a1.alloc());
    const double *d_A = m->has_A ? m->d_A : nullptr;
    NHP_HIP(ctx, hipMemsetAsync(d_sc, 0, sizeof(fc_scal), st));
    k_sim_rows<<<dd_grid(N, SIM_ROWS), SIM_ROWS, 0, st>>>(m->d_W, d_A, m->d_p1, m->d_p2, N, m->impulse_kind, d_G, d_R,
                                                          d_sc);
    const bool live = Tend > T0;                      // (T0, Tend] holds a double
    if (expo && live) {
        k_fc_state<<<N, SIM_BLOCK, 0, st>>>(ds->d_child, ds->d_boff, m->d_W, d_A, m->d_p1, N, T0, horizon, d_CP);
        k_fc_colprefix<<<dd_grid(N, SIM_BLOCK), SIM_BLOCK, 0, st>>>(d_CP, N, o_carry, d_sc);
    } else if (live) {
        k_fc_window<<<1, 1, 0, st>>>(ds->d_times, M, T0, m->dt_max, d_sc);
    }
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 1) {
        nhp_set_error(ctx, "forecast: every W[p,c]·A[p,c] must be finite and >= 0 with row sums <= 2^32, and every link with weight "
                           "needs a finite positive θ (finite μ, positive τ)");
        return NHP_EDOMAIN;
    }
    if (h->bad & 4) {
        nhp_set_error(ctx, "forecast: the expected carry-over of a node must be finite (at most 2^40 events)");
        return NHP_EDOMAIN;
    }
    const int64_t w0 = expo || !live ? M : h->w0, wn = M - w0, n_pro = S * wn;
    if (!live) {                                      // an empty interval: zero counts, empty paths; the baseline is still checked
        fc_args z = {};
        z.N = N; z.seed = seed;
        k_fc_root_counts<<<dd_grid(N, SIM_BLOCK), SIM_BLOCK, 0, st>>>(z, m->d_lambda0, N, d_chk, d_sc);
        NHP_HIP(ctx, hipGetLastError());
        NHP_TRY(sim_read(ctx, h, d_sc));
        if (h->bad & 2) {
            nhp_set_error(ctx, "forecast: baseline intensities must be finite and >= 0 (at most 2^40 expected events per node)");
            return NHP_EDOMAIN;
        }
        return finish(0, nullptr, nullptr);
    }
    if (n_pro + cap >= ((int64_t)1 << 31)) {
        nhp_set_error(ctx, "forecast: nsamples x events inside the look-back window (%lld x %lld) + max_events must stay below 2^31 "
                           "(arena indices are 32-bit)", (long long)S, (long long)wn);
        return NHP_ENOTIMPL;
    }
    if (phase_ms) phase_ms[0] = fc_ms_since(t_begin);
    const auto t_ensemble = std::chrono::steady_clock::now();

    // ---- scratch: root counts, the arena (window parents + max_events entries), one chunk of child slots
    const int64_t acap = n_pro + cap, ncnt = std::max(n_pro, cap);
    const int64_t CH = std::min(std::max(cap, SIM_CHUNK_MIN), SIM_CHUNK_MAX);
    dd_arena a2;
    a2.st = st;
    double *d_at = nullptr, *d_ct = nullptr;
    int64_t *d_cnt0 = nullptr, *d_off0 = nullptr, *d_cnt = nullptr, *d_off = nullptr, *d_tmp64 = nullptr;
    int32_t *d_anode = nullptr, *d_arep = nullptr, *d_cn = nullptr, *d_cr = nullptr;
    uint32_t *d_keep = nullptr, *d_pos = nullptr, *d_tmp32 = nullptr;
    a2.ask(&d_cnt0, 2 * SN); a2.ask(&d_off0, 2 * SN + 1);
    a2.ask(&d_tmp64, dd_grid(std::max<int64_t>(ncnt, 2 * SN), DD_TILE));
    a2.ask(&d_at, acap); a2.ask(&d_anode, acap); a2.ask(&d_arep, acap); a2.ask(&d_cnt, ncnt); a2.ask(&d_off, ncnt + 1);
    a2.ask(&d_ct, CH); a2.ask(&d_cn, CH); a2.ask(&d_cr, CH); a2.ask(&d_keep, CH); a2.ask(&d_pos, CH + 1);
    a2.ask(&d_tmp32, dd_grid(CH, DD_TILE));
    NHP_HIP(ctx, a2.alloc());

    fc_args a;
    a.G = d_G; a.R = d_R; a.p1 = m->d_p1; a.p2 = m->d_p2; a.CP = d_CP; a.carry = expo ? o_carry : nullptr;
    a.T0 = T0; a.Tend = Tend; a.h = horizon; a.dt_max = m->dt_max; a.N = N; a.impulse_kind = m->impulse_kind; a.seed = seed;

    // ---- root counts, the window parents; readback: {arena fill, child slots of generation 0, baseline check}
    if (!expo && wn > 0)
        k_fc_carry_ln<<<dd_grid(N, SIM_BLOCK), SIM_BLOCK, 0, st>>>(ds->d_times, ds->d_nodes, w0, M, m->d_W, d_A, m->d_p1, m->d_p2, N, T0, Tend,
                                                                   m->dt_max, o_carry);
    k_fc_root_counts<<<dd_grid(SN, SIM_BLOCK), SIM_BLOCK, 0, st>>>(a, m->d_lambda0, SN, d_cnt0, d_sc);
    dd_scan<int64_t>(st, d_cnt0, d_off0, 2 * SN, d_tmp64);
    if (n_pro > 0)
        k_fc_prologue<<<dd_grid(n_pro, SIM_BLOCK), SIM_BLOCK, 0, st>>>(a, ds->d_times, ds->d_nodes, w0, wn, n_pro, d_at, d_anode, d_arep, d_cnt,
                                                                      d_sc);
    k_fc_start<<<1, 1, 0, st>>>(d_sc, d_off0 + 2 * SN, n_pro);
    NHP_HIP(ctx, hipGetLastError());
    NHP_TRY(sim_read(ctx, h, d_sc));
    if (h->bad & 2) {
        nhp_set_error(ctx, "forecast: baseline intensities must be finite and >= 0 (at most 2^40 expected events per node)");
        return NHP_EDOMAIN;
    }
    const int64_t n_roots = h->fill - n_pro;
    if (n_roots > cap) return sim_exploded(ctx);

    // ---- generations: parents [g0, g1) of generation gen with C child slots in all; the roots join as generation 1
    int64_t g0 = 0, g1 = n_pro, C = (int64_t)h->next;
    uint64_t gen = 0;
    do {
        const int64_t np = g1 - g0;
        if (C > 0) dd_scan<int64_t>(st, d_cnt, d_off, np, d_tmp64);
        k_fc_clear_next<<<1, 1, 0, st>>>(d_sc);
        if (gen == 0 && n_roots > 0)                  // after the scan: their child counts take the place of generation 0's
            k_fc_roots<<<dd_grid(n_roots, SIM_BLOCK), SIM_BLOCK, 0, st>>>(a, d_off0, 2 * SN, n_roots, n_pro, d_at, d_anode, d_arep, d_cnt, d_sc);
        for (int64_t s0 = 0; s0 < C; s0 += CH) {
            const int64_t mc = std::min<int64_t>(CH, C - s0);
            const unsigned gr = dd_grid(mc, SIM_BLOCK);
            k_fc_children<<<gr, SIM_BLOCK, 0, st>>>(a, gen, s0, mc, d_off, np, g0, d_at, d_anode, d_arep, d_ct, d_cn, d_cr, d_keep);
            dd_scan<uint32_t>(st, d_keep, d_pos, mc, d_tmp32);
            k_fc_keep<<<gr, SIM_BLOCK, 0, st>>>(a, gen + 1, mc, d_keep, d_pos, d_ct, d_cn, d_cr, d_sc, g1, acap, d_at, d_anode, d_arep, d_cnt);
            k_fc_advance<<<1, 1, 0, st>>>(d_sc, d_pos + mc);
            NHP_HIP(ctx, hipGetLastError());
            if (s0 + CH < C) {                        // a generation of several chunks: stop as soon as it overflows
                NHP_TRY(sim_read(ctx, h, d_sc));
                if (h->fill > acap) return sim_exploded(ctx);
            }
        }
        NHP_HIP(ctx, hipGetLastError());
        NHP_TRY(sim_read(ctx, h, d_sc));
        if (h->fill > acap) return sim_exploded(ctx);
        g0 = g1; g1 = h->fill; C = (int64_t)h->next;
        ++gen;
    } while (C > 0);
    const int64_t n = g1 - n_pro;                     // kept events: arena [n_pro, g1)

    // ---- counts, and the paths: by time, then stably by replica
    const double *e_at = d_at + n_pro;
    const int32_t *e_node = d_anode + n_pro, *e_rep = d_arep + n_pro;
    dd_arena a3;
    a3.st = st;
    double *o_t = times;
    int64_t *o_n = nodes;
    if (n > 0) k_fc_count<<<dd_grid(n, SIM_BLOCK), SIM_BLOCK, 0, st>>>(e_node, e_rep, n, N, (unsigned long long *)o_counts);
    if (paths) {
        k_fc_replica_totals<<<(unsigned)S, 64, 0, st>>>(o_counts, N, d_cnt0);
        dd_scan<int64_t>(st, d_cnt0, o_off, S, d_tmp64);
    }
    NHP_HIP(ctx, hipGetLastError());
    if (paths && n > 0) {
        uint64_t *d_key = nullptr, *k_sorted = nullptr;
        uint32_t *d_rkey = nullptr, *r_sorted = nullptr;
        int32_t *by_time = nullptr, *by_rep = nullptr;
        dd_sort_buf<uint64_t> sb;
        dd_sort_buf<uint32_t> rb;
        const int64_t ntn = dd_grid(n, DD_TILE);
        a3.ask(&d_key, n); a3.ask(&sb.k2, n); a3.ask(&sb.v1, n); a3.ask(&sb.v2, n);
        a3.ask(&sb.hist, (int64_t)DD_RADIX * ntn); a3.ask(&sb.offs, (int64_t)DD_RADIX * ntn + 1);
        a3.ask(&sb.tmp, dd_grid((int64_t)DD_RADIX * ntn, DD_TILE));
        a3.ask(&d_rkey, n); a3.ask(&rb.k2, n); a3.ask(&rb.v1, n); a3.ask(&rb.v2, n);
        if (!output_on_device) { a3.ask(&o_t, n); a3.ask(&o_n, n); }
        NHP_HIP(ctx, a3.alloc());
        rb.hist = sb.hist; rb.offs = sb.offs; rb.tmp = sb.tmp;
        uint64_t bits0, bits1;
        memcpy(&bits0, &T0, sizeof bits0);
        memcpy(&bits1, &Tend, sizeof bits1);          // every key is <= bits1 - bits0
        const unsigned gn = dd_grid(n, SIM_BLOCK);
        k_fc_time_keys<<<gn, SIM_BLOCK, 0, st>>>(e_at, n, bits0, d_key);
        dd_sort<uint64_t>(st, d_key, n, dd_bitlen(bits1 - bits0), sb, &k_sorted, &by_time);
        k_fc_replica_keys<<<gn, SIM_BLOCK, 0, st>>>(e_rep, by_time, n, d_rkey);
        dd_sort<uint32_t>(st, d_rkey, n, dd_bitlen((uint64_t)(S - 1)), rb, &r_sorted, &by_rep);
        k_fc_gather<<<gn, SIM_BLOCK, 0, st>>>(by_time, by_rep, n, e_at, e_node, o_t, o_n);
        NHP_HIP(ctx, hipGetLastError());
    }
    NHP_TRY(finish(n, o_t, o_n));
    if (phase_ms) phase_ms[1] = fc_ms_since(t_ensemble);
    return NHP_OK;
}
