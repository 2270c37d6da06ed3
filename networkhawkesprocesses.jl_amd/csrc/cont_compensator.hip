// compensator(process, data): the exact time integral of the intensity, Λ_c(t) = ∫ λ_c(s) ds from 0 (grid_x[0]) to t, at every
// event of its own node, its increments between consecutive events of a node (the time-rescaling residuals, Exp(1) under
// the true model) and Λ_c(T) for every node (expected counts).  λ is what intensity(process, data, t) evaluates
// (reference src/continuous.jl:84-96), conventions included: parents of t are the events with t - Δtmax < t_i < t, the
// exponential impulse is cut at Δtmax and not renormalised, the logit-normal pdf is not divided by Δtmax, so
// with H_{p,c}(d) = ∫_0^{min(d,Δtmax)} pdf_{p,c}
//     exponential   H = 1 - exp(-θ min(d, Δtmax))
//     logit-normal  H = Δtmax Φ(√τ (logit(d/Δtmax) - μ)) for d < Δtmax, Δtmax from there on
//     Λ_c(t) = base_c(t) + Σ_{i: t_i < t} W[n_i,c] A[n_i,c] H_{n_i,c}(t - t_i).
// The reference integrates no impulse: its log-likelihood charges every event the full mass ΣW ("approximate (exact
// requires cdf)", src/continuous.jl:247).
//
// An event older than Δtmax contributes its saturated mass V[p,c] = W A H(Δtmax), whatever its age, so
//     Λ_c(t_k) = base_c(t_k) + S_c(ws_k) + Σ_{i in [ws_k, k), t_i < t_k} W A H(t_k - t_i),   S_c(j) = Σ_{i < j} V[n_i, c]
// with ws_k the event's window start (nhp_child::first).  S is a prefix sum over the event list of gathered rows of V,
// needed at M cut points of M different columns:
//   k_comp_chunk_sums  the event list in chunks of COMP_CHUNK events: D[j][c] = Σ_{i in chunk j} V[n_i, c], lanes across c
//                      reading rows of the row-major copy of V (coalesced), the chunk's nodes in LDS.  M·N adds: the only
//                      O(M·N) step (a dense histogram x V product would be M/COMP_CHUNK·N² multiply-adds: more, for N above
//                      the chunk length).
//   k_comp_group_scan  exclusive prefix of D inside groups of COMP_GROUP chunks (in place) + the groups' totals
//   k_comp_super_scan  exclusive prefix of the groups' totals: S_c(j·COMP_CHUNK) = super[j / COMP_GROUP][c] + D[j][c]
//   k_comp_events      one workgroup per item (a run of one node's children, as in the windowed kernels) with the node's
//                      columns of θ | μ, √τ, W·A and V in LDS; COMP_LANES lanes per child walk the events from the start
//                      of the window's chunk to the child: V gathers before ws_k, then W·A·H from there (the pairs the
//                      windowed intensity visits, a CDF in place of a pdf), then a fixed butterfly over the lanes.
//   k_comp_residuals   differences of consecutive values of a node in bucket order (the first event of a node keeps Λ)
//   k_comp_total       one workgroup per node: S_c at the first event inside (T - Δtmax, T], H(T - t_i) from there
// Δtmax = ∞ (the exponential default) has no saturated part: ws_k = 0 and every earlier event is walked, as the windowed
// routes do.  Sums are fp64 over non-negative terms in a fixed order (no floating-point atomics): results are identical
// from run to run and for every way the dataset was built.
#include "nhp_internal.h"

#define COMP_CHUNK 128
#define COMP_GROUP 64
#define COMP_LANES 8
#define COMP_COLS 256      // columns per workgroup of the chunk kernels

// WA[p + cN] = W·A, Vc[p + cN] = W·A·H(Δtmax) (column-major, like the model), Vt[p·N + c] the same row-major
__global__ __launch_bounds__(256) void k_comp_tables(nhp_cont_args a, double *__restrict__ WA, double *__restrict__ Vc,
                                                     double *__restrict__ Vt)
{
    __shared__ double tile[32][33];
    const int N = a.N, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + tx, c = c0 + r;
        if (p < N && c < N) {
            const size_t k = (size_t)p + (size_t)c * N;
            double w = a.W[k];
            if (a.A) w = a.A[k] * w;
            double v = 0.0;
            if (w != 0.0) {
                if (a.impulse_kind == NHP_IMPULSE_EXPONENTIAL) v = a.dt_max < INFINITY ? w * -expm1(-(a.p1[k] * a.dt_max)) : w;
                else v = w * a.dt_max;
            }
            WA[k] = w;
            Vc[k] = v;
            tile[r][tx] = v;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        if (p < N && c < N) Vt[(size_t)p * N + c] = tile[tx][r];
    }
}

// D[j][c] = Σ V[n_i, c] over the events of chunk j = [j·COMP_CHUNK, min((j + 1)·COMP_CHUNK, M)); rows j = 0 .. M / COMP_CHUNK
__global__ __launch_bounds__(COMP_COLS) void k_comp_chunk_sums(const int32_t *__restrict__ nodes, int64_t M, int N,
                                                               const double *__restrict__ Vt, double *__restrict__ D)
{
    __shared__ int32_t nd[COMP_CHUNK];
    const int64_t i0 = (int64_t)blockIdx.x * COMP_CHUNK;
    const int cnt = (int)(M - i0 < COMP_CHUNK ? M - i0 : COMP_CHUNK);
    if ((int)threadIdx.x < cnt) nd[threadIdx.x] = nodes[i0 + threadIdx.x];
    __syncthreads();
    const int c = blockIdx.y * COMP_COLS + threadIdx.x;
    if (c >= N) return;
    double acc = 0.0;
#pragma unroll 8
    for (int e = 0; e < cnt; ++e) acc += Vt[(size_t)nd[e] * N + c];
    D[(size_t)blockIdx.x * N + c] = acc;
}

// rows [g·COMP_GROUP, (g + 1)·COMP_GROUP) of D -> their exclusive prefix (in place); G[g][c] = the group's total
__global__ __launch_bounds__(COMP_COLS) void k_comp_group_scan(double *__restrict__ D, int64_t rows, int N, double *__restrict__ G)
{
    const int c = blockIdx.y * COMP_COLS + threadIdx.x;
    if (c >= N) return;
    const int64_t j0 = (int64_t)blockIdx.x * COMP_GROUP, j1 = j0 + COMP_GROUP < rows ? j0 + COMP_GROUP : rows;
    double run = 0.0;
#pragma unroll 8
    for (int64_t j = j0; j < j1; ++j) {
        const double d = D[(size_t)j * N + c];
        D[(size_t)j * N + c] = run;
        run += d;
    }
    G[(size_t)blockIdx.x * N + c] = run;
}

__global__ __launch_bounds__(COMP_COLS) void k_comp_super_scan(double *__restrict__ G, int64_t groups, int N)
{
    const int c = blockIdx.x * COMP_COLS + threadIdx.x;
    if (c >= N) return;
    double run = 0.0;
#pragma unroll 8
    for (int64_t g = 0; g < groups; ++g) {
        const double d = G[(size_t)g * N + c];
        G[(size_t)g * N + c] = run;
        run += d;
    }
}

// LGCP baseline: cum[c·grid_n + g] = ∫ of the piecewise-linear λ_c from grid_x[0] to grid_x[g] (a trapezoid per cell)
__global__ __launch_bounds__(256) void k_comp_lgcp_cum(nhp_cont_args a, double *__restrict__ cum)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.N) return;
    const double *x = a.grid, *y = a.lambda0 + (size_t)c * a.grid_n;
    double run = 0.0;
    cum[(size_t)c * a.grid_n] = 0.0;
    for (int g = 1; g < a.grid_n; ++g) {
        run += 0.5 * (x[g] - x[g - 1]) * (y[g] + y[g - 1]);
        cum[(size_t)c * a.grid_n + g] = run;
    }
}

// ∫ of the baseline of node c from 0 (grid_x[0]) to t; t lies inside the grid (checked on the host)
__device__ __forceinline__ double comp_base(const nhp_cont_args &a, const double *__restrict__ cum, int c, double t)
{
    if (a.baseline_kind == NHP_BASELINE_HOMOGENEOUS) return a.lambda0[c] * t;
    const double *x = a.grid, *y = a.lambda0 + (size_t)c * a.grid_n;
    int lo = 0, hi = a.grid_n - 1;
    if (!(t < x[hi])) return cum[(size_t)c * a.grid_n + hi];
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t >= x[mid]) lo = mid; else hi = mid;
    }
    const double h = t - x[lo];
    const double yt = (y[lo + 1] * h + y[lo] * (x[lo + 1] - t)) / (x[lo + 1] - x[lo]);      // the interpolant at t
    return cum[(size_t)c * a.grid_n + lo] + 0.5 * h * (y[lo] + yt);
}

// H(d) for d > 0: p1 = θ | μ, p2 = √τ
template <int IMP>
__device__ __forceinline__ double comp_H(double p1, double p2, double d, double dt_max)
{
    if (IMP == NHP_IMPULSE_EXPONENTIAL) return -expm1(-(p1 * (d < dt_max ? d : dt_max)));
    if (!(d < dt_max)) return dt_max;
    const double x = d / dt_max;
    const double z = p2 * (log(x / (1.0 - x)) - p1);
    return dt_max * (0.5 * erfc(-0.7071067811865476 * z));
}

// S_c at the start of chunk j
__device__ __forceinline__ double comp_prefix(const double *__restrict__ D, const double *__restrict__ G, int N, int64_t j, int c)
{
    return G[(size_t)(j / COMP_GROUP) * N + c] + D[(size_t)j * N + c];
}

// ---- several trials ---------------------------------------------------------------------------------------
// Λ^{(r)} is the compensator of trial r alone, from the trial's start: base at the local time t - o_r, saturated masses and
// window terms over the trial's own events [f_r, ...).  The stacked prefix S_c(j) and its scans stay as they are; the
// saturated mass of trial r before ws is S_c(ws) - S_c(f_r), with S_c(f_r) made once per call for every (trial, column):
// Sf[r][c] = S_c at the start of f_r's chunk + (the chunk's events before f_r, added up from 0 in index order).  Where f_r lies
// at or after the start of ws's chunk the gather simply starts at f_r and no prefix is read (no subtraction, no extra error).
// Both prefixes are sums of non-negative terms; with d(.) the prefix depth of tests/compensator_exact_ref.py and P_c(j) the
// stacked mass before j the subtraction adds at most 2^-53·((d(ws) + 1)·P_c(ws) + d(f_r)·P_c(f_r)) to a value's error:
// absolute in the STACKED mass, so a late trial of a long stack is known less well, relative to its own Λ, than an early one.
struct comp_trials {
    const int32_t *f;      // [R + 1] event offsets
    const double *o;       // [R + 1] time offsets
    const double *Sf;      // [R][N] S_c(f_r); null: no saturated part
    int32_t R;
};

// the trial of event i: the last r in [0, R) with f[r] <= i
__device__ __forceinline__ int comp_trial_of(const comp_trials &tr, int i)
{
    int lo = 0, hi = tr.R;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tr.f[mid] <= i) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(COMP_COLS) void k_comp_trial_prefix(const int32_t *__restrict__ nodes, const int32_t *__restrict__ trial_f, int N,
                                                                 const double *__restrict__ Vt, const double *__restrict__ D,
                                                                 const double *__restrict__ G, double *__restrict__ Sf)
{
    const int c = blockIdx.y * COMP_COLS + threadIdx.x;
    if (c >= N) return;
    const int r = blockIdx.x, fr = trial_f[r], j = fr / COMP_CHUNK;
    double acc = 0.0;
    for (int i = j * COMP_CHUNK; i < fr; ++i) acc += Vt[(size_t)nodes[i] * N + c];
    Sf[(size_t)r * N + c] = comp_prefix(D, G, N, j, c) + acc;
}

// at_b[k] (bucket order) and at_t[idx] (time order, nullable) <- Λ_{n_k}(t_k).  D = nullptr: no saturated part (Δtmax = ∞).
// TR: a dataset of several trials (above); the one-recording call instantiates the kernel without it.
template <int IMP, bool TR>
__global__ __launch_bounds__(NHP_BLOCK) void k_comp_events(nhp_cont_args a, const double *__restrict__ WA, const double *__restrict__ Vc,
                                                           const double *__restrict__ D, const double *__restrict__ G,
                                                           const double *__restrict__ cum, double *__restrict__ at_b,
                                                           double *__restrict__ at_t, comp_trials tr)
{
    extern __shared__ double comp_lds[];
    const nhp_item it = a.items[blockIdx.x];
    if (it.kbeg >= it.kend) return;                                      // workgroup-uniform
    const int N = a.N, c = it.node;
    double *s_p1 = comp_lds, *s_wa = s_p1 + N, *s_v = s_wa + N, *s_p2 = s_v + N;
    for (int p = threadIdx.x; p < N; p += NHP_BLOCK) {
        const size_t k = (size_t)p + (size_t)c * N;
        s_p1[p] = a.p1[k];
        s_wa[p] = WA[k];
        s_v[p] = Vc[k];
        if (IMP == NHP_IMPULSE_LOGITNORMAL) s_p2[p] = __builtin_sqrt(a.p2[k]);
    }
    __syncthreads();
    const int sub = threadIdx.x & (COMP_LANES - 1), slot = threadIdx.x / COMP_LANES;
    for (int k0 = it.kbeg; k0 < it.kend; k0 += NHP_BLOCK / COMP_LANES) {
        const int k = k0 + slot;
        const bool valid = k < it.kend;
        nhp_child ch;
        ch.t = 0.0; ch.first = 0; ch.idx = 0;
        if (valid) ch = a.child[k];
        int i0 = D ? ch.first / COMP_CHUNK * COMP_CHUNK : ch.first;
        int r = 0;
        bool own = false;                                               // the gather starts at the trial's first event: no prefix
        double t0 = 0.0;
        if (TR) {
            r = comp_trial_of(tr, ch.idx);
            const int fr = tr.f[r];
            t0 = tr.o[r];
            own = fr >= i0;
            if (own) i0 = fr;
        }
        double acc = 0.0;
        // two loops, so that the lanes of a wave are all gathering or all evaluating H
        for (int i = i0 + sub; i < ch.first; i += COMP_LANES) acc += s_v[a.nodes[i]];
        for (int i = ch.first + sub; i < ch.idx; i += COMP_LANES) {
            const nhp_event e = a.ev[i];
            if (e.t < ch.t) {
                const double w = s_wa[e.node];
                if (w != 0.0) acc += w * comp_H<IMP>(s_p1[e.node], IMP == NHP_IMPULSE_LOGITNORMAL ? s_p2[e.node] : 0.0, ch.t - e.t, a.dt_max);
            }
        }
        for (int off = COMP_LANES / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (valid && sub == 0) {
            if (TR) {
                if (D && !own) acc = (comp_prefix(D, G, N, ch.first / COMP_CHUNK, c) - tr.Sf[(size_t)r * N + c]) + acc;
            } else if (D) acc = comp_prefix(D, G, N, ch.first / COMP_CHUNK, c) + acc;
            const double v = comp_base(a, cum, c, TR ? ch.t - t0 : ch.t) + acc;
            at_b[k] = v;
            if (at_t) at_t[ch.idx] = v;
        }
    }
}

// res[idx_k] = Λ(k) - Λ(previous event of the node); the node's first event keeps Λ (the integral starts at 0)
__global__ __launch_bounds__(256) void k_comp_residuals(nhp_cont_args a, const double *__restrict__ at_b, double *__restrict__ res)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.M) return;
    const nhp_child ch = a.child[k];
    const int c = a.nodes[ch.idx];
    res[ch.idx] = k == a.boff[c] ? at_b[k] : at_b[k] - at_b[k - 1];
}

// several trials: a node's first event INSIDE ITS TRIAL keeps Λ (its predecessor in the bucket belongs to an earlier trial)
__global__ __launch_bounds__(256) void k_comp_residuals_trials(nhp_cont_args a, const double *__restrict__ at_b, double *__restrict__ res,
                                                               comp_trials tr)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.M) return;
    const nhp_child ch = a.child[k];
    const int c = a.nodes[ch.idx];
    const bool head = k == a.boff[c] || a.child[k - 1].idx < tr.f[comp_trial_of(tr, ch.idx)];
    res[ch.idx] = head ? at_b[k] : at_b[k] - at_b[k - 1];
}

// several trials: part[r][c] = Λ_c^{(r)}(T_r), one workgroup per (trial, node); k_comp_total_sum adds the trials up in order
template <int IMP>
__global__ __launch_bounds__(NHP_BLOCK) void k_comp_total_trials(nhp_cont_args a, const double *__restrict__ WA, const double *__restrict__ Vc,
                                                                 const double *__restrict__ D, const double *__restrict__ G,
                                                                 const double *__restrict__ cum, comp_trials tr, double *__restrict__ part)
{
    __shared__ double red[NHP_WAVES];
    const int N = a.N, r = blockIdx.x, c = blockIdx.y;
    const int fb = tr.f[r], fe = tr.f[r + 1];
    const double t0 = tr.o[r], T = tr.o[r + 1], thr = T - a.dt_max;
    int lo = fb, hi = fe;                                                // the trial's first event with t_i > T - Δtmax
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.times[mid] > thr) hi = mid; else lo = mid + 1; }
    const int jT = lo, cs = D ? jT / COMP_CHUNK * COMP_CHUNK : jT;
    const bool own = fb >= cs;
    double acc = 0.0;
    for (int i = (own ? fb : cs) + (int)threadIdx.x; i < fe; i += NHP_BLOCK) {
        const nhp_event e = a.ev[i];
        const size_t k = (size_t)e.node + (size_t)c * N;
        if (i < jT) acc += Vc[k];
        else if (e.t < T) {
            const double w = WA[k];
            if (w != 0.0) acc += w * comp_H<IMP>(a.p1[k], IMP == NHP_IMPULSE_LOGITNORMAL ? __builtin_sqrt(a.p2[k]) : 0.0, T - e.t, a.dt_max);
        }
    }
    acc = nhp_block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (D && !own) acc = (comp_prefix(D, G, N, jT / COMP_CHUNK, c) - tr.Sf[(size_t)r * N + c]) + acc;
        part[(size_t)r * N + c] = comp_base(a, cum, c, T - t0) + acc;
    }
}

__global__ __launch_bounds__(256) void k_comp_total_sum(const double *__restrict__ part, int R, int N, double *__restrict__ total)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double run = 0.0;
    for (int r = 0; r < R; ++r) run += part[(size_t)r * N + c];
    total[c] = run;
}

template <int IMP>
__global__ __launch_bounds__(NHP_BLOCK) void k_comp_total(nhp_cont_args a, const double *__restrict__ WA, const double *__restrict__ Vc,
                                                          const double *__restrict__ D, const double *__restrict__ G,
                                                          const double *__restrict__ cum, double *__restrict__ total)
{
    __shared__ double red[NHP_WAVES];
    const int N = a.N, c = blockIdx.x;
    const double T = a.duration, thr = T - a.dt_max;
    int64_t lo = 0, hi = a.M;                                            // first event with t_i > T - Δtmax
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.times[mid] > thr) hi = mid; else lo = mid + 1; }
    const int64_t jT = lo, i0 = D ? jT / COMP_CHUNK * COMP_CHUNK : jT;
    double acc = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < a.M; i += NHP_BLOCK) {
        const nhp_event e = a.ev[i];
        const size_t k = (size_t)e.node + (size_t)c * N;
        if (i < jT) acc += Vc[k];
        else if (e.t < T) {
            const double w = WA[k];
            if (w != 0.0) acc += w * comp_H<IMP>(a.p1[k], IMP == NHP_IMPULSE_LOGITNORMAL ? __builtin_sqrt(a.p2[k]) : 0.0, T - e.t, a.dt_max);
        }
    }
    acc = nhp_block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (D) acc = comp_prefix(D, G, N, jT / COMP_CHUNK, c) + acc;
        total[c] = comp_base(a, cum, c, T) + acc;
    }
}

extern "C" nhp_status nhp_cont_compensator(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t output_on_device,
                                           double *at_events, double *residuals, double *total)
{
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (!at_events && !residuals && !total) { nhp_set_error(ctx, "compensator: no output requested"); return NHP_EINVAL; }
    NHP_WHOLE_DATASET(ctx, ds, "compensator");
    if (m->baseline_kind == NHP_BASELINE_LGCP && ds->duration > m->grid_end) {
        nhp_set_error(ctx, "Value is outside interpolation support (0, %g)", m->grid_end);
        return NHP_EDOMAIN;
    }
    const bool ln = m->impulse_kind == NHP_IMPULSE_LOGITNORMAL;
    const size_t N = (size_t)ds->N, NN = N * N, M = (size_t)ds->M;
    const size_t lds = 8 * N * (ln ? 4 : 3);
    if (lds > 160 * 1024) {
        nhp_set_error(ctx, "compensator: n_nodes = %d exceeds the 160 KiB LDS budget (%d columns of the parameter tables)", ds->N, ln ? 4 : 3);
        return NHP_ENOTIMPL;
    }
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const bool events = (at_events || residuals) && M > 0;
    const bool finite = ds->dt_max < INFINITY && M > 0;
    const size_t rows = finite ? M / COMP_CHUNK + 1 : 0, groups = (rows + COMP_GROUP - 1) / COMP_GROUP;
    const size_t n_cum = m->baseline_kind == NHP_BASELINE_LGCP ? N * (size_t)m->grid_n : 0;
    const bool host_out = !output_on_device;
    const bool trials = nhp_multi_trial(ds);
    const size_t R = trials ? (size_t)ds->n_trials : 0;
    size_t need = 3 * NN + rows * N + groups * N + n_cum + (events ? M : 0) + 2 * R * N;
    if (host_out) need += (at_events ? M : 0) + (residuals ? M : 0) + (total ? N : 0);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, 8 * need + 64));
    double *WA = (double *)ctx->d_scratch, *Vc = WA + NN, *Vt = Vc + NN, *D = Vt + NN, *G = D + rows * N, *cum = G + groups * N;
    double *at_b = cum + n_cum, *Sf = at_b + (events ? M : 0), *part = Sf + R * N, *next = part + R * N;
    double *o_at = at_events, *o_res = residuals, *o_tot = total;
    if (host_out) {
        if (at_events) { o_at = next; next += M; }
        if (residuals) { o_res = next; next += M; }
        if (total) { o_tot = next; next += N; }
    }
    if (!finite) D = G = nullptr;
    if (!n_cum) cum = nullptr;

    const nhp_cont_args a = nhp_make_args(ds, m);
    const unsigned nt = (unsigned)((N + 31) / 32), ncol = (unsigned)((N + COMP_COLS - 1) / COMP_COLS);
    hipLaunchKernelGGL(k_comp_tables, dim3(nt, nt), dim3(256), 0, st, a, WA, Vc, Vt);
    if (cum) hipLaunchKernelGGL(k_comp_lgcp_cum, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a, cum);
    if (finite) {
        hipLaunchKernelGGL(k_comp_chunk_sums, dim3((unsigned)rows, ncol), dim3(COMP_COLS), 0, st, ds->d_nodes, ds->M, (int)N, Vt, D);
        hipLaunchKernelGGL(k_comp_group_scan, dim3((unsigned)groups, ncol), dim3(COMP_COLS), 0, st, D, (int64_t)rows, (int)N, G);
        hipLaunchKernelGGL(k_comp_super_scan, dim3(ncol), dim3(COMP_COLS), 0, st, G, (int64_t)groups, (int)N);
    }
    NHP_HIP(ctx, hipGetLastError());
    const comp_trials tr = trials ? comp_trials{ds->d_trial_f, ds->d_trial_o, finite ? Sf : nullptr, ds->n_trials} : comp_trials{};
    if (trials && finite) {
        hipLaunchKernelGGL(k_comp_trial_prefix, dim3((unsigned)R, ncol), dim3(COMP_COLS), 0, st, ds->d_nodes, ds->d_trial_f, (int)N, Vt, D, G, Sf);
        NHP_HIP(ctx, hipGetLastError());
    }
    if (events) {
#define COMP_EVENTS(IMP, TR)                                                                                                        \
        do {                                                                                                                       \
            if (lds > 64 * 1024)                                                                                                   \
                NHP_HIP(ctx, hipFuncSetAttribute((const void *)k_comp_events<IMP, TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            hipLaunchKernelGGL((k_comp_events<IMP, TR>), dim3((unsigned)ds->n_items), dim3(NHP_BLOCK), lds, st, a, WA, Vc, D, G, cum, at_b, \
                               at_events ? o_at : nullptr, tr);                                                                    \
        } while (0)
        if (trials && ln) COMP_EVENTS(NHP_IMPULSE_LOGITNORMAL, true);
        else if (trials) COMP_EVENTS(NHP_IMPULSE_EXPONENTIAL, true);
        else if (ln) COMP_EVENTS(NHP_IMPULSE_LOGITNORMAL, false);
        else COMP_EVENTS(NHP_IMPULSE_EXPONENTIAL, false);
#undef COMP_EVENTS
        if (residuals && trials) hipLaunchKernelGGL(k_comp_residuals_trials, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, a, at_b, o_res, tr);
        else if (residuals) hipLaunchKernelGGL(k_comp_residuals, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, a, at_b, o_res);
        NHP_HIP(ctx, hipGetLastError());
    }
    if (total && trials) {
        if (ln) hipLaunchKernelGGL(k_comp_total_trials<NHP_IMPULSE_LOGITNORMAL>, dim3((unsigned)R, (unsigned)N), dim3(NHP_BLOCK), 0, st, a, WA, Vc, D, G, cum, tr, part);
        else hipLaunchKernelGGL(k_comp_total_trials<NHP_IMPULSE_EXPONENTIAL>, dim3((unsigned)R, (unsigned)N), dim3(NHP_BLOCK), 0, st, a, WA, Vc, D, G, cum, tr, part);
        hipLaunchKernelGGL(k_comp_total_sum, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, part, (int)R, (int)N, o_tot);
        NHP_HIP(ctx, hipGetLastError());
    } else if (total) {
        if (ln) hipLaunchKernelGGL(k_comp_total<NHP_IMPULSE_LOGITNORMAL>, dim3((unsigned)N), dim3(NHP_BLOCK), 0, st, a, WA, Vc, D, G, cum, o_tot);
        else hipLaunchKernelGGL(k_comp_total<NHP_IMPULSE_EXPONENTIAL>, dim3((unsigned)N), dim3(NHP_BLOCK), 0, st, a, WA, Vc, D, G, cum, o_tot);
        NHP_HIP(ctx, hipGetLastError());
    }
    if (host_out) {
        if (at_events && M > 0) NHP_TRY(nhp_download(ctx, at_events, o_at, 8 * M));
        if (residuals && M > 0) NHP_TRY(nhp_download(ctx, residuals, o_res, 8 * M));
        if (total) NHP_TRY(nhp_download(ctx, total, o_tot, 8 * N));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    return NHP_OK;
}
