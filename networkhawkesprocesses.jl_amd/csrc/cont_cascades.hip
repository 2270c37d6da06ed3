// Most likely parents and the cascades a parent assignment forms (no counterpart in the reference).
//
// nhp_cont_map_parents.  For event i the categories are those of the parent sampler, in its order: the events i-1, i-2, ...,
// `first` of the look-back window with weight A·W·ħ(t_i - t_j), then the baseline λ0_c(t_i); every weight is evaluated by
// the sampler's own helpers (nhp_samp.h), so the bits are the sampler's.  The posterior mode is the FIRST maximum in that
// order (of equal parent weights the most recent wins, a parent beats the baseline on equality) and prob = w_max / Σw.
// One pass over the window: 8 lanes share a child (one contiguous 128-byte run of event records per child and load
// instruction, as in k_sampler8 / k_comp_events), lane l takes the categories k ≡ l (mod 8) in ascending order and carries
// its partial sum and its running (max, k); a fixed butterfly over the 8 lanes adds the sums and keeps the smaller k on
// equal values, so the tie rule survives and two calls give the same bits.
//
// nhp_cont_cascades.  Any parent vector in the convention of resample_parents / nhp_cont_simulate (0 = immigrant, else the
// 1-based index of an EARLIER event, which rules out cycles) is a forest; its roots are the immigrants.  Pointer doubling,
// O(M log depth): with a_k[i] the ancestor of i at distance min(2^k, generation(i)) and d_k[i] that distance,
//     a_{k+1}[i] = a_k[a_k[i]],  d_{k+1}[i] = d_k[i] + d_k[a_k[i]]        (saturating at the root: d_k[root] = 0)
// converges to (root, generation), and i has an ancestor up_k[i] at distance EXACTLY 2^k iff d_k[i] == 2^k (it is a_k[i]).
// With c_k[j] the number of descendants of j, itself included, at distance < 2^k (c_0 = 1),
//     c_{k+1}[j] = c_k[j] + Σ_{i: up_k[i] = j} c_k[i].
// Round k adds c_k[i] to S_k[up_k[i]] with integer atomics and folds S_{k-1}[i] into c[i] on the way (two S buffers take
// turns; thread i clears the one it has just read), so a round is one kernel.  The rounds stop when no event has an
// up-pointer left (one flag read per round): ⌈log2(depth + 1)⌉ rounds.  Cascades are compacted by a flag and an exclusive
// scan over the events; their depth and end are atomicMax (the end on the time's bit pattern: non-negative doubles order
// as unsigned integers), the per-node tables atomicAdd on 64-bit integers.  Integer atomics only, so every output is
// identical from run to run.  Lanes of a wave that hit the same address (a star's hub, the diagonal of `reach` at small
// N) are combined before the atomic (casc_combine).
#include "nhp_samp.h"

// ---- most likely parents ----------------------------------------------------------------------------------------------
// CACHED: logit-normal impulses through the dataset's pair cache (the data half of every pdf, made once: the same bits)
template <int IMP, bool CACHED>
__global__ __launch_bounds__(NHP_BLOCK) void k_map8(nhp_cont_args a, int64_t *__restrict__ parents, int64_t *__restrict__ pnodes,
                                                    double *__restrict__ prob, int *__restrict__ err)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    double2 *col = reinterpret_cast<double2 *>(smem);
    double *colw = reinterpret_cast<double *>(col + a.N);
    const nhp_item it = a.items[blockIdx.x];
    const int c = it.node, N = a.N, tid = threadIdx.x, gl = tid & 7, gid = tid >> 3;
    for (int p = tid; p < N; p += NHP_BLOCK) {               // column c of the tables, as k_sampler stages it
        const size_t k = (size_t)p + (size_t)c * N;
        double w = a.W[k];
        if (a.A) w = a.A[k] * w;
        if (IMP == NHP_IMPULSE_EXPONENTIAL) {
            const double scale = 1.0 / a.p1[k];            // Exponential(1/θ) ...
            col[p] = make_double2(1.0 / scale, w);         // ... and its rate inv(scale)
        } else {
            col[p] = make_double2(a.p1[k], __builtin_sqrt(a.p2[k]));
            colw[p] = w;
        }
    }
    __syncthreads();
    const samp_col sc{col, colw};

    const int nchild = it.kend - it.kbeg;
    for (int k0 = 0; k0 < nchild; k0 += NHP_BLOCK / 8) {    // block-uniform trip count; idle groups are masked
        const int kq = k0 + gid;
        const bool live = kq < nchild;
        const int kw = it.kbeg + (live ? kq : 0);
        const nhp_child ch = a.child_w[kw];                 // window-sorted order: the groups of a wave walk windows of similar length
        const int i = ch.idx;
        const double t = ch.t;
        const int n = (live && i > 0) ? i - ch.first + 1 : 0;           // categories; the first event has none: (0, 0), prob 1
        const double base = n > 0 ? samp_baseline(a, c, t) : 0.0;
        const double2 *lq = CACHED ? a.plq + a.poff[kw] : nullptr;
        const uint16_t *nd = CACHED ? a.pnode + a.poff[kw] : nullptr;
        // category k of the child: k < n-1 -> parent i-1-k, k == n-1 -> baseline
        double s = 0.0, vmax = -1.0;
        int kmax = 0x7fffffff;
        for (int k = gl; k < n; k += 8) {
            double w = base;
            if (k < n - 1) w = CACHED ? samp_weight_cached(sc, lq[k], nd[k]) : samp_weight<IMP>(a, sc, t, i - 1 - k);
            s = s + w;
            if (w > vmax) { vmax = w; kmax = k; }           // strict: the first maximum of the lane's ascending categories
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            s = s + __shfl_xor(s, o);
            const double ov = __shfl_xor(vmax, o);
            const int ok = __shfl_xor(kmax, o);
            if (ov > vmax || (ov == vmax && ok < kmax)) { vmax = ov; kmax = ok; }
        }
        if (live && gl == 0) {
            int parent = -1;
            double pr = 1.0;
            if (n > 0) {
                if (!(s > 0.0) || !(s < __builtin_inf())) *err = 1;
                if (kmax < n - 1) parent = i - 1 - kmax;    // kmax in [0, n-2]: an event of [first, i-1]
                pr = vmax / s;
            }
            if (parents) parents[i] = (int64_t)parent + 1;  // 1-based event index, 0 = baseline
            if (pnodes) pnodes[i] = parent >= 0 ? (int64_t)a.nodes[parent] + 1 : 0;
            if (prob) prob[i] = pr;
        }
    }
}

extern "C" nhp_status nhp_cont_map_parents(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t output_on_device,
                                           int64_t *parents, int64_t *parentnodes, double *prob)
{
    NHP_TRY(nhp_check_pair(ctx, ds, m));
    if (!parents && !parentnodes && !prob) { nhp_set_error(ctx, "map_parents: no output requested"); return NHP_EINVAL; }
    NHP_WHOLE_DATASET(ctx, ds, "map_parents");
    const bool expo = m->impulse_kind == NHP_IMPULSE_EXPONENTIAL;
    const size_t N = (size_t)ds->N, M = (size_t)ds->M;
    const size_t lds = (expo ? 16 : 24) * N;
    if (lds > 160 * 1024) { nhp_set_error(ctx, "map_parents: n_nodes = %d exceeds the 160 KiB LDS column budget", ds->N); return NHP_ENOTIMPL; }
    if (M == 0 || ds->n_items == 0) return NHP_OK;
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    int64_t *o_par = parents, *o_pno = parentnodes;
    double *o_prob = prob;
    if (!output_on_device) {
        NHP_TRY(nhp_ctx_reserve_scratch(ctx, 3 * 8 * M));
        int64_t *b = (int64_t *)ctx->d_scratch;
        if (parents) o_par = b;
        if (parentnodes) o_pno = b + M;
        if (prob) o_prob = (double *)(b + 2 * M);
    }
    nhp_cont_args a = nhp_make_args(ds, m);
    if (!expo) (void)nhp_ensure_pair_cache(ctx, ds, &a);            // (no cache: the whole pdf per pair -- the same bits)
    NHP_HIP(ctx, hipMemsetAsync(ctx->d_err, 0, sizeof(int), st));
    const auto fn = expo ? k_map8<NHP_IMPULSE_EXPONENTIAL, false>
                         : (a.plq ? k_map8<NHP_IMPULSE_LOGITNORMAL, true> : k_map8<NHP_IMPULSE_LOGITNORMAL, false>);
    if (lds > 64 * 1024) NHP_HIP(ctx, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)ds->n_items), dim3(NHP_BLOCK), lds, st, a, o_par, o_pno, o_prob, ctx->d_err);
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipMemcpyAsync(ctx->h_err, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    if (*ctx->h_err) {
        *ctx->h_err = 0;
        nhp_set_error(ctx, "map_parents: weights of some event do not sum to a positive finite value");
        return NHP_EDOMAIN;
    }
    if (!output_on_device) {
        if (parents) NHP_TRY(nhp_download(ctx, parents, o_par, 8 * M));
        if (parentnodes) NHP_TRY(nhp_download(ctx, parentnodes, o_pno, 8 * M));
        if (prob) NHP_TRY(nhp_download(ctx, prob, o_prob, 8 * M));
    }
    return NHP_OK;
}

// ---- cascades -----------------------------------------------------------------------------------------------------------
#define CASC_BLOCK 256
#define CASC_HUBS 4          // hub targets combined per call before the remaining lanes issue their own atomics
#define CASC_MAX_ROUNDS 31   // d < 2^31
enum { CASC_ADD = 0, CASC_MAX = 1 };
typedef unsigned long long casc_u64;

// op(base[target], v) for every lane with target >= 0; EVERY lane of the wave calls it.  While the first pending lane
// shares its target with others (a hub), those lanes are reduced in the wave and issue one atomic between them.
template <int OP, typename T>
__device__ __forceinline__ void casc_combine(T *__restrict__ base, long long target, T v)
{
    const int lane = threadIdx.x & 63;
    bool pend = target >= 0;
    for (int r = 0; r < CASC_HUBS; ++r) {
        const casc_u64 m = __ballot(pend);
        if (!m) return;                                     // wave-uniform
        const int lead = __ffsll((long long)m) - 1;
        const long long t0 = __shfl(target, lead);
        const bool mine = pend && target == t0;
        if (__popcll(__ballot(mine)) == 1) break;           // nobody shares the leader's target: no hub in sight
        T x = mine ? v : (T)0;                              // values are non-negative: 0 is neutral for both operations
        for (int o = 32; o > 0; o >>= 1) {
            const T y = __shfl_xor(x, o);
            x = OP == CASC_ADD ? x + y : (y > x ? y : x);
        }
        if (lane == lead) { if (OP == CASC_ADD) atomicAdd(base + t0, x); else atomicMax(base + t0, x); }
        pend = pend && !mine;
    }
    if (pend) { if (OP == CASC_ADD) atomicAdd(base + target, v); else atomicMax(base + target, v); }
}

// flags[0]: some parents[k] is neither 0 nor the index of an earlier event; flags[1 + k]: round k has an up-pointer
__global__ __launch_bounds__(CASC_BLOCK) void k_casc_check(const int64_t *__restrict__ parents, int64_t M, int2 *__restrict__ ad,
                                                           int *__restrict__ c, int *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * CASC_BLOCK + threadIdx.x;
    if (i >= M) return;
    const int64_t p = parents[i];
    if (p < 0 || p > i) { flags[0] = 1; return; }           // 1 <= p <= i (0-based i): strictly earlier
    ad[i] = p ? make_int2((int)(p - 1), 1) : make_int2((int)i, 0);
    c[i] = 1;
    if (p) flags[1] = 1;
}

__global__ __launch_bounds__(CASC_BLOCK) void k_casc_round(int64_t M, int k, const int2 *__restrict__ ad, int2 *__restrict__ adn,
                                                           int *__restrict__ c, int *__restrict__ s_prev, int *__restrict__ s_cur,
                                                           int *__restrict__ flag_next)
{
    const int64_t i = (int64_t)blockIdx.x * CASC_BLOCK + threadIdx.x;
    long long target = -1;
    int ci = 0;
    if (i < M) {
        const int2 x = ad[i];
        const int2 y = ad[x.x];
        const int2 nx = make_int2(y.x, x.y + y.y);
        adn[i] = nx;
        ci = c[i] + s_prev[i];                              // c_k = c_{k-1} + S_{k-1}
        c[i] = ci;
        s_prev[i] = 0;                                      // ... which becomes S_{k+1}
        if ((unsigned)x.y == (1u << k)) target = x.x;       // up_k[i]
        if ((unsigned)nx.y == (2u << k)) *flag_next = 1;
    }
    casc_combine<CASC_ADD, int>(s_cur, target, ci);
}

// immigrants of each block of CASC_BLOCK events
__global__ __launch_bounds__(CASC_BLOCK) void k_casc_count(int64_t M, const int2 *__restrict__ ad, int *__restrict__ blk)
{
    __shared__ int red[CASC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * CASC_BLOCK + threadIdx.x;
    const casc_u64 b = __ballot(i < M && ad[i].y == 0);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive prefix of blk[0 .. nb) in place (one workgroup: every thread a contiguous run); *total = the sum
__global__ __launch_bounds__(CASC_BLOCK) void k_casc_scan_blocks(int *__restrict__ blk, int64_t nb, int64_t *__restrict__ total)
{
    __shared__ long long part[CASC_BLOCK];
    const int64_t per = (nb + CASC_BLOCK - 1) / CASC_BLOCK;
    const int64_t j0 = per * threadIdx.x < nb ? per * threadIdx.x : nb, j1 = j0 + per < nb ? j0 + per : nb;
    long long sum = 0;
    for (int64_t j = j0; j < j1; ++j) sum += blk[j];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int w = 0; w < CASC_BLOCK; ++w) { const long long v = part[w]; part[w] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    int run = (int)part[threadIdx.x];
    for (int64_t j = j0; j < j1; ++j) { const int v = blk[j]; blk[j] = run; run += v; }
}

// rank[i] = number of immigrants before i (for immigrants: their cascade); the cascade's root and size, depth and end cleared
__global__ __launch_bounds__(CASC_BLOCK) void k_casc_rank(int64_t M, const int2 *__restrict__ ad, const int *__restrict__ c,
                                                          const int *__restrict__ s_last, const int *__restrict__ blk,
                                                          int *__restrict__ rank, int64_t *__restrict__ casc_root,
                                                          int64_t *__restrict__ casc_size, casc_u64 *__restrict__ casc_depth,
                                                          casc_u64 *__restrict__ casc_end)
{
    __shared__ int red[CASC_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * CASC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool isroot = i < M && ad[i].y == 0;
    const casc_u64 b = __ballot(isroot);
    if (lane == 0) red[wave] = __popcll(b);
    __syncthreads();
    if (!isroot) return;
    int r = blk[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) r += red[w];
    rank[i] = r;
    casc_root[r] = i + 1;
    casc_size[r] = (int64_t)c[i] + s_last[i];
    casc_depth[r] = 0;
    casc_end[r] = 0;
}

__global__ __launch_bounds__(CASC_BLOCK) void k_casc_finish(int64_t M, int N, const int2 *__restrict__ ad, const int *__restrict__ c,
                                                            const int *__restrict__ s_last, const int *__restrict__ rank,
                                                            const double *__restrict__ times, const int32_t *__restrict__ nodes,
                                                            int64_t *__restrict__ root, int64_t *__restrict__ generation,
                                                            int64_t *__restrict__ descendants, casc_u64 *__restrict__ casc_depth,
                                                            casc_u64 *__restrict__ casc_end, casc_u64 *__restrict__ immigrants,
                                                            casc_u64 *__restrict__ offspring, casc_u64 *__restrict__ reach)
{
    const int64_t i = (int64_t)blockIdx.x * CASC_BLOCK + threadIdx.x;
    const bool live = i < M;
    int r = 0, gen = 0, cn = 0;
    long long desc = 0;
    if (live) {
        const int2 x = ad[i];
        r = x.x; gen = x.y;
        desc = (long long)c[i] + s_last[i] - 1;
        cn = nodes[i];
        if (root) root[i] = (int64_t)r + 1;
        if (generation) generation[i] = gen;
        if (descendants) descendants[i] = desc;
    }
    if (casc_depth) {                                       // (kernel-uniform branches: every lane reaches the combines)
        const long long rk = live ? rank[r] : -1;
        casc_combine<CASC_MAX, casc_u64>(casc_depth, rk, (casc_u64)gen);
        casc_combine<CASC_MAX, casc_u64>(casc_end, rk, live ? (casc_u64)__double_as_longlong(times[i] + 0.0) : 0ull);
    }
    if (immigrants) casc_combine<CASC_ADD, casc_u64>(immigrants, live && r == i ? cn : -1, 1ull);
    if (offspring) casc_combine<CASC_ADD, casc_u64>(offspring, live && desc > 0 ? cn : -1, (casc_u64)desc);
    if (reach) casc_combine<CASC_ADD, casc_u64>(reach, live ? (long long)nodes[r] + (long long)cn * N : -1, 1ull);
}

extern "C" nhp_status nhp_cont_cascades(nhp_ctx *ctx, const nhp_cont_dataset *ds, const int64_t *parents, int32_t parents_on_device,
                                        int32_t output_on_device, int64_t *root, int64_t *generation, int64_t *descendants,
                                        int64_t *casc_root, int64_t *casc_size, int64_t *casc_depth, double *casc_end,
                                        int64_t *n_cascades, int64_t *immigrants, int64_t *offspring, int64_t *reach, int32_t *n_rounds)
{
    if (!ctx || !ds) return NHP_EINVAL;
    if (ds->ctx != ctx) { nhp_set_error(ctx, "dataset belongs to another ctx"); return NHP_EINVAL; }
    const int n_casc_out = (casc_root != nullptr) + (casc_size != nullptr) + (casc_depth != nullptr) + (casc_end != nullptr);
    if (n_casc_out != 0 && n_casc_out != 4) { nhp_set_error(ctx, "cascades: casc_root, casc_size, casc_depth and casc_end come together or not at all"); return NHP_EINVAL; }
    if (!parents && ds->M > 0) { nhp_set_error(ctx, "cascades: parents is NULL"); return NHP_EINVAL; }
    NHP_WHOLE_DATASET(ctx, ds, "cascades");
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const size_t M = (size_t)ds->M, N = (size_t)ds->N, NN = N * N, Mp = M ? M : 1;
    const bool casc = n_casc_out == 4, host_out = !output_on_device;
    const size_t nb = (Mp + CASC_BLOCK - 1) / CASC_BLOCK;

    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t r = off; off += (bytes + 255) & ~(size_t)255; return r; };
    const size_t o_ad0 = carve(8 * Mp), o_ad1 = carve(8 * Mp), o_c = carve(4 * Mp), o_s = carve(2 * 4 * Mp), o_rank = carve(4 * Mp);
    const size_t o_blk = carve(4 * nb), o_flags = carve(4 * 64), o_total = carve(8);
    const size_t o_par = carve(parents_on_device ? 0 : 8 * Mp);
    const size_t o_ev = carve(host_out ? 3 * 8 * Mp : 0), o_cs = carve(host_out && casc ? 4 * 8 * Mp : 0);
    const size_t o_nd = carve(host_out ? 8 * (2 * N + NN) : 0);
    NHP_TRY(nhp_ctx_reserve_scratch(ctx, off));
    char *base = (char *)ctx->d_scratch;
    int2 *ad[2] = {(int2 *)(base + o_ad0), (int2 *)(base + o_ad1)};
    int *c = (int *)(base + o_c), *s[2] = {(int *)(base + o_s), (int *)(base + o_s) + Mp}, *rank = (int *)(base + o_rank);
    int *blk = (int *)(base + o_blk), *flags = (int *)(base + o_flags);
    int64_t *d_total = (int64_t *)(base + o_total);
    // where the kernels write: the caller's device memory, or device twins of the requested host outputs
    void *const h_out[10] = {root, generation, descendants, casc_root, casc_size, casc_depth, casc_end, immigrants, offspring, reach};
    if (host_out) {
        int64_t *e = (int64_t *)(base + o_ev), *q = (int64_t *)(base + o_cs), *nd = (int64_t *)(base + o_nd);
        if (root) root = e;
        if (generation) generation = e + Mp;
        if (descendants) descendants = e + 2 * Mp;
        if (casc) { casc_root = q; casc_size = q + Mp; casc_depth = q + 2 * Mp; casc_end = (double *)(q + 3 * Mp); }
        if (immigrants) immigrants = nd;
        if (offspring) offspring = nd + N;
        if (reach) reach = nd + 2 * N;
    }
    const void *const d_out[10] = {root, generation, descendants, casc_root, casc_size, casc_depth, casc_end, immigrants, offspring, reach};

    int rounds = 0;
    int64_t total = 0;
    const unsigned grid = (unsigned)nb;
    if (M > 0) {
        const int64_t *d_par = parents;
        if (!parents_on_device) {
            NHP_HIP(ctx, hipMemcpyAsync(base + o_par, parents, 8 * M, hipMemcpyHostToDevice, st));
            d_par = (const int64_t *)(base + o_par);
        }
        NHP_HIP(ctx, hipMemsetAsync(flags, 0, 4 * 64, st));
        NHP_HIP(ctx, hipMemsetAsync(s[0], 0, 2 * 4 * Mp, st));
        hipLaunchKernelGGL(k_casc_check, dim3(grid), dim3(CASC_BLOCK), 0, st, d_par, (int64_t)M, ad[0], c, flags);
        NHP_HIP(ctx, hipGetLastError());
        int h[2] = {0, 0};
        NHP_TRY(nhp_download(ctx, h, flags, sizeof(h)));
        if (h[0]) { nhp_set_error(ctx, "parents[k] must be 0 or the index of an earlier event"); return NHP_EDOMAIN; }
        int active = h[1];
        while (active && rounds < CASC_MAX_ROUNDS) {
            const int k = rounds;
            hipLaunchKernelGGL(k_casc_round, dim3(grid), dim3(CASC_BLOCK), 0, st, (int64_t)M, k, ad[k & 1], ad[(k + 1) & 1], c,
                               s[(k + 1) & 1], s[k & 1], flags + 2 + k);
            NHP_HIP(ctx, hipGetLastError());
            ++rounds;
            NHP_TRY(nhp_download(ctx, &active, flags + 2 + k, sizeof(int)));
        }
    }
    const int2 *adf = ad[rounds & 1];
    const int *s_last = s[(rounds + 1) & 1];                // S of the last round (rounds = 0: a buffer of zeros)
    if (immigrants) NHP_HIP(ctx, hipMemsetAsync(immigrants, 0, 8 * N, st));
    if (offspring) NHP_HIP(ctx, hipMemsetAsync(offspring, 0, 8 * N, st));
    if (reach) NHP_HIP(ctx, hipMemsetAsync(reach, 0, 8 * NN, st));
    if (M > 0) {
        hipLaunchKernelGGL(k_casc_count, dim3(grid), dim3(CASC_BLOCK), 0, st, (int64_t)M, adf, blk);
        hipLaunchKernelGGL(k_casc_scan_blocks, dim3(1), dim3(CASC_BLOCK), 0, st, blk, (int64_t)nb, d_total);
        if (casc)
            hipLaunchKernelGGL(k_casc_rank, dim3(grid), dim3(CASC_BLOCK), 0, st, (int64_t)M, adf, (const int *)c, s_last, (const int *)blk, rank,
                               casc_root, casc_size, (casc_u64 *)casc_depth, (casc_u64 *)casc_end);
        hipLaunchKernelGGL(k_casc_finish, dim3(grid), dim3(CASC_BLOCK), 0, st, (int64_t)M, (int)N, adf, (const int *)c, s_last, (const int *)rank,
                           (const double *)ds->d_times, (const int32_t *)ds->d_nodes, root, generation, descendants,
                           (casc_u64 *)(casc ? casc_depth : nullptr), (casc_u64 *)(casc ? casc_end : nullptr), (casc_u64 *)immigrants,
                           (casc_u64 *)offspring, (casc_u64 *)reach);
        NHP_HIP(ctx, hipGetLastError());
        NHP_TRY(nhp_download(ctx, &total, d_total, 8));
    }
    if (host_out) {
        const size_t len[10] = {M, M, M, (size_t)total, (size_t)total, (size_t)total, (size_t)total, N, N, NN};
        for (int j = 0; j < 10; ++j)
            if (h_out[j] && len[j]) NHP_TRY(nhp_download(ctx, h_out[j], d_out[j], 8 * len[j]));
    }
    NHP_HIP(ctx, hipStreamSynchronize(st));
    if (n_cascades) *n_cascades = total;
    if (n_rounds) *n_rounds = rounds;
    return NHP_OK;
}
