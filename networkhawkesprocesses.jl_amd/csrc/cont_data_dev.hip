// Continuous datasets built on the device: nhp_cont_dataset_create_device.
//
// The pre-pass of nhp_cont_dataset_create_columns (cont_data.hip) is integer bookkeeping and exact fp64 comparisons
// over sorted data.  Here it runs as binary searches, scans and one stable LSD radix sort (the node bucketing and the
// window-length sort are the same primitive); only the work partition is decided on the host, by the function the
// host route calls (nhp_cont_partition).  Every array comes out byte for byte equal to the host route's, so every
// kernel downstream runs on it unchanged.
//
// Two synchronisations: after the per-event pass and the node bucketing (the bucket offsets, the pair offsets per node,
// the validation result and a few scalars come back for the partition), and at the end.
#include <chrono>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>

#include "nhp_dd.h"                      // scans, the radix sort, the scratch arena

#define DD_SORTED 0x80000000u            // window-sort segment: sorted by window length (else kept in place)

// scalars of the per-event pass (integers: the reductions do not depend on the order of the atomics)
struct dd_scal {
    int32_t bad;                         // first event failing validation (M: none)
    int32_t max_window;
    int32_t n_zero;                      // first event whose time is not exactly 0.0 (M: none)
    int32_t max_rows;                    // longest window of any child slice
    unsigned long long rows;             // rows of all child slices
    double t0, t1;                       // first and last time
};

// ---- the pre-pass ---------------------------------------------------------------------------------------------------

__global__ void k_dd_init(dd_scal *sc, int64_t M)
{
    sc->bad = (int32_t)M; sc->max_window = 0; sc->n_zero = (int32_t)M; sc->max_rows = 0; sc->rows = 0;
    sc->t0 = 0.0; sc->t1 = 0.0;
}

// validation flags, the window start of every event (the host's look-back pointer as a binary search: on sorted times
// `events[f] > t_i - dt_max` is false then true over f), 0-based nodes (clamped into range, so that nothing below
// indexes outside its arrays before the validation result is looked at), and the per-event reductions.
// TR (a dataset of several trials; the one-recording build instantiates the kernel without it): the event's
// trial r = the last one starting at or before it (trial_f: R + 1 event offsets, checked on the host: 0 .. M, non-decreasing),
// the event has to lie inside [trial_o[r], trial_o[r + 1]] and its window search starts at trial_f[r].
template <bool TR>
__global__ void __launch_bounds__(DD_BLOCK) k_dd_events(const double *__restrict__ t, const int64_t *__restrict__ nodes, int64_t M,
                                                        int32_t N, double dt_max, uint32_t *__restrict__ node32,
                                                        int32_t *__restrict__ first, dd_scal *__restrict__ sc,
                                                        const int32_t *__restrict__ trial_f, const double *__restrict__ trial_o, int32_t R)
{
    const int64_t i = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    int bad = INT_MAX, maxw = 0, nz = INT_MAX;
    if (i < M) {
        const double ti = t[i];
        const int64_t nd = nodes[i];
        const double tp = i > 0 ? t[i - 1] : ti;
        bool fails = (nd < 1) | (nd > N) | !(ti >= 0.0) | (ti < tp);            // (no short circuit: one select)
        int32_t fr = 0;
        if (TR) {
            int32_t a = 0, b = R;                                               // last r in [0, R) with trial_f[r] <= i
            while (b - a > 1) { const int32_t mid = (a + b) >> 1; if ((int64_t)trial_f[mid] <= i) a = mid; else b = mid; }
            fr = trial_f[a];
            fails |= !((ti >= trial_o[a]) & (ti <= trial_o[a + 1]));
        }
        bad = fails ? (int)i : INT_MAX;
        node32[i] = (uint32_t)(nd < 1 ? 0 : (nd > N ? N - 1 : nd - 1));
        const double thr = ti - dt_max;
        int32_t lo = fr, hi = (int32_t)i;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (t[mid] > thr) hi = mid; else lo = mid + 1;
        }
        first[i] = lo;
        maxw = (int32_t)i - lo;
        if (!(ti == 0.0)) nz = (int)i;
        if (i == 0) sc->t0 = ti;
        if (i == M - 1) sc->t1 = ti;
    }
    for (int o = 32; o > 0; o >>= 1) {
        bad = min(bad, __shfl_xor(bad, o, 64));
        maxw = max(maxw, __shfl_xor(maxw, o, 64));
        nz = min(nz, __shfl_xor(nz, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad != INT_MAX) atomicMin(&sc->bad, bad);
        if (maxw) atomicMax(&sc->max_window, maxw);
        if (nz != INT_MAX) atomicMin(&sc->n_zero, nz);
    }
}

// trial_g[r] = the first index in [trial_f[r], trial_f[r + 1]] whose time is above trial_o[r] (sorted times inside the trial)
__global__ void k_dd_trial_g(const double *__restrict__ t, const int32_t *__restrict__ trial_f, const double *__restrict__ trial_o,
                             int32_t R, int32_t *__restrict__ trial_g)
{
    const int32_t r = (int32_t)(blockIdx.x * DD_BLOCK + threadIdx.x);
    if (r >= R) return;
    const double o = trial_o[r];
    int32_t lo = trial_f[r], hi = trial_f[r + 1];
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (t[mid] > o) hi = mid; else lo = mid + 1; }
    trial_g[r] = lo;
}

// child records in bucket order and their window lengths
__global__ void k_dd_child(const double *__restrict__ t, const int32_t *__restrict__ first, const int32_t *__restrict__ perm, int64_t M,
                           nhp_child *__restrict__ child, int64_t *__restrict__ len)
{
    const int64_t k = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (k >= M) return;
    const int32_t i = perm[k], f = first[i];
    nhp_child r;
    r.t = t[i]; r.first = f; r.idx = i;
    child[k] = r;
    len[k] = (int64_t)(i - f);
}

// bucket offsets from the sorted node keys: boff[c] = first position whose node is >= c
__global__ void k_dd_boff(const uint32_t *__restrict__ key, int64_t M, int32_t N, int32_t *__restrict__ boff)
{
    const int64_t k = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (k > M) return;
    const int64_t prev = k > 0 ? (int64_t)key[k - 1] : -1, cur = k < M ? (int64_t)key[k] : (int64_t)N;
    for (int64_t c = prev + 1; c <= cur; ++c) boff[c] = (int32_t)k;
}

// pair offsets per node (the prefix of the window lengths in bucket order, at each bucket's start) and, where the XCD
// layout may cut nodes into time parts, the bucket position of each node's first child at or after M*j/8, j = 0..8
// (the time-part bounds for TP = 2, 4, 8: M*s/TP = M*(8s/TP)/8 exactly)
__global__ void k_dd_node_tables(const int32_t *__restrict__ boff, const int64_t *__restrict__ lscan, const nhp_child *__restrict__ child,
                                 int64_t M, int32_t N, int64_t *__restrict__ pair_off, int32_t *__restrict__ bounds)
{
    const int64_t x = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (x <= N) pair_off[x] = lscan[boff[x]];
    if (!bounds || x >= (int64_t)N * 9) return;
    const int32_t c = (int32_t)(x / 9), j = (int32_t)(x % 9);
    const int64_t bound = M * j / 8;
    int32_t lo = boff[c], hi = boff[c + 1];
    while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (child[mid].idx < bound) lo = mid + 1; else hi = mid; }
    bounds[x] = lo;
}

// window-sort keys: (segment, longest first) -- a segment is an item (NHP_SORT=2), a round of one (=1) or a stretch of
// bucket positions outside every item (a column shard's other nodes), which keeps its order
__global__ void k_dd_wkey(const uint32_t *__restrict__ seg, int32_t nseg, const int64_t *__restrict__ len, int64_t M, int32_t maxw,
                          uint64_t *__restrict__ key)
{
    const int64_t k = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (k >= M) return;
    int32_t lo = 0, hi = nseg;                  // last segment starting at or before k
    while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if ((int64_t)(seg[mid] & ~DD_SORTED) <= k) lo = mid; else hi = mid; }
    const uint64_t w = (seg[lo] & DD_SORTED) ? (uint64_t)(maxw - len[k]) : 0;
    key[k] = (uint64_t)lo * (uint64_t)(maxw + 1) + w;
}

__global__ void k_dd_child_w(const nhp_child *__restrict__ child, const int32_t *__restrict__ wpos, int64_t M,
                             nhp_child *__restrict__ child_w, uint32_t *__restrict__ wlen)
{
    const int64_t k = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (k >= M) return;
    const nhp_child r = child[wpos[k]];
    child_w[k] = r;
    wlen[k] = (uint32_t)(r.idx - r.first);
}

// rows of each child slice = the longest window of its 64 children
__global__ void __launch_bounds__(DD_BLOCK) k_dd_slice_rows(const nhp_item *__restrict__ items, const int32_t *__restrict__ sl_item0,
                                                            int32_t n_items, int32_t n_slices, const uint32_t *__restrict__ wlen,
                                                            uint32_t *__restrict__ longest, dd_scal *__restrict__ sc)
{
    const int64_t j = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    uint32_t best = 0;
    if (j < n_slices) {
        int32_t lo = 0, hi = n_items;           // the item holding slice j: last q with sl_item0[q] <= j
        while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if (sl_item0[mid] <= j) lo = mid; else hi = mid; }
        const nhp_item it = items[lo];
        const int32_t k0 = it.kbeg + 64 * (int32_t)(j - sl_item0[lo]), k1 = min(k0 + 64, it.kend);
        for (int32_t k = k0; k < k1; ++k) best = max(best, wlen[k]);
        longest[j] = best;
    }
    unsigned long long rows = best;
    uint32_t mx = best;
    for (int o = 32; o > 0; o >>= 1) {
        rows += __shfl_xor(rows, o, 64);
        mx = max(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && rows) {
        atomicAdd(&sc->rows, rows);
        atomicMax(&sc->max_rows, (int32_t)mx);
    }
}

// 16-byte and 8-byte event records (cont_data.hip: the same clamp and rounding)
__global__ void k_dd_records(const double *__restrict__ t, const uint32_t *__restrict__ node32, int64_t M, double t0, double scale,
                             nhp_event *__restrict__ ev, uint64_t *__restrict__ ev8)
{
    const int64_t i = (int64_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (i >= M) return;
    const double ti = t[i];
    const uint32_t c = node32[i];
    nhp_event e;
    e.t = ti; e.node = (int32_t)c; e.pad = 0;
    ev[i] = e;
    if (ev8) {
        double q = rint((ti - t0) * scale);
        if (q < 0.0) q = 0.0;
        if (q > 281474976710655.0) q = 281474976710655.0;
        ev8[i] = ((uint64_t)c << 48) | (uint64_t)q;
    }
}

template <typename T>
static hipError_t dd_alloc(T **p, int64_t n) { return hipMalloc((void **)p, sizeof(T) * (size_t)std::max<int64_t>(n, 1)); }

static nhp_status dd_create(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t M, int32_t N, double dt_max,
                            bool on_device, nhp_cont_dataset *ds, const int64_t *trial_f = nullptr, const double *trial_o = nullptr,
                            int32_t R = 1)
{
    static const bool timing = getenv("NHP_TIMING") && atoi(getenv("NHP_TIMING")) != 0;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[nhp dataset, device] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    hipStream_t st = ctx->main();
    const unsigned gM = dd_grid(M, DD_BLOCK);
    const unsigned ntM = dd_grid(M, DD_TILE);
    const bool want_bounds = N >= 8 && M >= 16 * (int64_t)N;    // the XCD layout's time parts are possible

    // ---- phase 1: per-event pass, node bucketing, per-node tables
    dd_arena a1;
    a1.st = st;
    int64_t *d_nodes64 = nullptr, *d_len = nullptr, *d_lscan = nullptr, *d_pair_off = nullptr, *d_tmp64 = nullptr;
    int32_t *d_first = nullptr, *d_bounds = nullptr;
    uint32_t *d_key = nullptr;
    dd_scal *d_sc = nullptr;
    dd_sort_buf<uint32_t> nb;
    if (!on_device) a1.ask(&d_nodes64, M);
    a1.ask(&d_first, M); a1.ask(&d_key, M); a1.ask(&nb.k2, M); a1.ask(&nb.v1, M); a1.ask(&nb.v2, M);
    a1.ask(&nb.hist, (int64_t)DD_RADIX * ntM); a1.ask(&nb.offs, (int64_t)DD_RADIX * ntM + 1);
    a1.ask(&nb.tmp, dd_grid((int64_t)DD_RADIX * ntM, DD_TILE));
    a1.ask(&d_len, M); a1.ask(&d_lscan, M + 1); a1.ask(&d_tmp64, ntM); a1.ask(&d_pair_off, (int64_t)N + 1); a1.ask(&d_sc, 1);
    if (want_bounds) a1.ask(&d_bounds, (int64_t)N * 9);
    NHP_HIP(ctx, a1.alloc());
    NHP_HIP(ctx, dd_alloc(&ds->d_times, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_nodes, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_child, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_boff, (int64_t)N + 1));
    if (M > 0) {
        NHP_HIP(ctx, hipMemcpyAsync(ds->d_times, events, sizeof(double) * M, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (!on_device) NHP_HIP(ctx, hipMemcpyAsync(d_nodes64, nodes, sizeof(int64_t) * M, hipMemcpyHostToDevice, st));
    }
    const int64_t *d_in_nodes = on_device ? nodes : d_nodes64;
    lap("allocation + upload (enqueued)");

    k_dd_init<<<1, 1, 0, st>>>(d_sc, M);
    const bool trials = trial_f != nullptr;       // (one trial too: its events are held to [0, T])
    std::vector<int32_t> f32;
    if (trials) {                             // the tables first: the per-event pass reads them
        f32.resize((size_t)R + 1);
        for (int32_t r = 0; r <= R; ++r) f32[(size_t)r] = (int32_t)trial_f[r];
        NHP_HIP(ctx, dd_alloc(&ds->d_trial_f, (int64_t)R + 1));
        NHP_HIP(ctx, dd_alloc(&ds->d_trial_o, (int64_t)R + 1));
        NHP_HIP(ctx, dd_alloc(&ds->d_trial_g, (int64_t)R));
        NHP_HIP(ctx, hipMemcpyAsync(ds->d_trial_f, f32.data(), sizeof(int32_t) * ((size_t)R + 1), hipMemcpyHostToDevice, st));
        NHP_HIP(ctx, hipMemcpyAsync(ds->d_trial_o, trial_o, sizeof(double) * ((size_t)R + 1), hipMemcpyHostToDevice, st));
    }
    if (M > 0 && trials)
        k_dd_events<true><<<gM, DD_BLOCK, 0, st>>>(ds->d_times, d_in_nodes, M, N, dt_max, (uint32_t *)ds->d_nodes, d_first, d_sc, ds->d_trial_f,
                                                   ds->d_trial_o, R);
    else if (M > 0)
        k_dd_events<false><<<gM, DD_BLOCK, 0, st>>>(ds->d_times, d_in_nodes, M, N, dt_max, (uint32_t *)ds->d_nodes, d_first, d_sc, nullptr,
                                                    nullptr, 1);
    std::vector<int32_t> g32(trials ? (size_t)R : 0);
    if (trials) {
        k_dd_trial_g<<<dd_grid(R, DD_BLOCK), DD_BLOCK, 0, st>>>(ds->d_times, ds->d_trial_f, ds->d_trial_o, R, ds->d_trial_g);
        NHP_HIP(ctx, hipMemcpyAsync(g32.data(), ds->d_trial_g, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, st));
    }
    // node bucketing: stable radix sort of the 0-based nodes (d_nodes is kept: the sort works on a copy)
    uint32_t *k_sorted = nullptr;
    int32_t *perm = nullptr;
    if (M > 0) NHP_HIP(ctx, hipMemcpyAsync(d_key, ds->d_nodes, sizeof(uint32_t) * M, hipMemcpyDeviceToDevice, st));
    dd_sort<uint32_t>(st, d_key, M, dd_bitlen((uint64_t)(N - 1)), nb, &k_sorted, &perm);
    if (M > 0) k_dd_child<<<gM, DD_BLOCK, 0, st>>>(ds->d_times, d_first, perm, M, ds->d_child, d_len);
    k_dd_boff<<<dd_grid(M + 1, DD_BLOCK), DD_BLOCK, 0, st>>>(k_sorted, M, N, ds->d_boff);
    dd_scan<int64_t>(st, d_len, d_lscan, M, d_tmp64);
    const int64_t nx = want_bounds ? (int64_t)N * 9 : (int64_t)N + 1;
    k_dd_node_tables<<<dd_grid(std::max<int64_t>(nx, (int64_t)N + 1), DD_BLOCK), DD_BLOCK, 0, st>>>(ds->d_boff, d_lscan, ds->d_child, M, N,
                                                                                                   d_pair_off, d_bounds);
    NHP_HIP(ctx, hipGetLastError());
    dd_scal sc;
    std::vector<int32_t> bounds(want_bounds ? (size_t)N * 9 : 0);
    ds->h_boff.resize((size_t)N + 1);
    ds->h_pair_off.resize((size_t)N + 1);
    NHP_HIP(ctx, hipMemcpyAsync(&sc, d_sc, sizeof(sc), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipMemcpyAsync(ds->h_boff.data(), ds->d_boff, sizeof(int32_t) * (N + 1), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipMemcpyAsync(ds->h_pair_off.data(), d_pair_off, sizeof(int64_t) * (N + 1), hipMemcpyDeviceToHost, st));
    if (want_bounds) NHP_HIP(ctx, hipMemcpyAsync(bounds.data(), d_bounds, sizeof(int32_t) * bounds.size(), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    lap("per-event pass + bucketing");

    if (sc.bad < M) {          // the host route's message: its checks in its order at the first failing event
        const int64_t i = sc.bad;
        double ti = 0.0, tp = 0.0;
        int64_t nd = 0;
        NHP_HIP(ctx, hipMemcpy(&ti, ds->d_times + i, sizeof(double), hipMemcpyDeviceToHost));
        if (i > 0) NHP_HIP(ctx, hipMemcpy(&tp, ds->d_times + i - 1, sizeof(double), hipMemcpyDeviceToHost));
        NHP_HIP(ctx, hipMemcpy(&nd, d_in_nodes + i, sizeof(int64_t), hipMemcpyDeviceToHost));
        if (nd < 1 || nd > N) {
            nhp_set_error(ctx, "node id %lld at event %lld outside 1..%d", (long long)nd, (long long)(i + 1), N);
            return NHP_EDOMAIN;
        }
        if (!(ti >= 0.0)) { nhp_set_error(ctx, "time must be non-negative (event %lld)", (long long)(i + 1)); return NHP_EDOMAIN; }
        if (i > 0 && ti < tp) { nhp_set_error(ctx, "events must be sorted (event %lld)", (long long)(i + 1)); return NHP_EINVAL; }
        if (trials) {
            int32_t r = 0;
            while (r + 1 < R && trial_f[r + 1] <= i) ++r;
            return nhp_cont_trials_bad_event(ctx, i, r, ti, trial_o[r], trial_o[r + 1]);
        }
        nhp_set_error(ctx, "events must be sorted (event %lld)", (long long)(i + 1));
        return NHP_EINVAL;
    }
    ds->pairs = ds->h_pair_off[(size_t)N];
    ds->max_window = sc.max_window;
    ds->n_zero_time = sc.n_zero;
    ds->t_last = M > 0 ? sc.t1 : 0.0;
    ds->h_cnt.resize((size_t)N);
    for (int32_t c = 0; c < N; ++c) ds->h_cnt[(size_t)c] = (double)(ds->h_boff[c + 1] - ds->h_boff[c]);

    nhp_cont_plan plan;
    nhp_cont_partition(ds, [&](int32_t c, int32_t s, int32_t TP) { return bounds[(size_t)c * 9 + (size_t)(s * 8 / TP)]; }, plan);
    const std::vector<nhp_item> &items = plan.items;
    // window-sort segments in bucket order
    std::vector<uint32_t> seg;
    if (plan.sort_mode == 1 || plan.sort_mode == 2) {
        std::vector<std::pair<int32_t, int32_t>> runs;
        for (const nhp_item &it : items)
            if (it.kend > it.kbeg) runs.push_back({it.kbeg, it.kend});
        std::sort(runs.begin(), runs.end());
        int32_t pos = 0;
        for (const auto &r : runs) {
            if (r.first > pos) seg.push_back((uint32_t)pos);
            if (plan.sort_mode == 2) seg.push_back((uint32_t)r.first | DD_SORTED);
            else for (int32_t k = r.first; k < r.second; k += plan.round) seg.push_back((uint32_t)k | DD_SORTED);
            pos = r.second;
        }
        if (pos < M || seg.empty()) seg.push_back((uint32_t)pos);
    }
    // child slices: sl_item0 from the item sizes (64 children a slice)
    std::vector<int32_t> sl_item0;
    int32_t n_slices = 0;
    if (plan.sliced) {
        sl_item0.resize(items.size() + 1);
        for (size_t q = 0; q < items.size(); ++q) {
            sl_item0[q] = n_slices;
            n_slices += (items[q].kend - items[q].kbeg + 63) / 64;
        }
        sl_item0[items.size()] = n_slices;
    }
    double t0 = 0.0, scale = 0.0;
    const bool with_ev8 = M > 0 && nhp_ev8_params(N, M, sc.t0, sc.t1, &t0, &scale);
    lap("partition (host)");

    // ---- phase 2: window sort, child_w, pair offsets, slice rows, records
    dd_arena a2;
    a2.st = st;
    uint64_t *d_wkey = nullptr;
    uint32_t *d_seg = nullptr, *d_wlen = nullptr, *d_longest = nullptr, *d_tmp32 = nullptr;
    dd_sort_buf<uint64_t> wb;
    const bool wsort = !seg.empty() && M > 0;
    if (wsort) {
        a2.ask(&d_wkey, M); a2.ask(&d_seg, (int64_t)seg.size()); a2.ask(&wb.k2, M); a2.ask(&wb.v1, M); a2.ask(&wb.v2, M);
        a2.ask(&wb.hist, (int64_t)DD_RADIX * ntM); a2.ask(&wb.offs, (int64_t)DD_RADIX * ntM + 1);
        a2.ask(&wb.tmp, dd_grid((int64_t)DD_RADIX * ntM, DD_TILE));
    }
    a2.ask(&d_wlen, M); a2.ask(&d_tmp32, dd_grid(std::max<int64_t>(M, n_slices), DD_TILE));
    if (plan.sliced) a2.ask(&d_longest, n_slices);
    NHP_HIP(ctx, a2.alloc());
    NHP_HIP(ctx, dd_alloc(&ds->d_child_w, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_wpos, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_ev, M));
    NHP_HIP(ctx, dd_alloc(&ds->d_items, (int64_t)items.size()));
    NHP_HIP(ctx, dd_alloc(&ds->d_cnt, N));
    if (with_ev8) NHP_HIP(ctx, dd_alloc(&ds->d_ev8, M));
    if (plan.plist) NHP_HIP(ctx, dd_alloc(&ds->d_poff, M + 1));
    if (plan.sliced) {
        NHP_HIP(ctx, dd_alloc(&ds->d_sl_row, (int64_t)n_slices + 1));
        NHP_HIP(ctx, dd_alloc(&ds->d_sl_item0, (int64_t)sl_item0.size()));
    }
    if (hipMalloc((void **)&ds->d_pn, 4 * (size_t)(M ? M : 1)) != hipSuccess) {
        nhp_set_error(ctx, "out of device memory (parent-node buffer)");
        return NHP_ENOMEM;
    }
    if (!items.empty()) NHP_HIP(ctx, hipMemcpyAsync(ds->d_items, items.data(), sizeof(nhp_item) * items.size(), hipMemcpyHostToDevice, st));
    NHP_HIP(ctx, hipMemcpyAsync(ds->d_cnt, ds->h_cnt.data(), sizeof(double) * N, hipMemcpyHostToDevice, st));
    if (plan.sliced) NHP_HIP(ctx, hipMemcpyAsync(ds->d_sl_item0, sl_item0.data(), sizeof(int32_t) * sl_item0.size(), hipMemcpyHostToDevice, st));
    if (wsort) {
        NHP_HIP(ctx, hipMemcpyAsync(d_seg, seg.data(), sizeof(uint32_t) * seg.size(), hipMemcpyHostToDevice, st));
        const int32_t maxw = ds->max_window;
        k_dd_wkey<<<gM, DD_BLOCK, 0, st>>>(d_seg, (int32_t)seg.size(), d_len, M, maxw, d_wkey);
        uint64_t *kd = nullptr;
        int32_t *wpos = nullptr;
        dd_sort<uint64_t>(st, d_wkey, M, dd_bitlen((uint64_t)seg.size() * (uint64_t)(maxw + 1) - 1), wb, &kd, &wpos);
        NHP_HIP(ctx, hipMemcpyAsync(ds->d_wpos, wpos, sizeof(int32_t) * M, hipMemcpyDeviceToDevice, st));
    } else if (M > 0) {
        k_dd_iota<<<gM, DD_BLOCK, 0, st>>>(ds->d_wpos, M);
    }
    if (M > 0) k_dd_child_w<<<gM, DD_BLOCK, 0, st>>>(ds->d_child, ds->d_wpos, M, ds->d_child_w, d_wlen);
    if (plan.plist) dd_scan<uint32_t>(st, d_wlen, ds->d_poff, M, d_tmp32);
    if (plan.sliced) {
        k_dd_slice_rows<<<dd_grid(n_slices, DD_BLOCK), DD_BLOCK, 0, st>>>(ds->d_items, ds->d_sl_item0, (int32_t)items.size(), n_slices,
                                                                          d_wlen, d_longest, d_sc);
        dd_scan<uint32_t>(st, d_longest, ds->d_sl_row, n_slices, d_tmp32);
    }
    if (M > 0) k_dd_records<<<gM, DD_BLOCK, 0, st>>>(ds->d_times, (const uint32_t *)ds->d_nodes, M, t0, scale, ds->d_ev,
                                                     with_ev8 ? ds->d_ev8 : nullptr);
    NHP_HIP(ctx, hipGetLastError());
    NHP_HIP(ctx, hipMemcpyAsync(&sc, d_sc, sizeof(sc), hipMemcpyDeviceToHost, st));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    lap("window sort + records");
    if (with_ev8) { ds->ev8_t0 = t0; ds->ev8_scale = scale; }
    if (plan.sliced && !nhp_cont_slices_keep(ds, sc.rows, n_slices, sc.max_rows)) {
        (void)hipFree(ds->d_sl_row); ds->d_sl_row = nullptr;
        (void)hipFree(ds->d_sl_item0); ds->d_sl_item0 = nullptr;
    } else if (plan.sliced && timing) {
        fprintf(stderr, "[nhp dataset, device] child slices: %d slices, %lld rows = %.3f records per pair\n", ds->n_slices,
                (long long)sc.rows, (double)sc.rows * 64.0 / (double)ds->pairs);
    }
    if (trial_f) {
        std::vector<int64_t> g((size_t)R);
        for (int32_t r = 0; r < R; ++r) g[(size_t)r] = g32[(size_t)r];
        NHP_TRY(nhp_cont_trials_keep(ctx, ds, trial_f, trial_o, g.data(), R));
    }
    return NHP_OK;
}

nhp_status nhp_cont_dataset_create_device_trials(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t M, int32_t N,
                                                 double duration, double dt_max, bool input_on_device, const int64_t *trial_f,
                                                 const double *trial_o, int32_t R, nhp_cont_dataset **out)
{
    NHP_TRY(nhp_cont_dataset_check_args(ctx, M, N, duration, dt_max, 0, N));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_cont_dataset *ds = new nhp_cont_dataset();
    ds->uid = nhp_new_dataset_uid();
    ds->ctx = ctx; ds->M = M; ds->N = N; ds->duration = duration; ds->dt_max = dt_max;
    ds->col_begin = 0; ds->col_end = N;
    const nhp_status s = dd_create(ctx, events, nodes, M, N, dt_max, input_on_device, ds, trial_f, trial_o, R);
    if (s != NHP_OK) {
        nhp_cont_dataset_destroy(ds);
        return s;
    }
    *out = ds;
    return NHP_OK;
}

extern "C" nhp_status nhp_cont_dataset_create_device(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t M, int32_t N,
                                                     double duration, double dt_max, int32_t col_begin, int32_t col_end,
                                                     int32_t input_on_device, nhp_cont_dataset **out)
{
    if (!ctx || !out || M < 0 || N < 1 || (M > 0 && (!events || !nodes))) return NHP_EINVAL;
    *out = nullptr;
    NHP_TRY(nhp_cont_dataset_check_args(ctx, M, N, duration, dt_max, col_begin, col_end));
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    nhp_cont_dataset *ds = new nhp_cont_dataset();
    ds->uid = nhp_new_dataset_uid();
    ds->ctx = ctx; ds->M = M; ds->N = N; ds->duration = duration; ds->dt_max = dt_max;
    ds->col_begin = col_begin; ds->col_end = col_end;
    const nhp_status s = dd_create(ctx, events, nodes, M, N, dt_max, input_on_device != 0, ds);
    if (s != NHP_OK) {
        nhp_cont_dataset_destroy(ds);
        return s;
    }
    *out = ds;
    return NHP_OK;
}
