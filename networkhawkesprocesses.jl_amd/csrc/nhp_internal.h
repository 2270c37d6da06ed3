// Internal declarations shared by the translation units of libnhp.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <functional>
#include <vector>
#include <utility>

#include "../../include/nhp.h"

#define NHP_BLOCK 256          // 4 waves of 64 lanes
#define NHP_WAVES (NHP_BLOCK / 64)
// children a group keeps in flight in the windowed kernels (host sorting and kernel must agree)
#ifndef NHP_U_SMALL
#define NHP_U_SMALL 4   // G <= 8
#endif
#ifndef NHP_U_MID
#define NHP_U_MID 4     // G = 16, 32 (tools/uvar.sh: 4 beats 2 by 5-8 % at K=64, 512)
#endif

// Which result slots hold a DEFERRED sum: an evaluation enqueued through nhp_cont_loglik_enqueue on the slices
// route leaves its workgroups' partial sums in the slot's own buffer and the slot is marked here; the next join adds them
// up, every marked slot in one launch.  Plain bookkeeping, no device call: mark (the later launch into a slot replaces the
// earlier), clear (a launch that writes the slot's value itself) and drain (the join: every slot still marked, in the order
// of its first mark, and none marked afterwards).
struct nhp_pending {
    int32_t n[NHP_MAX_SLOTS] = {};          // partial pairs the slot's deferred launch wrote; 0: not marked
    uint16_t block[NHP_MAX_SLOTS] = {};     // that launch's workgroup size: the order of the sum follows it
    uint8_t listed[NHP_MAX_SLOTS] = {};     // the slot is in `order` (marked now or cleared since)
    std::vector<int32_t> order;
    void mark(int32_t slot, int32_t n_partials, int32_t block_size)
    {
        n[slot] = n_partials;
        block[slot] = (uint16_t)block_size;
        if (!listed[slot]) { listed[slot] = 1; order.push_back(slot); }
    }
    void clear(int32_t slot) { n[slot] = 0; }
    bool any() const { return !order.empty(); }
    // -> slots[k], counts[k], blocks[k] of the marked slots; returns how many
    int32_t drain(int32_t *slots, int32_t *counts, int32_t *blocks)
    {
        int32_t k = 0;
        for (const int32_t s : order) {
            listed[s] = 0;
            if (n[s] > 0) { slots[k] = s; counts[k] = n[s]; blocks[k] = block[s]; ++k; }
            n[s] = 0;
        }
        order.clear();
        return k;
    }
};

struct nhp_ctx {
    int device = 0;
    // The main stream.  Reached only through main() (or lane() at the launch lines of the pipelined log-likelihood
    // routes): see the lanes below.
    hipStream_t stream_main = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double *d_results = nullptr;        // [NHP_MAX_SLOTS] log-likelihood results
    double *h_results = nullptr;        // pinned mirror
    double *d_partials = nullptr;       // per-workgroup partial sums
    size_t partials_cap = 0;            // in doubles
    void *d_scratch = nullptr;          // general scratch (gradients, sampler output)
    size_t scratch_cap = 0;             // bytes
    unsigned int *d_counter = nullptr;  // arrival ticket of the fused last-block reduction (kept at 0 between launches)
    // Second lane for independent evaluations (nhp_cont_loglik_enqueue: odd result slots; nhp_cont_loglik_batch: every
    // other launch): its own stream, partial sums and tickets.  A launch has fixed costs -- dispatch / completion,
    // column staging, the reduction tail -- during which the chip idles; with two lanes they run under the other
    // lane's pair loops (profiles/README.md: two streams).  Ordering is kept by the two accessors below, not by the
    // callers: everything but the launch lines of the pipelined routes goes through main(), which first makes the main
    // stream wait for whatever lane 2 still has in flight (the JOIN) and notes that the main stream has new work; the
    // launch lines go through lane(), which before a launch on lane 2 makes it wait for that new work (the FORK) and
    // otherwise adds nothing -- a streak of enqueues costs one launch each and no event.  nhp_lane_guard switches the
    // lane around a launch by swapping the partial sums and tickets, so the launch code is shared.
    // Deferred sampler error (nhp_cont_gibbs_step): the sweep's "weights do not sum to a positive finite value" flag is
    // copied to a pinned word behind the sweep and looked at when the NEXT sweep has been enqueued (or at any call that
    // synchronises), so a chain keeps one step in flight instead of draining the GPU every step.
    int *d_err = nullptr, *h_err = nullptr;
    hipEvent_t ev_err = nullptr;
    bool err_pending = false;
    void *h_stage = nullptr;            // pinned staging buffer for large downloads (gradients, parameters, moments)
    size_t stage_cap = 0;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    double *d_partials2 = nullptr;
    size_t partials2_cap = 0;
    unsigned int *d_counter2 = nullptr;
    bool on_lane2 = false;              // the fields above are swapped (nhp_lane_guard): lane() is stream2
    bool lane2_busy = false;            // lane 2 has launches the main stream has not waited for
    bool main_touched = true;           // the main stream got work through main() since lane 2 last waited for it
    // A failed event call inside the accessors would lose a fork or a join without a word: its status is kept here and
    // reported by the next NHP_HIP check on this context (and so by fetch / synchronize / timer_stop at the latest).
    hipError_t lane_err = hipSuccess;
    void lane_call(hipError_t e) { if (e != hipSuccess && lane_err == hipSuccess) lane_err = e; }
    // Deferred sums of the enqueue route: a partial-sum buffer per result slot (grown on demand, 2 doubles per
    // workgroup), the slots whose sum is still owed, and the switch NHP_DEFER_FINALIZE (read when the context is made; 0:
    // the enqueue route keeps the fused ticket).  The buffers belong to the context, so a pending slot outlives its dataset
    // and model.
    double *d_slot_partials[NHP_MAX_SLOTS] = {};
    uint32_t slot_cap[NHP_MAX_SLOTS] = {};      // in doubles
    nhp_pending pend;
    bool defer_finalize = true;
    int64_t finalize_launches = 0;              // k_finalize_slots launches so far (nhp_debug_finalize_launches)
    void finalize_pending();                    // context.hip: one launch (per 240 slots) on the main stream
    // Paired enqueues: inside a streak -- a deferred slot is already pending -- nhp_cont_loglik_enqueue may hold
    // ONE eligible evaluation back and launch it with the next one in a single pass over the records (cont_loglik.hip).
    // Whatever is held is launched alone at the next enqueue that cannot share its pass and at every join, before the join
    // does anything else: it sees the parameters it was enqueued with, its dataset and model are alive, timer_stop spans it.
    // NHP_PAIR_ENQUEUE=0 (read when the context is made): nothing is ever held.
    struct held_eval { const struct nhp_cont_dataset *ds = nullptr; const struct nhp_cont_model *m = nullptr; int32_t flags = 0, slot = -1; };
    held_eval held;
    bool pair_enqueue = true;
    int64_t pair_launches = 0;                  // launches that carried two evaluations (nhp_debug_pair_launches)
    void flush_held();                          // cont_loglik.hip
    // A paired launch takes the lane the last enqueue did not, so a slot can meet another lane than its last launch took.
    // The lane (1: main stream, 2: second) of every slot's launches since the last join is kept here; an enqueue into a slot
    // last launched on the other lane joins first, which keeps two evaluations into one slot in order.
    uint8_t slot_lane[NHP_MAX_SLOTS] = {};
    std::vector<int32_t> laned;                 // the slots with an entry
    int last_enq_lane = 2;                      // (the first pair of a context's life goes to the main stream's partner)
    void note_lane(int32_t slot, int ln)
    {
        if (!slot_lane[slot]) laned.push_back(slot);
        slot_lane[slot] = (uint8_t)ln;
        last_enq_lane = ln;
    }
    // the JOIN: the main stream waits for what lane 2 has in flight, then adds up the deferred slots of both lanes before
    // anything else is given to it, and is noted as having new work
    void join_lanes()
    {
        if (held.ds) flush_held();
        for (const int32_t s : laned) slot_lane[s] = 0;
        laned.clear();
        if (lane2_busy) {
            lane2_busy = false;
            lane_call(hipEventRecord(ev_join, stream2));
            lane_call(hipStreamWaitEvent(stream_main, ev_join, 0));
        }
        if (pend.any()) finalize_pending();
        main_touched = true;
    }
    // the main stream, for everything that is not an independent evaluation: ordered after both lanes
    hipStream_t main() { join_lanes(); return stream_main; }
    // the current lane's stream, for the launch of an independent evaluation: ordered after what main() has been given
    hipStream_t lane()
    {
        if (!on_lane2) return stream_main;
        if (main_touched) {
            main_touched = false;
            lane_call(hipEventRecord(ev_fork, stream_main));
            lane_call(hipStreamWaitEvent(stream2, ev_fork, 0));
        }
        return stream2;
    }
    int cu_count = 256;
    // the device optimizer's state (nhp_lbfgs.h): kept between mle! runs -- allocating and freeing ~400 MB per run cost
    // several ms of a 30 ms run
    void *d_mle = nullptr;
    size_t mle_cap = 0;
    double *h_mle_scal = nullptr;       // pinned scalars of its readbacks
    std::string err;
};

// Switches the context to its second lane and back (flip / flip, or the destructor): the launch code reads d_partials,
// d_counter and lane() and so serves either lane.  Flipping back notes that lane 2 may have work in flight.
struct nhp_lane_guard {
    nhp_ctx *c;
    bool on = false;
    void flip()
    {
        std::swap(c->d_partials, c->d_partials2); std::swap(c->partials_cap, c->partials2_cap);
        std::swap(c->d_counter, c->d_counter2);
        c->on_lane2 = on = !on;
        if (!on) c->lane2_busy = true;
    }
    ~nhp_lane_guard() { if (on) flip(); }
};

// One contiguous run of bucketed children of a single node, processed by one workgroup.
struct nhp_item {
    int32_t node;      // child node c (0-based)
    int32_t kbeg;      // first child slot in bucket order
    int32_t kend;      // one past the last
    int32_t first;     // bit 0: the first item of its node (owns the column's integral term); bit 1: its only item
};

// A child event in node-bucketed order: everything a wave needs to walk its window.
struct __attribute__((aligned(16))) nhp_child {
    double t;          // event time
    int32_t first;     // index of the first parent inside the look-back window
    int32_t idx;       // original (time-ordered) index of this event; window = [first, idx)
};

// An event in time order, packed so that one 16-byte load fetches a parent.
struct __attribute__((aligned(16))) nhp_event {
    double t;
    int32_t node;      // 0-based
    int32_t pad;
};

struct nhp_cont_dataset {
    nhp_ctx *ctx = nullptr;
    uint64_t uid = 0;                   // process-unique id (caches keyed on "this dataset", never on its address or size)
    int64_t M = 0;
    int32_t N = 0;
    double duration = 0.0, dt_max = 0.0, t_last = 0.0;
    int64_t pairs = 0;
    int32_t group = 8;                  // lanes cooperating on one child in the windowed kernels
    int32_t n_items = 0;
    int32_t max_item = 0;               // most children in one item (sizes the deferred-log LDS buffer)
    int32_t max_window = 0;             // longest look-back window, in parents
    nhp_event *d_ev = nullptr;          // [M] time order, packed (t, node)
    // the same records in 8 bytes: node << 48 | round((t - ev8_t0) * ev8_scale), ev8_scale = 2^s with the largest s that keeps
    // the time field below 2^48 (a resolution of 2^-49 of the data's span).  Read by the short-window log-likelihood kernel,
    // whose time goes into fetching ~8 scattered parent records per event: half the bytes per record.
    uint64_t *d_ev8 = nullptr;
    double ev8_t0 = 0.0, ev8_scale = 0.0;
    // Short windows only (pairs <= 40 per event on average, finite dt_max): the parent-child pairs themselves, child by child
    // in child_w order, most recent parent first -- node << 48 | Δt as a 48-bit fraction of dt_max, 8 bytes a pair.  The
    // exponential log-likelihood kernel then STREAMS its item's pairs (contiguous) instead of fetching ~8 scattered records per
    // child behind each child record.  d_poff: pair offsets by child_w position (host-made with the dataset);
    // d_plist: built on the device at the first evaluation that wants it.
    uint32_t *d_poff = nullptr;         // [M + 1]
    uint64_t *d_plist = nullptr;        // [pairs]
    // the same pairs for the logit-normal parent sampler: {logit(x), 1/(x(1-x))} at x = Δt/Δtmax -- the data half of the
    // impulse pdf, evaluated ONCE with the operation sequence the sampler (and the oracle) use, so the weights keep their
    // bits -- and the parent's node; built at the first logit-normal sweep
    double2 *d_plq = nullptr;           // [pairs]
    uint16_t *d_pnode = nullptr;        // [pairs]
    // Child slices (cont_slices.hip): the same short-window pairs, laid out for one LANE per child.  A slice is
    // 64 consecutive children of one item in child_w order = one wavefront's work; its pairs are stored row by row, row r
    // = the r-th most recent parent of each of the 64 children (64 records, one per lane: a wave-wide coalesced load), as
    // many rows as the slice's longest window (children are sorted by window length, so a slice's windows are nearly
    // equal; shorter ones are padded with zero-weight records on node N).  A record is 6 bytes in two planes: lo = low 32
    // bits of the delay, hi = node << (16 - nb) | high bits of the delay; the delay is round(Δt/Δtmax · 2^(48 - nb)),
    // nb = bit length of N.  d_sl_row / d_sl_item0 are host-made with the dataset; the planes are filled on the device at
    // the first evaluation that uses them.
    uint32_t *d_sl_row = nullptr;       // [n_slices + 1] first row of each slice
    int32_t *d_sl_item0 = nullptr;      // [n_items + 1] first slice of each item
    uint32_t *d_sl_lo = nullptr;        // [(sl_rows + 16) * 64]
    uint16_t *d_sl_hi = nullptr;        // [(sl_rows + 16) * 64]
    // logit-normal impulses: the data half of every record's pdf, {logit(x), 1/(x(1-x))} at x = Δt/Δtmax from the EXACT times with
    // the operation sequence of nhp_logitnormal_data (the bits of d_plq), in the same rows as d_sl_lo / d_sl_hi (whose node
    // field the consumers read); padding records hold {0, 0}.  Built at the first logit-normal parent sweep over the slices.
    double *d_sl_L = nullptr, *d_sl_Q = nullptr;   // [(sl_rows + 16) * 64] each
    double *d_sl_D = nullptr;                       // [(sl_rows + 16) * 64] exact delays t_i - t_j (exponential parent sampler)
    int64_t sl_rows = 0;
    int32_t n_slices = 0, sl_nb = 0;    // node bits
    int32_t sl_max_rows = 0;            // most rows of one slice
    // Parent slices (cont_slices.hip, the gradient's second phase): the same pairs of every item grouped by PARENT node --
    // lane = parent node (the item's parent nodes sorted by their number of pairs, 64 to a slice, every node present),
    // row r = the node's r-th pair as {child slot inside the item, delay}; a record is again 6 bytes: lo = low 32 bits of
    // the delay, hi = slot << (16 - sb) | high bits, sb = bit length of max_item; padding records point at slot max_item
    // (whose 1/λ is 0).  Built on the device at the first gradient that uses them; every lane's records are sorted by
    // (slot, delay), so the list -- and with it the order of every gradient sum -- is the same for every build.
    uint32_t *d_ps_row = nullptr;       // [n_items * ps_spi + 1] first row of each parent slice
    uint16_t *d_ps_perm = nullptr;      // [n_items * ps_spi * 64] parent node of each lane (0xFFFF: none)
    uint32_t *d_ps_lo = nullptr;        // [(ps_rows + 16) * 64]
    uint16_t *d_ps_hi = nullptr;
    int64_t ps_rows = 0;
    int32_t ps_spi = 0, ps_sb = 0;      // parent slices per item = ceil(N / 64); slot bits
    bool all_sole = false;              // every item is the only item of its node (the gradient then stores, never adds)
    // device arrays
    double *d_times = nullptr;          // [M] time order
    int32_t *d_nodes = nullptr;         // [M] 0-based
    nhp_child *d_child = nullptr;       // [M] bucket order (time order inside a node)
    // column shard (nhp_cont_dataset_create_columns): only children on nodes [col_begin, col_end) are evaluated, every
    // event is still a parent; the whole dataset has col_begin = 0, col_end = N
    int32_t col_begin = 0, col_end = 0;
    nhp_child *d_child_w = nullptr;
    int32_t *d_wpos = nullptr;          // [M] bucket position (index into `child`) of the child at each child_w position     // [M] same, but inside each item sorted by window length (windowed kernels)
    int32_t *d_boff = nullptr;          // [N+1] bucket offsets
    nhp_item *d_items = nullptr;        // [n_items]
    double *d_cnt = nullptr;            // [N] events per node
    int32_t *d_pn = nullptr;            // [M] bucket order: parent node of each child from the latest parent sweep (-1 = baseline)
    mutable bool pn_valid = false;      // d_pn holds an assignment (set by the sampler / nhp_cont_lgcp_loglik)
    // adjacency sweep: the data-only pair lists (per child column, sorted by parent node), built on first use
    int32_t *d_adj_k = nullptr, *d_adj_p = nullptr;   // [pairs] child slot within the column, parent node
    double *d_adj_dt = nullptr;                       // [pairs] t_child - t_parent
    double2 *d_adj_lq = nullptr;                      // [pairs] logit-normal impulses: {logit(x), 1/(x(1-x))} at x = Δt/Δtmax (data only; {0, 0} outside (0, 1)), made at the first logit-normal sweep
    int32_t *d_adj_start = nullptr;                   // [N*(N+1)] per-column offsets by parent node
    int64_t *d_adj_off = nullptr;                     // [N+1] first pair of each column
    // recursive ll evaluated as a truncated window (cont_recursive.hip): children with window starts for `cut_cached`
    nhp_child *d_child_cut = nullptr;
    mutable double cut_cached = -1.0;
    mutable int64_t cut_pairs = 0;
    int64_t n_zero_time = 0;            // events at exactly t = 0.0 (the recursion's seen-flag skips them: SURVEY D9)
    // O(M·N) recursion, one wave per (column, part of the parent nodes) (k_recursive_waves): the events with t > 0 part by
    // part (rec_h parts of rec_np nodes; node = index inside the part; 192 records of padding), the parts' offsets and,
    // per part and bucket position, how many of the part's events precede the child.  Data only; made at the first call.
    nhp_event *d_rec_ev = nullptr;
    int32_t *d_rec_poff = nullptr;      // [rec_h + 1]
    int32_t *d_rec_rank = nullptr;      // [rec_h][M]
    int32_t rec_np = 0, rec_h = 0;
    unsigned char *d_adj_group = nullptr;             // [N*N] grouping code of entry (p, c): see k_adj_build
    // host copies kept for host-side helpers
    std::vector<int32_t> h_boff;
    std::vector<double> h_cnt;
    // crowding of the data: h_slab_max[k] = most events inside any closed time window of length h_slab_len[k]
    // (lengths double from the mean gap up to the duration).  Tightens the truncated-window bound of the recursive
    // formulation (cont_recursive.hip): events older than `cut` arrive at most h_slab_max per slab.
    std::vector<double> h_slab_len;
    std::vector<int64_t> h_slab_max;
    bool slab_done = false;             // the two vectors above have been made (nhp_dataset_slab_stats: at the recursion's first bound)
    std::vector<int64_t> h_pair_off;    // [N+1] prefix of window pairs per child node (adjacency sweep scratch)
    // Independent trials stacked along time (nhp_cont_dataset_create_trials): trial r owns the events
    // [trial_f[r], trial_f[r+1]) and the clock interval [trial_o[r], trial_o[r+1]]; trial_g[r] = the first index in
    // [trial_f[r], trial_f[r+1]] whose time is not exactly trial_o[r] (the recursion's D9 per trial).  No window crosses a trial
    // start: nhp_child::first is clipped at trial_f[r] when the dataset is made, and everything built from the windows follows.
    // n_trials = 1 (every other entry point): one recording, no device tables; the host tables are then {0, M} / {0, duration}.
    int32_t n_trials = 1;
    std::vector<int64_t> h_trial_f, h_trial_g;      // [R + 1], [R]
    std::vector<double> h_trial_o;                  // [R + 1]
    int32_t *d_trial_f = nullptr, *d_trial_g = nullptr;
    double *d_trial_o = nullptr;
};
inline bool nhp_multi_trial(const nhp_cont_dataset *ds) { return ds->n_trials > 1; }
// the entry points that read events by time, or continue one recording, refuse a dataset of several trials
#define NHP_ONE_RECORDING(ctx, ds, what, why)                                                                  \
    do {                                                                                                      \
        if (nhp_multi_trial(ds)) {                                                                            \
            nhp_set_error(ctx, what ": not available on a dataset of %d trials (" why ")", (ds)->n_trials);    \
            return NHP_ENOTIMPL;                                                                              \
        }                                                                                                     \
    } while (0)

struct nhp_cont_model {
    nhp_ctx *ctx = nullptr;
    int32_t N = 0, baseline_kind = 0, grid_n = 0, impulse_kind = 0, has_A = 0;
    double dt_max = 0.0, grid_end = 0.0;
    // params(process) = [λ0; θ | μ; τ; W] as ONE device block of nhp_layout(m).P doubles (owned); the tables point into it
    double *d_params = nullptr;
    double *d_lambda0 = nullptr;
    double *d_p1 = nullptr;             // theta (exp) or mu (logit-normal)
    double *d_p2 = nullptr;             // tau (logit-normal; null for exponential impulses)
    double *d_W = nullptr;
    double *d_grid = nullptr, *d_A = nullptr;
    // parameters change through create/update/set_params and the device-side draws: `version` counts the changes, so
    // quantities derived from the parameters (the recursive path's truncation window) are recomputed only when stale
    uint64_t version = 1;
    mutable uint64_t rec_version = 0;
    mutable uint64_t rec_ds = 0;        // uid of the dataset whose slab statistics the cached bound was derived from
    mutable double rec_cut = 0.0;       // look-back beyond which the full-history sum is below 2^-60 of every λ_i (0: no bound)
    // running sums of the chain's samples (nhp_cont_model_moments_*): Σx and Σx² over [λ0; θ | μ; τ; W; vec(A)], so a
    // chain's posterior summaries never cross PCIe step by step
    double *d_mom = nullptr;            // [2][mom_len]
    int64_t mom_len = 0, mom_count = 0;
    // BernoulliNetworkModel.ρ on the device (nhp_cont_model_set_rho / nhp_cont_network_step): {ρ, Σρ, Σρ², ΣA of the
    // latest sweep}; the sums follow the moments above
    double *d_rho = nullptr;
    // StochasticBlockNetworkModel on the device (sbm.hip: nhp_cont_model_set_sbm / nhp_cont_sbm_step): labels, ρ[K x K], π,
    // the link-probability matrix the adjacency sweep reads and the running sums of the kept steps; null: no block network
    struct nhp_sbm_state *sbm = nullptr;
    // LatentDistanceNetworkModel on the device (latent.hip: nhp_cont_model_set_latent / nhp_cont_latent_step): positions, the
    // offset b, the link-probability matrix and the running sums of the kept steps; null: no latent distance network.  At
    // most one of sbm and latent is set.
    struct nhp_latent_state *latent = nullptr;
    // streaming convergence diagnostics (cont_diagnostics.hip: nhp_cont_model_diagnostics_*): the batch planes and the
    // snapshots of the sums above; null: not configured, _accumulate runs the moments kernel alone
    struct nhp_diag_state *diag = nullptr;
    // scorers attached for nhp_cont_mcmc_run (cont_score.hip: nhp_cont_model_attach_score; not owned): slot k scores every
    // score_every[k]-th kept step, score_kept[k] counts the kept steps seen since the attach (it persists across calls)
    struct nhp_cont_score *score[2] = {nullptr, nullptr};
    int64_t score_every[2] = {1, 1}, score_kept[2] = {0, 0};
    // streaming quantiles (chain_quantiles.hip: nhp_cont_model_quantiles_*; nhp_quant.h): the marker planes; null: not
    // configured, nothing is launched
    struct nhp_quant_state *quant = nullptr;
};
// chain_quantiles.hip, for either model: release the marker planes; their share of a moments reset (zero the planes, fitted
// to the model's entries; NHP_ENOMEM: quantiles off); the driver's kept step (feeds every `every`-th one)
void nhp_quant_release(struct nhp_quant_state **q);
nhp_status nhp_quant_reset(nhp_ctx *ctx, nhp_cont_model *m);
nhp_status nhp_quant_kept_step(nhp_ctx *ctx, nhp_cont_model *m);
// cont_score.hip: grow the context's scratch to what nhp_cont_score_accumulate(score, model) stages, ahead of a loop
nhp_status nhp_cont_score_reserve(nhp_ctx *ctx, const struct nhp_cont_score *score, const nhp_cont_model *m);
// cont_diagnostics.hip: release the diagnostic planes; their share of nhp_cont_model_moments_reset (zero the planes, fitted
// to the sums' current length) and of _accumulate (the fused kernel IN PLACE of the moments kernel, then the snapshots) --
// all asynchronous on the main stream
void nhp_diag_free(nhp_cont_model *m);
nhp_status nhp_diag_reset(nhp_ctx *ctx, nhp_cont_model *m);
nhp_status nhp_diag_accumulate(nhp_ctx *ctx, nhp_cont_model *m);
// sbm.hip: release the block network's state; its share of nhp_cont_model_moments_reset / _accumulate (asynchronous)
void nhp_sbm_free(nhp_cont_model *m);
nhp_status nhp_sbm_detach(nhp_ctx *ctx, nhp_cont_model *m);      // set_rho: the model's network is no block model (any more)
nhp_status nhp_sbm_moments_reset(nhp_ctx *ctx, nhp_cont_model *m);
nhp_status nhp_sbm_moments_accumulate(nhp_ctx *ctx, nhp_cont_model *m);
// sbm.hip: A [N x N doubles on the device] -> colb[n*W + w] bit j = A[32w + j, n], rowb[n*W + w] bit j = A[n, 32w + j] (asynchronous)
nhp_status nhp_sbm_enqueue_pack(nhp_ctx *ctx, const double *d_A, int N, uint32_t *colb, uint32_t *rowb);
// latent.hip: the same four for the latent distance network's state
void nhp_latent_free(nhp_cont_model *m);
nhp_status nhp_latent_detach(nhp_ctx *ctx, nhp_cont_model *m);
nhp_status nhp_latent_moments_reset(nhp_ctx *ctx, nhp_cont_model *m);
nhp_status nhp_latent_moments_accumulate(nhp_ctx *ctx, nhp_cont_model *m);

// RCCL communicator of one rank (comm.hip); librccl.so.1 is dlopen'ed on first use
struct nhp_comm {
    nhp_ctx *ctx = nullptr;
    void *nccl = nullptr;               // ncclComm_t
    int rank = 0, world = 1;
};
// in-place sum / gather of device doubles over the ranks, on the ctx stream (asynchronous)
nhp_status nhp_comm_allreduce_dev(nhp_ctx *ctx, nhp_comm *comm, double *d_buf, size_t n);
nhp_status nhp_comm_allgather_dev(nhp_ctx *ctx, nhp_comm *comm, const double *d_mine, size_t n, double *d_all);
// cont_grad.hip: enqueue log-likelihood (-> ctx->d_results[0]) + gradient (-> *d_grad, P doubles in ctx->d_scratch, with one
// spare double in front of it at (*d_grad)[-1] for the packed [ll; grad] exchange)
nhp_status nhp_grad_enqueue(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, int64_t grad_len,
                            double **d_grad);
// comm.hip: the same, with the shards' [ll; grad] summed over the ranks on the device when `comm` is given (nullable)
nhp_status nhp_grad_enqueue_reduced(nhp_ctx *ctx, nhp_comm *comm, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags,
                                    int64_t grad_len, double **d_grad);
// cont_em.hip, shared with cont_vb.hip: the refusals of em! (LGCP baseline, a model with A, a column shard; `what` names the
// caller), and the E-step at the DEVICE vector d_x in params! order (through nhp_model_view): log-likelihood ->
// ctx->d_results[0], gradient -> *d_grad (scratch), by whichever route nhp_grad_enqueue picks; an empty dataset is handled
nhp_status nhp_em_check(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const char *what);
nhp_status nhp_em_estep(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags, const double *d_x, int64_t P,
                        double **d_grad);
struct nhp_em_host {                 // one pinned scalar and the event behind its copy: the stopping rule's read per iteration
    double *h = nullptr;
    hipEvent_t ev = nullptr;
    ~nhp_em_host()
    {
        if (h) (void)hipHostFree(h);
        if (ev) (void)hipEventDestroy(ev);
    }
};
// cont_adjacency.hip: enqueue one sweep of A; per-column link counts land at *d_links [N] (scratch).  d_rho_matrix
// (nullable): the N x N link probabilities already on the device (outside the context's scratch), used when rho_matrix is null
nhp_status nhp_adj_enqueue(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, const double *rho_matrix, double rho,
                           const double *d_rho_scalar, const double *u, uint64_t seed, uint64_t step, double **d_links,
                           const double *d_rho_matrix = nullptr);


// Kernel-side view of model + data (passed by value).
struct nhp_cont_args {
    const double *times;
    const int32_t *nodes;
    const nhp_event *ev;
    const uint64_t *ev8;             // packed records (or null): see nhp_cont_dataset::d_ev8
    const uint32_t *poff;            // pair list of short-window datasets (or null): see nhp_cont_dataset::d_poff
    const uint64_t *plist;
    const double2 *plq;              // logit-normal pair cache (or null): see nhp_cont_dataset::d_plq
    const uint16_t *pnode;
    double ev8_t0, ev8_scale, ev8_inv;
    const nhp_child *child;
    const nhp_child *child_w;
    const int32_t *wpos;             // child_w position -> bucket position
    int32_t col_begin, col_end;      // columns (child nodes) this dataset owns
    const int32_t *boff;
    const nhp_item *items;
    const double *cnt;
    const double *lambda0, *grid;
    const double *p1, *p2, *W, *A;
    int64_t M;
    int32_t N, grid_n, baseline_kind, impulse_kind;
    double dt_max, inv_dtmax, duration;
    int32_t dbg;        // phase-ablation bits; only read in -DNHP_ABLATE builds (tools/ablate.sh)
};

// Where the tables sit in the parameter vector, params! order [λ0; θ | μ; τ; W] (src/continuous.jl:121-129): the one definition
// for the host entry points and the kernels.  The baseline block is λ (N) or vcat(λ...) (N·grid_n grid intensities of the
// LGCP: src/baselines.jl:41,173); p1 = θ | μ follows it, then τ (logit-normal only: p2 == W otherwise), then W.
struct nhp_layout {
    size_t nb = 0, p1 = 0, p2 = 0, W = 0, P = 0;    // length of the baseline block; offsets of the tables; length of the vector
    nhp_layout() = default;
    __host__ __device__ nhp_layout(int32_t N, int32_t grid_n, int32_t baseline_kind, int32_t impulse_kind)
    {
        const size_t NN = (size_t)N * (size_t)N;
        nb = baseline_kind == NHP_BASELINE_HOMOGENEOUS ? (size_t)N : (size_t)N * (size_t)grid_n;
        p1 = nb; p2 = p1 + NN;
        W = impulse_kind == NHP_IMPULSE_EXPONENTIAL ? p2 : p2 + NN;
        P = W + NN;
    }
    explicit nhp_layout(const nhp_cont_model *m) : nhp_layout(m->N, m->grid_n, m->baseline_kind, m->impulse_kind) {}
    __host__ __device__ explicit nhp_layout(const nhp_cont_args &a) : nhp_layout(a.N, a.grid_n, a.baseline_kind, a.impulse_kind) {}
};

struct nhp_disc_dataset {
    nhp_ctx *ctx = nullptr;
    int32_t N = 0, B = 0, L = 0;
    int64_t T = 0;
    double *d_dataT = nullptr;          // [T*N] counts as f64, t fastest (GEMM operand)
    uint8_t *d_data8 = nullptr;         // [T*N] the same counts in one byte each (when none exceeds 255): what the convolution reads
    double *d_conv = nullptr;           // [T*N*B] t fastest
    double *d_colsum = nullptr;         // [2N] Σ_t data[n,t], then Σ_t loggamma(data[n,t]+1)
    double lgamma_sum = 0.0;            // Σ_{n,t} loggamma(data[n,t]+1): the data-only term of the Poisson ll
    // occupied bins (count > 0) in time-major order, for the discrete adjacency sweep
    int64_t nocc = 0;                                 // occupied bins
    // the discrete adjacency sweep's entry lists: the time axis cut into `da_nspans` spans of at most NHP_DA_SPAN bins (a
    // balanced round of two workgroups per CU where T allows); within a span the occupied bins are sorted by (node, bin)
    // and padded with empty entries (count 0) to a multiple of 4, so a thread takes whole 16-byte groups of consecutive
    // entries that mostly share their node
    int32_t da_nspans = 0, da_max_entries = 0;        // spans; the most entries (incl. padding) any span holds
    int64_t nocc_pad = 0;                             // entries incl. padding
    int32_t *d_occ_t = nullptr, *d_occ_c = nullptr;   // [nocc_pad] bin, node (0-based)
    double *d_occ_s = nullptr;                        // [nocc_pad] the count
    uint32_t *d_occ_pack = nullptr;                   // [nocc_pad] node << 16 | count << 8 | bin % 256 (null when a node index or count does not fit)
    int32_t *d_occ_off = nullptr;                     // [da_nspans + 1] first entry of each span
    int32_t *d_span_t = nullptr;                      // [da_nspans + 1] first bin of each span
    double *d_convsum = nullptr;                      // [N*B] Σ_t Ŝ[t, p, b] (filled with the convolution)
    // time-varying baseline of a DiscreteLogGaussianCoxProcess (nhp_disc_set_lgcp_baseline); used when a call passes lambda0 = NULL
    double *d_baseT = nullptr;                        // [T*N] baseline intensity per bin, t fastest
    int32_t *d_base_counts = nullptr;                 // [T*N] events attributed to the baseline by the latest parent sweep
    bool base_counts_valid = false;
    std::vector<double> h_grid_x;                     // the LGCP grid [G]
    // independent trials stacked along time (nhp_disc_dataset_set_trials): the convolution stops at their first bins
    std::vector<int64_t> trial_off;                   // [R + 1] first bin of each trial, then T; empty while R = 1
    uint8_t *d_trial_start = nullptr;                 // [T] 1 at the first bin of every trial but the first; null while R = 1
};

#ifndef NHP_DA_SPAN
#define NHP_DA_SPAN 256  // bins of a workgroup's span in the discrete adjacency sweep, at most (the packed entry keeps bin % 256)
#endif

// disc.hip pieces shared with disc_gibbs.hip: upload W, θ, A (and λ0) and build the bump table E [N·B x N] on the device
// (GEMM order k = p + b·N, or the reference's category order p·B + b with cat_order) plus base[c] = λ0[c]·dt; `extra`
// doubles of scratch follow at *extra_ptr.  Layout after E: base (N) | λ0 (N) | W (N²) | θ (N²B) | A (N²) | extra.
// `on_device`: the four sources are device pointers outside the scratch (a device-resident model: nhp_disc_model), copied
// device to device into the same layout -- everything behind the copies is the same launch on the same bits.
nhp_status nhp_disc_stage_bump(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0, const double *W,
                               const double *theta, const double *A, double dt, double **E, double **base, size_t extra,
                               double **extra_ptr, int cat_order = 0, bool on_device = false);

// nhp_disc_model (include/nhp.h, disc_chain.hip): the state of a discrete chain on the device.  ONE block in the order
// nhp_disc_stage_bump lays its copies out -- λ0 (N) | W (N²) | θ (N²B) | A (N², has_A) -- so staging is one copy per piece and
// the sums below follow the block entry by entry.
struct nhp_disc_model {
    nhp_ctx *ctx = nullptr;
    int32_t N = 0, B = 0, has_A = 0;
    double dt = 1.0;
    double *d_block = nullptr;          // owned
    double *d_lambda0 = nullptr, *d_W = nullptr, *d_theta = nullptr, *d_A = nullptr;      // into d_block
    // the network's scalars {ρ, Σρ, Σρ², ΣA of the latest sweep} (has_A: allocated with the model) and ΣA once more as the
    // exact integer the sweep's route is chosen from
    double *d_rho = nullptr;
    long long *d_links = nullptr;
    bool rho_set = false;
    // ΣA of the current A as the host knows it: counted at _set, read back (8 bytes) after a sweep when the next one asks
    int64_t links = 0;
    bool links_on_device = false;
    // running sums over the kept steps (nhp_disc_model_moments_*): Σx | Σx² [2][mom_len] in params(process) order --
    // network: the block itself; standard: [λ0; vec(W∘θ)]
    double *d_mom = nullptr;
    int64_t mom_len = 0, mom_count = 0;
    struct nhp_diag_state *diag = nullptr;              // nhp_diag.h; null: not configured
    // scorers attached for nhp_disc_mcmc_run (nhp_disc_model_attach_score; not owned): slot k scores every score_every[k]-th
    // kept step, score_kept[k] counts the kept steps since the attach (so a chain cut into calls keeps its rhythm)
    struct nhp_disc_score *score[2] = {nullptr, nullptr};
    int64_t score_every[2] = {1, 1}, score_kept[2] = {0, 0};
    struct nhp_quant_state *quant = nullptr;            // nhp_quant.h; null: not configured
};
// chain_quantiles.hip: the discrete model's share of the streaming quantiles (as for nhp_cont_model above)
nhp_status nhp_quant_reset(nhp_ctx *ctx, nhp_disc_model *m);
nhp_status nhp_quant_kept_step(nhp_ctx *ctx, nhp_disc_model *m);
// disc_score.hip: grow the context's scratch to what nhp_disc_score_accumulate(score, model) stages, ahead of a loop
nhp_status nhp_disc_score_reserve(nhp_ctx *ctx, const struct nhp_disc_score *score);
// disc_gibbs.hip: the two halves of a chain step on device-resident state, asynchronous on the main stream.  The Gibbs half
// reads and overwrites λ0, W, θ (the bits of nhp_disc_gibbs_step); the sweep overwrites A (the bits of
// nhp_disc_resample_adjacency with the scalar *d_rho and Philox uniforms), `links` = ΣA of the A it starts from.
nhp_status nhp_disc_gibbs_enqueue(nhp_ctx *ctx, const nhp_disc_dataset *ds, double *d_lambda0, double *d_W, double *d_theta,
                                  const double *d_A, double dt, double alpha0, double beta0, double kappa, double nu, double gamma0,
                                  uint64_t seed, uint64_t step);
nhp_status nhp_disc_adjacency_enqueue(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *d_lambda0, const double *d_W,
                                      const double *d_theta, double *d_A, double dt, const double *d_rho, uint64_t seed, uint64_t step,
                                      size_t links);
nhp_status nhp_disc_launch_intensity(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base,
                                     bool per_bin_baseline, double *dlam);
// the same GEMM on rows [t0, t0 + R) of Ŝ alone, homogeneous baseline: λ[t0 + r, c] lands at dlam[r + R·c] (disc_score.hip)
nhp_status nhp_disc_launch_intensity_rows(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base, int64_t t0,
                                          int64_t R, double *dlam);
// disc.hip launches re-driven by disc_information.hip: the log-likelihood of a staged bump table (-> ctx->d_results[0], the
// bits of nhp_disc_loglik), and the gradient's split-T Gᵀ·R (R [T x N], t fastest) into `splits` slabs of N·B x N
nhp_status nhp_disc_launch_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *E, const double *base);
void nhp_disc_gtr_plan(nhp_ctx *ctx, const nhp_disc_dataset *ds, int *splits, int *k_chunk);
nhp_status nhp_disc_launch_gtr(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *dR, int splits, int k_chunk, double *dslab);

// ---- error plumbing -------------------------------------------------------------------
void nhp_set_error(nhp_ctx *ctx, const char *fmt, ...);
// the status a fork or join inside main() / lane() left behind, once (hipSuccess: none; ctx may be null)
inline hipError_t nhp_take_lane_error(nhp_ctx *ctx)
{
    if (!ctx || ctx->lane_err == hipSuccess) return hipSuccess;
    const hipError_t e = ctx->lane_err;
    ctx->lane_err = hipSuccess;
    return e;
}
#define NHP_HIP(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ == hipSuccess) e_ = nhp_take_lane_error(ctx);                                 \
        if (e_ != hipSuccess) {                                                              \
            nhp_set_error(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return NHP_EHIP;                                                                 \
        }                                                                                    \
    } while (0)
#define NHP_TRY(expr)                      \
    do {                                   \
        nhp_status s_ = (expr);            \
        if (s_ != NHP_OK) return s_;       \
    } while (0)

// a caller's vector against the model's: the one length check of every entry point that takes params(process)
inline nhp_status nhp_layout_check(nhp_ctx *ctx, const nhp_layout &L, int64_t len)
{
    if ((size_t)len == L.P) return NHP_OK;
    nhp_set_error(ctx, "Parameter vector length does not match model parameter length.");
    return NHP_ESHAPE;
}
// The model with its tables pointing into the DEVICE vector d_x (params! order) instead of its own block: what mle! and em!
// evaluate a trial through, so no parameter is copied per evaluation (read-only through the view).
inline nhp_cont_model nhp_model_view(const nhp_cont_model *m, const double *d_x)
{
    const nhp_layout L(m);
    nhp_cont_model v = *m;
    double *x = const_cast<double *>(d_x);
    v.d_lambda0 = x; v.d_p1 = x + L.p1; v.d_W = x + L.W;
    if (m->impulse_kind == NHP_IMPULSE_LOGITNORMAL) v.d_p2 = x + L.p2;
    return v;
}
// ... and the recursive route's cached bound, which an evaluation through a view may have renewed, back to the model
inline void nhp_model_view_keep_bound(nhp_cont_model *m, const nhp_cont_model &view)
{
    m->rec_version = view.rec_version; m->rec_ds = view.rec_ds; m->rec_cut = view.rec_cut;
}

nhp_status nhp_ctx_reserve_partials(nhp_ctx *ctx, size_t n_doubles);
// the deferred sums' buffer of one result slot (ctx->d_slot_partials[slot]), grown on demand like d_partials
nhp_status nhp_ctx_reserve_slot_partials(nhp_ctx *ctx, int32_t slot, size_t n_doubles);
// the device optimizers' block (ctx->d_mle: mle!, em!, expected_statistics), grown on demand and kept between runs; `what`
// names the state in the out-of-memory message
nhp_status nhp_ctx_reserve_mle(nhp_ctx *ctx, size_t bytes, const char *what);
nhp_status nhp_dataset_slab_stats(nhp_ctx *ctx, const nhp_cont_dataset *ds);      // cont_data.hip
int nhp_pick_group(double mean_window);
// Dataset creation: the decisions the host pre-pass (nhp_cont_dataset_create_columns) and the device pre-pass
// (nhp_cont_dataset_create_device, cont_data_dev.hip) share, so the two builds cannot drift apart.
struct nhp_cont_plan {
    std::vector<nhp_item> items;
    bool sliced = false;                // child slices (d_sl_row / d_sl_item0)
    bool plist = false;                 // pair offsets (d_poff)
    int sort_mode = 2;                  // NHP_SORT: 2 = each item by window length, 1 = inside rounds, 0 = bucket order
    int round = 0;                      // children per round of the windowed kernels
};
uint64_t nhp_new_dataset_uid();       // process-unique (nhp_cont_dataset::uid)
// lower(c, s, TP): the first bucket position of node c whose event index is >= M*s/TP (the time parts of the XCD layout)
typedef std::function<int32_t(int32_t c, int32_t s, int32_t TP)> nhp_lower_fn;
// needs ds->M, N, pairs, dt_max, col_begin/col_end and h_boff; sets ds->group, n_items, max_item, all_sole
void nhp_cont_partition(nhp_cont_dataset *ds, const nhp_lower_fn &lower, nhp_cont_plan &p);
// the argument checks before the per-event validation (same status and message on both routes)
nhp_status nhp_cont_dataset_check_args(nhp_ctx *ctx, int64_t M, int32_t N, double duration, double dt_max, int32_t col_begin,
                                       int32_t col_end);
// independent trials (cont_data.hip): the message of an event outside its trial's interval, the tables of a
// finished dataset, and the device route of nhp_cont_dataset_create_trials (cont_data_dev.hip; the tables are host pointers)
nhp_status nhp_cont_trials_bad_event(nhp_ctx *ctx, int64_t i, int32_t r, double t, double lo, double hi);
nhp_status nhp_cont_trials_keep(nhp_ctx *ctx, nhp_cont_dataset *ds, const int64_t *trial_f, const double *trial_o, const int64_t *trial_g,
                                int32_t R);
nhp_status nhp_cont_dataset_create_device_trials(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t M, int32_t N,
                                                 double duration, double dt_max, bool input_on_device, const int64_t *trial_f,
                                                 const double *trial_o, int32_t R, nhp_cont_dataset **out);
// child slices with `rows` rows in all: kept (sets sl_rows, n_slices, sl_nb, sl_max_rows) or dropped (false)
bool nhp_cont_slices_keep(nhp_cont_dataset *ds, uint64_t rows, int32_t n_slices, int32_t max_rows);
// the 8-byte event records' origin and scale from the first and the last time (false: no 8-byte records)
bool nhp_ev8_params(int32_t N, int64_t M, double e0, double e1, double *t0, double *scale);
// recursion_cost: what the caller's O(M·N) kernel costs relative to its windowed route, in units of the log-likelihood's
// ratio (1 for the log-likelihood; the gradient's recursion is 3.5x the log-likelihood's, its windowed route 2.9x).
// derivatives: the caller differentiates the sum (gradient, observed information) -- the empty window of a model without any
// excitation (all W = 0) is exact for the log-likelihood alone, so these callers get the recursion there
nhp_status nhp_recursive_window(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_child **child_cut,
                                int *group, double recursion_cost = 1.0, bool derivatives = false);
nhp_status nhp_launch_recursive_flags(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, double *d_out);
nhp_status nhp_launch_event_intensity_as(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_child *child_w,
                                         int group, int mask_integral, double *d_lambda);
nhp_status nhp_launch_windowed_as(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const nhp_child *child_w,
                                  int group, int mask_integral, double *d_out);
nhp_status nhp_ctx_reserve_scratch(nhp_ctx *ctx, size_t bytes);
nhp_status nhp_ensure_pair_cache(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_args *a);   // cont_sampler.hip
// The child-slice A/B switches, read on every call (the tests flip them inside one process): true when NHP_SLICES=0 (no
// dataset is sliced, no route uses slices) or the route's own switch (NHP_SLICES_LN, NHP_GRAD_SLICES, NHP_BATCH_SLICES,
// NHP_SAMPLER_SLICES; or null) is 0
inline bool nhp_slices_off(const char *route_switch)
{
    const char *all = getenv("NHP_SLICES"), *route = route_switch ? getenv(route_switch) : nullptr;
    return (all && atoi(all) == 0) || (route && atoi(route) == 0);
}
// How an item's child slices are dealt to the nw waves of its workgroup: in snake order.  Round r hands out slices
// r·nw .. r·nw + nw - 1, forwards when r is even and backwards when it is odd.  Children are sorted longest window first, so
// slice j has about as many rows as the item's 64·j-th longest window: dealt forwards every round, wave 0 would take the
// longest slice of each.  Round 0 is j = wave (a kernel's head requests that slice's rows before anything else).  A wave's
// slices increase with the round, so once one is past the item's last every later one is too.
__host__ __device__ inline int32_t nhp_slice_of(int32_t round, int32_t wave, int32_t nw)
{
    return round * nw + ((round & 1) ? nw - 1 - wave : wave);
}
// cont_slices.hip: the exponential log-likelihood of the dataset's own short windows, one lane per child over the child
// slices.  *launched = false (and NHP_OK) when the dataset has no slices or the model is not covered.
// defer_slot >= 0 (nhp_cont_loglik_enqueue only, d_out = ctx->d_results + defer_slot): the workgroups leave their partial sums
// in that slot's buffer and the slot is marked pending instead of the fused last-workgroup sum; *deferred says whether the
// launch took that exit (it keeps the fused sum where the deferred one could not repeat its order: workgroups of 1024).
nhp_status nhp_launch_windowed_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int mask_integral,
                                      double *d_out, bool *launched, int32_t defer_slot = -1, bool *deferred = nullptr);
nhp_status nhp_launch_windowed_slices_ln(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int mask_integral,
                                      double *d_out, double *d_lambda, bool *launched, int32_t defer_slot = -1,
                                      bool *deferred = nullptr);
// the same with the analytic gradient (params! order, P doubles at d_grad) from one fused launch over the child and the
// parent slices; *launched = false when the pair is not covered
nhp_status nhp_launch_grad_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_out, double *d_grad,
                                  bool *launched);
// true: that launch stores every entry of the gradient itself; false: it adds to what k_grad_init left
bool nhp_grad_slices_direct(const nhp_cont_dataset *ds, const nhp_cont_model *m);
// resample_parents for logit-normal impulses over the child slices (one lane per child, rows coalesced, the first weights of a
// child kept in LDS between the sum and the scan): same bits as k_sampler.  *launched = false when not covered.
nhp_status nhp_launch_sampler_slices(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, const double *d_u, uint64_t seed,
                                     uint64_t step, int64_t *parents, int64_t *pnodes, int32_t *pn_b, double *dt_b, int *d_err, bool *launched);
// S = 2 or 4 exponential models with homogeneous baselines on one dataset in ONE pass over its child slices (every record is
// fetched and decoded once, S columns sit in LDS): results -> ctx->d_results[slot0 .. slot0 + S).  *launched = false when the
// models are not covered (the caller falls back to its other kernels).
nhp_status nhp_launch_slices_batch(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *const *ms, int S, int32_t slot0,
                                   bool *launched);
// Two enqueued evaluations in one pass (k_slices_batch<B, C, 2, DEFER>): _eligible says whether an enqueue of (ds, m) would take
// k_windowed_slices' deferred exit and may share a pass; _pair launches ms[0] -> slot[0], ms[1] -> slot[1] (both eligible,
// batch-compatible, different slots) on the current lane with that kernel's (B, C) and marks both slots pending.  Each
// slot gets the bits the single launch would have left.
bool nhp_slices_pair_eligible(const nhp_cont_dataset *ds, const nhp_cont_model *m);
nhp_status nhp_launch_slices_pair(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *const *ms, const int32_t *slot);
nhp_cont_args nhp_make_args(const nhp_cont_dataset *ds, const nhp_cont_model *m);
nhp_status nhp_check_pair(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m);
// Device -> caller memory through the context's pinned staging buffer: DMA at link speed into pinned memory, then one
// host copy (a direct copy into pageable caller memory ran at ~1 GB/s here).  Synchronises the stream.
nhp_status nhp_download(nhp_ctx *ctx, void *dst, const void *d_src, size_t bytes);
// report (once) the deferred sampler error of an earlier nhp_cont_gibbs_step, waiting for that sweep if need be
nhp_status nhp_check_deferred(nhp_ctx *ctx);
bool nhp_is_column_shard(const nhp_cont_dataset *ds);
// entry points that need every column (samplers, intensity tables): refuse a column shard
#define NHP_WHOLE_DATASET(ctx, ds, what)                                                                       \
    do {                                                                                                      \
        if (nhp_is_column_shard(ds)) {                                                                        \
            nhp_set_error(ctx, what ": not available on a column shard (log-likelihood and gradient only)");  \
            return NHP_ENOTIMPL;                                                                              \
        }                                                                                                     \
    } while (0)

// launchers implemented in the kernel translation units (all asynchronous on the main stream, after a join)
nhp_status nhp_launch_windowed(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_out);
nhp_status nhp_launch_recursive(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_out);
nhp_status nhp_launch_finalize(nhp_ctx *ctx, const nhp_cont_args &a, int n_partials, double *d_out);
nhp_status nhp_launch_event_intensity(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_lambda);

// wave-local ordering of LDS traffic: wait for this wave's outstanding LDS operations (lgkmcnt(0)
// only -- global stores stay in flight) and keep the compiler from moving LDS accesses across it
#define NHP_LDS_SYNC()                                   \
    do {                                                 \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_s_waitcnt(0xc07f);              \
        __builtin_amdgcn_wave_barrier();                 \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)


// ---- wave-partitioned O(M·N) recursion (cont_recursive.hip; its gradient pass in cont_grad.hip) -----------------------
struct nhp_rec_parts {          // kernel-side view of the per-part lists (nhp_cont_dataset::d_rec_*)
    const nhp_event *ev;        // [Σ part lengths + 192] events with t > 0 (D9), part by part, time order inside; node = index inside the part
    const int32_t *poff;        // [H + 1] first record of each part
    const int32_t *rank;        // [H][M] by bucket position k: events of the part with time index < idx_k
};
nhp_status nhp_rec_parts_for(nhp_ctx *ctx, const nhp_cont_dataset *ds, int *PQ, int *H, nhp_rec_parts *rp);
nhp_status nhp_launch_recursive_waves(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, double *d_out, double *d_ginv);
// the (parents per lane, parts) shapes nhp_rec_parts_for picks, which both kernels are instantiated for: X(PQ, H) launches
// (N <= 64: 1 x 1, then 1 x 2, 1 x 4, 2 x 4, 4 x 4 up to N = 1024, 4 x 8, 4 x 16 up to N = 4096)
#define NHP_REC_SHAPES(X)                         \
    do {                                          \
        if (PQ == 1 && H == 1) X(1, 1);           \
        else if (PQ == 1 && H == 2) X(1, 2);      \
        else if (PQ == 1 && H == 4) X(1, 4);      \
        else if (PQ == 2 && H == 4) X(2, 4);      \
        else if (PQ == 4 && H == 4) X(4, 4);      \
        else if (PQ == 4 && H == 8) X(4, 8);      \
        else X(4, 16);                            \
    } while (0)
// Ordering of one wave's own LDS traffic without draining it: the LDS unit executes a wave's instructions in issue order (an
// atomic of lane A is seen by a later read of lane B of the same wave), so only the compiler must be kept from reordering.
#define NHP_LDS_ORDER()                                         \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
#ifndef NHP_RECW_SYNC
#define NHP_RECW_SYNC() NHP_LDS_ORDER()
#endif

// ---- device helpers --------------------------------------------------------------------
__device__ __forceinline__ double nhp_dpp_add(double v, const int sel)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int plo, phi;
    switch (sel) {
    case 0: plo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true); break;   // quad_perm [1,0,3,2]
    case 1: plo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, true); break;   // quad_perm [2,3,0,1]
    case 2: plo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, true); break; // row_half_mirror
    default: plo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, true); phi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, true); break; // row_mirror
    }
    return v + __hiloint2double(phi, plo);
}

// Sum over the 64 lanes of a wave; every lane returns the total.  Rows of 16 are reduced in the
// VALU with DPP, the four row sums are combined through scalar lane reads (no LDS round trips).
__device__ __forceinline__ double nhp_wave_sum(double v)
{
    v = nhp_dpp_add(v, 0);
    v = nhp_dpp_add(v, 1);
    v = nhp_dpp_add(v, 2);
    v = nhp_dpp_add(v, 3);
    const int lo = __double2loint(v), hi = __double2hiint(v);
    double r = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
    r += __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
    r += __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
    r += __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
    return r;
}

// Maximum over the 64 lanes of a wave, in the VALU/SALU only (DPP inside rows of 16, scalar reads across rows): no LDS round trips.
__device__ __forceinline__ int nhp_wave_max_i32(int v)
{
    int o;
    o = __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); v = o > v ? o : v;      // quad_perm [1,0,3,2]
    o = __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); v = o > v ? o : v;      // quad_perm [2,3,0,1]
    o = __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true); v = o > v ? o : v;     // row_half_mirror
    o = __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true); v = o > v ? o : v;     // row_mirror
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

__device__ __forceinline__ double nhp_wave_sum_shfl(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over a block of NW waves; result valid in thread 0.  `red` holds >= NW doubles.
template <int NW>
__device__ __forceinline__ double nhp_block_sum_n(double v, double *red)
{
    v = nhp_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NW; ++w) s += red[w];
    return s;
}

__device__ __forceinline__ double nhp_block_sum(double v, double *red) { return nhp_block_sum_n<NHP_WAVES>(v, red); }

// Two sums with one pair of barriers; results valid in thread 0.  `red` holds >= 2·NW doubles.
template <int NW>
__device__ __forceinline__ void nhp_block_sum2_n(double &x, double &y, double *red)
{
    x = nhp_wave_sum(x);
    y = nhp_wave_sum(y);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = x; red[NW + (threadIdx.x >> 6)] = y; }
    __syncthreads();
    double sx = 0.0, sy = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NW; ++w) { sx += red[w]; sy += red[NW + w]; }
    x = sx; y = sy;
}

// Phase ablation for timing experiments (tools/ablate.sh): compiled in only with -DNHP_ABLATE,
// where env NHP_DBG selects phases to skip (results are then wrong by design).
#ifdef NHP_ABLATE
#define NHP_SKIP(a, bit) ((a).dbg & (bit))
#else
#define NHP_SKIP(a, bit) 0
#endif

// workgroup size of the windowed log-likelihood kernel (its own knob: more waves per staged column)
#ifndef NHP_WBLOCK
#define NHP_WBLOCK 256
#endif
