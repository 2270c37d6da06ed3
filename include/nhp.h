/*
 * include/nhp.h -- C ABI of libnhp.so, the MI355X (gfx950) hot path for network Hawkes
 * processes.
 *
 * The reference (cswaney/NetworkHawkesProcesses.jl v0.1.0) is pure Julia and has no FFI:
 * its "plug-in API" is multiple dispatch on Baseline / ImpulseResponse / Weights / Network
 * components composed into process structs (src/continuous.jl:108-112,315-321;
 * src/discrete.jl:161-170,395-402).  This header is the boundary a Julia shim binds with
 * `ccall`: each component lowers to plain arrays + a kind enum in
 * nhp_cont_model_desc, and each entry point below replaces the Julia method cited next to
 * it.  Citations are file:line in the reference checkout.
 *
 * Conventions
 *  - Julia layout is kept so the shim passes its arrays untouched: matrices are
 *    column-major, X[p,c] at p + c*N (p = parent node, c = child node,
 *    src/continuous.jl:303); theta[p,c,b] at p + c*N + b*N*N; data[n,t] at n + t*N;
 *    convolved[t,n,b] at t + n*T + b*T*N.
 *  - `nodes` are the reference's 1-based Int64 (src/continuous.jl:14).  Parent indices
 *    returned are 1-based event indices, 0 = baseline (src/parents.jl:41-45).
 *  - Host pointers are borrowed for the duration of the call only.  Device memory belongs
 *    to the ctx / dataset / model handles and is released by the *_destroy functions.
 *  - No exception crosses the boundary: every function returns an nhp_status; the message
 *    is available from nhp_last_error().  The shim maps NHP_EDOMAIN -> DomainError
 *    (src/baselines.jl:100,106,111,116), NHP_ESHAPE/NHP_EINVAL -> ErrorException
 *    (src/impulses.jl:44-45, src/weights.jl:10-11).
 *  - A ctx owns one HIP device and one stream and is not thread-safe; distinct ctx are
 *    independent (one host thread or process per GPU).
 */
#ifndef NHP_H
#define NHP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    NHP_OK = 0,
    NHP_EINVAL = 1,   /* bad argument / unsorted events */
    NHP_EDOMAIN = 2,  /* negative time or duration, node id out of 1..N, non-positive intensity */
    NHP_ESHAPE = 3,   /* array length does not match the model */
    NHP_ENOMEM = 4,
    NHP_EHIP = 5,     /* HIP runtime error (no device, launch failure, ...) */
    NHP_ENOTIMPL = 6,
    NHP_ERCCL = 7     /* RCCL unavailable (librccl.so.1 not loadable) or a collective failed */
} nhp_status;

enum { NHP_BASELINE_HOMOGENEOUS = 0, NHP_BASELINE_LGCP = 1 };
enum { NHP_IMPULSE_EXPONENTIAL = 0, NHP_IMPULSE_LOGITNORMAL = 1 };

/* flags for nhp_cont_loglik* */
enum {
    NHP_LL_RECURSIVE = 1,        /* loglikelihood(...; recursive=true) for exponential impulses
                                    (src/continuous.jl:212-214,361-363): O(M*N) recursion that
                                    ignores dt_max; for other impulses the flag is ignored, as
                                    in the reference */
    NHP_LL_FULL_RECURSION = 2,   /* with NHP_LL_RECURSIVE: always run the O(M*N) recursion, never its
                                    truncated-window evaluation (same value to fp64 resolution) */
};
/* further flags of nhp_cont_vb_step / nhp_cont_vb_run, or-ed to the ones above */
enum {
    NHP_VB_RESUME = 256,         /* nhp_cont_vb_run: S, R hold a state on entry and the run continues it (x is output only) */
    NHP_VB_FROM_MODEL = 512,     /* nhp_cont_vb_step: step from the model's current parameters, used as if they were a
                                    surrogate (iteration 0 of a run), instead of from the state in S, R */
    NHP_VB_DENSE_NETWORK = 1024, /* nhp_cont_netvb_step / _run: a DenseNetworkModel (ρ ≡ 1): ρv ≡ 1 is written, no network update
                                    runs, net[2..3] are ignored and Q's (αv, βv) pass through */
};

typedef struct nhp_ctx nhp_ctx;
typedef struct nhp_cont_dataset nhp_cont_dataset;
typedef struct nhp_cont_model nhp_cont_model;
typedef struct nhp_disc_dataset nhp_disc_dataset;
typedef struct nhp_comm nhp_comm;      /* RCCL communicator bound to a ctx (multi-GPU section at the end) */

/* The lowered form of (Baseline, ImpulseResponse, Weights, adjacency_matrix):
 *   HomogeneousProcess.λ                      src/baselines.jl:27-39
 *   LogGaussianCoxProcess.x / .λ              src/baselines.jl:148-173 (evaluator only)
 *   ExponentialImpulseResponse.θ / .Δtmax     src/impulses.jl:30-37
 *   LogitNormalImpulseResponse.μ / .τ / .Δtmax src/impulses.jl:138-148
 *   DenseWeightModel.W                        src/weights.jl:47-55
 *   ContinuousNetworkHawkesProcess.adjacency_matrix  src/continuous.jl:315-321 */
typedef struct {
    int32_t n_nodes;
    int32_t baseline_kind;
    const double *lambda0;   /* homogeneous: [N]; LGCP: [N*grid_n], node c at c*grid_n */
    const double *grid_x;    /* LGCP grid points [grid_n], strictly increasing, x[0] = 0 */
    int32_t grid_n;          /* 0 for the homogeneous baseline */
    int32_t impulse_kind;
    const double *theta;     /* exponential: [N*N] */
    const double *mu;        /* logit-normal: [N*N] */
    const double *tau;       /* logit-normal: [N*N] */
    double dt_max;           /* must equal the dataset's dt_max */
    const double *W;         /* [N*N] */
    const double *A;         /* [N*N] of 0.0/1.0, or NULL for the standard (dense) process */
} nhp_cont_model_desc;

/* Gibbs sufficient statistics emitted by the parent sampler in the same pass
 * (src/baselines.jl:87-96; src/parents.jl:61-79; src/impulses.jl:84-96,216-252).
 * Any pointer may be NULL.  All are [N] or [N*N] column-major doubles, as the reference
 * stores counts in Float64 `zeros`. */
typedef struct {
    double *cnt0;   /* [N]   baseline-attributed events per node */
    double *Mn;     /* [N]   events per node */
    double *Mnm;    /* [N*N] events on c attributed to a parent on p */
    double *Xnm;    /* [N*N] exponential: mean Δt (NaN -> 0); logit-normal: mean log(Δt/(Δtmax-Δt)) (NaN kept) */
    double *Vnm;    /* [N*N] logit-normal: Σ (log-duration - Xnm)^2; untouched for exponential */
} nhp_cont_stats;

/* ---- context ------------------------------------------------------------------------- */
nhp_status nhp_ctx_create(int32_t device, nhp_ctx **out);
void nhp_ctx_destroy(nhp_ctx *ctx);
const char *nhp_last_error(const nhp_ctx *ctx);      /* ctx may be NULL: last global error */
nhp_status nhp_ctx_synchronize(nhp_ctx *ctx);
/* hipEvent pair on the ctx stream, for measuring kernel time without host overhead */
nhp_status nhp_ctx_timer_start(nhp_ctx *ctx);
nhp_status nhp_ctx_timer_stop(nhp_ctx *ctx, double *elapsed_ms);
int32_t nhp_abi_version(void);
/* sizeof / offsetof of every struct that crosses this boundary, so a binding (ctypes Structure, Julia `struct`) can
 * assert its layout against the library it loaded instead of trusting a header it cannot include.  Writes up to `cap`
 * int32 entries into `out` and returns the number of entries the library has (NHP_ABI_LAYOUT_LEN):
 *   [0] sizeof(nhp_cont_model_desc), then offsetof n_nodes, baseline_kind, lambda0, grid_x, grid_n, impulse_kind, theta, mu,
 *       tau, dt_max, W, A                                                            (entries 1..12)
 *   [13] sizeof(nhp_gibbs_priors), then offsetof alpha0, beta0, kappa, nu, a, b, mu_mu, kappa_mu   (14..21)
 *   [22] sizeof(nhp_cont_stats), then offsetof cnt0, Mn, Mnm, Xnm, Vnm                             (23..27)
 *   [28] NHP_MAX_SLOTS, [29] NHP_COMM_ID_BYTES */
#define NHP_ABI_LAYOUT_LEN 30
int32_t nhp_abi_layout(int32_t *out, int32_t cap);

/* ---- continuous data: (events, nodes, duration)  src/continuous.jl:14,29-36 ----------- */
/* Validates (sorted, >= 0, nodes in 1..N, duration >= 0), runs the look-back pre-pass for
 * dt_max (window starts, node buckets, work partition) and uploads once. */
nhp_status nhp_cont_dataset_create(nhp_ctx *ctx, const double *events, const int64_t *nodes,
                                   int64_t n_events, int32_t n_nodes, double duration,
                                   double dt_max, nhp_cont_dataset **out);
/* Column shard of the same data for evaluating ONE log-likelihood / gradient on several GPUs (second
 * way): the log-likelihood (src/continuous.jl:216-237) is a sum over child nodes c of
 *   -∫λ0_c - Σ_p cnt[p]·[A·]W[p,c] + Σ_{i: c_i = c} log λ_i
 * and the gradient is block-separable in the same columns.  The shard holds every event (all of them are parents) but
 * evaluates only the children on the 0-based nodes [col_begin, col_end); nhp_cont_loglik / _enqueue / _batch / _grad
 * on it return that part (gradient entries of other columns are 0), so the parts of a partition of [0, n_nodes) add up
 * to the whole -- one scalar (or P-vector) all-reduce per evaluation.  The Gibbs sweep is separable in the same way
 * (parents of the children on c, the statistics and conjugate draws of column c and the sweep of A[:, c] involve column c
 * only, and every random stream is keyed by global event / entry indices), so nhp_cont_resample_parents,
 * nhp_cont_gibbs_step and nhp_cont_resample_adjacency on a shard update exactly their columns -- with the same values
 * a whole-dataset sweep gives them -- and leave the rest untouched (returned parents / statistics of other columns are
 * 0; n_links counts the shard's links).  nhp_cont_event_intensity and nhp_cont_lgcp_loglik need every column and
 * return NHP_ENOTIMPL on a shard. */
nhp_status nhp_cont_dataset_create_columns(nhp_ctx *ctx, const double *events, const int64_t *nodes,
                                           int64_t n_events, int32_t n_nodes, double duration, double dt_max,
                                           int32_t col_begin, int32_t col_end, nhp_cont_dataset **out);
/* The same dataset nhp_cont_dataset_create_columns makes -- every device array byte for byte, every scalar equal --
 * with its pre-pass run on the device (window starts, node bucketing and window sort by a stable radix sort, pair
 * offsets, child-slice rows, event records); only the work partition is decided on the host, by the same code.
 * input_on_device = 0: events / nodes are host pointers (one raw upload, then the device build);
 * input_on_device = 1: they are device pointers on ctx's device, read on ctx's stream (the caller orders its own producer
 * before the call); they are not read after the call returns: the dataset owns copies.  Errors (status and message)
 * are those of nhp_cont_dataset_create_columns. */
nhp_status nhp_cont_dataset_create_device(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t n_events,
                                          int32_t n_nodes, double duration, double dt_max, int32_t col_begin,
                                          int32_t col_end, int32_t input_on_device, nhp_cont_dataset **out);
/* Several independent recordings ("trials") of one system as ONE dataset.  Trial r = 0 .. n_trials - 1 owns
 * the events [trial_event_offsets[r], trial_event_offsets[r + 1]) and the interval [trial_time_offsets[r],
 * trial_time_offsets[r + 1]] of the stacked clock; `events` are stacked times (the trial's own time + its time offset,
 * ascending over the whole array), duration = trial_time_offsets[n_trials].  Both tables have n_trials + 1 entries and are
 * HOST pointers for every `where`.  The event index, never the time, decides the trial of an event (an event at the end
 * of one trial and one at the start of the next share a stacked time); a trial may be empty (exposure only).
 * No look-back window crosses a trial's first event, and everything made from the windows follows: log-likelihood,
 * gradient, event intensities, the parent sampler and its statistics, the adjacency sweep, EM, the information matrices,
 * map_parents / cascades.  The recursive formulation (NHP_LL_RECURSIVE) is the reference's on each trial alone, summed: it
 * always runs as a window sum that starts at the trial's first event after its local time 0 (exact; a cut shortens it
 * where the model gives one), NHP_LL_FULL_RECURSION included.  nhp_cont_compensator integrates every trial from its own
 * start.  nhp_cont_intensity, nhp_cont_forecast, nhp_cont_lgcp_loglik and every model with an LGCP baseline answer
 * NHP_ENOTIMPL on a dataset of more than one trial.
 * where = 0: host pre-pass; 1: device pre-pass, events / nodes host pointers; 2: device pre-pass, events / nodes device
 * pointers on ctx's device (as nhp_cont_dataset_create_device).  The routes give the same dataset byte for byte, and
 * n_trials = 1 gives the dataset of nhp_cont_dataset_create_columns / _create_device over all columns.
 * Errors beyond theirs: NHP_EINVAL for event offsets that do not start at 0, decrease or do not end at n_events;
 * NHP_EDOMAIN for time offsets that do not start at 0, do not increase strictly or are not finite, and for an event
 * outside its trial's interval; the message names the entry. */
nhp_status nhp_cont_dataset_create_trials(nhp_ctx *ctx, const double *events, const int64_t *nodes, int64_t n_events,
                                          int32_t n_nodes, const int64_t *trial_event_offsets,
                                          const double *trial_time_offsets, int32_t n_trials, double dt_max, int32_t where,
                                          nhp_cont_dataset **out);
/* *n_trials (1 for a dataset of the other entry points) and, where not NULL, the event offsets [n_trials + 1], the time
 * offsets [n_trials + 1] and per trial the first event index whose time is not exactly the trial's start [n_trials] */
nhp_status nhp_cont_dataset_get_trials(const nhp_cont_dataset *ds, int32_t *n_trials, int64_t *event_offsets,
                                       double *time_offsets, int64_t *first_positive);
void nhp_cont_dataset_destroy(nhp_cont_dataset *ds);
/* Σ_i K_i: parent-child pairs inside the look-back window (SURVEY 8d F_alg) */
int64_t nhp_cont_dataset_pairs(const nhp_cont_dataset *ds);
/* Introspection (tests, tools): copy one of the dataset's arrays to host memory.  *bytes = its size (0: the dataset has no
 * such array); out = NULL asks for the size only; NHP_ESHAPE if cap_bytes is smaller. */
enum {
    NHP_DS_TIMES = 0, NHP_DS_NODES = 1, NHP_DS_EV = 2, NHP_DS_EV8 = 3, NHP_DS_POFF = 4, NHP_DS_SL_ROW = 5,
    NHP_DS_SL_ITEM0 = 6, NHP_DS_CHILD = 7, NHP_DS_CHILD_W = 8, NHP_DS_WPOS = 9, NHP_DS_BOFF = 10, NHP_DS_ITEMS = 11,
    NHP_DS_CNT = 12, NHP_DS_PAIR_OFF = 13,
    NHP_DS_CHILD_CUT = 14,       /* the children with the recursive route's truncated-window starts (nhp_child, bucket order);
                                  * none before the first evaluation that took the window */
    NHP_DS_N_ARRAYS = 15
};
nhp_status nhp_cont_dataset_export(nhp_ctx *ctx, const nhp_cont_dataset *ds, int32_t which, void *out, int64_t cap_bytes,
                                   int64_t *bytes);
/* the dataset's scalars as int64, in this order: M, N, pairs, group, n_items, max_item, max_window, n_zero_time,
 * all_sole, sl_rows, n_slices, sl_nb, sl_max_rows and the bit patterns of t_last, ev8_t0, ev8_scale; writes
 * min(cap, NHP_DS_N_SCALARS) values */
#define NHP_DS_N_SCALARS 16
nhp_status nhp_cont_dataset_scalars(const nhp_cont_dataset *ds, int64_t *out, int32_t cap);

/* ---- continuous model: device-resident parameter blob --------------------------------- */
nhp_status nhp_cont_model_create(nhp_ctx *ctx, const nhp_cont_model_desc *desc, nhp_cont_model **out);
/* re-upload all parameters (same kinds / shapes as at creation) */
nhp_status nhp_cont_model_update(nhp_ctx *ctx, nhp_cont_model *model, const nhp_cont_model_desc *desc);
/* params!(process, x) for the standard process: x = [λ0; θ | μ; τ; W]  src/continuous.jl:121-129 */
nhp_status nhp_cont_model_set_params(nhp_ctx *ctx, nhp_cont_model *model, const double *x, int64_t len);
void nhp_cont_model_destroy(nhp_cont_model *model);

/* ---- loglikelihood(process, data; recursive)  src/continuous.jl:210-276,360-442 -------- */
nhp_status nhp_cont_loglik(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                           int32_t flags, double *ll);
/* Asynchronous form for batches (finite-difference sweeps, chains): enqueue evaluations
 * into result slots [0, NHP_MAX_SLOTS), then fetch them with one synchronisation.
 * Ordering: evaluations enqueued in succession may run concurrently -- odd and even slots go to the context's two
 * internal streams, so alternate the slots to overlap them; two evaluations into the same slot stay in order.  Each
 * evaluation is ordered after every earlier call on the context that is not an enqueue (parameter uploads, dataset
 * builds, samplers, nhp_ctx_timer_start) and before every later one (nhp_cont_model_set_params, the destroy functions,
 * ...), so a model or dataset may be changed or destroyed right after the enqueue.  A slot's value EXISTS only after the
 * next joining call on the context -- any call that is not an enqueue; the caller reads it after nhp_ctx_fetch,
 * nhp_ctx_synchronize or nhp_ctx_timer_stop.  An evaluation over a dataset's child slices leaves the partial sums of its
 * workgroups in a buffer the CONTEXT keeps for the slot and marks the slot pending; the joining call adds up every pending
 * slot in one small launch, in the order the evaluation itself would have used (the same bits), before it does anything
 * else.  The buffer is the context's, so the sum is still made when the slot's dataset or model has been destroyed in
 * between; a later evaluation into the slot replaces the earlier one, pending or not.  NHP_DEFER_FINALIZE=0 in the
 * environment when the context is created: every evaluation adds its own sums up (one launch each, nothing pending).
 * Inside a streak of enqueues an evaluation may be LAUNCHED only at the next enqueue or at the next joining call,
 * whichever comes first: two evaluations on one dataset's child slices (exponential impulses, flat baselines, different
 * slots) then share one pass over its records.  Nothing else changes: the evaluation reads the parameters its model had
 * when it was enqueued (a joining call launches what is held before it does anything else), each slot gets the bits
 * nhp_cont_loglik gives for its model, two evaluations into one slot stay in order, and an enqueue that no other enqueue
 * precedes since the last joining call starts at once.  NHP_PAIR_ENQUEUE=0 when the context is created: one launch
 * per evaluation, at the enqueue.
 * The recursive formulation (NHP_LL_RECURSIVE, exponential impulses) is not overlapped: it is a call like any other. */
#define NHP_MAX_SLOTS 4096
nhp_status nhp_cont_loglik_enqueue(nhp_ctx *ctx, const nhp_cont_dataset *ds,
                                   const nhp_cont_model *model, int32_t flags, int32_t slot);
nhp_status nhp_ctx_fetch(nhp_ctx *ctx, int32_t first_slot, int32_t n, double *out);
/* nb log-likelihoods of nb device-resident models on one dataset (the 2P objective calls of a
 * finite-difference gradient, a population of chains), one synchronisation.  The evaluations are independent, so at
 * short windows compatible models share one pass over the data (up to eight per launch) and the launches alternate
 * between the context's two internal streams; every result is the same as from nhp_cont_loglik on that model. */
nhp_status nhp_cont_loglik_batch(nhp_ctx *ctx, const nhp_cont_dataset *ds,
                                 const nhp_cont_model *const *models, int32_t nb, int32_t flags, double *ll);

/* log-likelihood and its analytic gradient in params! order [λ0; θ | μ; τ; W] (homogeneous
 * baseline).  Replaces the 2P finite-difference objective calls Optim makes inside mle!
 * (src/continuous.jl:144-198). */
nhp_status nhp_cont_loglik_grad(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                                int32_t flags, double *ll, double *grad, int64_t grad_len);

/* total_intensity at every event, λ_{c_i}(t_i)  src/continuous.jl:286-300,391-405 */
nhp_status nhp_cont_event_intensity(nhp_ctx *ctx, const nhp_cont_dataset *ds,
                                    const nhp_cont_model *model, double *lambda /* [M] */);

/* intensity(process, data, times) -> Q x N column-major  src/continuous.jl:76-96 */
nhp_status nhp_cont_intensity(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                              const double *times, int64_t n_times, double *out);

/* resample_parents(process, data)  src/parents.jl:1-46.  One categorical draw per event from
 * an explicit uniform stream: `u` (host, [M]) if non-NULL, else Philox4x32-10 keyed by
 * (seed, step, event index).  parents / parentnodes may be NULL (statistics only). */
nhp_status nhp_cont_resample_parents(nhp_ctx *ctx, const nhp_cont_dataset *ds,
                                     const nhp_cont_model *model, const double *u,
                                     uint64_t seed, uint64_t step,
                                     int64_t *parents, int64_t *parentnodes, nhp_cont_stats *stats);
/* One Gibbs sweep of resample!(process, data) (src/continuous.jl:202-208,350-358) entirely on the
 * device: parents + statistics as above, then the conjugate draws of HomogeneousProcess
 * (src/baselines.jl:72-77), DenseWeightModel (src/weights.jl:59-64) and the impulse response
 * (src/impulses.jl:68-73 or :204-214) written straight into the device-resident model.  Draws are
 * Philox-keyed by (seed, step, element): reproducible; distributionally (not bitwise) equal to
 * Julia's samplers.  The adjacency matrix is left unchanged. */
typedef struct {
    double alpha0, beta0;    /* HomogeneousProcess.α0, β0 */
    double kappa, nu;        /* DenseWeightModel.κ, ν */
    double a, b;             /* ExponentialImpulseResponse.α, β  |  LogitNormalImpulseResponse.α0, β0 */
    double mu_mu, kappa_mu;  /* LogitNormalImpulseResponse.μμ, κμ */
} nhp_gibbs_priors;
/* Asynchronous: the sweep is enqueued and the call returns without draining the GPU, so a chain keeps one sweep in
 * flight.  The sampler's only run-time failure (the weights of some event do not sum to a positive finite value, the
 * error nhp_cont_resample_parents reports at once) therefore surfaces as NHP_EDOMAIN from the NEXT nhp_cont_gibbs_step
 * on this context, or from the next call that synchronises it (nhp_ctx_synchronize, the parameter / moment / result
 * downloads), once. */
nhp_status nhp_cont_gibbs_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model,
                               const nhp_gibbs_priors *priors, uint64_t seed, uint64_t step);
/* resample_adjacency_matrix!(process, data)  src/continuous.jl:444-487: one Gibbs sweep over the
 * N x N adjacency matrix of the device-resident model (updated in place).  Link probabilities
 * (src/networks.jl:65-68): `rho_matrix` [N*N] if non-NULL, else the scalar `rho`.  Bernoulli draws
 * (u <= p, as Distributions.jl) use `u` [N*N] if non-NULL, else Philox keyed (seed, step, p + c*N).
 * A_out (nullable) receives the new matrix, n_links (nullable) its number of ones (the statistic
 * BernoulliNetworkModel's resample! needs, src/networks.jl:70-78). */
nhp_status nhp_cont_resample_adjacency(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model,
                                       const double *rho_matrix, double rho, const double *u,
                                       uint64_t seed, uint64_t step, double *A_out, double *n_links);
/* loglikelihood(process::LogGaussianCoxProcess, data, node, y)  src/baselines.jl:247-254, for all
 * nodes in one call: ll[c] = -trapezoid(lam_c) + Σ log lam_c(t_i) over node c's events that
 * split_extract (:227-238) attributes to the baseline (sampled parent node 0).  lam [N*grid_n]
 * (node c at c*grid_n) is the candidate intensity exp.(m .+ y_c) on grid_x [grid_n].  The
 * attribution is `parentnodes` [M] (resample_parents' second vector) if non-NULL -- it then
 * stays on the device with the dataset -- else the one left there by the latest
 * nhp_cont_resample_parents / nhp_cont_gibbs_step on this dataset.  NHP_EDOMAIN if an event lies
 * outside [grid_x[0], grid_x[end]] (the interpolator's DomainError, src/utils/interpolation.jl:27). */
nhp_status nhp_cont_lgcp_loglik(nhp_ctx *ctx, const nhp_cont_dataset *ds, const int64_t *parentnodes,
                                const double *grid_x, int32_t grid_n, const double *lam, double *ll);
/* rand(process, duration)  src/continuous.jl:16-48,131-142,335-348 on the device, from the device-resident model (so a
 * posterior-predictive draw from the state nhp_cont_mcmc_run leaves needs no download).  Generation-wise branching:
 * Poisson immigrants per node (homogeneous: Poisson(λ0_c T) at uniform positions on [0, T); LGCP: Poisson(trapezoid ∫λ_c)
 * positions by rejection from the piecewise-linear λ_c, src/baselines.jl:190-210), then Poisson(R_p) children per event,
 * R_p = Σ_c W[p,c]·A[p,c], child node c with probability W[p,c]·A[p,c] / R_p, delay Exp(θ[p,c]) (not cut at dt_max,
 * src/impulses.jl:53-66) or dt_max·logistic(μ[p,c] + Z/√τ[p,c]) (src/impulses.jl:180-202); events after `duration`
 * are dropped with their descendants.
 * Outputs: buffers of capacity max_events, host or device pointers by output_on_device (as input_on_device of
 * nhp_cont_dataset_create_device); times ascending, nodes 1-based, parents (nullable) 0 for a baseline event, else the
 * 1-based index of the parent in the returned order (a parent precedes its children).  Synchronous: the ctx stream is
 * drained before the call returns.  Errors: NHP_EDOMAIN for a negative / non-finite duration, an LGCP duration other than
 * the grid's end ("Sample duration does not match process duration.", src/baselines.jl:191), or parameters no process
 * has (negative / non-finite weights or baseline, θ <= 0 or τ <= 0 on a link with weight, a row total W·A above 2^32);
 * NHP_EINVAL for null pointers or max_events outside [0, 2^31); NHP_ENOMEM "branching process exploded (unstable
 * weights?)" when the kept events pass max_events (nothing is written past the buffers; the ctx stays usable).
 * The result depends on (model, duration, seed) only -- not on max_events or launch geometry.  Random numbers: the
 * Philox4x32-10 block of nhp_rng.h, counter (c0, c1, c2, c3) = (e mod 2^32, (e >> 32) ^ (attempt << 8), step mod 2^32,
 * step >> 32), key = seed ^ F for a family constant F, ten rounds; of the four output words, ua = (((w0:w1) >> 11) + 1)·2^-53
 * and ub = (((w2:w3) >> 11) + 1)·2^-53 lie in (0, 1], u = ua - 2^-53 in [0, 1).  Poisson(m): m <= 0 -> 0; m < 10 inversion
 * with u of attempt 0 (p = e^-m, F = p, k = 0; while u >= F and k < 100: k += 1, p = p·m/k, F += p); m >= 10 PTRS (Hörmann
 * 1993) with U = u - 0.5 and V = ub of attempt 0, 1, 2, ...  Families, in draw order:
 *   0x9E3779B97F4A7C15  immigrant count of node c:  Poisson(λ0_c T | ∫λ_c), step 0, e = c
 *   0xBF58476D1CE4E5B9  immigrant k (immigrants numbered node by node): step 0, e = k; t = u·T (attempt 0); LGCP: attempt
 *                       a = 0, 1, ... until ub·max λ_c <= λ_c(t)
 *   0x94D049BB133111EB  child count of event i: Poisson(R_node), step = generation of i (immigrants 0), e = arena index i
 *   0xD6E8FEB86659FD93  child slot s of generation g (slots numbered by parent arena index, then child): step g, e = s;
 *                       attempt 0: node = first c with prefix_p[c] > u·R_p (sequential row prefix of W∘A; if none, the first
 *                       prefix_p[c] >= u·R_p), exponential delay -log(ub)/θ; attempt 1: Z = sqrt(-2 log ua)·cos(2π w2/2^32)
 * The arena holds the immigrants (index k), then each generation's surviving children in slot order.  Output order: a
 * stable sort of the arena by time. */
nhp_status nhp_cont_simulate(nhp_ctx *ctx, const nhp_cont_model *model, double duration, uint64_t seed, int64_t max_events,
                             int32_t output_on_device, double *times, int64_t *nodes, int64_t *parents /* nullable */,
                             int64_t *n_events);
/* The compensator Λ_c(t) = ∫ λ_c(s) ds from 0 (LGCP baseline: from grid_x[0]) to t, exactly, of the intensity as
 * nhp_cont_intensity evaluates it (src/continuous.jl:84-96) -- the reference has no such function: its log-likelihood
 * charges every event the full mass ΣW ("approximate (exact requires cdf)", src/continuous.jl:247).  Conventions of the
 * intensity, literally: parents of time t are the events with t - dt_max < t_i < t (both strict); link weight W[p,c]
 * (times A[p,c]); the exponential impulse θ e^{-θd} is cut at dt_max and not renormalised; the logit-normal pdf at
 * x = d/dt_max is NOT divided by dt_max, so a link's total mass is W·dt_max; homogeneous baseline λ0_c; LGCP baseline = the
 * piecewise-linear interpolant of (grid_x, λ_c), integrated exactly (a trapezoid per cell, a partial last cell).  With
 *   H_{p,c}(d) = ∫_0^{min(d,dt_max)} pdf_{p,c} = 1 - e^{-θ min(d,dt_max)}                     (exponential)
 *                                             = dt_max·Φ(√τ (logit(d/dt_max) - μ)) for d < dt_max, dt_max from there on   (logit-normal)
 *   Λ_c(t) = base_c(t) + Σ_{i: t_i < t} W[n_i,c]·A[n_i,c]·H_{n_i,c}(t - t_i).
 * Outputs (each nullable, not all three), events in the caller's (time) order:
 *   at_events[k] = Λ_{n_k}(t_k), the compensator of the event's own node at the event;
 *   residuals[k] = Λ_{n_k}(t_k) - Λ_{n_k}(t_prev), t_prev the previous event of the same node (the lower limit for the
 *                  node's first event): i.i.d. Exp(1) under the true model (time rescaling);
 *   total[c]     = Λ_c(duration): the expected number of events of node c.
 * Host or device pointers by output_on_device (as in nhp_cont_simulate).  Synchronous; fp64 sums in a fixed order, so the
 * results are identical from run to run.  Errors: NHP_EINVAL (null handles, no output requested), the dataset / model
 * mismatches of the other entry points, NHP_EDOMAIN (an event or the duration outside the LGCP grid), NHP_ENOTIMPL on a
 * column shard and when a node's columns of the parameter tables exceed the 160 KiB of LDS. */
nhp_status nhp_cont_compensator(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                                int32_t output_on_device, double *at_events /* [M] nullable */,
                                double *residuals /* [M] nullable */, double *total /* [N] nullable */);
/* map_parents(process, data): the posterior-mode parent of every event and its posterior probability -- the reference has no
 * such function.  The categories of event i are those of nhp_cont_resample_parents in its order: the events i-1, i-2, ...,
 * down to the first of the look-back window with weight A·W·ħ(t_i - t_j), then the baseline λ0_c(t_i); weights are the
 * sampler's bits.  parents[i] = 0 (baseline) or the 1-based event index, parentnodes[i] = 0 or the 1-based node, prob[i] =
 * w_max / Σw.  The FIRST maximum in category order wins: of equal parent weights the most recent, a parent before the
 * baseline.  The first event gets (0, 0) and prob 1.  Sums in a fixed order: two calls give the same bits.  Outputs are host
 * or device pointers by output_on_device (as in nhp_cont_compensator).  Synchronous.  Errors: NHP_EINVAL (null handles, no
 * output requested), the dataset / model mismatches of the other entry points, NHP_EDOMAIN when some event's weights do
 * not sum to a positive finite value, NHP_ENOTIMPL on a column shard and beyond the 160 KiB LDS column budget. */
nhp_status nhp_cont_map_parents(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                                int32_t output_on_device, int64_t *parents /* [M] nullable */,
                                int64_t *parentnodes /* [M] nullable */, double *prob /* [M] nullable; not all three NULL */);
/* cascades(process, data, parents): the forest a parent vector forms on the dataset's events.  parents[k] (k = 0 .. M-1) is 0
 * for an immigrant, else the 1-based index of an event that precedes k: 1 <= parents[k] <= k (the convention of
 * nhp_cont_resample_parents / nhp_cont_simulate / nhp_cont_map_parents); anything else is NHP_EDOMAIN, checked on the device
 * before anything is written.  `parents` is a host or a device pointer by parents_on_device, the array outputs by
 * output_on_device; n_cascades and n_rounds are host pointers.
 *   per event:    root[k] 1-based index of the immigrant ancestor (k + 1 for an immigrant), generation[k] 0 for an immigrant
 *                 else the parent's + 1, descendants[k] the events of k's subtree, k excluded
 *   per cascade:  one per immigrant in ascending root order, *n_cascades of them (capacity M; all four arrays or none):
 *                 casc_root, casc_size (root included), casc_depth (largest generation), casc_end (time of the last event)
 *   per node:     immigrants[c] roots on node c, offspring[c] = Σ descendants over the events on c, reach[p + c*N] events on
 *                 node c whose root is on node p, roots included (Σ reach = M)
 * O(M log depth) by pointer doubling, *n_rounds rounds (<= 31); integer atomics only: identical from run to run.  M < 2^31.
 * Synchronous.  NHP_EINVAL (null handles, some but not all cascade arrays), NHP_ENOTIMPL on a column shard. */
nhp_status nhp_cont_cascades(nhp_ctx *ctx, const nhp_cont_dataset *ds, const int64_t *parents /* [M] */,
                             int32_t parents_on_device, int32_t output_on_device,
                             int64_t *root, int64_t *generation, int64_t *descendants /* [M] each, nullable */,
                             int64_t *casc_root, int64_t *casc_size, int64_t *casc_depth, double *casc_end,
                             int64_t *n_cascades /* host, nullable */, int64_t *immigrants, int64_t *offspring /* [N] nullable */,
                             int64_t *reach /* [N*N] column-major, nullable */, int32_t *n_rounds /* host, nullable */);
/* forecast(process, data, horizon): `nsamples` = S independent continuations of the observed events on (T0, T0 + h], T0 = the
 * dataset's duration, h = horizon, conditional on those events -- the reference has no such function.  The law is the
 * GENERATIVE model's, the one nhp_cont_simulate samples (src/continuous.jl:16-48), not the likelihood's convention: exponential
 * delays are not cut at dt_max, and a link's expected child count is W[p,c]·A[p,c] for both impulse kinds (the logit-normal
 * mass carries no dt_max factor, unlike nhp_cont_compensator).  With the delay CDF F_pc(d) = -expm1(-θ d) (exponential) or
 * Φ(√τ (logit(d/dt_max) - μ)) for 0 < d < dt_max, 0 below and 1 from there on (logit-normal), one continuation is the union of
 * three independent parts, exactly:
 *   carry-over: the not-yet-realised direct children of the observed events; event j (node p, time t_j) has
 *     Poisson(W[p,c]A[p,c]·(F_pc(T0+h-t_j) - F_pc(T0-t_j))) of them on node c, their delays from F_pc given the interval;
 *   new immigrants: Poisson(λ0_c h) per node, uniform on (T0, T0+h];
 *   descendants of both, by the generation loop of nhp_cont_simulate with the end time Tend = fl(T0 + h).
 * Exponential impulses (memoryless): the events of node p enter through G[p,c] = Σ_{j on p} e^{-θ[p,c](T0 - t_j)} (one fp64 running
 * sum per (p,c) over p's events in time order, terms below e^-708 are exactly 0: at most M·N exponentials, once per call), the
 * carry mass of a link is m[p,c] = W·A·G·(-expm1(-θh)), CP[p,c] = the running sum of m[0..p, c] over p, carry[c] = CP[N-1, c].
 * Logit-normal impulses (thinning): the events with T0 - t_j < dt_max (j >= w0, Wn of them) are the parents of generation 0 in
 * every replica, draw Poisson(R_p) children as every event does, and the children with T0 < t <= Tend stay;
 * carry[c] = Σ_{j >= w0} W·A·(F(Tend - t_j) - F(T0 - t_j)) in time order.
 * Outputs, host or device pointers by output_on_device (as in nhp_cont_simulate):
 *   carry[N] (nullable): the expected number of carry-over events per node, deterministic (fixed-order fp64 sums);
 *   counts[S*N], replica-major: the events of node c in (T0, Tend] in replica r;
 *   times / nodes [capacity max_events] and offsets[S+1] (all three or none): replica r owns [offsets[r], offsets[r+1]), its
 *     times absolute and ascending, its nodes 1-based; counts[r, :] is the bincount of its nodes.  Order: a stable sort of the
 *     kept events by time, then stably by replica;
 *   phase_ms[2] (nullable, host): wall milliseconds of the boundary state (tables, G, carry masses) and of the ensemble.
 * max_events caps the kept events of all replicas together.  The result depends on (model, dataset, horizon, nsamples, seed)
 * only -- not on max_events, the chunk size or launch geometry; replica r's draws are NOT promised to be the same for different
 * nsamples.  Synchronous.  Errors: NHP_EDOMAIN for a negative / non-finite horizon or the parameter checks of
 * nhp_cont_simulate; NHP_EINVAL for null handles, nsamples < 1, max_events outside [0, 2^31), paths given in part; the dataset /
 * model mismatches of the other entry points; NHP_ENOTIMPL for an LGCP baseline (the grid ends where the data end), a column
 * shard, nsamples·N >= 2^30 or nsamples·Wn + max_events >= 2^31 (32-bit arena indices; no kernel stages a table in LDS, so N
 * itself has no limit); NHP_ENOMEM "branching process exploded (unstable weights?)" when the kept events pass max_events
 * (nothing is written past the buffers; the ctx stays usable).
 * Random numbers: the Philox block, uniforms ua, ub, u and the Poisson sampler of nhp_cont_simulate above, with these families
 * (key = seed ^ F), in draw order; e = r·N + c numbers the (replica, node) pairs:
 *   0xA0761D6478BD642F  immigrant count of (r, c): Poisson(λ0_c·h), step 0, element e
 *   0xE7037ED1A0B428DB  exponential carry-over count of (r, c): Poisson(carry[c]), step 0, element e (logit-normal: none)
 *   0x8EBC6AF09C88C6E3  root k -- roots numbered by e, the immigrants of a pair before its carry-over children: step 0, element k,
 *                       attempt 0; immigrant: t = T0 + ua·h; carry-over child of node c: parent node = first p with
 *                       CP[p,c] > u·carry[c] (if none, the first CP[p,c] >= u·carry[c]), delay d = min(-log1p(-ub·q)/θ[p,c], h) with
 *                       q = -expm1(-θ[p,c]·h), t = T0 + d; a t that rounds to T0 becomes the next double after T0
 *   0x589965CC75374CC3  child count of arena entry i: Poisson(R_node), step = generation of i, element i
 *   0x1D8E4E27C47D124F  child slot s of generation g: step g, element s; node and delay as family 0xD6E8... of nhp_cont_simulate
 * The arena holds [generation 0: entry r·Wn + (j - w0) = window event j in replica r (logit-normal; none for exponential) |
 * generation 1: the roots, entry S·Wn + k, then the surviving children of generation 0 | generation g + 1: the surviving
 * children of generation g], survivors (T0 < t <= Tend) in slot order, slots numbered by parent arena index, then child.
 * Generation 0 is not part of the result. */
nhp_status nhp_cont_forecast(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, double horizon,
                             int32_t nsamples, uint64_t seed, int64_t max_events, int32_t output_on_device,
                             double *carry /* [N] nullable */, int64_t *counts /* [S*N] */, double *times /* nullable */,
                             int64_t *nodes, int64_t *offsets /* [S+1] */, double *phase_ms /* [2] nullable */);
/* params(process) of the device-resident model: [λ0; θ | μ; τ; W]  src/continuous.jl:116-119 */
nhp_status nhp_cont_model_get_params(nhp_ctx *ctx, const nhp_cont_model *model, double *x, int64_t len);
/* process.adjacency_matrix of the device-resident model (after nhp_cont_network_step / nhp_cont_mcmc_run): [N*N] 0.0/1.0 */
nhp_status nhp_cont_model_get_adjacency(nhp_ctx *ctx, const nhp_cont_model *model, double *A, int64_t len);
/* Sample store on the device.  mcmc! appends params(process) after every sweep (src/inference.jl:61):
 * 4N²+N doubles per step, 33.5 MB at N = 1024 -- more PCIe time than the sweep itself.  These keep Σx and Σx² of the
 * device-resident parameters instead: _reset zeroes them, _accumulate adds the current [λ0; θ | μ; τ; W; vec(A) if the
 * model has an adjacency matrix] (call it once per sweep), _fetch returns the two sums and the number of samples;
 * len = N + N²·(1 | 2) + N² [+ N²].  Posterior mean = sum / count, second moment = sumsq / count. */
nhp_status nhp_cont_model_moments_reset(nhp_ctx *ctx, nhp_cont_model *model);
nhp_status nhp_cont_model_moments_accumulate(nhp_ctx *ctx, nhp_cont_model *model);
nhp_status nhp_cont_model_moments_fetch(nhp_ctx *ctx, const nhp_cont_model *model, double *sum, double *sumsq,
                                        int64_t len, int64_t *count);
/* Streaming convergence diagnostics of a chain that keeps no samples: effective sample size, Monte-Carlo standard error and
 * split R-hat of every entry the sums above cover, accumulated in the same pass (csrc/cont_diagnostics.hip: with
 * diagnostics configured, _accumulate launches ONE fused kernel in place of the moments kernel).  The definitions are the
 * contract; tests/chain_diagnostics_ref.py restates them in numpy.
 *
 * One scalar entry x of [λ0; θ | μ; τ; W; vec(A) if any]; kept steps t = 0 … n−1 (one _accumulate each).  Fixed by
 * _configure: batch_len b ≥ 1, n_planned ≥ 0 (the kept steps the chain is going to make), h = ⌊n_planned/2⌋.
 *   S1 = Σx, S2 = Σx²: the sums above -- same expressions, same bits, still in the moments' own planes.
 *   B: sum over the current batch.  At every kept step whose 1-based count is a multiple of b:
 *        m = B/b;  SB += m;  QB += m·m (the product rounded, then added);  B = 0.   A trailing partial batch is never folded in.
 *   snapA = (S1, S2) when the kept count reaches h, snapB = (S1, S2) when it reaches n_planned − h (one copy when
 *        n_planned is even); taken only when h ≥ 2.
 * At fetch, with n kept steps (n ≥ 1), a = ⌊n/b⌋ and pos(v) = v if v > 0, else 0 (so a NaN gives 0):
 *   s²     = pos(S2 − S1·S1/n)/(n−1)
 *   σ²_bm  = b·pos(QB − SB·SB/a)/(a−1);  NaN when a < 2
 *   MCSE   = √(σ²_bm/n)
 *   ESS    = n·s²/σ²_bm, not capped at n;  NaN when s² = 0
 *   split R-hat: only when n = n_planned and h ≥ 2, NaN otherwise.  First half: sums snapA; second half: (S1, S2) − snapB,
 *        h steps each (the middle step of an odd n is dropped).  m_i = S1_i/h, v_i = pos(S2_i − S1_i·S1_i/h)/(h−1),
 *        W = (v₁+v₂)/2, R-hat = √((h−1)/h + (m₁−m₂)·(m₁−m₂)/(2W));  NaN when W = 0.
 *   An entry with s² = 0 (a link of A that never flipped) is "undefined": it is counted and takes no part in any extreme
 *   or count below; so does a NaN (excluded, not counted as undefined).
 * The Bernoulli network's scalar ρ (nhp_cont_model_set_rho) gets the same treatment next to its Σρ, Σρ².  A block network's
 * ρ / π and a latent distance network's b are not diagnosed (labels and positions are not identified anyway).
 *
 * summary [NHP_DIAG_GROUPS * NHP_DIAG_FIELDS], group g at g·NHP_DIAG_FIELDS.  Groups: 0 λ0, 1 θ | μ, 2 τ (no entries for
 * exponential impulses), 3 W, 4 vec(A) (no entries without one), 5 ρ (one entry when the model has a scalar ρ and neither
 * a block nor a latent distance network).  Fields: 0 entries, 1 undefined, 2 min ESS, 3 its index inside the group
 * (p + N·c; −1: none), 4 max R-hat, 5 its index, 6 entries with ESS < ess_below, 7 entries with R-hat > rhat_above,
 * 8 max MCSE.  Ties go to the lower index; an extreme nobody defines is NaN.  The reduction is exact (minima, maxima and
 * integer counts in a fixed order, no atomics): two runs give the same bits.
 *
 * _configure(b, n_planned) allocates 3 planes of len doubles (+ 2 per snapshot: 5–7 when h ≥ 2; ≈ 235 MB for the
 * logit-normal network at N = 1024) and zeroes them and the kept count; (0, 0) turns diagnostics off and frees them.  It
 * leaves the moments alone: configure before the chain's first kept step (or call _moments_reset, which zeroes the
 * diagnostic planes too); a fetch whose diagnostics saw fewer steps than the moments is NHP_EINVAL.  NHP_ENOMEM leaves
 * diagnostics off and the moments usable.  nhp_cont_mcmc_run on a column shard with diagnostics configured is NHP_ENOTIMPL.
 * _fetch: ess, mcse, rhat nullable, [len] each in the order of the sums; NHP_EINVAL with nothing configured or accumulated. */
#define NHP_DIAG_GROUPS 6
#define NHP_DIAG_FIELDS 9
nhp_status nhp_cont_model_diagnostics_configure(nhp_ctx *ctx, nhp_cont_model *model, int64_t batch_len, int64_t n_planned);
nhp_status nhp_cont_model_diagnostics_fetch(nhp_ctx *ctx, const nhp_cont_model *model, double ess_below, double rhat_above,
                                            double *summary, double *ess, double *mcse, double *rhat, int64_t len);
/* Streaming quantiles of a chain that keeps no samples: credible intervals of every parameter entry by the extended P²
 * algorithm (csrc/chain_quantiles.hip), one separate launch after a kept step's _moments_accumulate -- the
 * sums and the diagnostics keep their kernels and their bits, and with nothing configured nothing is launched.  The
 * definition is the contract; tests/chain_quantiles_ref.py restates it in numpy and the tests hold the kernel to it bit
 * for bit.
 *
 * m probabilities 0 < p_1 < … < p_m < 1, 1 ≤ m ≤ NHP_QUANT_MAX; K = 2m + 3 markers.  With p_0 = 0 and p_{m+1} = 1 the marker
 * probabilities are d_{2j} = p_j and d_{2j+1} = (p_j + p_{j+1})/2 (the sum rounded, then halved), so d_0 = 0, d_{K−1} = 1.
 * Per entry: heights q_0 … q_{K−1} (fp64), positions pos_1 … pos_{K−2} (int32; pos_0 = 1 and pos_{K−1} = n are implied) and n,
 * the number of values seen (one host-side counter for all entries).  Feeding a value x:
 *   n < K:  insert x into the sorted prefix q_0 … q_{n−1}, after equal values; n += 1; when n reaches K, pos_i = i + 1.
 *   otherwise, in this order:
 *     1. x < q_0: q_0 = x, k = 0;  else x ≥ q_{K−1}: q_{K−1} = x, k = K − 2;  else k = the largest i ≤ K − 2 with q_i ≤ x.
 *     2. pos_i += 1 for every i > k; n += 1.
 *     3. for i = 1 … K − 2 ascending, each step seeing the positions and heights the earlier ones left:
 *          δ = (1 + (n − 1)·d_i) − pos_i, in fp64 as written (n − 1 and pos_i converted, product, sum, difference);
 *          s = +1 if δ ≥ 1 and pos_{i+1} − pos_i > 1;  s = −1 if δ ≤ −1 and pos_{i−1} − pos_i < −1;  otherwise nothing moves;
 *          a = pos_i − pos_{i−1}, b = pos_{i+1} − pos_i, c = pos_{i+1} − pos_{i−1}, converted to fp64:
 *          q′ = q_i + (s/c)·( ((a + s)·(q_{i+1} − q_i))/b + ((b − s)·(q_i − q_{i−1}))/a );
 *          q_i = q′ if q_{i−1} < q′ < q_{i+1}, else q_i + (s·(q_{i+s} − q_i))/(pos_{i+s} − pos_i);  then pos_i += s.
 * IEEE fp64 + − × ÷ and int32 → fp64 conversions only, every operation rounded on its own (no contraction).
 * At fetch the estimate of p_j is q_{2j}; the smallest and largest value seen are q_0 and q_{K−1}.  With n < K every estimate
 * is NaN while min and max are exact once n ≥ 1 (q_0 and q_{n−1} of the sorted prefix; NaN at n = 0).  A constant entry gives
 * that constant everywhere.
 *
 * Entries: the first P = N + N²·(2 | 3) of the sums' order, [λ0; θ | μ; τ; W].  vec(A) is 0 / 1, its mean says everything: it
 * has no state and its slots of `values`, `min`, `max` are NaN.  effective_weights (fixed at _configure) feeds A[p,c]·W[p,c],
 * ONE rounded product, for W[p,c] of a model with an adjacency matrix -- the quantity whose interval answers "is this link
 * there"; 0: the raw W, as the moments see it.  The Bernoulli network's scalar ρ (nhp_cont_model_set_rho; neither a block nor
 * a latent distance network) has one state of its own: rho [m + 2] = {the m estimates, min, max}, NaN otherwise.
 *
 * _configure(probs, m, every, effective_weights): m = 0 turns quantiles off and frees the planes; anything else (re)allocates
 * K planes of P + 1 doubles and K − 2 of P + 1 int32 (100 bytes per entry at m = 3) and zeroes them and n.  NHP_EINVAL for
 * m > NHP_QUANT_MAX, probabilities that do not increase strictly inside (0, 1), every < 1; NHP_ENOTIMPL for an LGCP baseline;
 * NHP_ENOMEM leaves quantiles off and the moments and diagnostics usable.  _moments_reset zeroes the planes and n too.
 * _accumulate feeds the model's current state (step-by-step drivers call it after _moments_accumulate, on the kept steps they
 * choose); nhp_cont_mcmc_run calls it itself after every `every`-th kept step's _moments_accumulate, counted from the
 * configure or the last _moments_reset, and is NHP_ENOTIMPL on a column shard with quantiles configured.
 * _fetch: values [m][len] (row j: the estimate of p_{j+1}), min, max [len] nullable, rho [m + 2] nullable, len = the sums'
 * length, *count = n; NHP_EINVAL with nothing configured. */
#define NHP_QUANT_MAX 4
nhp_status nhp_cont_model_quantiles_configure(nhp_ctx *ctx, nhp_cont_model *model, const double *probs, int32_t m, int32_t every,
                                              int32_t effective_weights);
nhp_status nhp_cont_model_quantiles_accumulate(nhp_ctx *ctx, nhp_cont_model *model);
nhp_status nhp_cont_model_quantiles_fetch(nhp_ctx *ctx, const nhp_cont_model *model, double *values /* [m][len] */,
                                          double *min, double *max /* [len], nullable */, double *rho /* [m+2], nullable */,
                                          int64_t len, int64_t *count);
/* the uniform stream itself (host side, same bits as the kernel draws) */
void nhp_uniform_stream(uint64_t seed, uint64_t step, int64_t n, double *u);

/* diagnostics: evaluate a device math primitive elementwise (op 0 exp, 1 log, 2 sqrt, 3 x/y,
 * 4 exp for x<=0, 5 exponential pdf(θ=x, Δt=y), 6 logit-normal pdf(τ=x, Δt=y; μ=.25, Δtmax=2), 7 the log-likelihood
 * kernels' table-driven exp for x<=0 (nhp_exp_neg_tab: within 2 ulp, not part of the bitwise contract), 8 θ·e^{-θΔt} through it;
 * the device library's functions as nhp_cont_compensator calls them, good to a few ulp and outside the bitwise contract:
 * 9 -expm1(-x), 10 log(x/(1-x)), 11 0.5*erfc(-0.7071067811865476*x) = Φ(x));
 * lets tests hold the kernels' fixed operation sequences to a bitwise contract, and measure the library functions' errors */
nhp_status nhp_probe_math(nhp_ctx *ctx, int32_t op, const double *x, const double *y, int64_t n, double *out);
/* diagnostics: n device-side random variates with the generators and Philox keying of the Gibbs kernels (nhp_rng.h):
 * kind 0 Gamma(shape a[i], scale b[i]) keyed (seed, step, i); 1 standard normal keyed (seed, step, i); 2 Beta(a[i], b[i]) as
 * X/(X+Y) from Gammas keyed (seed, step, 2i) and (seed, step, 2i+1).  Lets tests hold the draws to their distributions
 * (Kolmogorov-Smirnov) and to known answers of the Philox -> uniform -> variate chain. */
nhp_status nhp_probe_draws(nhp_ctx *ctx, int32_t kind, uint64_t seed, uint64_t step, int64_t n, const double *a, const double *b,
                           double *out);
/* throughput calibration on register operands: mode 0 = exponential pair terms per second (the
 * fp64-VALU ceiling of the windowed kernels), mode 1 = fp64 fma per second */
nhp_status nhp_probe_rate(nhp_ctx *ctx, int32_t mode, int32_t iters, int32_t blocks, double *ops_per_s);
/* gather calibration: n_windows scattered windows of `recs` 16-byte records out of an array of array_recs records,
 * 8 lanes per window, no arithmetic -- microseconds per launch (the floor of the short-window kernels) */
nhp_status nhp_probe_gather(nhp_ctx *ctx, int32_t n_windows, int32_t recs, int64_t array_recs, int32_t blocks,
                            double *us_per_launch);
/* streaming-read calibration: `blocks` workgroups of `threads` (256 | 512) sweep contiguous shares of a `bytes`-byte buffer,
 * mode 0 = 16 bytes per lane, mode 1 = the child slices' two planes (4 + 2 bytes per lane) -- microseconds per launch
 * (launched back to back: below 256 MB the Infinity Cache serves it, as it does the repeated log-likelihood) */
nhp_status nhp_probe_stream(nhp_ctx *ctx, int32_t mode, int64_t bytes, int32_t blocks, int32_t threads, double *us_per_launch,
                            int64_t *bytes_read /* nullable: what a launch really reads (whole rows per wave) */);
/* the mle! optimizer alone (csrc/nhp_lbfgs.h: the projected L-BFGS both nhp_cont_mle_run and nhp_disc_mle_run drive) on the
 * separable quadratic f(x) = 1/2 sum_i h[i] (x[i] - c[i])^2 over the box [lower, upper]^n, host vectors h, c and x (start in,
 * minimiser out): step counts that can be held against another L-BFGS without a likelihood in between */
nhp_status nhp_probe_lbfgs(nhp_ctx *ctx, int64_t n, const double *h, const double *c, double lower, double upper, double f_abstol,
                           int32_t max_steps, double *x, double *loss, int32_t *steps, int32_t *converged, int32_t *evaluations);
/* which way an evaluation with NHP_LL_RECURSIVE goes for (dataset, model): decides exactly as the log-likelihood
 * (recursion_cost 1.0), the gradient (1.2) and the observed information (1e9) decide, caches included, so it may renew the
 * model's bound and the dataset's window starts.  out = {cut (the model's look-back for this dataset; 0: no usable bound or
 * not asked for), used (1: the truncated window, 0: the O(M*N) recursion), group (lanes per child of the windowed kernel;
 * 0 when not used), cut_pairs (pairs inside the windows that NHP_DS_CHILD_CUT holds; 0 before the first)}.  The switch
 * NHP_REC_WINDOW=0 (read on every call) gives used = 0.  A recursion_cost other than 1.0 asks as the gradient and the
 * information do: for a model without any excitation (every W = 0, cut = 1e-300) the empty window is exact for the
 * log-likelihood alone, and they take the recursion.  Synchronous. */
nhp_status nhp_probe_recursive_window(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, double recursion_cost,
                                      double out[4]);

/* ---- discrete data: N x T counts  src/discrete.jl:18,80 -------------------------------- */
/* data [N*T], node fastest.  A negative count anywhere in the matrix is refused with NHP_EDOMAIN ("counts must be
 * non-negative"), found in the host pass over the matrix before any kernel runs; nothing stays allocated. */
nhp_status nhp_disc_dataset_create(nhp_ctx *ctx, const int64_t *data, int32_t n_nodes, int64_t n_bins,
                                   nhp_disc_dataset **out);
void nhp_disc_dataset_destroy(nhp_disc_dataset *ds);
/* Independent trials of one system, stacked along time: trial r holds the bins offsets[r] <= t < offsets[r + 1].  `offsets`
 * has n_trials + 1 entries, starts at 0, is strictly increasing and ends at the dataset's n_bins; anything else is
 * NHP_EINVAL with a message that names the offending entry.  nhp_disc_convolve then stops at the boundaries,
 *     Ŝ[t, n, b] = max(0, Σ_{l = 1 .. min(L, t − offsets[r])} data[n, t − l]·ϕ_b[l]),
 * the lags in increasing order with a separate multiply and add: a trial's rows are bit for bit the rows of that trial
 * convolved alone.  Every other call reads Ŝ row by row and takes the dataset as it is; two convolve across time on their
 * own and answer NHP_ENOTIMPL on a dataset of several trials: nhp_disc_set_lgcp_baseline (the grid is a function of time)
 * and the streamed mode of nhp_disc_svi_run, nhp_disc_netsvi_run and nhp_disc_sbmsvi_run.  The call drops an existing Ŝ
 * and its column sums: nhp_disc_convolve must run again.  n_trials = 1 leaves the dataset as if the call had never been
 * made.  Bin ranges elsewhere (nhp_disc_score_create) stay in stacked bins. */
nhp_status nhp_disc_dataset_set_trials(nhp_ctx *ctx, nhp_disc_dataset *ds, const int64_t *offsets, int32_t n_trials);
/* The trials of a dataset: *n_trials (1 for a dataset that was never cut) and, if non-NULL, offsets [*n_trials + 1]. */
nhp_status nhp_disc_dataset_get_trials(const nhp_disc_dataset *ds, int32_t *n_trials, int64_t *offsets);
/* basis(impulse)  src/impulses.jl:321-335 -> phi [L*B], lag fastest (host) */
nhp_status nhp_disc_basis(int32_t n_lags, int32_t n_basis, double dt, double *phi);
/* convolve(process, data)  src/discrete.jl:146-151; keeps the T x N x B result on the device
 * and copies it to `out` if non-NULL */
nhp_status nhp_disc_convolve(nhp_ctx *ctx, nhp_disc_dataset *ds, const double *phi, int32_t n_lags,
                             int32_t n_basis, double *out);
/* The column sums Σ_t Ŝ[t, n, b] that nhp_disc_convolve leaves beside Ŝ (the gradient and the adjacency sweep read them)
 * -> out [N*B], node fastest.  NHP_EINVAL before the first convolution. */
nhp_status nhp_disc_dataset_get_convsum(nhp_ctx *ctx, const nhp_disc_dataset *ds, double *out);
/* intensity(process, convolved)  src/discrete.jl:115-129 -> T x N; A may be NULL */
nhp_status nhp_disc_intensity(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                              const double *W, const double *theta, const double *A, double dt,
                              double *lam);
/* loglikelihood(process, data, convolved)  src/discrete.jl:91-102 */
nhp_status nhp_disc_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                           const double *W, const double *theta, const double *A, double dt,
                           double *ll);
/* loglikelihood(process, data, convolved) and its gradient in mle!'s parameter vector
 * [λ0 (N); vec(W .* θ) (N*N*B)]  (params / params! src/discrete.jl:174-201): what the 2P finite-difference
 * objective calls per gradient inside mle! (src/discrete.jl:211-296) are replaced by */
nhp_status nhp_disc_loglik_grad(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                const double *W, const double *theta, double dt, double *ll, double *grad,
                                int64_t grad_len);
/* one update!(process, data, convolved) mean-field step  src/discrete.jl:369-375;
 * variational parameters are read and overwritten in place (host arrays) */
nhp_status nhp_disc_vb_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                            double alpha0, double beta0, double kappa, double nu, double gamma,
                            double *alpha_v, double *beta_v, double *kappa_v, double *nu_v,
                            double *gamma_v);
/* Parent counts of one discrete Gibbs sweep: resample_parents(process, data, convolved)
 * src/parents.jl:82-116 summed over time, counts[c + N*k] = Σ_t parents[t, c, k] with k = 0 the
 * baseline and k = 1 + p*B + b (0-based p, b) parent node p through basis b -- the statistic the
 * discrete resample! methods consume (src/baselines.jl:413-419, src/weights.jl:28-35,
 * src/impulses.jl:337-353).  A bin's Multinomial draw is taken as n categorical draws through
 * explicit Philox uniforms keyed (seed, step, bin, event): same distribution as Distributions.jl's
 * sampler, reproducible, and equal to the oracle bit for bit.  counts: [N * (1 + N*B)] int64. */
nhp_status nhp_disc_resample_parents(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                     const double *W, const double *theta, const double *A, double dt,
                                     uint64_t seed, uint64_t step, int64_t *counts);
/* resample!(process::DiscreteStandardHawkesProcess, data, convolved)  src/discrete.jl:362-368 in one call: the
 * parent counts above, then the conjugate draws on the device (Philox-keyed; distributional parity with Julia):
 * λ0 ~ Gamma(α0 + counts[:, 0], 1/(β0 + T dt)) (the intended form of src/baselines.jl:413-419),
 * W ~ Gamma(κ + Σ_b counts, 1/(ν + Σ_t data[p, :]))  src/weights.jl:59-64,
 * θ[p, c, :] ~ Dirichlet(γ + counts)  src/impulses.jl:337-353.  lambda0, W, theta are read and overwritten. */
nhp_status nhp_disc_gibbs_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, double *lambda0, double *W, double *theta,
                               const double *A, double dt, double alpha0, double beta0, double kappa, double nu,
                               double gamma0, uint64_t seed, uint64_t step);
/* resample_adjacency_matrix!(process::DiscreteNetworkHawkesProcess, data, convolved)
 * src/discrete.jl:424-480: one Gibbs sweep over A [N*N] (host, updated in place), columns in parallel,
 * entries of a column in sequence, each conditional on the current column.  Link probabilities
 * (src/networks.jl:65-68): rho_matrix [N*N] if non-NULL, else the scalar rho; Bernoulli draws (u <= q, as
 * Distributions.jl) from u [N*N] if non-NULL, else Philox keyed (seed, step, p + c*N).  n_links
 * (nullable) receives ΣA for BernoulliNetworkModel's resample! (src/networks.jl:70-78). */
nhp_status nhp_disc_resample_adjacency(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0,
                                       const double *W, const double *theta, double *A, double dt,
                                       const double *rho_matrix, double rho, const double *u,
                                       uint64_t seed, uint64_t step, double *n_links);

/* ---- the discrete chain on the device (csrc/disc_chain.hip) ---------------------------------------------------
 * nhp_disc_model: the state of a discrete mcmc! chain as ONE device block, [λ0 (N); vec(W) (N²); vec(θ) (N²B); vec(A) (N², only
 * with has_A)], column-major as every nhp_disc_* entry takes them, and next to it -- with has_A -- the network's scalars
 * {ρ, Σρ, Σρ², ΣA of the latest sweep}, as nhp_cont_model keeps them.  Homogeneous baseline only.  `dt` is the process's bin
 * width (the entries above take it per call; a resident chain has one).  _set / _get copy host arrays in and out, each
 * nullable (A: NHP_EINVAL without has_A); both are synchronous.  _set_rho / _get_rho are nhp_cont_model_set_rho / _get_rho:
 * NHP_EDOMAIN outside [0, 1], _get_rho returns {ρ, Σρ, Σρ²}.  Every entry below that takes a dataset refuses one whose N or B
 * differs from the model's (NHP_EINVAL). */
typedef struct nhp_disc_model nhp_disc_model;
nhp_status nhp_disc_model_create(nhp_ctx *ctx, int32_t n_nodes, int32_t n_basis, int32_t has_A, double dt, nhp_disc_model **out);
void nhp_disc_model_destroy(nhp_disc_model *model);
nhp_status nhp_disc_model_set(nhp_ctx *ctx, nhp_disc_model *model, const double *lambda0, const double *W, const double *theta,
                              const double *A);
nhp_status nhp_disc_model_get(nhp_ctx *ctx, const nhp_disc_model *model, double *lambda0, double *W, double *theta, double *A);
nhp_status nhp_disc_model_set_rho(nhp_ctx *ctx, nhp_disc_model *model, double rho);
nhp_status nhp_disc_model_get_rho(nhp_ctx *ctx, const nhp_disc_model *model, double *rho_sum_sumsq /* [3] */);
/* nhp_disc_gibbs_step on the model, in place: the same launches, Philox keys and arithmetic, so the same bits -- but E and
 * base are staged from the device block, the draws land in it, and the call is asynchronous (no copy to or from the host, no
 * stream synchronise). */
nhp_status nhp_disc_model_gibbs_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *model, double alpha0, double beta0,
                                     double kappa, double nu, double gamma0, uint64_t seed, uint64_t step);
/* The network half of a step: the sweep of nhp_disc_resample_adjacency on the model's A with the model's scalar ρ and Philox
 * uniforms (seed, step), then ΣA on the device (an exact integer sum in one fixed order, no atomics), then
 * ρ ~ Beta(net_alpha + ΣA, net_beta + N² − ΣA) with the kernel and key of nhp_cont_network_rho; net_alpha = net_beta = 0 holds
 * ρ fixed (DenseNetworkModel: set ρ = 1).  nhp_disc_model_set_rho must have run.  The sweep chooses between its two routes
 * to the initial λ from ΣA of the A it starts from, as nhp_disc_resample_adjacency does from its host copy: after _set that
 * count is the upload's, afterwards it is the previous sweep's device count, read back as 8 bytes at the start of this call --
 * the one host read of a step; the route, and so the bits, are those of the host entry.  Otherwise asynchronous. */
nhp_status nhp_disc_model_network_step(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *model, double net_alpha,
                                       double net_beta, uint64_t seed, uint64_t step);
/* Running sums and streaming convergence diagnostics of the model's kept steps.  The contracts are those of
 * nhp_cont_model_moments_reset / _accumulate / _fetch and nhp_cont_model_diagnostics_configure / _fetch above, definition by
 * definition: the same planes, the same expressions operation by operation (Σx² += x·x as one fused multiply-add, with or
 * without diagnostics), the same NaN and "undefined" rules, the same summary fields, the same errors.  What differs is the
 * entries.  Their order is that of params(process) without the network's ρ (the scalar beside them):
 *   has_A:  [λ0; vec(W); vec(θ); vec(A)], len = N + N² + N²B + N²;
 *   else:   [λ0; vec(W .* θ)], len = N + N²B, x = W[p,c]·θ[p,c,b] formed in the pass as ONE rounded product (no contraction).
 * Summary groups: 0 λ0; 1 θ (has_A) or W∘θ; 2 no entries; 3 W (no entries without has_A); 4 vec(A); 5 ρ (one entry once
 * nhp_disc_model_set_rho has run).  The index fields count inside the group: p + N·c (+ N²·b). */
nhp_status nhp_disc_model_moments_reset(nhp_ctx *ctx, nhp_disc_model *model);
nhp_status nhp_disc_model_moments_accumulate(nhp_ctx *ctx, nhp_disc_model *model);
nhp_status nhp_disc_model_moments_fetch(nhp_ctx *ctx, const nhp_disc_model *model, double *sum, double *sumsq, int64_t len,
                                        int64_t *count);
nhp_status nhp_disc_model_diagnostics_configure(nhp_ctx *ctx, nhp_disc_model *model, int64_t batch_len, int64_t n_planned);
nhp_status nhp_disc_model_diagnostics_fetch(nhp_ctx *ctx, const nhp_disc_model *model, double ess_below, double rhat_above,
                                            double *summary, double *ess, double *mcse, double *rhat, int64_t len);
/* Streaming quantiles of the model's kept steps: the contract of nhp_cont_model_quantiles_* above, definition by definition.
 * The entries with a state are the first P of the sums' order:
 *   has_A:  [λ0; vec(W); vec(θ)], P = N + N² + N²B; vec(A)'s slots are NaN; effective_weights feeds A[p,c]·W[p,c];
 *   else:   [λ0; vec(W .* θ)], P = len, x the one rounded product the sums take (effective_weights has nothing to act on).
 * rho: the scalar's state once nhp_disc_model_set_rho has run.  nhp_disc_mcmc_run feeds every `every`-th kept step. */
nhp_status nhp_disc_model_quantiles_configure(nhp_ctx *ctx, nhp_disc_model *model, const double *probs, int32_t m, int32_t every,
                                              int32_t effective_weights);
nhp_status nhp_disc_model_quantiles_accumulate(nhp_ctx *ctx, nhp_disc_model *model);
nhp_status nhp_disc_model_quantiles_fetch(nhp_ctx *ctx, const nhp_disc_model *model, double *values /* [m][len] */,
                                          double *min, double *max /* [len], nullable */, double *rho /* [m+2], nullable */,
                                          int64_t len, int64_t *count);
/* mcmc!(process::DiscreteHawkesProcess, data) inside the library, the loop of nhp_cont_mcmc_run: n_steps times
 * nhp_disc_model_gibbs_step with the priors (alpha0 … gamma0), nhp_disc_model_network_step when the model has A, and one
 * nhp_disc_model_moments_accumulate from chain step `burn` on (burn < 0: never); ONE host synchronise, at the end; between the
 * steps nothing crosses PCIe but the 8-byte link count.  Steps are step0 … step0 + n_steps − 1 and the kept count lives in
 * the model: a chain cut into calls gives the planes of the chain in one call. */
nhp_status nhp_disc_mcmc_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, nhp_disc_model *model, double alpha0, double beta0,
                             double kappa, double nu, double gamma0, double net_alpha, double net_beta, uint64_t seed,
                             uint64_t step0, int64_t n_steps, int64_t burn);

/* ---- scoring a discrete chain: held-out predictive log-likelihood and WAIC (csrc/disc_score.hip) -------------
 * Cell (t, c) of the count matrix is Poisson(λ[t,c]) given the past (nhp_disc_loglik), so with ℓ_i(θ) = log p(s_i | θ) over the
 * cells i of bins [t0, t1), all nodes, and S kept draws θ_1 … θ_S:
 *   lppd_i = log mean_s exp ℓ_i(θ_s),  p_i = the sample variance of ℓ_i(θ_s) (denominator S − 1),  elpd_i = lppd_i − p_i,
 *   joint  = log mean_s exp Σ_i ℓ_i(θ_s): the predictive log-likelihood of the bins as a whole (held-out bins: the metric).
 * A scorer keeps, per cell, a running log-sum-exp and Welford's mean and M2 of ℓ_i, and the same three scalars for Σ_i ℓ_i:
 * 24·R·N bytes for R = t1 − t0 (t fastest), plus 8·R·N of context scratch for λ while a draw is scored.
 * _create: `ds` must be convolved (NHP_EINVAL) and outlive the scorer; 0 <= t0 < t1 <= T (NHP_EINVAL); a dataset with an LGCP
 *   baseline is NHP_ENOTIMPL, and so is N > 65535 (the pass takes one grid row per node column); NHP_ENOMEM leaves nothing
 *   allocated.
 * _accumulate: the model's current state as one draw -- the bump table from its block, λ for rows [t0, t1) alone with the
 *   fp64 GEMM of nhp_disc_intensity, one pass over the cells (ℓ in the arithmetic of nhp_disc_loglik), one fold of the
 *   workgroup partials.  Asynchronous on the main stream, no host read; no atomics and every sum in one fixed order, so two
 *   runs give the same bits.  A model whose N or B differs from the dataset's is NHP_EINVAL.
 * _reset: forget the draws.  _fetch (synchronous): NHP_EINVAL ("nothing accumulated") with S = 0;
 *   summary[10] = {S, cells = R·N, lppd = Σ lppd_i, p_waic = Σ p_i, elpd_waic = Σ elpd_i, waic = −2·elpd_waic,
 *                  se_elpd = sqrt(cells · var_i elpd_i) (sample variance over the cells, two passes),
 *                  joint_lpd, joint_mean = mean_s Σ_i ℓ_i(θ_s), joint_sd = its sample standard deviation};
 *   per_node[3N] = lppd, p_waic, elpd_waic per node column; pointwise[R·N] (nullable, index r + R·c) = elpd_i.
 *   With S = 1, p_i and everything built on it (and joint_sd) are NaN: undefined, as in the diagnostics.
 * _fetch_planes (synchronous): the running planes themselves, each nullable, [R·N] at index r + R·c -- lse_i, mean_i and M2_i
 *   of ℓ_i WITHOUT its loggamma(s_i + 1) (the same constant in lse_i and mean_i, absent from M2_i), so that lse_i − log S >=
 *   mean_i and M2_i >= 0 can be checked on what the device holds; NHP_EINVAL with S = 0.
 * nhp_disc_model_attach_score: at most two scorers per model (a third is NHP_EINVAL; not owned: detach or destroy the model
 *   first).  nhp_disc_mcmc_run then calls _accumulate for each on every kept step whose kept index -- counted per scorer
 *   from the attach on, across calls -- is a multiple of `every` (>= 1, else NHP_EINVAL).  Kept steps are those from `burn`
 *   on; with the moments off (burn < 0) those from −(burn + 1) on, so −1 keeps every step.  score = NULL detaches all.
 *   With nothing attached nhp_disc_mcmc_run launches exactly what it launched before. */
typedef struct nhp_disc_score nhp_disc_score;
nhp_status nhp_disc_score_create(nhp_ctx *ctx, const nhp_disc_dataset *ds, int64_t t0, int64_t t1, nhp_disc_score **out);
void nhp_disc_score_destroy(nhp_disc_score *score);
nhp_status nhp_disc_score_reset(nhp_ctx *ctx, nhp_disc_score *score);
nhp_status nhp_disc_score_accumulate(nhp_ctx *ctx, nhp_disc_score *score, const nhp_disc_model *model);
nhp_status nhp_disc_score_fetch(nhp_ctx *ctx, const nhp_disc_score *score, double *summary /* [10] */, double *per_node /* [3N] */,
                                double *pointwise /* [R*N] or NULL */);
nhp_status nhp_disc_score_fetch_planes(nhp_ctx *ctx, const nhp_disc_score *score, double *lse, double *mean, double *m2);
nhp_status nhp_disc_model_attach_score(nhp_ctx *ctx, nhp_disc_model *model, nhp_disc_score *score, int64_t every);

/* DiscreteLogGaussianCoxProcess(x, λ, Σ, m, dt) as this dataset's baseline (src/baselines.jl:461-509): lam
 * [grid_n * N] (λ[:, n] at n*grid_n) on grid_x [grid_n].  The per-bin baseline intensity(p, 1:T)
 * (src/discrete.jl:117, src/baselines.jl:531-537) is built on the device and kept with the dataset; the other
 * nhp_disc_* calls use it when their lambda0 argument is NULL (nhp_disc_loglik_grad then returns the gradient
 * in [vec(λ) (grid_n*N); vec(W .* θ)] order).  NHP_EDOMAIN if a bin time 1..T lies outside the grid. */
nhp_status nhp_disc_set_lgcp_baseline(nhp_ctx *ctx, nhp_disc_dataset *ds, const double *grid_x, int32_t grid_n,
                                      const double *lam, double dt);
/* loglikelihood(p::DiscreteLogGaussianCoxProcess, data, node, y)  src/baselines.jl:571-584 for all nodes:
 * data = parents[:, :, 1] of the latest nhp_disc_resample_parents on this dataset (kept on the device),
 * cand [grid_n * N] = exp.(m .+ y) per node -- the body of every elliptical_slice round (:640-679). */
nhp_status nhp_disc_lgcp_loglik(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *cand, double dt, double *ll);
/* n_steps consecutive update! steps of vb! (src/inference.jl:153-181) with the variational parameters
 * resident on the device in between (one upload, one download) */
nhp_status nhp_disc_vb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                           double alpha0, double beta0, double kappa, double nu, double gamma, int32_t n_steps,
                           double *alpha_v, double *beta_v, double *kappa_v, double *nu_v, double *gamma_v);
/* svi!(process, data) -- a stub in the reference (src/inference.jl:190): n_steps steps of stochastic variational inference
 * for DiscreteStandardHawkesProcess + DenseWeightModel + DiscreteHomogeneousProcess, the variational parameters resident on
 * the device in between (one upload, one download, no synchronisation inside the loop).
 * Blocks: Tb = min(batch_bins, T); the bins are cut into nb = ceil(T / Tb) consecutive blocks, block j = [j·Tb, min(T, (j+1)·Tb)).
 * batch_bins >= T gives one block; otherwise it must be a multiple of 16 and >= 16 (NHP_EINVAL; nothing is rounded).
 * Step k of the call is global step i = step0 + k + 1 on block j_i = blocks[k] (each in [0, nb)) or, with blocks = NULL, the
 * draw nhp_disc_svi_blocks documents.  With (α', κ', γ') the update! of nhp_disc_vb_step with every sum over t restricted to
 * the block (the factors from the current parameters; Ŝ is the convolution of the whole data):
 *   α̂ = α0 + nb (α' - α0),  γ̂ = γ + nb (γ' - γ),  κ̂ = κ + Σ_b (γ̂ - γ),  β̂ = 1/β0 + T·dt,  ν̂[p,c] = ν + Σ_{t<T} data[p,t],
 * and every parameter x <- (1 - ρ_i) x + ρ_i x̂ with ρ_i = (i + delay)^(-forgetting), delay >= 0, forgetting in (0.5, 1].
 * Resident mode (phi = NULL): the dataset holds Ŝ (nhp_disc_convolve).  Streamed mode (phi [n_lags*n_basis], lag fastest,
 * as nhp_disc_basis makes it): every step convolves its block into a Tb x N x B image, bit for bit the resident rows; the
 * dataset needs no Ŝ and keeps none, and scratch is O(Tb·N·B).  Argument errors are NHP_EINVAL / NHP_ENOTIMPL with a message,
 * before any launch. */
nhp_status nhp_disc_svi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                            double alpha0, double beta0, double kappa, double nu, double gamma,
                            int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0, int32_t n_steps,
                            const int32_t *blocks /* nullable [n_steps] */, const double *phi /* nullable */, int32_t n_lags,
                            int32_t n_basis, double *alpha_v, double *beta_v, double *kappa_v, double *nu_v, double *gamma_v);
/* update! / vb! for DiscreteNetworkHawkesProcess + SparseWeightModel + DiscreteHomogeneousProcess (broken wiring in the
 * reference; every formula is in src/weights.jl:141-173, src/discrete.jl:482-492, src/networks.jl:80-93).
 * Mean-field family q(A[p,c] = 1) = rho_v[p,c], q(W | A = a) = Gamma(kappa_v<a>, nu_v<a>); arrays column-major [p, c(, b)].
 * One step, factors from the OLD parameters:  ElogW = (1 - ρv)(ψ(κv0) - log νv0) + ρv (ψ(κv1) - log νv1) in the factor
 * E of nhp_disc_vb_run; its two GEMMs and its baseline update unchanged; with Γ = E ⊙ (Gᵀ·R):
 *   γv = γ + Γ,  κv_a = κ_a + Σ_b Γ,  νv_a[p,c] = ν_a + Σ_t data[p,t]                     (a = 0 spike, a = 1 slab)
 *   logit ρv = ψ(αv_net) - ψ(βv_net) + [κ1 log ν1 - lgamma κ1 + lgamma κv1 - κv1 log νv1]
 *                                    - [κ0 log ν0 - lgamma κ0 + lgamma κv0 - κv0 log νv0]   (new κv/νv, old network)
 *   ρv = 1/(1 + exp(-logit)), exactly 0 or 1 when saturated;  αv_net = α + Σρv,  βv_net = β + Σ(1 - ρv)   (all N² links)
 * net_kind 0 = DenseNetworkModel: rho_v is set to 1 on entry and stays 1, net_alpha_v / net_beta_v may be NULL and are not
 * touched; 1 = BernoulliNetworkModel with prior Beta(net_alpha, net_beta).  Any other kind is NHP_ENOTIMPL.  Every rho_v
 * must lie in [0, 1], every κ, ν, γ, α, β (priors and variational) must be > 0: NHP_EINVAL with a message, before any launch.
 * One upload, one download, no synchronisation inside the n_steps; the sums over links have one fixed order, so a run is
 * reproducible bit for bit. */
nhp_status nhp_disc_netvb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                              double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                              int32_t net_kind, double net_alpha, double net_beta, int32_t n_steps,
                              double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1, double *nu_v1,
                              double *gamma_v, double *rho_v, double *net_alpha_v /* nullable if dense */,
                              double *net_beta_v /* nullable if dense */);
/* svi! for the same model: the block step of nhp_disc_svi_run (its blocks, seeds, modes and argument rules) gives α̂, γ̂ and
 * Σ_b (γ̂ - γ);  κ̂v_a = κ_a + Σ_b (γ̂ - γ),  ν̂v_a = ν_a + Σ_{t<T} data[p,t],  ρ̂v from the logit above at (κ̂v, ν̂v) and the
 * current network parameters,  α̂v_net = α + Σρ̂v,  β̂v_net = β + Σ(1 - ρ̂v);  then every parameter, ρv included,
 * x <- (1 - ρ_i) x + ρ_i x̂.  One block, delay 0, forgetting 1, one step is one step of nhp_disc_netvb_run. */
nhp_status nhp_disc_netsvi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                               double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                               int32_t net_kind, double net_alpha, double net_beta,
                               int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0, int32_t n_steps,
                               const int32_t *blocks /* nullable [n_steps] */, const double *phi /* nullable */, int32_t n_lags,
                               int32_t n_basis, double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                               double *nu_v1, double *gamma_v, double *rho_v, double *net_alpha_v, double *net_beta_v);
/* update! / vb! for the same process with a StochasticBlockNetworkModel of n_blocks = K <= 64 blocks:
 *   z_n ~ Categorical(π),  π ~ Dirichlet(net_gamma·1_K),  ρ[k,l] ~ Beta(net_alpha, net_beta),  A[p,c] ~ Bernoulli(ρ[z_p, z_c]).
 * The family of nhp_disc_netvb_run plus q(z_n) = Categorical(m[n,:]), q(π) = Dirichlet(gamma_v_net), q(ρ[k,l]) =
 * Beta(net_alpha_v[k,l], net_beta_v[k,l]);  m [N*K] is column-major [n, k], the tables [K*K] column-major [k, l].
 * With E1 = ψ(αv) - ψ(αv + βv), E0 = ψ(βv) - ψ(αv + βv), D = E1 - E0, Eπ = ψ(γv) - ψ(Σγv) and the pair weight
 * ω[p,c,k,l] = m[p,k] m[c,l] for p != c, ω[p,p,k,l] = m[p,k] δ_kl (a node has one label), one step is the step of
 * nhp_disc_netvb_run with
 *   1. the network term of the logit per link, net[p,c] = Σ_kl ω D, from the OLD m and tables;
 *   2. αv[k,l] = α + Σ_pc ω ρv,  βv[k,l] = β + Σ_pc ω (1 - ρv),  γv[k] = γ + Σ_n m[n,k]  from the NEW ρv and the current m;
 *   3. when the step's global number step0 + 1, step0 + 2, ... (step0 = the steps earlier calls took: the caller counts
 *      them, as for nhp_disc_svi_run) is a multiple of labels_every, one sweep of coordinate ascent over
 *      the nodes 0 .. N-1, each reading the current m of all others and the tables of 2:  m[n,:] = softmax(s),
 *      s_k = Eπ[k] + ρv[n,n] E1[k,k] + (1 - ρv[n,n]) E0[k,k] + Σ_{c≠n} Σ_l m[c,l] (ρv[n,c] E1[k,l] + (1 - ρv[n,c]) E0[k,l])
 *                                                            + Σ_{p≠n} Σ_l m[p,l] (ρv[p,n] E1[l,k] + (1 - ρv[p,n]) E0[l,k]).
 * Every row of m must be non-negative and sum to 1 within 1e-12, every table and prior must be > 0: NHP_EINVAL before any
 * launch.  The sweep keeps m in LDS: 8 (N K + 2 N + 20 Kp) bytes, Kp the next power of two of K, must fit 160 KiB, else
 * NHP_ENOTIMPL with the byte count, before any launch.  One upload, one download, no synchronisation inside the n_steps,
 * every sum in one fixed order: n calls of one step, each with the step0 the calls before it reached, are one call of
 * n steps, bit for bit, for every labels_every. */
nhp_status nhp_disc_sbmvb_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                              double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                              int32_t n_blocks, double net_alpha, double net_beta, double net_gamma, int32_t labels_every,
                              int64_t step0, int32_t n_steps, double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                              double *nu_v1, double *gamma_v, double *rho_v, double *m, double *net_alpha_v, double *net_beta_v,
                              double *gamma_v_net);
/* svi! for the block network: the block step of nhp_disc_netsvi_run gives ρ̂v; the hats of the tables are 2. above at ρ̂v and
 * the current m, the hat of m is one sweep (at global steps i that are multiples of labels_every) over a copy of m with ρ̂v
 * and those hats; then every parameter, m included, x <- (1 - ρ_i) x + ρ_i x̂ (a convex combination keeps m on the
 * simplex); at a step without a sweep m has no hat and stays bit for bit.  Blocks, seeds, step0 and the two modes as nhp_disc_svi_run.  One block, delay 0, forgetting 1, one step is
 * one step of nhp_disc_sbmvb_run. */
nhp_status nhp_disc_sbmsvi_run(nhp_ctx *ctx, const nhp_disc_dataset *ds, double dt,
                               double alpha0, double beta0, double kappa0, double nu0, double kappa1, double nu1, double gamma,
                               int32_t n_blocks, double net_alpha, double net_beta, double net_gamma, int32_t labels_every,
                               int64_t batch_bins, double delay, double forgetting, uint64_t seed, int64_t step0, int32_t n_steps,
                               const int32_t *blocks /* nullable [n_steps] */, const double *phi /* nullable */, int32_t n_lags,
                               int32_t n_basis, double *alpha_v, double *beta_v, double *kappa_v0, double *nu_v0, double *kappa_v1,
                               double *nu_v1, double *gamma_v, double *rho_v, double *m, double *net_alpha_v, double *net_beta_v,
                               double *gamma_v_net);
/* The blocks nhp_disc_svi_run draws for global steps step0 + 1 .. step0 + n (host side, no device): out[k] =
 * min(nb - 1, floor(nb · u_i)), u_i the Philox4x32-10 uniform in [0, 1) with key seed ^ 0x5C1B10C5D2A7E391, counter words
 * (event = 0, step = i), i = step0 + k + 1 -- a function of (seed, i) alone. */
nhp_status nhp_disc_svi_blocks(uint64_t seed, int64_t step0, int64_t n, int32_t nb, int32_t *out);
/* rand(process::DiscreteHawkesProcess, steps)  src/discrete.jl:20-38 on the device: the N x T count matrix of a discrete
 * Hawkes process over bins t = 1..T.  The law: cell (c, t) receives Poisson(base[t,c]) immigrants, base[t,c] = lambda0[c]·dt
 * (homogeneous baseline) or the caller's per-bin means base [T*N], t fastest, already times dt (intensity(baseline, 1:T) of a
 * DiscreteLogGaussianCoxProcess) -- exactly one of lambda0 and base is given; every event at (p, t) has Poisson(h[p,c,l])
 * children in cell (c, t+l), independently for every c and every lag l = 1..L, h[p,c,l] = W[p,c]·A[p,c]·dt·Σ_b θ[p,c,b]·φ[l,b];
 * children past bin T are dropped with their descendants.  W, theta, A (nullable) are host arrays laid out as
 * nhp_disc_intensity takes them (column-major [p, c(, b)]), phi [L*B] lag fastest as nhp_disc_basis makes it (lags 1..L).
 * It is drawn in stages (Poisson superposition), with the tables
 *   cdf[l,b] = φ[1,b] + ... + φ[l,b] (sequential), m_b = cdf[L,b]·dt,
 *   S[p,c] = Σ_b θ[p,c,b]·m_b (sequential from 0, b ascending), G[p,c] = (W[p,c]·A[p,c])·S[p,c],
 *   prefix_p[c] = G[p,1] + ... + G[p,c] (sequential), R_p = prefix_p[N],
 * all in fp64 without contraction: an event has Poisson(R_p) children (an immigrant cell of multiplicity k draws
 * Poisson(k·R_p) once), a child takes its node from prefix_p, its basis from the running sums of θ[p,c,b]·m_b, its lag from
 * cdf[·,b].
 * Outputs, host or device pointers by output_on_device (as in nhp_cont_simulate): counts [N*T], node fastest (the layout
 * nhp_disc_dataset_create reads); background [N*T] (nullable), the immigrants alone -- parents[:, :, 1] of the reference's
 * augmented model, transposed; n_events (host) = Σ counts; n_generations (host, nullable) = the generations that hold an
 * event, the immigrants' included.  Synchronous.  The result depends on (parameters, T, seed) only
 * -- not on max_events, the chunk size or launch geometry (integer atomic sums).
 * Errors: NHP_EINVAL for null pointers, both or neither of lambda0 / base, non-positive n_nodes, n_bins, n_lags or n_basis,
 * max_events outside [0, 2^31); NHP_ENOTIMPL for n_bins >= 2^31 (32-bit bins in the arena) or n_nodes·n_bins >= 2^56 (int64
 * byte offsets into the matrix); NHP_EDOMAIN for a negative or non-finite dt, W, W·A, θ, φ or baseline mean, a cell mean above
 * 2^20 or a row total R_p above 2^32; NHP_ENOMEM "branching process exploded (unstable weights?)" when the events pass
 * max_events (nothing is written past the arena; the ctx stays usable), or when the device cannot hold the scratch (28 bytes per
 * event of max_events, 16 per slot of a chunk, the parameters, and the two matrices when the outputs are host pointers).
 * Random numbers: the Philox block, the uniforms ua, ub in (0, 1], u = ua - 2^-53, v = ub - 2^-53 in [0, 1) and the Poisson
 * sampler of nhp_cont_simulate above, with these families (key = seed ^ F), in draw order; nodes, bins and basis 0-based:
 *   0xA3B195354A39B70D  immigrants of cell (c, t): Poisson(base[t,c]), step 0, element e = c + N·t
 *   0x1B03738712FAD5C9  child count of arena entry i: Poisson(k_i·R_node), step = generation of i (immigrants 0), element i
 *   0xC2B2AE3D27D4EB4F  child slot s of generation g (slots numbered by parent arena index, then child): step g, element s;
 *                       attempt 0: node = first c with prefix_p[c] > u·R_p (if none, the first prefix_p[c] >= u·R_p); basis =
 *                       first b with S_b > v·S[p,c], S_b the running sum θ[p,c,0]·m_0 + ... + θ[p,c,b]·m_b (if none, the first
 *                       S_b >= v·S[p,c]); attempt 1: lag l = first l with cdf[l,b] > u·cdf[L,b] (if none, the first >=);
 *                       the child's bin is t_parent + l and it is kept when that is at most T
 * The arena holds the occupied cells in the order of e (entry = node, bin, multiplicity k), then each generation's surviving
 * children in slot order (k = 1). */
nhp_status nhp_disc_simulate(nhp_ctx *ctx, const double *lambda0 /* [N] or NULL */, const double *base /* [T*N] or NULL */,
                             const double *W, const double *theta, const double *A /* nullable */, const double *phi,
                             int32_t n_lags, int32_t n_basis, double dt, int32_t n_nodes, int64_t n_bins, uint64_t seed,
                             int64_t max_events, int32_t output_on_device, int64_t *counts /* [N*T] */,
                             int64_t *background /* [N*T] nullable */, int64_t *n_events, int32_t *n_generations /* nullable */);
/* disc_forecast(process, data, horizon): `nsamples` = S independent continuations of an observed count matrix s[p, 1..T0] over
 * the H = horizon_bins bins T0+1 .. T0+H, conditional on the counts -- the reference has no such function.  The law is the one
 * nhp_disc_simulate draws; with h[p,c,l] as there, one continuation is the union of three independent parts, exactly:
 *   carry-over: the children the observed events still have beyond T0; cell (c, T0+k) receives Poisson(carry[k,c]) of them,
 *     carry[k,c] = Σ_p Σ_{l=k..L, T0+k-l >= 1} s[p, T0+k-l]·h[p,c,l] (0 for k > L);
 *   new immigrants: Poisson(base[k,c]) per cell, base[k,c] = lambda0[c]·dt or the caller's per-bin means base [H*N], k fastest,
 *     already times dt (intensity(baseline, T0+1 .. T0+H) of a DiscreteLogGaussianCoxProcess) -- exactly one of the two is given;
 *   descendants of both, by the generation loop of nhp_disc_simulate; a child of an entry in forecast bin k at lag l lands in
 *     bin k+l of the same replica and is kept when k+l <= H.
 * `history` [n_history_bins*N] int64, node fastest (the layout nhp_disc_dataset_create reads), is the last n_history_bins bins
 * of the data, a host pointer or with history_on_device a device pointer; n_history_bins is at least min(L, T0), more is allowed
 * and changes nothing: only the last Tu = min(L, n_history_bins) bins are copied or read.  W, theta, A (nullable), phi are host
 * arrays as nhp_disc_simulate takes them.
 * Boundary state, all in fp64 without contraction, every sum sequential from 0.0 in the stated order (K = min(L, H); k, b, p, c
 * 0-based from here on, forecast bin k is T0+1+k; lags l = 1..L):
 *   cdf, m_b, S, G, prefix_p, R_p: the tables of nhp_disc_simulate;
 *   x[k,p,b] = Σ_l (double)s[p, T0+1+k-l]·φ[l,b] over l = k+1 .. min(L, Tu+k), l ascending, for k < K;
 *   carry[k,c] = dt·Σ_p Σ_b ((W[p,c]·A[p,c])·θ[p,c,b])·x[k,p,b], p ascending, b ascending inside (W[p,c] alone without A), for
 *     k < K; exactly 0.0 for k >= K;
 *   cm[k,c] = base[k,c] + carry[k,c]: the mean of the one Poisson draw that stands for carry-over and immigrants of a cell;
 *   expected[k,c] = μ_k[c], the exact predictive mean: μ_k = cm_k + Σ_{l=1..min(L,k)} H_lᵀ μ_{k-l}, H_l[p,c] = h[p,c,l], bin after
 *     bin as z[p,b] = Σ_l φ[l,b]·μ[k-l,p] (l ascending) and μ[k,c] = cm[k,c] + dt·Σ_p Σ_b ((W·A)·θ)[p,c,b]·z[p,b] in a fixed order
 *     (64 interleaved partial sums over p, joined by a butterfly): the same bits on every call, not a sequential sum.
 * Outputs, host or device pointers by output_on_device: totals [S*N], replica-major: the events of node c in replica r over the
 * horizon; cell_sum [H*N], node fastest: Σ_r of the counts of cell (k, c); paths [S*H*N] (nullable), node fastest, then bin, then
 * replica: the count matrix of every replica (one replica's slice has the layout nhp_disc_dataset_create reads; without it no
 * S·H·N buffer exists); carry [H*N] and expected [H*N] (both nullable), node fastest; n_events (host) = the events of all
 * replicas; n_generations (host, nullable) = the generations that hold an entry, the cells' included.  Synchronous.  The result
 * depends on (parameters, the last min(L, T0) bins of the data, H, S, seed) only -- not on max_events, the chunk size or launch
 * geometry (integer atomic sums); replica r's draws are NOT promised to be the same for different nsamples.
 * Errors: NHP_EINVAL for null pointers, both or neither of lambda0 / base, non-positive n_nodes, n_lags, n_basis,
 * n_history_bins, horizon_bins or nsamples, max_events outside [0, 2^31); NHP_ENOTIMPL for nsamples·horizon_bins >= 2^31 (32-bit
 * bins in the arena) or nsamples·horizon_bins·n_nodes >= 2^56; NHP_EDOMAIN for a negative history count, a negative or
 * non-finite dt, W, W·A, θ, φ or baseline mean, a cell mean cm above 2^20 or a row total R_p above 2^32 (checked flags: no draw
 * is made); NHP_ENOMEM "branching process exploded (unstable weights?)" when the events of all replicas together pass max_events
 * (nothing is written past the arena; the ctx stays usable), or when the device cannot hold the scratch.
 * Random numbers: the Philox block, the uniforms and the Poisson sampler of nhp_disc_simulate, with three families of its own
 * (key = seed ^ F), in draw order:
 *   0xDA942042E4DD58B5  carry-over + immigrants of cell (c, k) of replica r: Poisson(cm[k,c]), step 0, element e = c + N·(k + H·r)
 *   0xD1B54A32D192ED03  child count of arena entry i: Poisson(k_i·R_node), step = generation of i (cells 0), element i
 *   0x8CB92BA72F3D8DD7  child slot s of generation g (slots numbered by parent arena index, then child): step g, element s;
 *                       node, basis and lag from attempts 0 and 1 as family 0xC2B2... of nhp_disc_simulate; the child's bin is
 *                       k_parent + l in its parent's replica and it is kept when k_parent + l <= H - 1 (0-based)
 * The arena holds the occupied cells in the order of e (entry = node, bin k + H·r, multiplicity), then each generation's
 * surviving children in slot order (multiplicity 1); all replicas share it. */
nhp_status nhp_disc_forecast(nhp_ctx *ctx, const double *lambda0 /* [N] or NULL */, const double *base /* [H*N] or NULL */,
                             const double *W, const double *theta, const double *A /* nullable */, const double *phi,
                             int32_t n_lags, int32_t n_basis, double dt, int32_t n_nodes, const int64_t *history,
                             int64_t n_history_bins, int32_t history_on_device, int64_t horizon_bins, int64_t nsamples,
                             uint64_t seed, int64_t max_events, int32_t output_on_device, int64_t *totals /* [S*N] */,
                             int64_t *cell_sum /* [H*N] */, int64_t *paths /* [S*H*N] nullable */, double *carry /* [H*N] nullable */,
                             double *expected /* [H*N] nullable */, int64_t *n_events, int32_t *n_generations /* nullable */);
/* disc_residuals(process, data): goodness of fit of a discrete process on its count matrix -- the reference has no such
 * function.  The law is the one of nhp_disc_loglik (src/discrete.jl:91-102): cell (t, c) is Poisson(μ[t,c]), μ = the matrix
 * nhp_disc_intensity returns for the same arguments (dt is inside it; lambda0 = NULL: the dataset's LGCP baseline, as there).
 * nhp_disc_convolve must have run on `ds`.  With s the observed count, p(k) the Poisson(μ) pmf and F(k) = p(0) + ... + p(k),
 * F(-1) = 0, every cell gives
 *   pit     = F(s-1) + v·p(s), v in [0, 1) uniform: the randomized probability integral transform, uniform under the model;
 *   pearson = (s - μ)/√μ;
 *   D       = s·log(s/μ) + μ - s (μ at s = 0): half its deviance term,
 * and every node c the sums over its T cells
 *   expected[c] = Σμ, observed[c] = Σs (int64), chi2[c] = Σ (s-μ)²/μ, deviance[c] = 2·ΣD,
 *   histogram[c, j] = the cells with min(floor(pit·nbins), nbins - 1) = j (int64).
 * A cell with μ = 0 exactly: s = 0 gives pit = v, pearson = 0 and adds nothing to chi2 and deviance; s > 0 has probability 0
 * under the model: pit = 1, pearson = +inf, chi2[c] becomes +inf, the deviance leaves the cell out, and `impossible` (host)
 * counts it.  cumulative[t, c] = μ[1,c] + ... + μ[t,c], the compensator of node c at the end of bin t.
 * Arithmetic of a cell with μ > 0, in fp64 without contraction, exactly as written (√ and / correctly rounded; exp and log
 * are the device's, good to a few ulp, so a restatement agrees to rounding, not bit for bit):
 *   d = s - μ; pearson = d/√μ; the chi2 term is (d·d)/μ;
 *   s = 0: D = μ, p(s) = exp(-μ); otherwise
 *     D: if |d| < 0.1·(s+μ): x = d/(s+μ), w = x·x, q = (((((((((w/21 + 1/19)·w + 1/17)·w + 1/15)·w + 1/13)·w + 1/11)·w + 1/9)·w
 *          + 1/7)·w + 1/5)·w + 1/3)·w, D = d·x + ((2·s)·x)·q (the series of s·log(s/μ) + μ - s in x); else D = s·log(s/μ) + μ - s;
 *     δ(s), the Stirling error lgamma(s+1) - (s+½)·log s + s - ½·log 2π: for s < 16 its correctly rounded value (a table); from
 *          16 on, with z = s·s, (1/12 - (1/360 - (1/1260 - (1/1680 - (1/1188)/z)/z)/z)/z)/s;
 *     p(s) = exp(-δ(s) - D)/√(6.283185307179586·s) (the saddle-point form: no s·log μ - μ - lgamma(s+1), which loses 7 digits
 *          at μ = 2^20);
 *   s <= μ, the lower tail downward: t = p(s), a = 0, k = s; while k > 0: t = (t·k)/μ, a = a + t, k = k - 1, stop unless
 *          t > 2^-60·a; pit = a + v·p(s);
 *   s > μ, the upper tail upward: t = p(s), a = 0, k = s; repeat: k = k + 1, t = (t·μ)/k, a = a + t, until not
 *          t > (2^-60·a)·(1 - μ/(k+1)) (what is left is below t·r/(1-r), r = μ/(k+1)); pit = (1 - a) - (1 - v)·p(s);
 *   pit is then clamped to [0, 1].  A tail takes 77 steps at most for μ <= 64 and 8 487 at μ = 2^20 eight sigma out.
 * The node sums are formed in one fixed order (a workgroup's partial per 1024 bins, the partials joined in bin order by a second
 * kernel), the scan likewise, the integer sums by integer atomics: the same call gives the same bits, whatever the launch.
 * Random numbers: the Philox block and the uniform ua of nhp_disc_simulate with a family of its own (key = seed ^ F):
 *   0x2545F4914F6CDD1D  v of cell (c, t), c and t 0-based: step 0, element e = c + N·t, attempt 0, v = ua - 2^-53
 * The seed changes pit and the histogram, nothing else.
 * Outputs, host or device pointers by output_on_device (as in nhp_disc_forecast): the planes pit, pearson, cumulative [T*N], t
 * fastest (index t + T·c: the layout of nhp_disc_intensity; row-major it is the N x T matrix), each nullable, and an absent
 * plane is neither computed as a plane nor written; expected, chi2, deviance [N]; observed [N] int64; histogram [N*nbins] int64, bin
 * fastest; impossible: a host int64 whatever output_on_device says; pass_ms (host, nullable): the milliseconds k_disc_residuals
 * took on the device, between the two events of the ctx timer (a running nhp_ctx_timer_start is overwritten).  Synchronous.
 * Errors: NHP_EINVAL for null pointers (the planes excepted), nbins outside [1, 4096], no convolution on `ds`, lambda0 = NULL
 * without an LGCP baseline; NHP_EDOMAIN for a cell mean that is negative or not finite; NHP_ENOTIMPL for a cell mean or a count
 * above 2^20 (the cap nhp_disc_simulate puts on a cell mean; it bounds the tail loops) and for N·ceil(T/1024) >= 2^31;
 * NHP_ENOMEM when the device cannot hold the scratch (μ, and the requested planes when the outputs are host pointers).  The
 * domain and size checks run in a kernel of their own before the pass, so after them nothing has been written to the outputs
 * except *impossible = 0; after any error the ctx stays usable. */
nhp_status nhp_disc_residuals(nhp_ctx *ctx, const nhp_disc_dataset *ds, const double *lambda0 /* [N] or NULL */, const double *W,
                              const double *theta, const double *A /* nullable */, double dt, uint64_t seed, int32_t nbins,
                              int32_t output_on_device, double *pit /* [T*N] nullable */, double *pearson /* [T*N] nullable */,
                              double *cumulative /* [T*N] nullable */, double *expected /* [N] */, int64_t *observed /* [N] */,
                              double *chi2 /* [N] */, double *deviance /* [N] */, int64_t *histogram /* [N*nbins] */,
                              int64_t *impossible /* host */, double *pass_ms /* host, nullable */);

/* ---- several GPUs: RCCL over xGMI   ------------------------------------------------------------
 * One process (or host thread) per GPU, one nhp_ctx each.  The reference has no distributed code (README.md:42 lists
 * "multiple-trial inference" as future work; mcmc! has no cross-chain term, src/inference.jl:49-70), so these entry
 * points replace nothing: they are the exchange steps of the two ways the path shards --
 *   independent units (chains, restarts): no data-path collective, one gather of per-chain summaries at the end;
 *   one evaluation / one chain over all ranks by child-node column: one all-reduce per evaluation / per step --
 * and they hand RCCL DEVICE pointers: results are reduced where the kernels left them, on the ctx stream, and cross
 * PCIe once, reduced.  librccl.so.1 is opened on first use (dlopen): a single-GPU host needs no RCCL installed.
 * Rendezvous: rank 0 calls nhp_comm_unique_id and gives the 128 bytes to the other ranks through whatever channel
 * the host has (Julia: Distributed / a file / MPI.bcast; Python: torch.distributed or a TCP store); every rank then
 * calls nhp_comm_create -- collectively, it blocks until all `world` ranks have joined. */
#define NHP_COMM_ID_BYTES 128
nhp_status nhp_comm_unique_id(uint8_t *id /* [NHP_COMM_ID_BYTES] */);
nhp_status nhp_comm_create(nhp_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world, nhp_comm **out);
void nhp_comm_destroy(nhp_comm *comm);
int32_t nhp_comm_rank(const nhp_comm *comm);
int32_t nhp_comm_world(const nhp_comm *comm);
/* host vectors through a device staging buffer (small control data: link counts, log-likelihood traces, flags) */
nhp_status nhp_allreduce_sum(nhp_ctx *ctx, nhp_comm *comm, double *x, int64_t n);                 /* in place */
nhp_status nhp_allgather(nhp_ctx *ctx, nhp_comm *comm, const double *mine, int64_t n, double *all /* [world*n] */);
/* loglikelihood(process, data; recursive) by all ranks together: `ds` is this rank's column shard
 * (nhp_cont_dataset_create_columns); the partial result is all-reduced in place on the device and fetched once.
 * Every rank returns the same value. */
nhp_status nhp_cont_loglik_allreduce(nhp_ctx *ctx, nhp_comm *comm, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                                     int32_t flags, double *ll);
/* the mle! objective and its gradient (nhp_cont_loglik_grad) over all ranks: each rank's gradient is exact zeros outside
 * its columns, so the sum is the gradient; [ll; grad] is all-reduced on the device (P+1 doubles, 16.8 MB at N = 1024)
 * before the one download. */
nhp_status nhp_cont_loglik_grad_allreduce(nhp_ctx *ctx, nhp_comm *comm, const nhp_cont_dataset *ds, const nhp_cont_model *model,
                                          int32_t flags, double *ll, double *grad, int64_t grad_len);
/* BASELINE config 5: the per-chain posterior summaries (the running sums of nhp_cont_model_moments_*, still on each
 * rank's device) all-gathered over RCCL: sum_all / sumsq_all [world * len] (rank r at r*len), counts [world],
 * rho_all [world * 3] (ρ, Σρ, Σρ² of nhp_cont_model_get_rho; zeros for a model without a device-side ρ).
 * NHP_ENOTIMPL for a model with a block network or a latent distance network: their sums are not part of the exchange. */
nhp_status nhp_gather_moments(nhp_ctx *ctx, nhp_comm *comm, const nhp_cont_model *model, double *sum_all, double *sumsq_all,
                              int64_t len, int64_t *counts, double *rho_all);

/* ---- network model on the device + chain driver  (src/networks.jl:54-78, src/inference.jl:49-70) ---------------
 * BernoulliNetworkModel.ρ kept next to the model on the device so that a network mcmc! step never drains the stream:
 * _set_rho uploads it, _get_rho returns {ρ, Σρ, Σρ²} (the sums follow nhp_cont_model_moments_accumulate / _reset).
 * _set_rho also detaches a block network (nhp_cont_model_set_sbm) the model had: its network is the scalar ρ from then on. */
nhp_status nhp_cont_model_set_rho(nhp_ctx *ctx, nhp_cont_model *model, double rho);
nhp_status nhp_cont_model_get_rho(nhp_ctx *ctx, const nhp_cont_model *model, double *out /* [3] */);
/* resample_adjacency_matrix!(process, data) with the device-resident ρ (src/continuous.jl:444-487), then
 * resample!(network, A): ρ ~ Beta(α + ΣA, β + N² - ΣA) (src/networks.jl:70-78) drawn on the device as X/(X+Y) from two
 * Philox-keyed Gammas.  Asynchronous.  With a communicator, `ds` is a column shard: the shards' link counts are
 * all-reduced on the device and every rank draws the same ρ (same Philox key). */
/* alpha = beta = 0: ρ is held fixed (DenseNetworkModel, src/networks.jl:13-31: set ρ = 1). */
nhp_status nhp_cont_network_step(nhp_ctx *ctx, nhp_comm *comm /* nullable */, const nhp_cont_dataset *ds, nhp_cont_model *model,
                                 double alpha, double beta, uint64_t seed, uint64_t step);
/* The same step in two halves, for a host that exchanges the shards' link counts itself (no RCCL clique: ranks sharing
 * one GPU, a CPU-side rehearsal): _sweep runs the adjacency sweep with the device-resident ρ and returns this dataset's
 * link count (synchronises); _rho draws ρ ~ Beta(alpha + n_links, beta + n_entries - n_links) on the device with the same
 * Philox key as nhp_cont_network_step, so both routes give the same chain. */
nhp_status nhp_cont_network_sweep(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, uint64_t seed, uint64_t step,
                                  double *n_links);
nhp_status nhp_cont_network_rho(nhp_ctx *ctx, nhp_cont_model *model, double alpha, double beta, double n_links, double n_entries,
                                uint64_t seed, uint64_t step);
/* The body of mcmc!(process, data; nsteps) (src/inference.jl:55-62) for steps [step0, step0 + n_steps): per step one
 * nhp_cont_gibbs_step, for a network model one nhp_cont_network_step (net_alpha, net_beta = the Beta prior of ρ), and --
 * from chain step `burn` on -- one nhp_cont_model_moments_accumulate in place of push!(res.samples, params(process)).
 * Nothing crosses PCIe and the host synchronises once, at the end (where a sampler error of any step is reported).
 * comm (nullable): ONE chain swept by all ranks, each its column shard. */
nhp_status nhp_cont_mcmc_run(nhp_ctx *ctx, nhp_comm *comm /* nullable */, const nhp_cont_dataset *ds, nhp_cont_model *model,
                             const nhp_gibbs_priors *priors, double net_alpha, double net_beta, uint64_t seed,
                             uint64_t step0, int64_t n_steps, int64_t burn);

/* ---- scoring a continuous chain: held-out predictive log-likelihood and WAIC (csrc/cont_score.hip) -------------
 * The time axis is cut at edges b_0 < b_1 < ... < b_K with 0 <= b_0 and b_K <= duration.  Cell i = (k, c) is node c on the block
 * [b_k, b_{k+1}); its log-likelihood under a draw θ is
 *   ℓ_{k,c}(θ) = Σ_{events m of node c, b_k <= t_m < b_{k+1}} log λ_c(t_m)  −  (Λ_c(b_{k+1}) − Λ_c(b_k)),
 * λ the per-event intensity of nhp_cont_event_intensity (exact delays), Λ the compensator of nhp_cont_compensator with all of
 * its conventions (strict window, exponential cut at Δtmax and not renormalised, logit-normal mass W·Δtmax, mask A).  Events
 * before b_0 excite the scored range; events at or after b_K are not scored.  Each term is the density of the block given the
 * past, so the likelihood factorises over the cells sequentially and the pointwise definitions of nhp_disc_score_* carry over:
 * lppd_i, p_i (sample variance, S − 1), elpd_i, waic, se_elpd, joint_lpd, joint_mean, joint_sd.  Over edges covering
 * [0, duration], Σ_k ℓ_{k,c} = Σ log λ_c − Λ_c(duration): the exact log-likelihood, NOT nhp_cont_loglik, which charges every event
 * the full mass of its impulses (the reference's "approximate" integral).
 * A scorer keeps, per cell, a running log-sum-exp and Welford's mean and M2 of ℓ_i, and the same three scalars for Σ_i ℓ_i:
 * 24·K·N bytes of planes (k fastest), plus 8·(bx·N + 4N + K + 25) bytes of sums (bx = min(ceil(K / 256), max(1, 4096 / N)) workgroup partials per
 * column, so bx·N <= max(4096, N)).
 * While a draw is scored the context's scratch holds 8·(max(M, 1) + t·N² + s·K·N) bytes: λ, t = 3 row-major tables (W·A, V, θ;
 * 4 with √τ for logit-normal impulses) and the s <= 64 parts a block's events are summed in (s = 1 unless
 * K·ceil(N / 256) <= 4096 and M / K >= 512).
 * _create: `ds` must outlive the scorer.  NHP_EINVAL: fewer than 2 edges, edges not finite, outside [0, duration] or not
 *   strictly increasing.  NHP_ENOTIMPL: a dataset of several trials, a column shard, N > 65535.  NHP_ENOMEM leaves nothing
 *   allocated.
 * _accumulate: the model's current state as one draw -- λ[M], the tables, the block compensators ΔΛ[k, c] formed directly (a
 *   saturated mass for an event whose whole window lies inside the block, a difference of two CDF values only for events
 *   within Δtmax of an edge), one pass over the cells, one fold of the workgroup partials.  Asynchronous on the main stream, no
 *   host read; no atomics and every sum in one fixed order, so two runs give the same bits.  The dataset / model mismatches
 *   of nhp_cont_loglik apply (NHP_ESHAPE, NHP_EINVAL for another Δtmax); a model with an LGCP baseline and an N beyond the LDS
 *   column budget of the per-event intensity are NHP_ENOTIMPL.
 * _reset: forget the draws.  _fetch (synchronous): NHP_EINVAL ("nothing accumulated") with S = 0;
 *   summary[10] = {S, cells = K·N, lppd, p_waic, elpd_waic, waic = −2·elpd_waic, se_elpd = sqrt(cells · var_i elpd_i) (two
 *   passes), joint_lpd, joint_mean, joint_sd}; per_node[3N] = lppd, p_waic, elpd_waic per node; pointwise[K·N] (nullable,
 *   index k + K·c) = elpd_i.  With S = 1, p_i and everything built on it (and joint_sd) are NaN.
 * _fetch_planes (synchronous): the running planes, each nullable, [K·N] at index k + K·c; NHP_EINVAL with S = 0.
 * nhp_cont_model_attach_score: at most two scorers per model (a third is NHP_EINVAL; not owned: detach before a scorer is
 *   destroyed).  nhp_cont_mcmc_run then reserves their scratch once and calls _accumulate for each on every kept step whose
 *   kept index -- counted per scorer from the attach on, across calls -- is a multiple of `every` (>= 1, else NHP_EINVAL).
 *   Kept steps are those from `burn` on; with the moments off (burn < 0) those from −(burn + 1) on.  score = NULL detaches
 *   all.  With scorers attached a column shard / communicator is NHP_ENOTIMPL; with nothing attached nhp_cont_mcmc_run
 *   launches exactly what it launched before. */
typedef struct nhp_cont_score nhp_cont_score;
nhp_status nhp_cont_score_create(nhp_ctx *ctx, const nhp_cont_dataset *ds, const double *edges, int64_t n_edges, nhp_cont_score **out);
void nhp_cont_score_destroy(nhp_cont_score *score);
nhp_status nhp_cont_score_reset(nhp_ctx *ctx, nhp_cont_score *score);
nhp_status nhp_cont_score_accumulate(nhp_ctx *ctx, nhp_cont_score *score, const nhp_cont_model *model);
nhp_status nhp_cont_score_fetch(nhp_ctx *ctx, const nhp_cont_score *score, double *summary /* [10] */, double *per_node /* [3N] */,
                                double *pointwise /* [K*N] or NULL */);
nhp_status nhp_cont_score_fetch_planes(nhp_ctx *ctx, const nhp_cont_score *score, double *lse, double *mean, double *m2);
nhp_status nhp_cont_model_attach_score(nhp_ctx *ctx, nhp_cont_model *model, nhp_cont_score *score, int64_t every);

/* ---- StochasticBlockNetworkModel (csrc/sbm.hip; the reference's src/networks.jl ends in its empty stub) --------------
 * K blocks, N nodes: z_n ~ Categorical(π), π ~ Dirichlet(γ·1_K), ρ[k,l] ~ Beta(α, β), A[p,c] ~ Bernoulli(ρ[z_p, z_c]) for all
 * N² entries.  Labels are 0-based int32; ρ is K x K column-major (ρ[k,l] at k + K·l); A is N x N column-major.
 * resample!(network, A) = block counts, ρ | counts, π | sizes, then one collapsed-Gibbs sweep over the labels.
 * Errors: NHP_EINVAL for K outside 1..64, NHP_EDOMAIN for a label outside 0..K-1, a ρ entry outside (0, 1), π not positive or
 * not summing to 1 within 1e-12, a non-positive prior parameter; NHP_ENOTIMPL where the label sweep's tables do not fit the
 * LDS (8·N·K + 16·K·(K|1) + N/2 + N + 16 bytes <= 160 KiB and N <= 8192).
 *
 * Stand-alone entries on a host A (synchronous). */
/* L[k,l] = Σ A[p,c]·[z_p = k][z_c = l] (diagonal included) -> links [K*K]; block sizes -> sizes [K].  Exact integers. */
nhp_status nhp_sbm_block_counts(nhp_ctx *ctx, const double *A, int32_t n_nodes, int32_t n_blocks, const int32_t *z, int64_t *links,
                                int64_t *sizes);
/* ρ[k,l] ~ Beta(alpha + L, beta + n_k·n_l - L) as X/(X+Y) from two Philox-keyed Gammas (a pair with an empty block draws
 * from the prior), π ~ Dirichlet(gamma + n) as normalised Gammas, keyed (seed, step): csrc/nhp_rng.h. */
nhp_status nhp_sbm_draw(nhp_ctx *ctx, int32_t n_blocks, const int64_t *links, const int64_t *sizes, double alpha, double beta,
                        double gamma, uint64_t seed, uint64_t step, double *rho_out /* [K*K] */, double *pi_out /* [K] */);
/* n_sweeps label sweeps over n = 0..N-1 in order.  Step i = n + N·sweep draws z_n from
 *   p_k ∝ π_k · Π_l ρ[k,l]^out_l (1-ρ[k,l])^(cnt_l - out_l) · ρ[l,k]^in_l (1-ρ[l,k])^(cnt_l - in_l) · (A[n,n] ? ρ[k,k] : 1-ρ[k,k])
 * (out_l, in_l, cnt_l over the other nodes at their current labels) as the first k with u_i <= p_0 + ... + p_k.
 * u [n_sweeps*N] (nullable: the sweep's own Philox stream keyed (seed, step)); u_used (nullable) returns the uniforms,
 * probs (nullable) [n_sweeps*N*K] the conditional of step i at i·K.  Bit-reproducible for a fixed uniform stream. */
nhp_status nhp_sbm_resample_blocks(nhp_ctx *ctx, const double *A, int32_t n_nodes, int32_t n_blocks, int32_t *z_inout, const double *rho,
                                   const double *pi, const double *u, uint64_t seed, uint64_t step, int32_t n_sweeps, double *u_used,
                                   double *probs);
/* The model's state kept next to the continuous model on the device, as ρ of the Bernoulli model is.  _set_sbm uploads
 * (z, ρ, π) and the priors; _get_sbm returns them (every output nullable) with the running sums of the kept steps
 * (nhp_cont_model_moments_accumulate / _reset carry them; nhp_cont_model_set_rho detaches the block network again): sums = [Σρ (K²); Σρ² (K²); Σπ (K); Σπ² (K)] and block_counts
 * [N*K], the kept steps node n spent in block k at n + N·k. */
nhp_status nhp_cont_model_set_sbm(nhp_ctx *ctx, nhp_cont_model *model, int32_t n_blocks, const int32_t *z, const double *rho,
                                  const double *pi, double alpha, double beta, double gamma);
nhp_status nhp_cont_model_get_sbm(nhp_ctx *ctx, const nhp_cont_model *model, int32_t *z, double *rho, double *pi, double *sums,
                                  int64_t *block_counts);
/* The label sweep runs at the chain steps that are multiples of `every` (default 1: every step); ρ and π are drawn at every step. */
nhp_status nhp_cont_model_set_sbm_labels_every(nhp_ctx *ctx, nhp_cont_model *model, int32_t every);
/* One network step of mcmc! under the block model: the link-probability matrix ρ[z_p, z_c] from the current state, the
 * adjacency sweep (the Philox key of nhp_cont_network_step), then resample!(network, A).  Asynchronous; nothing crosses
 * PCIe.  NHP_ENOTIMPL on a column shard (the labels need every column).  nhp_cont_mcmc_run takes this step for a model
 * with a block network attached and ignores net_alpha / net_beta. */
nhp_status nhp_cont_sbm_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, uint64_t seed, uint64_t step);

/* ---- LatentDistanceNetworkModel (csrc/latent.hip; the other empty stub at the end of the reference's src/networks.jl) ----
 * N nodes in D latent dimensions: z_n ~ N(0, σ² I), b ~ N(μb, σb²), η[p,c] = b - ‖z_p - z_c‖², A[p,c] ~ Bernoulli(1/(1 + exp(-η[p,c])))
 * for all N² entries (the diagonal has η = b).  Positions are N x D column-major (z_n[d] at n + N·d); A is N x N column-major.
 * log p(A | z, b) = Σ A·η - softplus(η), softplus(η) = max(η, 0) + log1p(exp(-|η|)).
 * resample!(network, A) = a sweep over the positions n = 0..N-1, each by elliptical slice sampling given the others, on
 *   L_n(z) = Σ_{j≠n} s_nj·η_j - 2·softplus(η_j), η_j = b - ‖z - z_j‖², s_nj = A[n,j] + A[j,n]
 * with the prior ellipse ν ~ N(0, σ² I), then elliptical slice sampling of b - μb (prior N(0, σb²)) on the full log-likelihood.
 * A slice step follows the reference's elliptical_slice (src/baselines.jl:287-326): threshold L(current) + log u0, θ1 = 2π·u1,
 * bracket [θ1 - 2π, θ1], a rejected θ < 0 becomes the lower end and any other the upper end, θ_k uniform in the bracket by
 * u_k, candidate x·cos θ + ν·sin θ, the first with L >= threshold is accepted, 100 attempts; where the reference throws after
 * them the value is kept and the event counted (`exhausted`).
 * Errors: NHP_EINVAL for N < 1 or D < 1; NHP_ENOTIMPL for D > 8, N > 8192 or 8·N·D + 24·ceil(N/32) + 1576 bytes > 160 KiB (the
 * position sweep keeps every position in LDS); NHP_EDOMAIN for a non-finite position or offset, sigma or
 * sigma_b <= 0.
 *
 * Stand-alone entries on a host A (synchronous). */
/* out [1 + N]: log p(A | z, b), then the N conditional terms L_n at the current state. */
nhp_status nhp_latent_loglik(nhp_ctx *ctx, const double *A, int32_t n_nodes, int32_t n_dims, const double *z, double b, double *out);
/* n_sweeps position sweeps, each followed by the offset update when do_offset is set; n_sweeps = 0 with do_offset: the
 * offset update alone, once.  A sweep has N + 1 slice steps (the offset's is the last; with n_sweeps = 0 it is the only one).
 * draws (nullable: the kernel's own Philox stream keyed (seed, step), csrc/nhp_rng.h) holds the stream of every step: a
 * node's step [D standard normals; u0; u1..u100], the offset's step [1 normal; u0; u1..u100], N·(D + 101) + 102 doubles per
 * sweep (102 with n_sweeps = 0); the slots of an offset step that does not run are read by nothing.  Outputs, all nullable:
 * draws_used returns the stream; attempts [sweeps·(N + 1)] the index 1..100 of the accepted candidate (101: all 100 failed,
 * 0: the step did not run); ll_trace [sweeps·(N + 1)·101] per step the threshold, then L at the candidates 1..attempts
 * (entries after the accepted one are unspecified: a batch may have evaluated more); exhausted the number of steps that
 * used up their attempts.  Bit-reproducible for a fixed draw stream. */
nhp_status nhp_latent_resample(nhp_ctx *ctx, const double *A, int32_t n_nodes, int32_t n_dims, double *z_inout, double *b_inout,
                               double sigma, double mu_b, double sigma_b, const double *draws, uint64_t seed, uint64_t step,
                               int32_t n_sweeps, int32_t do_offset, double *draws_used, int32_t *attempts, double *ll_trace,
                               int64_t *exhausted);
/* The model's state kept next to the continuous model on the device.  _set_latent uploads (z, b) and the priors (the first
 * call allocates; it detaches a block network, as _set_sbm detaches a latent distance network and _set_rho both).
 * _get_latent returns them (every output nullable) with the running sums of the kept steps (nhp_cont_model_moments_accumulate
 * / _reset carry them): sums = [Σb; Σb²], p_sum [N*N] = Σ 1/(1 + exp(-η[p,c])) -- positions are identified only up to
 * rotation, reflection and sign, so the link probabilities are summed and not the positions -- and the count of exhausted
 * slice steps since _set_latent. */
nhp_status nhp_cont_model_set_latent(nhp_ctx *ctx, nhp_cont_model *model, int32_t n_dims, const double *z, double b, double sigma,
                                     double mu_b, double sigma_b);
nhp_status nhp_cont_model_get_latent(nhp_ctx *ctx, const nhp_cont_model *model, double *z, double *b, double *sums, double *p_sum,
                                     int64_t *exhausted);
/* The position sweep runs at the chain steps that are multiples of `every` (default 1); the offset update at every step. */
nhp_status nhp_cont_model_set_latent_positions_every(nhp_ctx *ctx, nhp_cont_model *model, int32_t every);
/* One network step of mcmc! under the latent distance model: the link-probability matrix from the current (z, b), the
 * adjacency sweep (the Philox key of nhp_cont_network_step), then resample!(network, A) with its own stream keyed (seed, step).
 * Asynchronous; nothing crosses PCIe.  NHP_ENOTIMPL on a column shard (the positions need every column).  nhp_cont_mcmc_run
 * takes this step for a model with a latent distance network attached and ignores net_alpha / net_beta. */
nhp_status nhp_cont_latent_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, uint64_t seed, uint64_t step);

/* mle!(process, data; f_abstol, guess) (src/continuous.jl:144-198) with the optimizer's state on the device: minimises
 * -loglikelihood(process, data) over params(process) = [λ0 | grid intensities; θ | μ, τ; W] on the reference's box
 * [lower, upper]^P (1e-6, 10: src/continuous.jl:185-186) by projected L-BFGS fed the analytic gradient; the iterate,
 * gradient and history stay in HBM, the host reads scalars.  Stops by the reference's callback rule
 * |f_k - f_{k-1}| < f_abstol (src/continuous.jl:168-181) or at a stationary point of the box problem (*converged = 1),
 * after max_steps iterations or when no step decreases the objective (*converged = 0).  x [P]: the guess on entry
 * (clamped to the box), the minimiser on return; the device-resident `model` holds it too (params!(process, x)).
 * flags: NHP_LL_RECURSIVE as for nhp_cont_loglik (the reference's objective calls loglikelihood with its default).
 * comm (nullable): `ds` is this rank's column shard, [ll; ∇ll] is summed over the ranks on the device per evaluation and
 * every rank runs the same iteration.  *evals (nullable): objective + gradient evaluations spent.  Standard process only. */
nhp_status nhp_cont_mle_run(nhp_ctx *ctx, nhp_comm *comm /* nullable */, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                            double lower, double upper, double f_abstol, int32_t max_steps, double *x, int64_t len,
                            double *loss, int32_t *steps, int32_t *converged, int32_t *evals);

/* Expectation-maximisation for the standard process with a homogeneous baseline (csrc/cont_em.hip).  The objective is the
 * one nhp_cont_loglik evaluates, ll = -T Σ λ0 - Σ_p cnt_p Σ_c W[p,c] + Σ_i log λ_i; with term_ij = W[n_j,c_i]·ħ(t_i - t_j) over
 * exactly the pairs λ_i sums under `flags` (the window, or every earlier event with NHP_LL_RECURSIVE and exponential
 * impulses), the responsibilities are r_ij = term_ij / λ_i and r_i0 = λ0[c_i] / λ_i.
 *
 * nhp_cont_em_stats: one E-step at the model's current parameters.  *ll the log-likelihood; bg [N]: bg[c] = Σ_{i on c} r_i0;
 * EM, S1, S2 [N*N] column-major [p + c*N] as the model (parent node p, child node c): EM = Σ r_ij;
 *   exponential:  S1 = Σ r_ij·Δt_ij; S2 is not written (nullable);
 *   logit-normal: S1 = Σ r_ij·z_ij, z = logit(Δt/dt_max); S2 = Σ r_ij·(z_ij - μ[p,c])², the second moment CENTRED at the
 *                 model's current μ (the raw Σ r z² loses EM·μ² to cancellation; Σ r z² = S2 + 2μ·S1 - μ²·EM if wanted).
 * Σ_p EM[p,c] + bg[c] = the number of events of node c.  Outputs are host or device pointers by output_on_device (as in
 * nhp_cont_compensator; ll is always a host pointer).  Synchronous.  The sums are the gradient kernels' (the statistics are
 * recovered from the fused log-likelihood + gradient launch without dividing by W, so weights on the lower bound keep theirs):
 * fixed order on the one-launch routes, LDS atomics on the two-pass windowed route.
 *
 * nhp_cont_em_run: the whole iteration on the device.  x [len = N + N²·(2 | 3)] in params! order [λ0; θ | μ; τ; W]: the
 * start on entry (clamped to [lower, upper]), the result on return; the device-resident `model` holds it too.  Iteration k
 * runs the E-step at x_k, whose objective f_k (log-likelihood, plus logprior(x_k) with `priors`) goes to trace[k] (nullable,
 * [max_steps + 1]), then the M-step, each coordinate clamped to the box:
 *   λ0 = bg/T, W = EM/cnt_p, θ = EM/S1 | μ = S1/EM then τ = EM/Σ r (z - μ)² with the clamped μ;
 *   with priors (Gamma(α0, β0) on λ0, Gamma(κ, ν) on W, Gamma(a, b) on θ | normal-gamma(μμ, κμ, a, b) on (μ, τ)) the modes
 *   λ0 = (bg + α0 - 1)/(T + β0), W = (EM + κ - 1)/(cnt_p + ν), θ = (EM + a - 1)/(S1 + b), μ = (S1 + κμ·μμ)/(EM + κμ),
 *   τ = (EM/2 + a - 1/2)/(Σ r (z - μ)²/2 + b + κμ(μ - μμ)²/2);
 *   a coordinate whose term is flat (numerator and denominator both zero) keeps its value, a non-positive numerator goes
 *   to `lower`, a zero denominator under a positive numerator to `upper`.
 * No step decreases the objective.  Stops when |f_k - f_{k-1}| < f_abstol (*converged = 1, *steps = k, x = x_k) or with
 * k = max_steps (*converged = 0); *loss = -f_k as nhp_cont_mle_run reports it.  The host reads one scalar per iteration.
 * An empty dataset is handled (λ0 goes to `lower`, the rest stays).
 *
 * Errors of both: NHP_ENOTIMPL for an LGCP baseline, a model with an adjacency matrix, a column shard and the LDS limits of
 * nhp_cont_loglik_grad; NHP_EDOMAIN when the intensity of some event is not positive and finite; NHP_ESHAPE for a wrong len. */
nhp_status nhp_cont_em_stats(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                             int32_t output_on_device, double *ll, double *bg /* [N] */, double *EM /* [N*N] */,
                             double *S1 /* [N*N] */, double *S2 /* [N*N] nullable */);
nhp_status nhp_cont_em_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                           const nhp_gibbs_priors *priors /* nullable: unregularised */, double lower, double upper, double f_abstol,
                           int32_t max_steps, double *x, int64_t len, double *loss, int32_t *steps, int32_t *converged,
                           double *trace /* nullable, [max_steps + 1] */);

/* Mean-field variational inference for the same model (csrc/cont_vb.hip): em!'s objective with the branching z kept,
 *   log p(events, z | λ0, W, ħ) = Σ_i [z_i0 log λ0[c_i] + Σ_j z_ij (log W[n_j,c_i] + log ħ(Δt_ij))] - T Σ λ0 - Σ_p cnt_p Σ_c W[p,c]
 * over the pairs of `flags`, under the priors of nhp_gibbs_priors (required): λ0 ~ Gamma(α0, β0), W ~ Gamma(κ, ν), θ ~ Gamma(a, b)
 * or (μ, τ) ~ NormalGamma(μμ, κμ, a, b).  One factor per entry, held in two planes S (shape-like) and R (rate-like) of
 * len = N + N²·(2 | 3) doubles in params! order, from the statistics bg, EM, S1, S2 of nhp_cont_em_stats:
 *   block λ0:  S = α' = α0 + bg,  R = β' = β0 + T               block W:  S = κ' = κ + EM,  R = ν' = ν + cnt_p
 *   block θ:   S = a' = a + EM,   R = b' = b + S1
 *   block μ:   S = m',  R = k'    block τ:  S = a',  R = b'     with, centred at the μ = c the statistics were taken at
 *              (D1 = Σ r (z - c), S2 = Σ r (z - c)², d0 = μμ - c):  k' = κμ + EM, m' = c + (D1 + κμ d0)/k', a' = a + EM/2,
 *              b' = b + ½[S2 + κμ d0² - k'(m' - c)²]
 * The statistics are em!'s E-step evaluated at the state's surrogate vector x̃ (not clamped to any box):
 *   λ̃0 = exp(ψ(α') - log β');  θ̃ = a'/b', W̃ = exp(ψ(κ') - log ν' + ψ(a') - log a');
 *   μ̃ = m', τ̃ = a'/b', W̃ = exp(ψ(κ') - log ν' + ½(ψ(a') - log a') - 1/(2k')),
 * whose responsibilities are q(z)'s and whose Σ_i log λ̃_i is its log-normaliser.  The ELBO of a state, q(z) optimal for it:
 *   L = Σ_i log λ̃_i - E_q[compensator] - KL_λ0 - KL_W - KL_imp,     E_q[compensator] = T Σ_c α'/β' + Σ_p cnt_p Σ_c κ'/ν',
 *   KL(Gamma(a₁,b₁)‖Gamma(a₀,b₀)) = (a₁-a₀)ψ(a₁) - lnΓ(a₁) + lnΓ(a₀) + a₀(log b₁ - log b₀) + a₁(b₀-b₁)/b₁, and for the normal-gamma
 *   factor the Gamma KL of (a', b') plus ½[κμ/k' - 1 + log(k'/κμ) + κμ (a'/b')(m' - μμ)²].
 * Every sum of the O(P) passes is taken in one fixed order (no atomics); the statistics' order is the E-step's.
 *
 * nhp_cont_vb_step: one coordinate-ascent update.  S, R [len]: the state on entry, the updated state on return (host or
 * device pointers by output_on_device); with NHP_VB_FROM_MODEL they are output only and the E-step runs at the model's
 * current parameters.  stats [9] (host): [0] Σ_i log λ̃_i at the surrogate stepped from; [1..4] E_q[compensator], KL_λ0, KL_W,
 * KL_imp of the state stepped from (0 with NHP_VB_FROM_MODEL), so that L of that state is stats[0] - stats[1] - ... - stats[4];
 * [5..8] the same four pieces of the updated state.  Synchronous; the model is not changed.  A step that returns
 * NHP_EDOMAIN leaves host S, R as they were passed in (device planes are updated in place and hold the update's output).
 *
 * nhp_cont_vb_run: the whole iteration on the device.  Iteration 0 runs the E-step at x (the guess, used as if it were a
 * surrogate; it has no ELBO) or, with NHP_VB_RESUME, at the surrogate of the state in S, R; iteration k >= 1 at the
 * surrogate of state k, whose ELBO L_k goes to trace[k] (nullable, [max_steps + 1]; trace[0] is NaN for a run from a guess);
 * then the update to state k + 1.  L_k never falls.  Stops when |L_k - L_{k-1}| < f_abstol (*converged = 1, *steps = k) or
 * with k = max_steps (*converged = 0; max_steps >= 1 for a run from a guess).  On return S, R hold state k, x its means
 * (α'/β'; a'/b' | m', a'/b'; κ'/ν') and the device-resident `model` holds them too; *elbo = L_k.  The host reads six
 * scalars per iteration through a pinned slot.  An empty dataset and nodes without events are handled (prior + exposure).
 *
 * Errors of both: the NHP_ENOTIMPL refusals of nhp_cont_em_run; NHP_EINVAL, before any launch, for a missing `priors` or a
 * hyper-parameter that is not positive and finite (μμ: finite; κμ and μμ are read for logit-normal impulses only);
 * NHP_EDOMAIN when the intensity of some event is not positive and finite; NHP_ESHAPE for a wrong len. */
nhp_status nhp_cont_vb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                            const nhp_gibbs_priors *priors, double *S /* [len] */, double *R /* [len] */, int64_t len,
                            int32_t output_on_device, double *stats /* [9] */);
nhp_status nhp_cont_vb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                           const nhp_gibbs_priors *priors, double f_abstol, int32_t max_steps, double *x /* [len] */,
                           double *S /* [len] */, double *R /* [len] */, int64_t len, double *elbo, int32_t *steps,
                           int32_t *converged, double *trace /* nullable, [max_steps + 1] */);

/* Mean-field variational inference for the continuous NETWORK process (csrc/cont_netvb.hip): spike-and-slab weights under a
 * dense or Bernoulli network.  `model` is the lowered network process (it has an adjacency matrix).
 *
 * Likelihood and priors.  The likelihood is nhp_cont_vb_run's full-mass likelihood with the branching z kept; no mask appears
 * in it.  The network acts through the prior of W:  A[p,c] ~ Bernoulli(ρ),  W[p,c] | A = a ~ Gamma(κ_a, ν_a)  (a = 0 the spike,
 * a Gamma of small mean the caller chooses; a = 1 the slab),  ρ ~ Beta(α, β) for a Bernoulli network, ρ ≡ 1 for a dense one
 * (NHP_VB_DENSE_NETWORK).  λ0 and the impulse factors are nhp_cont_vb_run's.  priors->kappa, priors->nu are the slab's
 * (κ1, ν1); net = [κ0, ν0, α, β].
 * Factors:  q(A = 1) = ρv[p,c],  q(W | A = a) = Gamma(κv_a, νv_a),  q(ρ) = Beta(αv, βv).  The state is S, R (nhp_cont_vb_run's
 * planes, device layout [λ0; impulses; W]; the W block holds the slab's κv1, νv1) and Q = [κv0; νv0; ρv; αv; βv] of
 * 3·N² + 2 doubles, matrices column-major [p + c·N].
 * One step from state k:
 *   1. surrogate: nhp_cont_vb_run's with  E log W = (1 - ρv)(ψ(κv0) - log νv0) + ρv (ψ(κv1) - log νv1)  in place of ψ(κ') - log ν'
 *      (two products and a sum, not contracted: ρv = 1 gives the slab's term exactly); the E-step runs at x̃ on a view of the
 *      model without its adjacency matrix, and bg, EM, S1 | D1, S2 are recovered from (x̃, ∇ll) as nhp_cont_vb_step does;
 *   2. λ0 and the impulse factors as nhp_cont_vb_run;  κv_a = κ_a + EM,  νv_a = ν_a + cnt_p  for both a;
 *   3. logit ρv = [ψ(αv) - ψ(βv)] + [κ1 log ν1 - lnΓκ1 + lnΓκv1 - κv1 log νv1] - [κ0 log ν0 - lnΓκ0 + lnΓκv0 - κv0 log νv0]  with the
 *      NEW κv, νv and the OLD (αv, βv);  ρv is the sigmoid of it (exactly 1 or 0 where it saturates, never NaN);
 *   4. αv = α + Σρv,  βv = β + Σ(1 - ρv),  the sums over all N² links, the diagonal included.
 * Every block is an exact coordinate-ascent update, so the ELBO never falls:
 *   L = Σ_i log λ̃_i - E_q[comp] - KL_λ0 - KL_W - KL_imp - KL_net
 *   E_q[comp] = T Σ α'/β' + Σ_p cnt_p Σ_c [(1-ρv) κv0/νv0 + ρv κv1/νv1]
 *   KL_W = Σ [(1-ρv) KL(Gamma(κv0,νv0)‖Gamma(κ0,ν0)) + ρv KL(Gamma(κv1,νv1)‖Gamma(κ1,ν1))]
 *   KL_net = Σ [ρv log ρv + (1-ρv) log(1-ρv) - ρv(ψ(αv) - ψ(αv+βv)) - (1-ρv)(ψ(βv) - ψ(αv+βv))] + KL(Beta(αv,βv)‖Beta(α,β)),
 *   0·log 0 = 0; KL_net = 0 for a dense network.
 * Every sum of the O(P) passes is taken in one fixed order (no atomics); the statistics' order is the E-step's.
 *
 * nhp_cont_netvb_step: one update.  S, R [len], Q: the state on entry, the updated state on return (host pointers, or all
 * three device pointers with output_on_device); with NHP_VB_FROM_MODEL the E-step runs at the model's current parameters
 * and of the state on entry only Q's (αv, βv) are read (step 3 needs the old ones in every mode).  stats [11] (host):
 * [0] Σ_i log λ̃_i at the surrogate stepped from; [1..5] E_q[comp], KL_λ0, KL_W, KL_imp, KL_net of the state stepped from (0 with
 * NHP_VB_FROM_MODEL); [6..10] the same of the state returned.  Synchronous; the model is not changed.
 *
 * nhp_cont_netvb_run: the whole iteration on the device; its loop, stopping rule, trace, NHP_VB_RESUME (S, R, Q hold a state)
 * and empty-dataset handling are nhp_cont_vb_run's.  A run from a guess x reads Q's (αv, βv) alone.  On return S, R, Q hold
 * state k, x its means (the slab's κv1/νv1 for W) and the device model holds them and A = (ρv > ½).  The host reads eight
 * scalars per iteration through a pinned slot.
 *
 * Errors of both, before any launch: NHP_ENOTIMPL for an LGCP baseline, a column shard, a model without A, a model with a
 * block or latent distance network attached; NHP_EINVAL for a missing argument, a prior hyper-parameter or one of κ0, ν0, α,
 * β that is not positive and finite, and (host pointers) αv, βv not positive and finite, and where a state is read a ρv
 * outside [0, 1] or a κv / νv that is not positive and finite.  Then NHP_EDOMAIN and NHP_ESHAPE as nhp_cont_vb_run. */
nhp_status nhp_cont_netvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                               const nhp_gibbs_priors *priors, const double *net /* [4] */, double *S /* [len] */,
                               double *R /* [len] */, int64_t len, double *Q /* [3*N*N + 2] */, int32_t output_on_device,
                               double *stats /* [11] */);
nhp_status nhp_cont_netvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                              const nhp_gibbs_priors *priors, const double *net /* [4] */, double f_abstol, int32_t max_steps,
                              double *x /* [len] */, double *S /* [len] */, double *R /* [len] */, int64_t len,
                              double *Q /* [3*N*N + 2] */, double *elbo, int32_t *steps, int32_t *converged,
                              double *trace /* nullable, [max_steps + 1] */);

/* Mean-field variational inference for the continuous network process under a STOCHASTIC BLOCK network (csrc/cont_netvb.hip,
 * DESIGN §3.31).  Likelihood, λ0, impulse and weight factors are exactly nhp_cont_netvb_run's; the network part is
 *   z_n ~ Categorical(π),  π ~ Dirichlet(γ·1_K),  ρ[k,l] ~ Beta(α, β),  A[p,c] ~ Bernoulli(ρ[z_p, z_c]),  diagonal included,
 *   q(z_n) = Categorical(m[n,:]),  q(π) = Dirichlet(γv),  q(ρ[k,l]) = Beta(αv[k,l], βv[k,l]),  q(A[p,c] = 1) = ρv[p,c].
 * With  E1 = ψ(αv) - ψ(αv+βv),  E0 = ψ(βv) - ψ(αv+βv),  D = ψ(αv) - ψ(βv),  Eπ = ψ(γv) - ψ(Σγv)  and
 *   ω[p,c,k,l] = m[p,k] m[c,l] (p ≠ c),   ω[p,p,k,l] = m[p,k] δ_kl   (a node has one label).
 * net = [κ0, ν0] (the spike), sbm = [α, β, γ], n_blocks = K in 1..64.  The state is S, R [len] (nhp_cont_netvb_run's),
 * Q = [κv0; νv0; ρv] of 3·N² doubles, column-major [p + c·N], and B = [vec αv; vec βv; γv; vec m] of 2K² + K + N·K doubles,
 * column-major (m is [n + k·N]).  One step from state k has the global number i = step0 + (steps taken in this call) + 1:
 *   1. surrogate and E-step as nhp_cont_netvb_step (E log W mixes spike and slab with ρv; the E-step runs at x̃ on the model
 *      without its adjacency matrix);
 *   2. λ0, the impulse factors and κv_a = κ_a + EM, νv_a = ν_a + cnt_p as nhp_cont_netvb_step;
 *   3. logit ρv[p,c] = net[p,c] + the prior and lnΓ / log ν terms of nhp_cont_netvb_step's step 3, in the same cancellation-free
 *      form, where  net[p,c] = Σ_kl ω[p,c,k,l] D[k,l]  from the OLD m, αv, βv:  m·D first (k increasing), then
 *      Σ_l (m·D)[p,l] m[c,l] (l increasing) off the diagonal and Σ_k m[p,k] D[k,k] on it;
 *   4. αv = α + Σ_pc ω ρv,  βv = β + Σ_pc ω (1 - ρv),  γv = γ + Σ_n m  from the NEW ρv and the current m;
 *   5. if i % labels_every == 0 the sequential label sweep over the nodes 0 .. N-1, each node reading the current m of the
 *      others:  m[n,:] = softmax(s),  s_k = Eπ[k] + ρv[n,n] E1[k,k] + (1 - ρv[n,n]) E0[k,k] + Σ_{c≠n} Σ_l m[c,l] (ρv[n,c] E1[k,l]
 *      + (1 - ρv[n,c]) E0[k,l] + ρv[c,n] E1[l,k] + (1 - ρv[c,n]) E0[l,k])  at the tables of step 4 (nhp_disc_sbmvb_run's sweep: there
 *      is one in the library); otherwise m stays bit for bit.
 * Each of (2-3), 4 and 5 is an exact block of coordinate ascent, so the ELBO never falls:
 *   L = Σ_i log λ̃_i - E_q[comp] - KL_λ0 - KL_W - KL_imp - KL_net          (the first five as nhp_cont_netvb_run)
 *   KL_net = Σ_pc [ρv ln ρv + (1-ρv) ln(1-ρv)] - [links + labels - KL_Dir - ΣKL_Beta]
 *   links = Σ_kl (T1 E1 + T0 E0),  T1 = Σ_pc ω ρv,  T0 = Σ_pc ω (1 - ρv)  at the state's OWN m (after the sweep, if one ran)
 *   labels = Σ_nk m (Eπ - ln m),  KL_Dir = KL(Dir(γv) ‖ Dir(γ·1_K)),  ΣKL_Beta = Σ_kl KL(Beta(αv,βv) ‖ Beta(α,β)),  0·ln 0 = 0.
 * With K = 1 every formula is the Bernoulli network's (m ≡ 1, Eπ = 0, KL_Dir = 0).  Every sum is taken in one fixed order.
 *
 * nhp_cont_sbmvb_step: one update, numbered step0 + 1.  S, R, Q, B: the state on entry, the updated state on return (host
 * pointers, or all four device pointers with output_on_device); with NHP_VB_FROM_MODEL the E-step runs at the model's current
 * parameters and of the state on entry B alone is read.  stats [21] (host): [0..10] as nhp_cont_netvb_step with KL_net as
 * above in [5] and [10]; [11..15] the network pieces (Σ entropy of ρv, links, labels, KL_Dir, ΣKL_Beta) of the state stepped
 * from (0 with NHP_VB_FROM_MODEL), [16..20] of the state returned.  Synchronous; the model is not changed.
 *
 * nhp_cont_sbmvb_run: the whole iteration on the device; loop, stopping rule, trace, NHP_VB_RESUME (S, R, Q hold a state; B
 * always does) and empty-dataset handling are nhp_cont_vb_run's.  On return S, R, Q, B hold state k, x its means and the
 * device model holds them and A = (ρv > ½), as nhp_cont_netvb_run leaves them.
 *
 * Errors of both, before any launch: NHP_ENOTIMPL for an LGCP baseline, a column shard, a model without A, a latent
 * distance network attached, and a label sweep whose LDS need exceeds a CU's; NHP_EINVAL for a missing argument, K outside
 * 1..64, labels_every < 1, step0 < 0, priors or (host pointers) tables that are not positive and finite, a row of m that
 * does not sum to 1 within 1e-12, the NHP_VB_DENSE_NETWORK flag, and nhp_cont_netvb_step's checks of κ0, ν0, ρv, κv, νv.  Then
 * NHP_EDOMAIN and NHP_ESHAPE as nhp_cont_vb_run.  nhp_cont_netvb_step / _run keep refusing a model with a block network. */
nhp_status nhp_cont_sbmvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                               const nhp_gibbs_priors *priors, const double *net /* [2] */, const double *sbm /* [3] */,
                               int32_t n_blocks, int32_t labels_every, int64_t step0, double *S /* [len] */, double *R /* [len] */,
                               int64_t len, double *Q /* [3*N*N] */, double *B /* [2*K*K + K + N*K] */, int32_t output_on_device,
                               double *stats /* [21] */);
nhp_status nhp_cont_sbmvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                              const nhp_gibbs_priors *priors, const double *net /* [2] */, const double *sbm /* [3] */,
                              int32_t n_blocks, int32_t labels_every, int64_t step0, double f_abstol, int32_t max_steps,
                              double *x /* [len] */, double *S /* [len] */, double *R /* [len] */, int64_t len,
                              double *Q /* [3*N*N] */, double *B /* [2*K*K + K + N*K] */, double *elbo, int32_t *steps,
                              int32_t *converged, double *trace /* nullable, [max_steps + 1] */);

/* Mean-field variational inference for the continuous network process under a LATENT DISTANCE network (csrc/cont_netvb.hip,
 * csrc/nhp_latvb_dev.h).  Likelihood, λ0, impulse and weight factors are exactly nhp_cont_netvb_run's; the network part is
 *   z_n ~ N(0, σ² I_D),  b ~ N(μb, σb²),  A[p,c] ~ Bernoulli(s(η[p,c])),  η[p,c] = b - ‖z_p - z_c‖²,  s the logistic function,
 * over all N² entries (the diagonal has η = b), D = n_dims in 1..8.  q(A[p,c] = 1) = ρv[p,c]; the network's factor is a POINT MASS at
 * (zv, bv): variational EM over the positions and the offset.  (η is quadratic in z, so a bound on the logistic likelihood would
 * still leave a quartic; a point estimate keeps the bound exact.)  Hence E_q[log s(η)] - E_q[log(1 - s(η))] = η[p,c] exactly.
 * net = [κ0, ν0] (the spike), lat = [σ, μb, σb].  The state is S, R [len] (nhp_cont_netvb_run's), Q = [κv0; νv0; ρv] of 3·N² doubles,
 * column-major [p + c·N], and Z = [vec zv; bv] of N·D + 1 doubles, zv column-major (z_n[d] at n + N·d).  One step from state k:
 *   1. surrogate and E-step as nhp_cont_netvb_step (the E-step runs at x̃ on the model without its adjacency matrix);
 *   2. λ0, the impulse factors and κv_a = κ_a + EM, νv_a = ν_a + cnt_p as nhp_cont_netvb_step;
 *   3. logit ρv[p,c] = η[p,c] + the prior and lnΓ / log ν terms of nhp_cont_netvb_step's step 3, in the same cancellation-free form,
 *      with η from the OLD (zv, bv), ‖z_p - z_c‖² added over d increasing;
 *   4. J = ascent_steps (0..64) iterations of a monotone ascent, at the NEW ρv, of
 *        F(z, b) = Σ_pc [ρv η - softplus(η)] - ‖z‖²/(2σ²) - (b - μb)²/(2σb²),   softplus(η) = max(η, 0) + log1p(exp(-|η|)).
 *      With C = ρv + ρvᵀ (η is symmetric):  Σ_pc [ρv η - softplus(η)] = ½ Σ_nj [C[j,n] η_nj - 2 softplus(η_nj)]  over all ordered (n, j),
 *        ∂F/∂z_n = -2 Σ_j (C[j,n] - 2 s(η_nj)) (z_n - z_j) - z_n/σ²,     ∂F/∂b = ½ Σ_nj (C[j,n] - 2 s(η_nj)) - (b - μb)/σb².
 *      One iteration takes G = ∇F at the current (z, b) and evaluates F at (z, b) + t_r·G for the R = 8 step sizes
 *        t_r = τ·4^(1-r),  r = 0..7,  τ = 1/(N + 1/σ²)
 *      and at t = 0 in ONE pass over the pairs: with Δz = z_n - z_j, Δg = G_n - G_j, a = ‖Δz‖², bb = Δz·Δg, c = ‖Δg‖²,
 *        η_nj(t) = (b + t·G_b) - (a + t·(2·bb + t·c)),   ‖z + tG_z‖² = Σz² + t·(2 Σz·g + t·Σg²).
 *      It moves to the rung with the largest F, the lowest index on ties, if that F EXCEEDS F at t = 0 (same pass, same form), and
 *      stays where it is otherwise (rung -1).  J = 0 holds the network fixed: zv, bv are returned bit for bit.
 * Steps (2-3) and every iteration of 4 are coordinate ascents of one bound, so the ELBO never falls:
 *   L = Σ_i log λ̃_i - E_q[comp] - KL_λ0 - KL_W - KL_imp - KL_net          (the first five as nhp_cont_netvb_run)
 *   KL_net = Σ_pc [ρv ln ρv + (1-ρv) ln(1-ρv)] - [links + ln p(zv) + ln p(bv)],   links = Σ_pc [ρv η - softplus(η)] at the state's OWN
 *   (zv, bv), evaluated directly (not through the ray's quadratic),  ln p(z) = -‖z‖²/(2σ²) - (N·D/2) ln(2πσ²),
 *   ln p(b) = -(b - μb)²/(2σb²) - ½ ln(2πσb²),  0·ln 0 = 0.
 * No floating-point atomics and no host round trip inside a step; every sum is taken in one fixed order.
 *
 * nhp_cont_latvb_step: one update.  S, R, Q, Z: the state on entry, the updated state on return (host pointers, or all four
 * device pointers with output_on_device); with NHP_VB_FROM_MODEL the E-step runs at the model's current parameters and of the
 * state on entry Z alone is read (Z is read in every mode).  stats [19 + J] (host): [0..10] as nhp_cont_netvb_step with KL_net as above in [5] and
 * [10]; [11..14] the network pieces (Σ entropy of ρv, links, ln p(zv), ln p(bv)) of the state stepped from (0 with
 * NHP_VB_FROM_MODEL), [15..18] of the state returned; [19..19+J-1] the rung each ascent iteration took (-1: it stayed).
 * Synchronous; the model is not changed.
 *
 * nhp_cont_latvb_run: the whole iteration on the device; loop, stopping rule, trace, NHP_VB_RESUME (S, R, Q hold a state; Z always
 * does) and empty-dataset handling are nhp_cont_vb_run's.  On return S, R, Q, Z hold state k, x its means and the device model
 * holds them and A = (ρv > ½), as nhp_cont_netvb_run leaves them.
 *
 * Errors of both, before any launch: NHP_ENOTIMPL for an LGCP baseline, a column shard, a model without A, a block network
 * attached; NHP_EINVAL for a missing argument, D outside 1..8, J outside 0..64, σ or σb not positive and finite, μb not finite,
 * (host pointers) a non-finite position or offset, the NHP_VB_DENSE_NETWORK flag, and nhp_cont_netvb_step's checks of κ0, ν0, ρv,
 * κv, νv.  Then NHP_EDOMAIN and NHP_ESHAPE as nhp_cont_vb_run.  nhp_cont_netvb_step / _run keep refusing a latent distance network. */
nhp_status nhp_cont_latvb_step(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                               const nhp_gibbs_priors *priors, const double *net /* [2] */, const double *lat /* [3] */,
                               int32_t n_dims, int32_t ascent_steps, double *S /* [len] */, double *R /* [len] */, int64_t len,
                               double *Q /* [3*N*N] */, double *Z /* [N*D + 1] */, int32_t output_on_device,
                               double *stats /* [19 + ascent_steps] */);
nhp_status nhp_cont_latvb_run(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *model, int32_t flags,
                              const nhp_gibbs_priors *priors, const double *net /* [2] */, const double *lat /* [3] */,
                              int32_t n_dims, int32_t ascent_steps, double f_abstol, int32_t max_steps, double *x /* [len] */,
                              double *S /* [len] */, double *R /* [len] */, int64_t len, double *Q /* [3*N*N] */,
                              double *Z /* [N*D + 1] */, double *elbo, int32_t *steps, int32_t *converged,
                              double *trace /* nullable, [max_steps + 1] */);
/* The soft-link counterpart of nhp_latent_loglik: out [N·D + 2] = F(z, b) as above for the link probabilities rho [N*N]
 * (column-major, each in [0, 1]), then ∇F in the layout of Z (N·D position entries, then ∂F/∂b).  Host pointers; synchronous.
 * NHP_EINVAL for N < 1, D outside 1..8, a non-finite position or offset, priors that cannot be, a rho outside [0, 1]. */
nhp_status nhp_latent_expected_loglik(nhp_ctx *ctx, const double *rho, int32_t n_nodes, int32_t n_dims, const double *z, double b,
                                      const double *lat /* [3]: sigma, mu_b, sigma_b */, double *out /* [N*D + 2] */);

/* Observed information and Hessian-vector products of the continuous log-likelihood (csrc/cont_information.hip).  The
 * objective nhp_cont_loglik evaluates separates by child node c, so its Hessian is block diagonal: one block per column
 * over the D = 1 + kinds·N parameters [λ0[c]; θ[:,c] | μ[:,c]; τ[:,c]; W[:,c]] (kinds = 2 exponential, 3 logit-normal), row and
 * column 0 λ0[c], then 1 + q·N + p for impulse kind q of parent p, then 1 + (kinds-1)·N + p for W[p,c].  Homogeneous baseline;
 * standard and network models (a = A[p,c] multiplies the pair sums).  flags: NHP_LL_RECURSIVE (exponential impulses) sums
 * every earlier event with t_j > 0 through the truncated windows of nhp_cont_loglik (less than 2^-60·λ_i dropped per event).
 *
 * nhp_cont_information: blocks[k] = MINUS the Hessian block of column columns[k] (all N columns in order when columns is
 * NULL), D·D doubles each, column-major, exactly symmetric; a host pointer, or a device pointer with on_device.  *ll
 * (nullable, host) the log-likelihood.  tile_nodes: parent nodes per tile of a block kept in LDS; 0 picks the whole block
 * where it fits the 160 KiB and the largest tile that does otherwise.  Sums are LDS and global fp64 atomics: entries are
 * not bit-reproducible from run to run.
 * nhp_cont_hessian_vec: out = H·v (the Hessian itself), v and out [len = P] in params! order [λ0; θ | μ; τ; W]; host
 * pointers, or device pointers with on_device.  Stores no block.
 *
 * Both are synchronous and write nothing when they refuse: NHP_ENOTIMPL for an LGCP baseline, a column shard,
 * NHP_LL_FULL_RECURSION, a recursive objective without a usable truncated window, and a tile or column that does not fit
 * the LDS; NHP_EINVAL for a column index outside [0, N) or repeated, n_columns <= 0 with columns given, tile_nodes outside
 * [0, N], and len != P; NHP_ENOMEM when the blocks do not fit in device memory.  nhp_last_error gives the reason. */
nhp_status nhp_cont_information(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                                const int32_t *columns /* [n_columns], 0-based; NULL: all */, int32_t n_columns,
                                int32_t tile_nodes /* 0: auto */, int32_t on_device,
                                double *ll /* nullable */, double *blocks /* [n_columns · D · D], each block column-major */);
nhp_status nhp_cont_hessian_vec(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *model, int32_t flags,
                                int32_t on_device, const double *v /* [P] */, double *out /* [P] */, int64_t len);

/* mle!(process::DiscreteStandardHawkesProcess, data; f_abstol, guess) (src/discrete.jl:211-296) the same way: x = params(process)
 * = [λ0; vec(W .* θ)] (src/discrete.jl:178-182; homogeneous baseline), the objective -loglikelihood(process, data, convolved) with
 * params!'s split W = Σ_b, θ = x ./ W (:195-203) redone on the device per evaluation, its gradient from the two GEMMs of
 * nhp_disc_loglik_grad, the box and the |f_k - f_{k-1}| < f_abstol rule of the callback (:247-258; a monotone line search never
 * meets its loss-increase rule).  nhp_disc_convolve must have run on `data`. */
nhp_status nhp_disc_mle_run(nhp_ctx *ctx, const nhp_disc_dataset *data, double dt, double lower, double upper, double f_abstol,
                            int32_t max_steps, double *x, int64_t len, double *loss, int32_t *steps, int32_t *converged, int32_t *evals);

/* Observed and Fisher information of the discrete log-likelihood nhp_disc_loglik evaluates, in mle!'s parameters
 * x = [λ0 (N); vec(η)], η = W∘θ (csrc/disc_information.hip; DiscreteStandardHawkesProcess with a homogeneous baseline, what
 * nhp_disc_mle_run fits).  λ[t,c] = dt·x_tᵀ z_c with x_t = [1; Ŝ[t,·,·]] and z_c = [λ0[c]; η[·,c,·]] is linear, so minus the
 * Hessian is block diagonal by child node c, one D x D block each, D = 1 + N·B:
 *     kind 0, observed:  J_c = dt²·Σ_t (s[t,c]/λ[t,c]²)·x_t x_tᵀ        kind 1, Fisher:  I_c = dt²·Σ_t (1/λ[t,c])·x_t x_tᵀ
 * Row and column 0 are λ0[c]; row 1 + b·N + p is η[p,c,b] (vec(η) restricted to column c).  Both kinds are positive
 * semi-definite.  nhp_disc_convolve must have run on the dataset.
 *
 * nhp_disc_information: blocks[k] = the block of column columns[k] (all N columns in order when columns is NULL), D·D
 * doubles each, column-major, exactly symmetric; a host pointer or a device pointer (the library asks the runtime which).
 * *ll (nullable, host): the log-likelihood of the same parameters, the value nhp_disc_loglik returns.  tile_rows: rows of
 * a tile of a block, a multiple of 16 up to 96; slab_bins: bins of a slab of the time axis (rounded up to whole 16-bin
 * chunks), whose partial blocks are summed in slab order; 0 picks either automatically.  No atomics: the same call gives
 * the same bits.  The observed kind loads only the 16-bin chunks of a column that hold an event.
 * nhp_disc_hessian_vec: out = J·v, the INFORMATION (minus the Hessian, positive semi-definite sign) of the given kind
 * times v; v and out are full-length vectors [N + N·N·B] in mle!'s order, host or device pointers.  Stores no block.
 *
 * Both are synchronous and write nothing when they refuse: NHP_ENOTIMPL for an LGCP baseline (lambda0 == NULL with a grid
 * attached); NHP_EDOMAIN for a column index outside [0, N) or repeated, and dt <= 0; NHP_EINVAL for null pointers, a kind
 * other than 0 / 1, n_columns <= 0 with columns given, tile_rows not a multiple of 16 in [0, 96], slab_bins < 0;
 * NHP_ENOMEM, with the byte count, when the blocks or the split-T workspace do not fit in device memory. */
nhp_status nhp_disc_information(nhp_ctx *ctx, const nhp_disc_dataset *data, const double *lambda0, const double *W,
                                const double *theta, double dt, int32_t kind /* 0 observed, 1 Fisher */,
                                const int32_t *columns /* [n_columns], 0-based; NULL: all */, int32_t n_columns,
                                int32_t tile_rows /* 0: auto */, int32_t slab_bins /* 0: auto */,
                                double *ll /* nullable */, double *blocks /* [n_columns · D · D], each block column-major */);
nhp_status nhp_disc_hessian_vec(nhp_ctx *ctx, const nhp_disc_dataset *data, const double *lambda0, const double *W,
                                const double *theta, double dt, int32_t kind, const double *v /* [P] */, double *out /* [P] */);

#ifdef __cplusplus
}
#endif
#endif
