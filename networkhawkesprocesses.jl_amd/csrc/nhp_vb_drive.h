// The host drivers of the continuous variational fits: ONE step and ONE run, which the six entry points of cont_vb.hip and
// cont_netvb.hip call after their own argument checks.  A fit is a plain struct (no base class, no virtual call) with
//   OUT, L_SLOT, STAT_PIECES   scalars an ELBO evaluation writes, which of them is L, pieces per state in stats[]
//   UNMASK                     the E-step sees the model without its adjacency matrix
//   state                      the device pointers of one state; x (its surrogate) is the member the drivers read
//   reserve_doubles()          the sizing function of what carve + carve_shared + two sets of scalars take
//   carve(bump, state), carve_shared(bump)
//   planes(state, out[PLANES]) the caller's arrays and where the state keeps them (`always`: read without a state too)
//   start(st, xin, s), surrogate(st, s), elbo(st, s, made_here, out), update(ctx, st, cur, nxt, grad, k), mean(st, s, x, m)
//   stats(h, from_model, stats)
// and, for the standard fit alone, place_step (a step that works in place on one pair of planes).
#pragma once
#include <algorithm>
#include <cmath>

#include "nhp_vb.h"

struct vb_plane { double *user, *dev; size_t n; bool always; };

// stats[0] = Σ log λ̃, then np pieces of the state stepped from (zeros without one) and np of the state stepped to
inline void vb_fill_stats(const double *h, int out, int np, bool from_model, double *stats)
{
    stats[0] = h[0];
    for (int j = 1; j <= np; ++j) { stats[j] = from_model ? 0.0 : h[j]; stats[np + j] = h[out + j]; }
}

// max_steps and len of a run, between the fit's own checks
inline nhp_status vb_run_args(nhp_ctx *ctx, const nhp_cont_model *m, bool resume, int32_t max_steps, int64_t len)
{
    if (max_steps < (resume ? 0 : 1)) {
        nhp_set_error(ctx, "vb!: max_steps = %d (a run from a guess needs at least one step to have a state)", max_steps);
        return NHP_EDOMAIN;
    }
    return nhp_layout_check(ctx, nhp_layout(m), len);
}

// reserve the block and carve two states, the fit's shared scratch and the scalars; nothing is launched unless the carving
// took exactly what the sizing function said
template <class FIT>
nhp_status vb_carve(nhp_ctx *ctx, FIT &f, typename FIT::state &cur, typename FIT::state &nxt, double **d_out)
{
    const size_t want = f.reserve_doubles();
    NHP_TRY(nhp_ctx_reserve_mle(ctx, 8 * want, "variational state"));
    vb_bump mem((double *)ctx->d_mle);
    f.carve(mem, cur);
    f.carve(mem, nxt);
    f.carve_shared(mem);
    *d_out = mem.take(2 * (size_t)FIT::OUT);
    if (mem.used() != want) {
        nhp_set_error(ctx, "variational state: carved %zu doubles of %zu reserved (sizing and carving disagree)", mem.used(), want);
        return NHP_EINVAL;
    }
    return NHP_OK;
}

// the caller's arrays into state s (`kind`: where they are); without a state only the ones read in every mode
template <class FIT>
nhp_status vb_upload(nhp_ctx *ctx, hipStream_t st, const FIT &f, const typename FIT::state &s, bool with_state, hipMemcpyKind kind)
{
    vb_plane pl[FIT::PLANES];
    f.planes(s, pl);
    for (const vb_plane &p : pl)
        if ((with_state || p.always) && p.dev != p.user) NHP_HIP(ctx, hipMemcpyAsync(p.dev, p.user, 8 * p.n, kind, st));
    return NHP_OK;
}

template <class FIT>
nhp_status vb_hand_back(nhp_ctx *ctx, hipStream_t st, const FIT &f, const typename FIT::state &s, bool on_device)
{
    vb_plane pl[FIT::PLANES];
    f.planes(s, pl);
    for (const vb_plane &p : pl) {
        if (p.dev == p.user) continue;
        if (on_device) NHP_HIP(ctx, hipMemcpyAsync(p.user, p.dev, 8 * p.n, hipMemcpyDeviceToDevice, st));
        else NHP_TRY(nhp_download(ctx, p.user, p.dev, 8 * p.n));
    }
    return NHP_OK;
}

inline nhp_cont_model vb_estep_view(const nhp_cont_model *m, bool unmask)
{
    nhp_cont_model v = *m;                                            // (the E-step bumps the version of what it evaluates)
    if (unmask) { v.has_A = 0; v.d_A = nullptr; }                     // the network acts through the prior of W alone
    return v;
}

// One coordinate-ascent update: state (or the model's parameters) -> surrogate -> E-step -> ELBO of the old state, update,
// ELBO of the new one.  Nothing reaches the caller's arrays unless Σ log λ̃ is finite.
template <class FIT>
nhp_status vb_step_drive(nhp_ctx *ctx, const nhp_cont_dataset *ds, const nhp_cont_model *m, int32_t flags, FIT &f, bool from_model,
                         bool on_device, double *stats)
{
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    typename FIT::state cur, nxt;
    double *d_out = nullptr;
    NHP_TRY(vb_carve(ctx, f, cur, nxt, &d_out));
    f.place_step(cur, nxt, on_device);
    NHP_TRY(vb_upload(ctx, st, f, cur, !from_model, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (from_model) f.start(st, (const double *)m->d_params, cur);
    else f.surrogate(st, cur);
    NHP_HIP(ctx, hipGetLastError());
    double *d_grad = nullptr;
    nhp_cont_model view = vb_estep_view(m, FIT::UNMASK);
    NHP_TRY(nhp_em_estep(ctx, ds, &view, flags, cur.x, (int64_t)nhp_layout(m).P, &d_grad));
    f.elbo(st, cur, false, d_out);
    NHP_TRY(f.update(ctx, st, cur, nxt, d_grad, 0));
    f.elbo(st, nxt, true, d_out + FIT::OUT);
    NHP_HIP(ctx, hipGetLastError());
    double h[2 * FIT::OUT];
    NHP_TRY(nhp_download(ctx, h, d_out, sizeof h));
    if (!std::isfinite(h[0])) {
        NHP_HIP(ctx, hipStreamSynchronize(st));
        nhp_set_error(ctx, "update!: the intensity of some event is not positive and finite");
        return NHP_EDOMAIN;
    }
    NHP_TRY(vb_hand_back(ctx, st, f, nxt, on_device));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    f.stats(h, from_model, stats);
    return NHP_OK;
}

// The whole iteration.  Two states: an update writes the other one only, so nothing is lost when the rule says stop.
template <class FIT>
nhp_status vb_run_drive(nhp_ctx *ctx, const nhp_cont_dataset *ds, nhp_cont_model *m, int32_t flags, FIT &f, bool resume, double f_abstol,
                        int32_t max_steps, double *x, double *elbo, int32_t *steps_out, int32_t *converged_out, double *trace)
{
    NHP_HIP(ctx, hipSetDevice(ctx->device));
    NHP_TRY(nhp_check_deferred(ctx));
    hipStream_t st = ctx->main();
    const size_t P = nhp_layout(m).P;
    nhp_em_host hs;
    if (hipHostMalloc((void **)&hs.h, 8 * FIT::OUT) != hipSuccess) { hs.h = nullptr; nhp_set_error(ctx, "out of pinned memory"); return NHP_ENOMEM; }
    NHP_HIP(ctx, hipEventCreateWithFlags(&hs.ev, hipEventDisableTiming));
    typename FIT::state cur, nxt;
    double *d_out = nullptr;
    NHP_TRY(vb_carve(ctx, f, cur, nxt, &d_out));

    NHP_TRY(vb_upload(ctx, st, f, cur, resume, hipMemcpyHostToDevice));
    if (resume) {
        f.surrogate(st, cur);
    } else {
        NHP_HIP(ctx, hipMemcpyAsync(nxt.x, x, 8 * P, hipMemcpyHostToDevice, st));
        f.start(st, (const double *)nxt.x, cur);
    }
    NHP_HIP(ctx, hipGetLastError());

    const double nan = std::nan("");
    double L = nan, L_prev = nan;
    bool has_state = resume, converged = false, made_here = false;    // made_here: `cur` came out of the fit's update
    nhp_cont_model view = vb_estep_view(m, FIT::UNMASK);
    nhp_cont_model *em = FIT::UNMASK ? &view : m;
    int k = 0;
    for (;; ++k) {
        // E-step at x̃_k and the ELBO of state k (which may complete the state: the network's scalars, read by the update); the
        // update is enqueued behind the scalars' copy, so it runs while the host looks at the stopping rule
        double *d_grad = nullptr;
        NHP_TRY(nhp_em_estep(ctx, ds, em, flags, cur.x, (int64_t)P, &d_grad));
        f.elbo(st, cur, made_here, d_out);
        NHP_HIP(ctx, hipGetLastError());
        NHP_HIP(ctx, hipMemcpyAsync(hs.h, d_out, 8 * FIT::OUT, hipMemcpyDeviceToHost, st));
        NHP_HIP(ctx, hipEventRecord(hs.ev, st));
        if (k < max_steps) NHP_TRY(f.update(ctx, st, cur, nxt, d_grad, k));
        NHP_HIP(ctx, hipEventSynchronize(hs.ev));
        if (!std::isfinite(hs.h[0])) {
            NHP_HIP(ctx, hipStreamSynchronize(st));
            nhp_set_error(ctx, "vb!: the intensity of some event is not positive and finite (iteration %d)", k);
            return NHP_EDOMAIN;
        }
        L_prev = L; L = has_state ? hs.h[FIT::L_SLOT] : nan;
        if (trace) trace[k] = L;
        if (has_state && std::fabs(L - L_prev) < f_abstol) { converged = true; break; }     // (false while L_prev is NaN)
        if (k == max_steps) break;
        std::swap(cur, nxt);
        has_state = true; made_here = true;
    }
    if (FIT::UNMASK) {
        m->version = view.version;
        nhp_model_view_keep_bound(m, view);
    }
    // the state, and its means (and A = (ρv > ½)) into x and the model's own block
    f.mean(st, cur, nxt.x, m);
    NHP_HIP(ctx, hipGetLastError());
    ++m->version;
    NHP_HIP(ctx, hipMemcpyAsync(m->d_params, nxt.x, 8 * P, hipMemcpyDeviceToDevice, st));
    NHP_TRY(nhp_download(ctx, x, nxt.x, 8 * P));
    NHP_TRY(vb_hand_back(ctx, st, f, cur, false));
    NHP_HIP(ctx, hipStreamSynchronize(st));
    *elbo = L; *steps_out = k; *converged_out = converged ? 1 : 0;
    return NHP_OK;
}
