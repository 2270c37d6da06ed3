// Streaming convergence diagnostics, the part both device-resident chains share (include/nhp.h: nhp_cont_model_diagnostics_*,
// nhp_disc_model_diagnostics_*).  A model keeps its own running sums Σx, Σx² (and the network scalars
// {ρ, Σρ, Σρ², ΣA}); the diagnostics add the batch planes and the snapshots of those sums.  What differs between the models
// is the SOURCE of x -- the continuous parameter block with the A seam (cont_diagnostics.hip: k_diag_accumulate), the
// discrete block with its product W∘θ (disc_chain.hip: k_disc_accumulate) -- so each model owns its accumulate kernel, built
// on diag_update below, and everything else (planes, snapshots, the finalize kernels) is cont_diagnostics.hip's, once.
#pragma once
#include "nhp_internal.h"

struct nhp_diag_state {
    int64_t b = 0, planned = 0, h = 0;      // batch length, planned kept steps, ⌊planned/2⌋
    int64_t count = 0;                      // kept steps the planes have seen
    int64_t len = 0;                        // entries
    int nsnap = 0;                          // 0 (h < 2), 1 (planned even) or 2
    double *d_bat = nullptr;                // ONE allocation: B | SB | QB [3][len], snapshots [nsnap][2][len], ρ's scalars [8]
    double *d_snap = nullptr;
    double *d_rho = nullptr;                // {B, SB, QB, snapA Σρ, Σρ², snapB Σρ, Σρ², -}
};

// a model's running sums as the diagnostics see them: Σx | Σx² [2][len], the kept steps behind them, and the network
// scalars {ρ, Σρ, Σρ², ΣA} (null: none)
struct nhp_diag_sums {
    double *d_mom;
    int64_t len, count;
    double *d_rho;
};

// the five array groups of the summary: entries [start, end) of the sums' order (a group may be empty, and the groups need
// not follow one another: the discrete network block is λ0 | W | θ | A with θ as group 1 and W as group 3)
struct nhp_diag_groups { int64_t start[NHP_DIAG_GROUPS - 1], end[NHP_DIAG_GROUPS - 1]; };

// every expression is the one include/nhp.h writes down, operation by operation (the tests hold it to a numpy restatement):
// no contraction.  The one fused multiply-add is explicit: Σx² += x·x, as the moments kernel compiles it.
template <bool BOUNDARY>
__device__ __forceinline__ void diag_update(double x, double &s1, double &s2, double &B, double &SB, double &QB, double b)
{
#pragma clang fp contract(off)
    s1 += x;
    s2 = __builtin_fma(x, x, s2);
    B += x;
    if (BOUNDARY) {
        const double m = B / b;
        SB += m;
        QB += m * m;
        B = 0.0;
    }
}

template <bool BOUNDARY>
__device__ __forceinline__ void diag_rho(double *__restrict__ rho, double *__restrict__ rd, double b)
{
    const double r = rho[0];
    double s1 = rho[1], s2 = rho[2], B = rd[0], SB = 0.0, QB = 0.0;
    if (BOUNDARY) { SB = rd[1]; QB = rd[2]; }
    diag_update<BOUNDARY>(r, s1, s2, B, SB, QB, b);
    rho[1] = s1; rho[2] = s2; rd[0] = B;
    if (BOUNDARY) { rd[1] = SB; rd[2] = QB; }
}

// cont_diagnostics.hip.  `d` is the model's own pointer to its state (null: not configured); all asynchronous on the main
// stream except where a plane is freed.
void nhp_diag_release(nhp_diag_state **d);
// _configure of either model: (0, 0) turns the diagnostics off, anything else (re)allocates the planes for `len` entries
// and zeroes them and the kept count
nhp_status nhp_diag_configure(nhp_ctx *ctx, nhp_diag_state **d, int64_t len, int64_t batch_len, int64_t n_planned);
// the diagnostics' share of a moments reset: the planes fitted to `len` entries and zeroed (NHP_ENOMEM: diagnostics off)
nhp_status nhp_diag_zero(nhp_ctx *ctx, nhp_diag_state **d, int64_t len);
// is the kept step about to be accumulated the last of its batch?
inline bool nhp_diag_boundary(const nhp_diag_state *d) { return (d->count + 1) % d->b == 0; }
// after the model's accumulate kernel: count the step and take the snapshots that fall on it
nhp_status nhp_diag_advance(nhp_ctx *ctx, nhp_diag_state *d, const nhp_diag_sums &s);
// _fetch of either model: per-entry values and the summary (nb: workgroups per group, at most 256; with_rho: ρ is group 5)
nhp_status nhp_diag_finalize(nhp_ctx *ctx, const nhp_diag_state *d, const nhp_diag_sums &s, const nhp_diag_groups &G, int nb,
                             bool with_rho, double ess_below, double rhat_above, double *summary, double *ess, double *mcse,
                             double *rhat, int64_t len);
