"""The recursive route's truncated window (csrc/cont_recursive.hip: k_rec_stats, rec_cut_for, k_rec_windows, nhp_recursive_window;
csrc/cont_data.hip: nhp_dataset_slab_stats) held to tests/rec_window_ref.py, case by case.  The route is read through
nhp_probe_recursive_window at recursion_cost 1.0 (log-likelihood), 1.2 (gradient) and 1e9 (observed information) BEFORE anything
is compared: a case that takes the other route fails, it does not pass as a second test of the recursion.
tests/test_rec_window_host.py shows without a GPU that every case contains what it is named for, that the reference's own cut
keeps the dropped tail below 2⁻⁶⁰·λ0_c for every child, and that the cost model leaves a factor of three on either side.

    uniform-1, -3, -64      the base: uniform times, three events at t = 0, ties, a busy column (N = 1: M = 1500)
    spread                  N = 3, θ from 2 to 400: min θ where W = 0 and A = 0, max W·θ at flat index N² - 1 under A = 0, min λ0 at the
                            last node -- the bound is governed by entries that contribute nothing
    second_trip             N = 130: N² = 16 900 > 64·256; min θ at flat 16 899, max W·θ at flat 16 384 (k_rec_stats' second trip)
    grid                    N = 130, G = 127: 16 510 grid intensities, the least one the last; events on grid points and at t = T
    burst                   400 events inside 0.01, children 0.5 .. 2 cuts behind it: one keeps the burst, one splits it, one drops
                            it; the slab count (406 against M = 2307) is what bounds the tail; one event at exactly fl(t_i - cut)
                            of a child (the window's edge is open)
    net                     N = 64, half of A zero, a zero row and a zero column; the integral is not masked (D7)
    early                   five events at t = 0 (children with idx < n_zero) and the first events behind them
    silent                  all W = 0: cut = 1e-300, every window empty, ll = the baseline's closed form.  The window at cost 1.0 only:
                            ∂/∂W[p,c] = -cnt[p] + Σ g_i·θ·e^{-θΔ} keeps its pair sums at W = 0, so the gradient takes the recursion
                            and the information refuses.  (This case found that they did not: the gradient's W entries came
                            back as -cnt[p], error/bound 1e13; nhp_recursive_window now tells its callers apart.)
    tiny                    M = 1, 2 at N = 1, 3: the recursion at cost 1.0 and 1.2, the window at 1e9
    no_bound                λ0 = 0 on a node without events; θ = 0 under W = 0: no bound, the recursion, finite values
    nan                     one θ = NaN: the probe only (cut = 0, not used); nothing is evaluated
    slow                    θ near 0.01: more than 8192 parents per window, the recursion; the observed information refuses
    shards                  uniform-3 and uniform-64 as columns [0,2) + [2,N) and the single column [1,2)

For a window case: the device's cut equals the reference's within 2⁻⁴⁸ relative (both sides evaluate one log, one division and a
few exp of the same doubles, the min/max reductions are exact: 32 ulp for libm); the exported child_cut starts equal
window_starts(times, the DEVICE's cut, n_zero) exactly and cut_pairs their sum; what those starts drop is at most 2⁻⁶⁰·λ0_c for
every child; the default log-likelihood is within 1e-12 of the FULL-history reference; every gradient entry is inside
cont_grad_ref's bound with the window's tail, entries without a pair equal their constant; the same two hold with
LL_FULL_RECURSION at the suite's 1e-11; default and forced agree at 1e-12; a repeated evaluation returns the same bits.

Caches (rec_version / rec_ds on the model, cut_cached on the dataset), each against the reference at the parameters in
force, downloaded: set_params fast -> θ/100 -> back; three steps of the device mle!; two steps of em!; one Gibbs step; one
model on two datasets of equal M and span (A, B, A); two models alternating on one dataset, synchronously and as a streak of
enqueues interleaved with windowed ones, a windowed and a recursive one into the same slot; NHP_REC_WINDOW=0 set and unset
in mid-process.

The shards' own log-likelihoods are held to 1e-12 of the WHOLE's value: a shard's value is a part of the whole's sum and
carries a part of its error (uniform-3's columns [0,2) sum to -31.9 out of terms of size 10³).

Seen on an MI355X (case by case in DESIGN.md 3.2): the cut is bit-identical to the reference's in every case; the dropped tail
is at most 0.46 of 2⁻⁶⁰·λ0_c (uniform-1); the window's ll error is at most 5.4e-13 (uniform-1; 9.1e-13 of the whole's value for a
shard of uniform-3) where the recursion's is 1e-16 on the same data -- the windowed kernel's 8-byte event records carry 2⁻⁴⁹ of the
span; gradient error/bound at most 0.081 through the window (second_trip) and 0.35 through the recursion (second_trip).
The enqueued values equal the synchronous ones to the bit, and so does every repeated evaluation.
    case          cut     tail/(2⁻⁶⁰·λ0_c)   ll rel. error window (recursion)   gradient error/bound window (recursion)
    uniform-1     1.30    0.46                5.4e-13 (1.1e-16)                   0.001 (0.009)
    uniform-3     2.27    0.036               2.3e-13 (3.7e-16)                   0.002 (0.009)
    uniform-64    2.20    0.027               6.3e-15 (1.8e-16)                   0.035 (0.15)
    spread        26.8    6e-150              0 (0)                               0.003 (0.014)
    second_trip   9.63    2e-16               2.4e-15 (1.8e-16)                   0.081 (0.35)
    grid          2.36    0.001               1.7e-16 (0)                         0.076 (0.32)
    burst         2.44    0.17                2.3e-13 (3.2e-16)                   0.008 (0.005)
    net           2.19    0.027               3.4e-16 (1.7e-16)                   0.037 (0.051)
    early         2.32    0.023               5.1e-13 (1.2e-15)                   0.009 (0.004)
    silent        1e-300  0                   1.6e-16 (1.6e-16)                   the recursion only: 0.055
    tiny          1.3-2.2 0                   at most 1.5e-16                     at most 0.031
    shards        as the whole                at most 9.1e-13 of the whole's ll   at most 0.035 (0.15)
    caches        set_params 0.24 <-> 22.5, mle! 0.24, em! 1.19, Gibbs 87.5: tail at most 0.058, ll at most 8.5e-13

Mistakes planted in scratch builds (one line each, one build and one run of this file each) and the tests that went red:
    cut halved                            everything with a cut: 24 of the 27 tests (not no_bound, nan)
    count fixed at 1                      all window cases but silent, tiny with two events, slow, shards, every cache case
    lmin over the first node's λ0 only    uniform-3 uniform-64 spread second_trip grid burst net tiny-3-* no_bound-lam slow shards
                                          mle em gibbs two-datasets
    k_rec_stats without its second trip   second_trip grid
    lo = 0 instead of n_zero              uniform-* spread second_trip grid net early silent shards set_params mle em gibbs two-models
                                          switch (every case with events at t = 0 inside a window)
    times[mid] >= lim                     silent (lim = t_i: the ties) burst two-datasets (the event at exactly fl(t_i - cut))
    rec_version check dropped             set_params mle em gibbs
    rec_ds check dropped                  two-datasets
    cut_cached never renewed              set_params mle em gibbs two-models
    mask_integral = 1 on the window       spread net (the log-likelihood's launch; the gradient's k_grad_init likewise)
With NHP_REC_WINDOW=0 in the environment every window case goes red at its route assertion.
"""
import ctypes as C

import numpy as np
import pytest

import cont_grad_ref as cr
import rec_window_ref as rw

pytestmark = pytest.mark.gpu

REL_WINDOW, REL_FULL, REL_CUT = 1e-12, 1e-11, 2.0 ** -48
FULL = 3                                                                  # LL_RECURSIVE | LL_FULL_RECURSION


class Device:
    """A case on the device: dataset, model and the C calls the tests make on them."""

    def __init__(self, nhp, case, columns=None, proc=None):
        from nhp_amd import _lib, continuous
        self.lib, self._lib, self.case = _lib.lib(), _lib, case
        self.ctx = nhp.default_context()
        self.proc = proc or cr.process_of(nhp, case)
        self.ds = continuous.DeviceDataset(self.ctx, (case["times"], case["nodes"], case["T"]), case["N"], case["dt_max"], columns=columns)
        self.model = self.proc.device_model(self.ctx)
        N, G = case["N"], 0 if case["grid_x"] is None else len(case["grid_x"])
        self.P = (N * G if G else N) + 2 * N * N

    def probe(self, cost, model=None, ds=None):
        out = np.full(4, np.nan)
        self._lib.check(self.lib.nhp_probe_recursive_window(self.ctx.h, (ds or self.ds).h, (model or self.model).h, cost, self._lib.dptr(out)),
                        self.ctx.h)
        return out

    def routes(self, **kw):
        return [self.probe(c, **kw) for c in rw.COSTS]

    def loglik(self, flags=1, model=None, ds=None):
        ll = C.c_double(np.nan)
        self._lib.check(self.lib.nhp_cont_loglik(self.ctx.h, (ds or self.ds).h, (model or self.model).h, flags, C.byref(ll)), self.ctx.h)
        return ll.value

    def gradient(self, flags=1):
        g, ll = np.full(self.P, np.nan), C.c_double(np.nan)
        self._lib.check(self.lib.nhp_cont_loglik_grad(self.ctx.h, self.ds.h, self.model.h, flags, C.byref(ll), self._lib.dptr(g), self.P),
                        self.ctx.h)
        return ll.value, g

    def params(self):
        x = np.full(self.P, np.nan)
        self._lib.check(self.lib.nhp_cont_model_get_params(self.ctx.h, self.model.h, self._lib.dptr(x), self.P), self.ctx.h)
        return x


def vector(case):
    """params(process) of a standard process with a homogeneous baseline: [λ0; θ; W], matrices p fastest."""
    return np.concatenate([case["lam0"], case["theta"].ravel(order="F"), case["W"].ravel(order="F")])


def case_at(case, x):
    """The case with the parameters of the vector x."""
    N = case["N"]
    out = dict(case)
    out.update(lam0=x[:N].copy(), theta=x[N:N + N * N].reshape((N, N), order="F").copy(),
               W=x[N + N * N:].reshape((N, N), order="F").copy())
    return out


def rel(a, b):
    return abs(a - b) / abs(b)


def hold_cut(label, dev, want_cut, expect, **kw):
    """The route at the three costs, then the cut against the reference's.  Returns the device's cut."""
    outs = dev.routes(**kw)
    assert [int(o[1]) for o in outs] == list(expect), (label, "route", [o.tolist() for o in outs], expect)
    got = outs[0][0]
    assert all(o[0] == got for o in outs), (label, outs)
    if want_cut in (0.0, 1e-300):
        assert got == want_cut, (label, got, want_cut)
    else:
        print(f"{label}: cut {got!r}, reference {want_cut!r}, relative difference {rel(got, want_cut):.3g}")
        assert rel(got, want_cut) <= REL_CUT, (label, got, want_cut)
    for o, used in zip(outs, expect):
        assert (o[2] in (1, 2, 4, 8, 16, 32)) if used else o[2] == 0, (label, o)           # nhp_pick_group's widths
    return got, outs


def hold_starts(label, dev, case, cut_dev, pairs, ds=None):
    """child_cut is child with first = window_starts(times, the device's cut, n_zero), cut_pairs the windows' sum, and what
    the windows drop stays below 2⁻⁶⁰·λ0_c for every child.  Returns the largest dropped tail over its bound."""
    ds = ds or dev.ds
    t = case["times"]
    child, child_cut = ds.array("child"), ds.array("child_cut")
    assert len(child_cut) == len(child) == len(t)
    assert np.array_equal(child_cut["t"], child["t"]) and np.array_equal(child_cut["idx"], child["idx"])
    assert np.array_equal(np.sort(child["idx"]), np.arange(len(t)))
    n_zero = ds.scalars()["n_zero_time"]
    assert n_zero == int((t == 0.0).sum())
    want = rw.window_starts(t, cut_dev, n_zero)
    bad = np.nonzero(child_cut["first"] != want[child_cut["idx"]])[0]
    assert len(bad) == 0, (label, len(bad), child_cut[bad[:5]], want[child_cut["idx"][bad[:5]]])
    assert int((child_cut["idx"].astype(np.int64) - child_cut["first"]).sum()) == int(pairs), (label, pairs)
    starts = np.empty(len(t), dtype=np.int64)
    starts[child_cut["idx"]] = child_cut["first"]
    tail, floor = rw.dropped_tail(cr.model_of(case), t, case["nodes"], starts)
    assert np.all(tail <= floor), (label, "dropped tail above 2^-60 λ0_c")
    worst = float((tail / floor).max()) if len(t) else 0.0
    print(f"{label}: {int(pairs)} pairs in the windows, largest dropped tail / (2^-60 λ0_c) {worst:.3g}")
    return worst


def hold_values(label, dev, case, res, expect, scale=None):
    """The default and the forced evaluation against the full-history reference; returns the gradient of the default one.
    scale: what the log-likelihood's tolerances are relative to (a column shard's value is a part of the whole's sum, with
    a part of its rounding: its tolerance is the whole's); default: the reference value itself."""
    m = cr.model_of(case)
    want = float(res.ll)
    scale = abs(want) if scale is None else scale
    rel = lambda a, b: abs(a - b) / scale
    ll = dev.loglik(1)
    tol = REL_WINDOW if expect[0] else REL_FULL
    print(f"{label}: ll {ll!r}, reference {want!r}, relative error {rel(ll, want):.3g}")
    assert rel(ll, want) <= tol, (label, ll, want)
    assert dev.loglik(1) == ll, (label, "a repeated evaluation differs")
    tail = cr.window_tail(res, m, case["times"], case["nodes"], case["T"]) if expect[1] else None
    gll, g = dev.gradient(1)
    assert rel(gll, want) <= (REL_WINDOW if expect[1] else REL_FULL), (label, gll, want)
    ratio, bad, err, B = cr.check(g, res, 0.0, tail)
    print(f"{label}: gradient error/bound {ratio:.3g}, {int((B == 0).sum())} entries equal to their constant")
    assert len(bad) == 0, f"{label}: {len(bad)} gradient entries outside the bound\n" + cr.explain(g, res, case["N"], bad, err, B)
    full = dev.loglik(FULL)
    print(f"{label}: forced recursion, ll relative error {rel(full, want):.3g}, default against forced {rel(ll, full):.3g}")
    assert rel(full, want) <= REL_FULL, (label, full, want)
    assert rel(ll, full) <= REL_WINDOW, (label, ll, full)
    fll, fg = dev.gradient(FULL)
    assert rel(fll, want) <= REL_FULL
    fratio, bad, err, B = cr.check(fg, res)
    print(f"{label}: forced recursion, gradient error/bound {fratio:.3g}")
    assert len(bad) == 0, f"{label} (forced): {len(bad)} gradient entries outside the bound\n" + cr.explain(fg, res, case["N"], bad, err, B)
    return g


def hold_case(nhp, name, columns=None, scale=None):
    case, res = rw.prepared(name, columns)
    expect = rw.EXPECT[name]
    dev = Device(nhp, case, columns)
    label = name if columns is None else f"{name} {columns}"
    assert len(dev.ds.array("child_cut")) == 0                          # nothing before the first use of the window
    cut_dev, outs = hold_cut(label, dev, rw.cut_of(name), expect)
    if any(expect):
        hold_starts(label, dev, case, cut_dev, outs[-1][3])
    g = hold_values(label, dev, case, res, expect, scale)
    return dev, case, res, g


@pytest.mark.parametrize("name", rw.WINDOW[:10])
def test_window_cases(nhp, name):
    dev, case, res, _ = hold_case(nhp, name)
    if name == "silent":
        t, n0 = case["times"], case["nodes"] - 1
        closed = float(np.sum(np.log(case["lam0"].astype(np.longdouble)[n0])) - np.longdouble(case["T"]) * case["lam0"].astype(np.longdouble).sum())
        assert dev.probe(1.0)[3] == 0 and np.array_equal(dev.ds.array("child_cut")["first"], dev.ds.array("child_cut")["idx"])
        assert rel(dev.loglik(1), closed) <= 1e-14
        # the empty window is the log-likelihood's alone: ∂/∂W[p,c] = -cnt[p] + Σ g_i θ e^{-θΔ} keeps its pair sums at W = 0 (the
        # gradient above went through the recursion and is inside its bound), and the information refuses
        N = case["N"]
        D = 1 + 2 * N
        out, val = np.full(N * D * D, np.nan), C.c_double(np.nan)
        rc = dev.lib.nhp_cont_information(dev.ctx.h, dev.ds.h, dev.model.h, 1, None, 0, 0, 0, C.byref(val), out.ctypes.data)
        assert rc == dev._lib.ENOTIMPL and np.all(np.isnan(out)) and np.isnan(val.value)


@pytest.mark.parametrize("name", rw.TINY)
def test_one_and_two_events(nhp, name):
    hold_case(nhp, name)


@pytest.mark.parametrize("name", ["no_bound-lam", "no_bound-theta"])
def test_without_a_bound_the_recursion_runs(nhp, name):
    dev, case, res, g = hold_case(nhp, name)
    assert np.isfinite(dev.loglik(1)) and np.all(np.isfinite(g))
    assert len(dev.ds.array("child_cut")) == 0


def test_a_nan_rate_gives_no_bound(nhp):
    """The probe only: k_rec_stats reads the tables, nothing is evaluated on NaN parameters."""
    case = rw.case_of("nan")
    dev = Device(nhp, case)
    hold_cut("nan", dev, 0.0, (0, 0, 0))
    assert len(dev.ds.array("child_cut")) == 0


def test_a_slow_decay_keeps_the_recursion_and_the_information_refuses(nhp):
    case, res = rw.prepared("slow")
    dev = Device(nhp, case)
    cut_dev, _ = hold_cut("slow", dev, rw.cut_of("slow"), (0, 0, 0))
    assert cut_dev * len(case["times"]) / case["times"][-1] > 8192.0
    ll = dev.loglik(1)
    assert rel(ll, float(res.ll)) <= REL_FULL and len(dev.ds.array("child_cut")) == 0
    N = case["N"]
    D = 1 + 2 * N
    out, val = np.full(N * D * D, np.nan), C.c_double(np.nan)
    rc = dev.lib.nhp_cont_information(dev.ctx.h, dev.ds.h, dev.model.h, 1, None, 0, 0, 0, C.byref(val), out.ctypes.data)
    msg = dev.lib.nhp_last_error(dev.ctx.h).decode()
    assert rc == dev._lib.ENOTIMPL and "no usable truncated window" in msg and "8192" in msg, (rc, msg)
    assert np.all(np.isnan(out)) and np.isnan(val.value)


@pytest.mark.parametrize("name", ["uniform-3", "uniform-64"])
def test_column_shards(nhp, name):
    case, whole = rw.prepared(name)
    N = case["N"]
    col = np.concatenate([np.arange(N), np.tile(np.repeat(np.arange(N), N), 2)])
    total_ll, total = 0.0, np.zeros(len(whole.grad))
    for cols in ((0, 2), (2, N), (1, 2)):
        dev, _, res, g = hold_case(nhp, name, cols, scale=abs(float(whole.ll)))
        foreign = (col < cols[0]) | (col >= cols[1])
        assert np.all(g[foreign] == 0.0) and not np.any(np.signbit(g[foreign])), f"{name} {cols}: foreign entries must be exactly 0.0"
        if cols != (1, 2):
            total_ll += dev.loglik(1)
            total += g
    assert rel(total_ll, float(whole.ll)) <= REL_WINDOW
    tail = cr.window_tail(whole, cr.model_of(case), case["times"], case["nodes"], case["T"])
    ratio, bad, err, B = cr.check(total, whole, 0.0, tail)
    assert len(bad) == 0, cr.explain(total, whole, N, bad, err, B)


# --------------------------------------------------------------------------------------------------------------- caches
def hold_in_force(label, dev, case, model=None, ds=None, name=None, used=None):
    """The route (where the caller names it), the cut, the starts and the default log-likelihood against the reference at the
    parameters `case` holds (name: a prepared case with the same parameters, so its reference is shared)."""
    m = cr.model_of(case)
    t = case["times"]
    want_cut = rw.cut_of(name) if name else rw.cut(m, t)
    out = dev.probe(1.0, model=model, ds=ds)
    assert used is None or out[1] == used, (label, "route", out.tolist())
    assert (want_cut == 0.0 and out[0] == 0.0) or rel(out[0], want_cut) <= REL_CUT, (label, out[0], want_cut)
    if out[1]:
        hold_starts(label, dev, case, out[0], out[3], ds=ds)
    res = rw.prepared(name)[1] if name else cr.evaluate(m, t, case["nodes"], case["T"], recursive=True)
    ll = dev.loglik(1, model=model, ds=ds)
    print(f"{label}: used {int(out[1])}, cut {out[0]:.6g}, ll relative error {rel(ll, float(res.ll)):.3g}")
    assert rel(ll, float(res.ll)) <= (REL_WINDOW if out[1] else REL_FULL), (label, ll, float(res.ll))
    return out, ll


def test_set_params_renews_the_bound(nhp):
    fast, slow = rw.case_of("cache-fast"), rw.case_of("cache-slow")
    dev = Device(nhp, fast)
    for step, (name, case) in enumerate((("cache-fast", fast), ("cache-slow", slow), ("cache-fast", fast), ("cache-slow", slow))):
        dev.model.set_params(vector(case))
        assert np.array_equal(dev.params(), vector(case))
        hold_in_force(f"set_params {step} {name}", dev, case, name=name, used=1)


def fitted(nhp, run):
    """Fill the caches at the fast start, let `run(dev, x)` change the parameters on the device, hold what is in force."""
    fast = rw.case_of("cache-fast")
    dev = Device(nhp, fast)
    out, _ = hold_in_force("start", dev, fast, name="cache-fast", used=1)
    x = vector(fast)
    run(dev, x)
    now = dev.params()
    assert np.all(np.isfinite(now)) and not np.array_equal(now, vector(fast))
    after = case_at(fast, now)
    new_cut = rw.cut(cr.model_of(after), fast["times"])
    print(f"cut {out[0]:.6g} -> {new_cut:.6g}")
    assert abs(new_cut - out[0]) > 2.0 ** -40 * out[0]                  # a stale cut would miss the 2⁻⁴⁸
    hold_in_force("after", dev, after)
    return dev, x, now


def test_device_mle_steps_renew_the_bound(nhp):
    def run(dev, x):
        loss, steps, conv, evals = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        dev._lib.check(dev.lib.nhp_cont_mle_run(dev.ctx.h, None, dev.ds.h, dev.model.h, 1, 1e-6, 1e3, 1e-300, 3, dev._lib.dptr(x), len(x),
                                                C.byref(loss), C.byref(steps), C.byref(conv), C.byref(evals)), dev.ctx.h)
        assert 1 <= steps.value <= 3
        run.loss = loss.value
    dev, x, now = fitted(nhp, run)
    assert np.array_equal(x, now)                                       # the committed parameters are the iterate returned
    assert rel(dev.loglik(1), -run.loss) <= REL_FULL


def test_em_steps_renew_the_bound(nhp):
    def run(dev, x):
        loss, steps, conv = C.c_double(), C.c_int32(), C.c_int32()
        dev._lib.check(dev.lib.nhp_cont_em_run(dev.ctx.h, dev.ds.h, dev.model.h, 1, None, 1e-6, 1e3, 1e-300, 2, dev._lib.dptr(x), len(x),
                                               C.byref(loss), C.byref(steps), C.byref(conv), None), dev.ctx.h)
        assert steps.value == 2
        run.loss = loss.value
    dev, x, now = fitted(nhp, run)
    assert np.array_equal(x, now)
    assert rel(dev.loglik(1), -run.loss) <= REL_FULL


def test_a_gibbs_step_renews_the_bound(nhp):
    def run(dev, x):
        pri = dev._lib.GibbsPriors(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0)
        dev._lib.check(dev.lib.nhp_cont_gibbs_step(dev.ctx.h, dev.ds.h, dev.model.h, C.byref(pri), 11, 0), dev.ctx.h)
    fitted(nhp, run)


def test_one_model_on_two_datasets(nhp):
    """Equal M and span, one of them with the burst: the cuts differ, the bound is keyed on the dataset."""
    from nhp_amd import continuous
    a, b = rw.case_of("no_burst"), rw.case_of("burst")
    dev = Device(nhp, a)
    ds_b = continuous.DeviceDataset(dev.ctx, (b["times"], b["nodes"], b["T"]), b["N"], b["dt_max"])
    assert np.array_equal(vector(a), vector(b)) and len(a["times"]) == len(b["times"])
    seen = []
    for step, (name, case, ds) in enumerate((("no_burst", a, dev.ds), ("burst", b, ds_b), ("no_burst", a, dev.ds), ("burst", b, ds_b))):
        out, ll = hold_in_force(f"datasets {step} {name}", dev, case, ds=ds, name=name, used=1)
        seen.append((out[0], ll))
    assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0][0] != seen[1][0]


def test_two_models_alternate_on_one_dataset(nhp):
    fast, slow = rw.case_of("cache-fast"), rw.case_of("cache-slow")
    dev = Device(nhp, fast)
    other = cr.process_of(nhp, slow).device_model(dev.ctx)
    models = {"cache-fast": (dev.model, fast), "cache-slow": (other, slow)}
    sync = {}
    for step, name in enumerate(("cache-fast", "cache-slow", "cache-fast", "cache-slow")):
        model, case = models[name]
        out, ll = hold_in_force(f"models {step} {name}", dev, case, model=model, name=name, used=1)
        assert sync.setdefault(name, ll) == ll
    assert rel(rw.cut_of("cache-slow"), rw.cut_of("cache-fast")) > 10.0
    F, S = dev.model, other
    windowed = {id(F): dev.loglik(0, model=F), id(S): dev.loglik(0, model=S)}
    recursive = {id(F): sync["cache-fast"], id(S): sync["cache-slow"]}
    assert rel(windowed[id(S)], recursive[id(S)]) > 1e-6                 # Δtmax = 0.05 cuts the slow model's sum: the two differ

    def enqueue(model, flags, slot):
        dev._lib.check(dev.lib.nhp_cont_loglik_enqueue(dev.ctx.h, dev.ds.h, model.h, flags, slot), dev.ctx.h)

    plan = [(F, 1, 0), (F, 0, 6), (S, 1, 1), (S, 0, 7), (F, 1, 2), (F, 0, 8), (S, 1, 3), (F, 1, 4), (S, 1, 5),
            (F, 0, 9), (S, 1, 9)]                                        # the last two share a slot: it holds the recursive value
    for model, flags, slot in plan:
        enqueue(model, flags, slot)
    got = dev.ctx.fetch(0, 10)
    want = np.full(10, np.nan)
    for model, flags, slot in plan:
        want[slot] = (recursive if flags else windowed)[id(model)]
    assert np.array_equal(got, want), (got - want)
    # and the other order in the shared slot
    enqueue(S, 1, 3)
    enqueue(F, 0, 3)
    assert dev.ctx.fetch(3, 1)[0] == windowed[id(F)]


def test_the_switch_is_read_on_every_call(nhp, monkeypatch):
    case = rw.case_of("cache-fast")
    dev = Device(nhp, case)
    monkeypatch.delenv("NHP_REC_WINDOW", raising=False)
    ll = dev.loglik(1)
    assert [int(o[1]) for o in dev.routes()] == [1, 1, 1]
    monkeypatch.setenv("NHP_REC_WINDOW", "0")
    assert [int(o[1]) for o in dev.routes()] == [0, 0, 0]
    forced = dev.loglik(1)
    assert forced == dev.loglik(FULL) and rel(forced, ll) <= REL_WINDOW
    monkeypatch.delenv("NHP_REC_WINDOW")
    assert [int(o[1]) for o in dev.routes()] == [1, 1, 1]
    assert dev.loglik(1) == ll
