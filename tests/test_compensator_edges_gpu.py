"""nhp_cont_compensator held to an exact reference at its edges (csrc/cont_compensator.hip: k_comp_tables, k_comp_chunk_sums,
k_comp_group_scan, k_comp_super_scan, k_comp_lgcp_cum, k_comp_events, k_comp_residuals, k_comp_total).  The expected values
and the per-entry bound come from tests/compensator_exact_ref.py (long double, Φ from mpmath; the derivation is in its
docstring); tests/test_compensator_edges_host.py ties that restatement down and shows that the cases contain what they are
named for.  Every at_events, residuals and total entry is compared: |got - want| <= bound, a value without a term is 0.0.

    W-exp, W-logit, W-net   N=7 M=3000 T=200 Δtmax=1 on a dyadic grid: ties, events at Δ = Δtmax exactly, Δ = 2⁻⁴¹ and 1 - 2⁻⁴¹
    W-net-logit, G-W        under μ = -28 / +28 (the link's mass at the ends of its window), θΔtmax up to 2000, zero weights, A
                            with a zero row and column, an empty node, a one-event node, a grid baseline with events on grid
                            points and T on the last one
    L-exp, L-logit          N=2, the first 300 events, Δtmax=64 >= T: nothing saturates; L-exp-inf: Δtmax = ∞
    P-127 .. P-8193         N=3, Δtmax=1, 3 events per unit: M on both sides of a chunk (128) and of a group (128·64), window
                            starts on multiples of 128 and just before, empty windows, a first event at t = 0
    S-tiny                  200 events inside 2⁻¹⁰: Λ is a sum of terms θ·Δ <= 1e-3
    far T                   T = t_last + 2·Δtmax: no event inside the last window, total = base + counts·V

The device library's three functions, measured through nhp_probe_math ops 9, 10, 11 against mpmath (40 digits) on an MI355X,
in units of 2⁻⁵³ (half an ulp); the reference's allowances A_EXPM1 = 3, A_LOGIT = 2, A_ERFC = 8 are twice these, rounded up:
    -expm1(-x), x in [1e-300, 745]          1.481 (at x = 0.374), relative to the value
    log(x/(1-x)), x in [2⁻⁶⁰, 1 - 2⁻⁵³]      0.893 (at x = 5.8e-8), relative to |ℓ| + 2: the quotient's roundings are absolute in ℓ,
                                            so there is no relative accuracy where ℓ -> 0 (x near 1/2), and Φ needs none
    0.5·erfc(-z/√2), z in [-38, 9]          3.196 for z >= -√2, relative to the value.  In the lower tail the relative error grows
                                            like z²/2 (1650 units at z = -36.65, where z²/2 = 672), as an evaluation through
                                            e^{-x²} with a rounded x² = z²/2 must; the values there are below 1e-290 and the
                                            absolute error is nothing next to any Λ.  Documented, not fixed: relative to
                                            max(1, z²/2) the largest error is 3.933 (at z = -1.435), and the reference allows
                                            the term that much.  Below 2⁻¹⁰⁰⁰ (z < -37.1) the error is held absolutely (`tiny`).

Largest error/bound seen on an MI355X: 0.24 (W-net-logit at_events; the float64 host evaluation reaches the same 0.24 there).
Case by case, the largest of at_events / residuals / total: W-exp 0.13, W-logit 0.17, W-net 0.14, W-net-logit 0.24, G-W 0.068,
L-exp 0.18, L-logit 0.12, L-exp-inf 0.18, S-tiny 0.18, P-127 0.075, P-128 0.075, P-129 0.052, P-8191 0.082, P-8192 0.12,
P-8193 0.14; the far-T totals 0.015 to 0.11.  No kernel defect was found.
"""
import mpmath
import numpy as np
import pytest

import compensator_exact_ref as ce
import cont_grad_ref as gr

pytestmark = pytest.mark.gpu

KEYS = ("at_events", "residuals", "total")


def probe(nhp, op, x):
    from nhp_amd import _lib
    ctx = nhp.default_context()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(len(x), np.nan)
    _lib.check(_lib.lib().nhp_probe_math(ctx.h, op, _lib.dptr(x), None, len(x), _lib.dptr(out)), ctx.h)
    return out


def units(got, want, scale=None):
    """|got - want| in units of 2⁻⁵³·scale (scale: |want| by default), want as mpmath numbers."""
    return np.array([float(abs(mpmath.mpf(float(g)) - w) / (abs(w) if s is None else s)) for g, w, s in
                     zip(got, want, [None] * len(got) if scale is None else scale)]) / ce.EPS


def test_library_functions_within_their_allowances(nhp):
    mpmath.mp.dps = 40
    rng = np.random.default_rng(9)
    f = mpmath.mpf
    # -expm1(-x)
    x = np.concatenate([10.0 ** rng.uniform(-300, np.log10(745.0), 1500), 10.0 ** rng.uniform(-4, 1, 1500), [1e-300, 745.0]])
    x = np.concatenate([x, ce.case_of("W-exp")["theta"].ravel(), ce.case_of("S-tiny")["theta"].ravel() * 2.0 ** -12])
    got = probe(nhp, 9, x)
    u = units(got, [-mpmath.expm1(-f(float(v))) for v in x])
    print(f"-expm1(-x): largest error {u.max():.3f} units of 2^-53 at x = {x[u.argmax()]!r}")
    assert 2.0 * u.max() <= ce.A_EXPM1
    # log(x/(1-x))
    k = np.arange(1.0, 61.0)
    x = np.concatenate([2.0 ** -k, 1.0 - 2.0 ** -k[:53], rng.uniform(0.0, 1.0, 1500), 0.5 + rng.uniform(-1e-3, 1e-3, 300),
                        0.5 * (1.0 + np.tanh(rng.uniform(-20, 20, 700)))])
    x = x[(x >= 2.0 ** -60) & (x <= 1.0 - 2.0 ** -53)]
    got = probe(nhp, 10, x)
    want = [mpmath.log(f(float(v)) / (1 - f(float(v)))) for v in x]
    u = units(got, want, scale=[abs(w) + 2 for w in want])
    print(f"log(x/(1-x)): largest error {u.max():.3f} units of 2^-53·(|l| + 2) at x = {x[u.argmax()]!r}")
    assert 2.0 * u.max() <= ce.A_LOGIT
    # 0.5·erfc(-z/√2)
    z = np.concatenate([rng.uniform(-38.0, 9.0, 2500), np.linspace(-38.0, 9.0, 95), rng.uniform(-1.0, 1.0, 400)])
    got = probe(nhp, 11, z)
    want = [mpmath.ncdf(f(float(v))) for v in z]
    normal = np.array([w >= f(2) ** -1000 for w in want])
    u = units(got[normal], [w for w, n in zip(want, normal) if n])
    body = z[normal] >= -np.sqrt(2.0)
    print(f"0.5*erfc(-z/sqrt2): largest error {u[body].max():.3f} units of 2^-53 for z >= -sqrt2, {u.max():.1f} at z = "
          f"{z[normal][u.argmax()]!r} in the tail")
    u = u / ce.erfc_scale(z[normal])
    print(f"0.5*erfc(-z/sqrt2): largest error {u.max():.3f} units of 2^-53*max(1, z^2/2 for z < 0) at z = {z[normal][u.argmax()]!r}; "
          f"{int((~normal).sum())} values below 2^-1000")
    assert 2.0 * u.max() <= ce.A_ERFC
    assert (~normal).sum() > 0
    sub = np.array([float(abs(f(float(g)) - w)) for g, w, n in zip(got, want, normal) if not n])
    assert np.all(sub <= 2.0 ** -1000)                                   # no relative precision down there: `tiny` in the bound


def run(nhp, case, T=None):
    proc = gr.process_of(nhp, case)
    data = (case["times"].copy(), case["nodes"].copy(), case["T"] if T is None else T)
    return proc, data, nhp.compensator(proc, data)


def hold(label, got, parts):
    worst = 0.0
    for key, g, part in zip(KEYS, got, parts):
        g = np.asarray(g)
        ratio, bad, err, B = ce.check(g, part)
        print(f"{label} {key}: error/bound {ratio:.3g}, {int((B == 0).sum())} exact zeros")
        assert len(bad) == 0, f"{label} {key}: {len(bad)} entries outside the bound\n" + ce.explain(g, part, bad, err, B)
        worst = max(worst, ratio)
    return worst


def same_bits(a, b):
    for x, y in zip(a, b):
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        y = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.parametrize("name", ce.COMPENSATOR_CASES)
def test_every_entry_within_its_bound(nhp, name):
    import torch
    case, res = ce.prepared(name)
    proc, data, got = run(nhp, case)
    assert len(got.at_events) == len(got.residuals) == len(case["times"]) and len(got.total) == case["N"]
    assert all(np.all(np.isfinite(g)) for g in got)
    hold(name, got, (res.at_events, res.residuals, res.total))
    # residuals are the differences of at_events inside a node, bit for bit
    order = np.argsort(case["nodes"], kind="stable")
    first = np.concatenate([[True], np.diff(case["nodes"][order]) != 0])
    at = got.at_events[order]
    assert np.array_equal(got.residuals[order], np.where(first, at, at - np.roll(at, 1)))
    # the same bits from a second call, from the device-built dataset and from device tensors
    same_bits(got, nhp.compensator(proc, data))
    ctx = nhp.default_context()
    same_bits(got, nhp.compensator(proc, nhp.DeviceDataset(ctx, data, case["N"], case["dt_max"], build="device")))
    dev = torch.device("cuda", ctx.device)
    out = nhp.compensator(proc, (torch.as_tensor(data[0]).to(dev), torch.as_tensor(data[1]).to(dev), data[2]), device=True)
    assert all(o.is_cuda and o.dtype == torch.float64 for o in out)
    same_bits(got, out)


@pytest.mark.parametrize("name", ce.FAR)
def test_no_event_inside_the_last_window(nhp, name):
    case, res = ce.prepared(name)
    T2 = ce.far_T(case)
    _, _, got = run(nhp, case, T=T2)
    hold(f"{name} T = {T2}", got, (res.at_events, res.residuals, ce.prepared_far(name)))
    _, _, near = run(nhp, case)
    same_bits((got.at_events, got.residuals), (near.at_events, near.residuals))      # neither depends on T
