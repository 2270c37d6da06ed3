"""tests/compensator_exact_ref.py tied down on the CPU before the GPU suites rely on it: the float64 evaluation of the same sums
in three orders stays well inside the bound, the older restatement (tests/compensator_ref.py) agrees with the extended values,
each of the four planted mistakes leaves the bound on the case named for it, the cases contain what they are named for, and
intensity_at agrees with the oracle.

Largest error/bound of the float64 evaluations (the largest of at_events / residuals / total over the three orders):
W-exp 0.13, W-logit 0.17, W-net 0.18, W-net-logit 0.24, G-W 0.13, L-exp 0.19, L-logit 0.14, L-exp-inf 0.19, S-tiny 0.22,
P-127 0.11, P-128 0.098, P-129 0.11, P-8191 0.082, P-8192 0.12, P-8193 0.14; the time-part cases of
tests/test_time_parts_gpu.py: P4-exp 0.21, P4-logit 0.16, P2-inf 0.20.  The mutants reach 1e10 to 1e14 on their cases
(a whole link mass or a run of them against a few 2⁻⁵³), 1 - exp(-x) 6.3e3 on S-tiny."""
import numpy as np
import pytest

import compensator_exact_ref as ce
import compensator_ref as cr
import cont_grad_ref as gr

KEYS = ("at_events", "residuals", "total")


def ratios(got, res):
    """error/bound of (at_events, residuals, total), asserting that no entry is outside."""
    out = []
    for key, g in zip(KEYS, got):
        part = getattr(res, key)
        g = np.asarray(g, dtype=np.float64)
        ratio, bad, err, B = ce.check(g, part)
        out.append((ratio, len(bad), ce.explain(g, part, bad, err, B)))
    return out


def f64(case, **kw):
    r = ce.evaluate(gr.model_of(case), case["times"], case["nodes"], case["T"], real=np.float64, **kw)
    return [np.asarray(getattr(r, k).value, dtype=np.float64) for k in KEYS]


@pytest.mark.parametrize("name", ce.COMPENSATOR_CASES + ce.TIME_PART_CASES)
def test_float64_sums_in_three_orders_within_the_bound(name):
    case, res = ce.prepared(name)
    for order in ("forward", "reverse", "shuffled"):
        rs = ratios(f64(case, order=order), res)
        print(f"{name} {order}: float64 error/bound " + " ".join(f"{k} {r[0]:.3g}" for k, r in zip(KEYS, rs)))
        for key, (ratio, nbad, text) in zip(KEYS, rs):
            assert nbad == 0, f"{name} {order} {key}\n{text}"
            assert ratio < 0.5, "float64 alone comes near the bound: look for a missing rounding, not a scale factor"
    for key in KEYS:
        part = getattr(res, key)
        assert np.all(np.isfinite(np.asarray(part.value, dtype=np.float64))) and np.all(part.S >= 0)
        zero = part.S == 0
        assert np.all(part.bound[zero] == 0) and np.all(np.asarray(part.value, dtype=np.float64)[zero] == 0.0)
        assert np.all(part.bound[~zero] > 0)


@pytest.mark.parametrize("name", [n for n in ce.FAR] + ["L-exp-inf"])
def test_total_with_no_event_inside_the_last_window(name):
    case = ce.case_of(name)
    if name == "L-exp-inf":                                               # Δtmax = ∞: every event stays inside, none saturates
        _, res = ce.prepared(name)
        assert np.all(res.ws == 0) and np.all(res.total.d <= np.ceil(300 / 256) + 11)
        return
    T2, part = ce.far_T(case), ce.prepared_far(name)
    t = case["times"]
    assert not np.any(t > T2 - case["dt_max"])
    # every event has saturated: base + counts·V, which float64 gives inside the bound
    r = ce.evaluate(gr.model_of(case), t, case["nodes"], T2, real=np.float64, parts=("total",))
    ratio, bad, err, B = ce.check(np.asarray(r.total.value, dtype=np.float64), part)
    print(f"{name} T = {T2}: float64 total error/bound {ratio:.3g}")
    assert len(bad) == 0 and ratio < 0.5
    m = cr.Model(case["lam0"], case["W"], case["dt_max"], theta=case["theta"] if case["kind"] == "exponential" else None,
                 mu=None if case["kind"] == "exponential" else case["mu"], tau=None if case["kind"] == "exponential" else case["tau"],
                 A=case["A"])
    want = case["lam0"] * T2 + np.bincount(case["nodes"] - 1, minlength=case["N"]) @ m.V()
    assert np.allclose(np.asarray(part.value, dtype=np.float64), want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["W-exp", "W-logit", "W-net-logit", "G-W", "L-exp", "L-logit", "L-exp-inf", "S-tiny", "P-129"])
def test_older_restatement_agrees(name):
    """compensator_ref.compensator (float64, one fsum per value, scipy's ndtr) inside the bound; ndtr is given 4 ulp on top of
    the logit-normal terms (8 units of 2⁻⁵³ relative to S)."""
    case, res = ce.prepared(name)
    expo = case["kind"] == "exponential"
    m = cr.Model(case["lam0"], case["W"], case["dt_max"], theta=case["theta"] if expo else None, mu=None if expo else case["mu"],
                 tau=None if expo else case["tau"], A=case["A"], grid_x=case["grid_x"])
    got = cr.compensator(m, case["times"], case["nodes"], case["T"])
    for key, g in zip(KEYS, got):
        part = getattr(res, key)
        ratio, bad, err, B = ce.check(g, part, extra=0.0 if expo else 8.0)
        print(f"{name} {key}: compensator_ref error/bound {ratio:.3g}")
        assert len(bad) == 0, f"{name} {key}\n" + ce.explain(g, part, bad, err, B)


MUTANT_CASES = {"le_dtmax": ("W-logit", "W-exp", "P-8192"), "ge_window": ("W-logit", "W-net", "P-128"),
                "no_group_prefix": ("P-129", "P-8193", "W-exp"), "one_minus_exp": ("S-tiny",)}


@pytest.mark.parametrize("mutant", ce.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    for name in MUTANT_CASES[mutant]:
        case, res = ce.prepared(name)
        got = f64(case, mutate=mutant)
        worst = {}
        for key, g in zip(KEYS, got):
            ratio, bad, _, _ = ce.check(g, getattr(res, key))
            worst[key] = (ratio, len(bad))
        print(f"{mutant} on {name}: error/bound " + " ".join(f"{k} {v[0]:.3g} ({v[1]} entries out)" for k, v in worst.items()))
        assert worst["at_events"][0] > 1.0 and worst["at_events"][1] > 0, (mutant, name)
        assert worst["residuals"][0] > 1.0
        if mutant == "no_group_prefix":
            assert worst["total"][0] > 1.0
    # and the mutants are silent where their edge does not occur, so the cases above are what catches them
    case, res = ce.prepared("L-exp-inf")
    if mutant != "one_minus_exp":
        for key, g, h in zip(KEYS, f64(case, mutate=mutant), f64(case)):
            assert np.array_equal(g, h)


@pytest.mark.parametrize("name", ce.COMPENSATOR_CASES)
def test_cases_contain_what_they_are_named_for(name):
    case, res = ce.prepared(name)
    t, n0, M, dt_max = case["times"], case["nodes"] - 1, len(case["times"]), case["dt_max"]
    ws, k = res.ws, np.arange(M)
    assert np.array_equal(ws, np.minimum(np.searchsorted(t, t - dt_max, side="right"), k))
    cnt = np.bincount(n0, minlength=case["N"])
    with np.errstate(invalid="ignore"):
        exact = np.isin(t - dt_max, t) & ((t - dt_max) + dt_max == t)       # a Δ of exactly Δtmax ends at this event
    ties = int((np.diff(t) == 0).sum())
    print(f"{name}: M {M} ties {ties} edge {int(exact.sum())} empty windows {int(((ws == k) & (k > 0)).sum())} "
          f"ws%128==0 {int(((ws % 128 == 0) & (ws > 0)).sum())} ws%128==127 {int((ws % 128 == 127).sum())}")
    if name.startswith(("W", "G")):
        assert ties >= 15 and exact.sum() >= 12 and (cnt == 0).sum() == 1 and (cnt == 1).sum() == 1
    if name.startswith("W") and "logit" in name:
        d = t[1:] - t[:-1]
        assert (d == 2.0 ** -41).sum() >= 3 and np.isin(t + (1.0 - 2.0 ** -41), t).sum() >= 3
        assert case["mu"][0, 1] == -28.0 and case["mu"][2, 3] == 28.0
    if name == "G-W":
        assert case["T"] == case["grid_x"][-1] and np.isin(case["grid_x"][1:], t).all()
    if name.startswith("L"):
        assert M == 300 and int((k - ws).sum()) == 44850 and dt_max >= case["T"]
    if name.startswith("P"):
        assert M == int(name[2:]) and cnt[2] == 0 and t[0] == 0.0 and res.at_events.S[0] == 0 and res.residuals.S[0] == 0
        assert ((ws == k) & (k > 0)).any() and exact.any() and ties > 0
        if M > 128:
            assert ((ws % 128 == 0) & (ws > 0)).any()
        if M > 8000:
            assert (ws % 128 == 127).any() and (ws // 128 >= 63).any()
        assert (M // 128 + 1) % 64 == 1 if M in (8192, 8193) else True       # the second group holds one row: empty for 8192
    if name == "S-tiny":
        assert np.all(ws == 0) and t[-1] - t[0] < 2.0 ** -10 and np.all(res.at_events.S[1:] < 0.2)
    T = case["T"]
    inside = (t > T - dt_max) & (t < T)
    assert inside.any()                                                    # the far-T runs cover the other side
    if name.startswith("L") or name == "S-tiny":
        assert inside.all()


@pytest.mark.parametrize("name", ce.INTENSITY_CASES)
def test_intensity_at_agrees_with_the_oracle(orc, name):
    case, q, lam = ce.prepared_intensity(name)
    m = gr.model_of(case)
    t = case["times"]
    assert q[0] == 0.0 and np.isin(t, q).sum() >= 12 and np.isin(t + case["dt_max"], q).sum() >= 10 and (q < t[0]).sum() >= 2
    if case["grid_x"] is not None:
        assert np.isin(case["grid_x"], q).all()
    else:
        assert q[-1] == max(case["T"] + 5.0, q[-1])
    if name in ("N-70", "N-300"):
        assert case["N"] % 32 != 0 and case["N"] > 64 and (name == "N-70" or case["N"] > ce.NHP_BLOCK)
    got = ce.intensity_at(m, t, case["nodes"], q, real=np.float64)
    ratio, bad = ce.check_intensity(np.asarray(got.value, dtype=np.float64), lam)
    print(f"{name}: Q {len(q)} largest K {int(lam.K.max())}; float64 error/bound {ratio:.3g}")
    assert len(bad) == 0 and ratio < 0.5
    want = orc.intensity(gr.oracle_model(orc, case), t, case["nodes"], q)
    ratio, bad = ce.check_intensity(want, lam)
    print(f"{name}: oracle error/bound {ratio:.3g}")
    assert len(bad) == 0, bad[:8]
    # strictness at both ends, from the data: a query on an event does not see it, a query at t_j + Δtmax does not see t_j
    j = len(t) // 2
    for v, side in ((t[j], "left"), (t[j] + case["dt_max"], "right")):
        K = ce.intensity_at(m, t, case["nodes"], np.array([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])).K
        same = int((t == t[j]).sum())
        assert (K[2] - K[1] == same if side == "left" else K[0] - K[1] == same), (name, side, K)


@pytest.mark.parametrize("name", ["W-exp", "W-logit"])
def test_event_intensity_agrees_with_the_oracle(orc, name):
    case, lam = ce.prepared_events(name)
    want = orc.total_intensity(gr.oracle_model(orc, case), case["times"], case["nodes"])
    ratio, bad = ce.check_intensity(want, lam)
    print(f"{name}: oracle total_intensity error/bound {ratio:.3g}")
    assert len(bad) == 0, bad[:8]


def test_intensity_of_an_empty_dataset_is_the_baseline():
    case = ce.case_of("W-exp")
    lam = ce.intensity_at(gr.model_of(case), np.zeros(0), np.zeros(0, dtype=np.int64), np.array([0.0, 1.0, 250.0]))
    assert np.array_equal(np.asarray(lam.value, dtype=np.float64), np.tile(case["lam0"], (3, 1))) and np.all(lam.K == 0)
    assert ce.intensity_at(gr.model_of(case), case["times"], case["nodes"], np.zeros(0)).value.shape == (0, 7)
