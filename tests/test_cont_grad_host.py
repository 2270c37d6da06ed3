"""tests/cont_grad_ref.py tied down on the CPU: its log-likelihood against oracle/mp_eval.py (50 digits, written from the
definitions), its gradient against closed forms, the oracle's float64 gradient and a float64 numpy evaluation of the same
sums in three orders inside the bound the GPU suite uses, and a census showing that every case contains what it is named for.

Largest error/bound of the float64 evaluations (the largest of forward / reversed / permuted; they differ in the third digit
at most except where noted), the headroom of the derivation: W-exp 0.059, W-logit 0.058, W-net 0.041, W-net-logit 0.064,
D 0.00076 (0.00046 forward), L-exp 0.0016 (0.00043 reversed), L-logit 0.00063, C 0.022, C-net 0.020, G-W 0.054, G-D 0.013, G-R 0.039,
R-1 0.00035, R-64 0.019, R-65 0.022, R-257 0.069, R-513 0.14, R-1025 0.12, P4-exp 0.012, P4-logit 0.011, P4-net 0.020,
P2-exp 0.041, P2-logit 0.057, P2-inf 0.025 (the P cases: the inputs of tests/test_time_parts_gpu.py, whose census here also
counts their time parts, the empty first item, the empty last node and the padding).  The largest ratios belong to entries of a few
terms with θΔ in the hundreds, where the error of a float64 exponential's argument is nearly all of the bound."""
import mpmath
import numpy as np
import pytest

import cont_grad_ref as cr
import slices_ref as sr
from oracle import mp_eval

REL_LL = 1e-11


def big(v):
    """A long double (or mpmath number) as an mpmath number, exactly."""
    if isinstance(v, mpmath.mpf):
        return v
    v = np.longdouble(v)
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def small(kind, network, lgcp, recursive, seed):
    rng = np.random.default_rng(seed)
    N, M, T = 3, 60, 12.0
    t = np.sort(rng.integers(0 if recursive else 1, int(T * 64), M)) / 64.0
    if recursive:
        t[:2] = 0.0
    t[20] = t[19]
    nodes = rng.integers(1, N + 1, M).astype(np.int64)
    A = (rng.uniform(size=(N, N)) < 0.6).astype(np.float64) if network else None
    gx = cr.GRID5 * T if lgcp else None
    lam0 = np.exp(rng.normal(0.0, 0.4, (N, 5))) if lgcp else rng.uniform(0.5, 1.5, N)
    return dict(N=N, T=T, times=t, nodes=nodes, kind=kind, dt_max=2.0, lam0=lam0, W=rng.uniform(0.0, 0.6, (N, N)),
                theta=rng.uniform(0.5, 4.0, (N, N)), mu=rng.normal(0.0, 1.0, (N, N)), tau=rng.uniform(0.5, 2.0, (N, N)), A=A,
                grid_x=gx, recursive=recursive)


@pytest.mark.parametrize("kind,network,lgcp,recursive", [("exponential", False, False, False), ("exponential", True, True, False),
                                                        ("logitnormal", False, True, False), ("logitnormal", True, False, False),
                                                        ("exponential", True, False, True), ("exponential", False, True, True)])
def test_loglikelihood_against_the_definitions(orc, kind, network, lgcp, recursive):
    case = small(kind, network, lgcp, recursive, seed=3)
    res = cr.evaluate(cr.model_of(case), case["times"], case["nodes"], case["T"], recursive=recursive)
    want = mp_eval.loglik(cr.oracle_model(orc, case), case["times"], case["nodes"], case["T"], recursive=recursive)
    assert abs(big(res.ll) - want) <= 1e-17 * abs(want)
    # a column shard's log-likelihoods add up to the whole
    parts = [cr.evaluate(cr.model_of(case), case["times"], case["nodes"], case["T"], recursive=recursive, columns=cols).ll
             for cols in ((0, 2), (2, 3))]
    assert abs(float(parts[0] + parts[1] - res.ll)) <= 1e-17 * abs(float(res.ll))


def one_node(times, T, **kw):
    t = np.asarray(times, dtype=np.float64)
    m = cr.model(np.array([0.8]), np.array([[0.4]]), dt_max=2.0, **kw)
    return cr.evaluate(m, t, np.ones(len(t), dtype=np.int64), T)


def test_closed_forms_with_two_and_three_events():
    mpmath.mp.dps = 50
    f = mpmath.mpf
    l0, w, th, T = f(0.8), f(0.4), f(1.7), f(5.0)
    res = one_node([1.0, 1.5], 5.0, theta=np.array([[1.7]]))
    e = mpmath.exp(-th * f(0.5))
    lam2 = l0 + w * th * e
    want = [-T + 1 / l0 + 1 / lam2, w * (1 - th * f(0.5)) * e / lam2, -2 + th * e / lam2]
    assert abs(big(res.ll) - (-l0 * T - 2 * w + mpmath.log(l0) + mpmath.log(lam2))) < 1e-17
    assert all(abs(big(g) - v) < 1e-17 for g, v in zip(res.grad, want))
    assert np.array_equal(res.const, [-5.0, 0.0, -2.0]) and np.array_equal(res.n, [2, 1, 1])
    # three events; the third sees only the second (Δ = 2.25 to the first is outside Δtmax = 2)
    res = one_node([1.0, 1.5, 3.25], 5.0, theta=np.array([[1.7]]))
    e3 = mpmath.exp(-th * f(1.75))
    lam3 = l0 + w * th * e3
    want = [-T + 1 / l0 + 1 / lam2 + 1 / lam3, w * ((1 - th * f(0.5)) * e / lam2 + (1 - th * f(1.75)) * e3 / lam3),
            -3 + th * (e / lam2 + e3 / lam3)]
    assert all(abs(big(g) - v) < 1e-17 for g, v in zip(res.grad, want))
    # S and Q of the θ entry: |term| with 1 - θΔ split, and the terms' derivatives in Δ
    u2, u3 = w * e / lam2, w * e3 / lam3
    assert abs(res.S[1] - float(u2 * (1 + th * f(0.5)) + u3 * (1 + th * f(1.75)))) < 1e-15
    assert abs(res.Q[1] - float(u2 * th * (2 + th * f(0.5)) + u3 * th * (2 + th * f(1.75)))) < 1e-15
    # logit-normal, two events at x = 1/4
    mu, tau = f(-0.3), f(1.3)
    res = one_node([1.0, 1.5], 5.0, mu=np.array([[-0.3]]), tau=np.array([[1.3]]))
    x = f(0.25)
    ell = mpmath.log(x / (1 - x))
    h = mpmath.exp(-tau * (ell - mu) ** 2 / 2) * mpmath.sqrt(tau / (2 * mpmath.pi)) / (x * (1 - x))
    lam2 = l0 + w * h
    want = [-T + 1 / l0 + 1 / lam2, w * h * tau * (ell - mu) / lam2, w * h * (1 / tau - (ell - mu) ** 2) / 2 / lam2, -2 + h / lam2]
    assert all(abs(big(g) - v) < 1e-17 for g, v in zip(res.grad, want))
    # the recursion: the third event sees the first as well, an event at t = 0 is nobody's parent
    m = cr.model(np.array([0.8]), np.array([[0.4]]), theta=np.array([[1.7]]), dt_max=2.0)
    res = cr.evaluate(m, np.array([0.0, 1.0, 1.5, 3.5]), np.ones(4, dtype=np.int64), 5.0, recursive=True)
    s3 = mpmath.exp(-th * f(2.0)) + mpmath.exp(-th * f(2.5))
    lam2, lam3 = l0 + w * th * e, l0 + w * th * s3
    assert abs(big(res.grad[2]) - (-4 + th * (e / lam2 + s3 / lam3))) < 1e-17
    assert abs(big(res.grad[0]) - (-T + 2 / l0 + 1 / lam2 + 1 / lam3)) < 1e-17


def test_closed_forms_with_a_single_tie():
    mpmath.mp.dps = 50
    f = mpmath.mpf
    l0, w, th = f(0.8), f(0.4), f(1.7)
    res = one_node([1.0, 1.0], 5.0, theta=np.array([[1.7]]))             # Δ = 0: a pair, ħ = θ
    lam2 = l0 + w * th
    want = [-5 + 1 / l0 + 1 / lam2, w / lam2, -2 + th / lam2]
    assert all(abs(big(g) - v) < 1e-17 for g, v in zip(res.grad, want))
    res = one_node([1.0, 1.0], 5.0, mu=np.array([[-0.3]]), tau=np.array([[1.3]]))   # x = 0: outside (0, 1), no term at all
    assert [float(g) for g in res.grad] == [-5 + 2 / 0.8, 0.0, 0.0, -2.0]
    assert np.array_equal(res.S[1:], [0.0, 0.0, 0.0]) and np.array_equal(res.n[1:], [0.0, 0.0, 0.0])
    res = one_node([1.0, 3.0], 5.0, theta=np.array([[1.7]]))             # Δ exactly Δtmax: not a pair
    assert [float(g) for g in res.grad] == [-5 + 2 / 0.8, 0.0, -2.0]


CENSUS = {
    # what a case must contain at the least; W-*: 15 ties made on purpose (+ those of the burst), 12 pairs at Δ = Δtmax
    "W-exp": dict(ties=15, edge=12, flushed=100, empty=1, single=1, never=5, longest=80),
    "W-logit": dict(ties=15, edge=12, near=6, empty=1, single=1, never=5, longest=80),
    "W-net": dict(ties=15, edge=12, flushed=100, empty=1, single=1, never=5),
    "W-net-logit": dict(ties=15, edge=12, near=6, empty=1, single=1, never=5),
    "D": dict(ties=10, empty=1), "L-exp": dict(ties=5, pairs=179700), "L-logit": dict(ties=5, pairs=179700),
    "C": dict(zero_time=3), "C-net": dict(zero_time=3), "G-W": dict(on_grid=4, at_end=1, last_cell=100, ties=15, empty=1),
    "G-D": dict(on_grid=4, at_end=1, last_cell=50, empty=1), "G-R": dict(on_grid=4, at_end=1, last_cell=100, zero_time=3, empty=1),
    "R-1": dict(zero_time=3, ties=10), "R-64": dict(zero_time=3, ties=10, empty=1), "R-65": dict(zero_time=3, ties=10, empty=1),
    "R-257": dict(zero_time=3, ties=10, empty=128), "R-513": dict(zero_time=3, ties=10, empty=1),
    "R-1025": dict(zero_time=3, ties=10, empty=1),
}
CENSUS.update({name: dict(ties=12, empty=1, single=1, edge=0 if name == "P2-inf" else 100) for name in cr.TIME_PART_CASES})
TIME_PARTS = {"P4-exp": (4, 40, 4), "P4-logit": (4, 40, 4), "P4-net": (4, 40, 4), "P2-exp": (2, 24, 4), "P2-logit": (2, 24, 4),
              "P2-inf": (2, 24, 4)}
"""(TP, items, padding items) of the cases the default rule lays out in XCD time parts."""


@pytest.mark.parametrize("name", list(cr.CASES))
def test_cases_contain_what_they_are_named_for(name):
    case, res = cr.prepared(name)
    m = cr.model_of(case)
    cs = cr.census(m, case["times"], case["nodes"], case["recursive"])
    print(name, cs)
    for key, least in CENSUS[name].items():
        assert cs[key] >= least, (name, key, cs)
    N = case["N"]
    if name.startswith("W"):
        assert (case["W"] == 0).sum() == 3 and cs["never"] >= 5
        th = case["theta"] * case["dt_max"]
        assert th.min() == 0.5 and np.sort(th.ravel())[-2] == 40.0 and th.max() > 708
        if case["A"] is not None:
            assert (case["A"].sum(axis=1) == 0).any() and (case["A"].sum(axis=0) == 0).any()
            assert ((case["W"] == 0) & (case["A"] == 1)).any()
    if name in TIME_PARTS:
        # the time-part count from the rule, the empty first item of the late node, the empty last node, the padding
        M = len(case["times"])
        TP, items = sr.time_parts(case["times"], case["nodes"], N, case["dt_max"])
        pairs_per_event = cs["pairs"] / M
        assert (TP, len(items)) == TIME_PARTS[name][:2] and N >= 8 and M >= 16 * N
        if name.startswith("P4"):
            assert pairs_per_event >= 192
        elif name == "P2-inf":                                           # Δtmax = ∞ is never sliced: TP = 2 from a mean window of 24 on
            assert 24 <= pairs_per_event < 192 and not np.isfinite(case["dt_max"])
        else:                                                             # above the 160 the plan slices at, below the 192 of TP = 4
            assert 160 < pairs_per_event < 192
        cnt = np.bincount(case["nodes"] - 1, minlength=N)
        assert cnt[N - 1] == 0 and cnt[N - 2] == 40 and cnt[N - 3] == 1 and np.all(cnt[:N - 3] > 16)
        assert np.all(np.nonzero(case["nodes"] == N - 1)[0] >= 3 * M // 4)           # all in the last quarter of the event indices
        late = items[items[:, 0] == N - 2]
        assert late[0, 3] == 1 and late[0, 1] == late[0, 2] and late[-1, 2] - late[-1, 1] > 0
        per_run = 8 // TP
        slot = (np.arange(len(items)) // 8) * per_run + (np.arange(len(items)) % 8) % per_run
        pad = items[slot >= N]
        assert len(pad) == TIME_PARTS[name][2] and np.all(pad[:, 0] == N - 1) and np.all(pad[:, 1] == pad[:, 2]) and np.all(pad[:, 3] == 0)
        assert (items[:, 3] & 1).sum() == N and np.all((items[:, 3] & 2) == 0)
        assert (case["W"] == 0).sum() == 3
        th = case["theta"] * (case["dt_max"] if np.isfinite(case["dt_max"]) else 1.0)
        assert (th.min() == 0.5 and th.max() == 40.0) if np.isfinite(case["dt_max"]) else (0.05 <= th.min() and th.max() <= 4.0)
        tied = np.nonzero(np.diff(case["times"]) == 0)[0]
        assert len(tied) == 12 and np.all(case["nodes"][tied] != case["nodes"][tied + 1])
        if case["A"] is not None:
            assert (case["A"].sum(axis=1) == 0).any() and (case["A"].sum(axis=0) == 0).any()
    if name == "R-257":                                               # part 3 of 4 (nodes 129..192), and part 4's first 64, have no events
        cnt = np.bincount(case["nodes"] - 1, minlength=N)
        assert cnt[128:256].sum() == 0 and cnt[256] > 0
    if case["recursive"] and case["A"] is None:
        assert name in ("R-1", "C")
    # entries without terms: the columns of empty nodes, absent links, exact-zero weights
    assert (res.S == 0).sum() >= (1 if name in ("L-exp", "L-logit", "R-1", "C") else N) - 1
    assert np.all(np.isfinite(np.asarray(res.grad, dtype=np.float64))) and np.all(res.S >= 0) and np.all(res.U <= res.S)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_oracle_gradient_within_the_bound(orc, name):
    case, res = cr.prepared(name)
    ll, g = orc.loglik_grad(cr.oracle_model(orc, case), case["times"], case["nodes"], case["T"], recursive=case["recursive"])
    assert abs(ll - float(res.ll)) <= REL_LL * abs(float(res.ll))
    ratio, bad, err, B = cr.check(g, res)
    print(f"{name}: oracle error/bound {ratio:.3g}")
    assert len(bad) == 0, cr.explain(g, res, case["N"], bad, err, B)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_float64_sums_in_three_orders_within_the_bound(name):
    case, res = cr.prepared(name)
    m = cr.model_of(case)
    for order in ("forward", "reversed", "permuted"):
        r64 = cr.evaluate(m, case["times"], case["nodes"], case["T"], recursive=case["recursive"], real=np.float64, order=order)
        assert abs(float(r64.ll) - float(res.ll)) <= REL_LL * abs(float(res.ll))
        ratio, bad, err, B = cr.check(np.asarray(r64.grad, dtype=np.float64), res)
        print(f"{name} {order}: float64 error/bound {ratio:.3g}")
        assert len(bad) == 0, cr.explain(np.asarray(r64.grad, dtype=np.float64), res, case["N"], bad, err, B)
        assert ratio < 0.25, "float64 alone comes near the bound: the derivation is wrong, not the cap"


def test_shards_are_exact_zeros_outside_their_columns():
    case, whole = cr.prepared("W-exp")
    parts = [cr.prepared("W-exp", cols)[1] for cols in ((0, 3), (3, 7))]
    N = case["N"]
    col = np.concatenate([np.arange(N), np.tile(np.repeat(np.arange(N), N), 2)])
    for (c0, c1), r in zip(((0, 3), (3, 7)), parts):
        foreign = (col < c0) | (col >= c1)
        assert np.all(np.asarray(r.grad, dtype=np.float64)[foreign] == 0.0) and np.all(r.S[foreign] == 0) and np.all(r.const[foreign] == 0)
        assert np.array_equal(np.asarray(r.grad)[~foreign], np.asarray(whole.grad)[~foreign])
    assert float(parts[0].ll + parts[1].ll - whole.ll) == pytest.approx(0.0, abs=1e-15 * abs(float(whole.ll)))
