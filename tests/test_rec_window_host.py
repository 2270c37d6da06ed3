"""tests/rec_window_ref.py held to its own definitions, and the inputs of tests/test_rec_window_gpu.py to what their names
promise -- no GPU.  For every case: a census in integers; with the reference's own cut, what the window drops is at most
2⁻⁶⁰·λ0_c for EVERY child (long double); and the cost model, read from the constants in nhp_recursive_window, puts the case on
its intended side by a factor of at least three at every recursion_cost the library uses -- so retuning the constants within
that factor leaves the GPU tests on the route they are about, and beyond it their route assertions go red.  For the
staleness cases: the log-likelihood evaluated with the stale cut differs from the right one by more than 1e-6 relative, so a
stale cache cannot pass the GPU tests' 1e-12."""
import math

import numpy as np
import pytest

import cont_grad_ref as cr
import rec_window_ref as rw


def test_slab_stats_against_a_brute_force_count():
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(0.0, 30.0, 300))
    t[100:140] = 12.0 + np.sort(rng.uniform(0.0, 0.01, 40))              # a burst
    t[200:210:2] = t[201:211:2]                                         # ties
    t = np.sort(t)
    lens, best = rw.slab_stats(t)
    lens2, brute = rw.slab_stats_brute(t)
    assert len(lens) >= 8 and lens[0] == (t[-1] - t[0]) / 300 and np.all(lens[1:] == 2.0 * lens[:-1]) and lens[-1] < t[-1] - t[0]
    assert np.array_equal(lens, lens2) and np.array_equal(best, brute)
    assert best[0] >= 40 and np.all(np.diff(best) >= 0) and best[-1] <= 300
    assert rw.slab_stats(t[:1])[0].size == 0 and rw.slab_stats(np.array([1.0, 1.0]))[0].size == 0


def test_window_starts_and_the_clamp():
    t = np.array([0.0, 0.0, 0.5, 1.0, 1.0, 1.5, 3.0])
    st = rw.window_starts(t, 1.0, 2)
    # t - cut: -1, -1, -0.5, 0, 0, 0.5, 2.0; first j >= n_zero with t_j > that, never beyond i; a child among the zeros is its own start
    assert st.tolist() == [0, 1, 2, 2, 2, 3, 6]
    assert rw.window_starts(t, 1e-300, 2).tolist() == [0, 1, 2, 3, 4, 5, 6]          # t - 1e-300 == t: an empty window, ties dropped
    assert rw.window_starts(t, 100.0, 2).tolist() == rw.full_starts(t).tolist()


def test_cut_special_values():
    m = cr.model(np.array([1.0, 2.0]), np.full((2, 2), 0.5), theta=np.full((2, 2), 10.0))
    t = np.linspace(0.1, 9.9, 50)
    c = rw.cut(m, t)
    lens, best = rw.slab_stats(t)
    count = min(50.0, min(b / (1.0 - math.exp(-10.0 * L)) for L, b in zip(lens, best)))
    assert c == (math.log(count * 5.0 / 1.0) + 60.0 * math.log(2.0)) / 10.0 and 4.0 < c < 5.0
    assert rw.cut(m._replace(W=np.zeros((2, 2))), t) == 1e-300
    assert rw.cut(m._replace(lam0=np.array([1e300, 1e300]), W=np.full((2, 2), 1e-300)), t) == 1e-300     # the quotient's log is very negative
    for bad in (m._replace(lam0=np.array([1.0, 0.0])), m._replace(theta=np.array([[10.0, 0.0], [10.0, 10.0]])),
                m._replace(theta=np.array([[10.0, np.nan], [10.0, 10.0]])), m._replace(W=np.array([[0.5, np.inf], [0.5, 0.5]])),
                m._replace(lam0=np.array([np.nan, 1.0]))):
        assert rw.cut(bad, t) == 0.0


def _flat(a):
    return np.asarray(a).ravel(order="F")


def census(name):
    case = rw.case_of(name)
    m, t, nodes, N = cr.model_of(case), case["times"], case["nodes"], case["N"]
    c = rw.cut_of(name)
    n_zero = int((t == 0.0).sum())
    ties = int(((np.diff(t) == 0.0) & (t[1:] > 0.0)).sum())
    cnt = np.bincount(nodes - 1, minlength=N)
    if name.startswith("uniform") or name in ("net", "cache-fast", "cache-slow"):
        assert n_zero == 3 and ties >= 10 and cnt.max() >= (2000 if N == 130 else 500)
    if name == "spread":
        th, wt, A = _flat(m.theta), _flat(m.W * m.theta), _flat(m.A)
        assert th.max() / th.min() == 200.0
        k = int(np.argmin(th))
        assert th[k] == 2.0 and _flat(m.W)[k] == 0.0 and A[k] == 0.0
        assert int(np.argmax(wt)) == N * N - 1 and A[N * N - 1] == 0.0 and wt[N * N - 1] == 400.0
        assert int(np.argmin(m.lam0)) == N - 1
        live = (A * _flat(m.W)) > 0                                     # the bound from the entries that do contribute is far shorter
        assert (math.log(len(t) * wt[live].max() / 0.9) + 60 * math.log(2.0)) / th[live].min() < 0.5 * c
    if name == "second_trip":
        th, wt = _flat(m.theta), _flat(m.W * m.theta)
        assert N * N == 16900 > rw.THREADS and int(np.argmin(th)) == 16899 and int(np.argmax(wt)) == rw.THREADS
        assert th[:rw.THREADS].min() >= 4.0 * th[16899] and wt[np.arange(N * N) != rw.THREADS].max() * 50.0 < wt[rw.THREADS]
        for skipped in (m._replace(theta=np.where(np.arange(N * N).reshape(N, N, order="F") < rw.THREADS, m.theta, 30.0)),
                        m._replace(W=np.where(np.arange(N * N).reshape(N, N, order="F") == rw.THREADS, 0.0, m.W))):
            assert abs(rw.cut(skipped, t) - c) > 0.05 * c               # a reduction without the second trip: another cut
        assert cnt.max() >= 2000
    if name == "grid":
        G = len(m.grid_x)
        lam = m.lam0.ravel()                                            # g fastest, one run of G per node
        assert N * G == 16510 > rw.THREADS and int(np.argmin(lam)) == N * G - 1 and lam[:rw.THREADS].min() > 20.0 * lam[-1]
        assert int(np.isin(t, m.grid_x).sum()) >= 7 and t[-1] == case["T"] == m.grid_x[-1] and cnt.max() >= 2000
        first_trip = m.lam0.copy()
        first_trip[N - 1, G - 1] = lam[:rw.THREADS].min()
        assert abs(rw.cut(m._replace(lam0=first_trip), t) - c) > 0.02 * c
    if name == "burst":
        assert len(t) == 2307 and case["rounds"] == 2
        burst = (t >= 100.0) & (t <= 100.01)
        assert int(burst.sum()) == 400
        st = rw.window_starts(t, c, n_zero)
        b0, b1 = np.nonzero(burst)[0][[0, -1]]
        kids = np.searchsorted(t, 100.005 + np.array(rw.BURST_AT) * c)
        assert np.all(t[kids] == 100.005 + np.array(rw.BURST_AT) * c)
        keeps, splits, drops = st[kids] <= b0, (st[kids] > b0) & (st[kids] <= b1), st[kids] > b1
        assert keeps.sum() >= 1 and splits.sum() >= 1 and drops.sum() >= 1, (keeps, splits, drops)
        assert keeps[0] and splits[3] and drops[-1]
        edge = t[kids[5]] - c                                           # an event exactly on the open edge of a window: not a parent
        k = np.searchsorted(t, edge)
        assert t[k] == edge and t[k + 1] > edge and st[kids[5]] == k + 1 and not burst[k]
        lens, best = rw.slab_stats(t)
        tmin = m.theta.min()
        count = min(b / (1.0 - math.exp(-tmin * L)) for L, b in zip(lens, best))
        assert 400.0 <= count <= 450.0 and count < len(t) / 5
        assert rw.cut(m, t, count_only_M=True) > c
    if name == "no_burst":
        other = rw.case_of("burst")
        assert len(t) == len(other["times"]) and t[0] == other["times"][0] and t[-1] == other["times"][-1]
        assert abs(rw.cut_of("burst") - c) > 2.0 ** -40 * c
        assert not np.array_equal(rw.window_starts(other["times"], c, 0), rw.window_starts(other["times"], rw.cut_of("burst"), 0))
    if name == "net":
        A = m.A
        assert 0.4 < A.mean() < 0.6 and not A[7, :].any() and not A[:, 1].any() and np.all(m.W > 0)
    if name == "early":
        assert n_zero == 5 and set(nodes[:n_zero]) == {1, 2, 3} and int(((t > 0.0) & (t < c)).sum()) >= 5
        assert t[n_zero] == 2.0 ** -40
    if name.startswith("tiny"):
        assert len(t) == int(name[-1]) and N == int(name[5]) and c > 0.0 and (len(t) == 1 or t[1] - t[0] < c)
    if name == "silent":
        assert c == 1e-300 and not m.W.any() and np.array_equal(rw.window_starts(t, c, n_zero), np.arange(len(t)))
    if name == "no_bound-lam":
        assert c == 0.0 and m.lam0[2] == 0.0 and cnt[2] == 0 and np.all(m.lam0[:2] > 0) and np.all(m.theta > 0)
    if name == "no_bound-theta":
        assert c == 0.0 and m.theta[1, 0] == 0.0 and m.W[1, 0] == 0.0 and int((m.theta == 0).sum()) == 1 and np.all(m.lam0 > 0)
    if name == "nan":
        assert c == 0.0 and int(np.isnan(m.theta).sum()) == 1
    if name == "slow":
        assert c > 0.0 and c * len(t) / t[-1] > 8192.0
    return case, m, c


@pytest.mark.parametrize("name", list(rw.CASES))
def test_case_holds_what_it_is_named_for(name):
    case, m, c = census(name)
    t, nodes = case["times"], case["nodes"]
    if c > 0.0:
        tail, floor = rw.dropped_tail(m, t, nodes, rw.window_starts(t, c, int((t == 0.0).sum())))
        worst = float((tail / np.where(floor > 0, floor, 1.0)).max()) if len(t) else 0.0
        print(f"{name}: cut {c:.6g}, largest dropped tail / (2^-60 λ0_c) {worst:.3g}")
        assert np.all(tail <= floor), name
    for cost, want in zip(rw.COSTS, rw.EXPECT[name]):
        r = rw.route(case, c, cost)
        assert r["used"] == bool(want), (name, cost, r)
        assert r["margin"] >= rw.MARGIN if want else r["margin"] <= 1.0 / rw.MARGIN, (name, cost, r)


def test_the_slab_count_is_what_holds_the_tail_behind_the_burst():
    """With count = 1 in place of the slab count, the child that sits one cut behind the burst loses more than the bound allows."""
    case = rw.case_of("burst")
    m, t, nodes = cr.model_of(case), case["times"], case["nodes"]
    tmin, wmax, lmin = rw.extremes(m)
    short = (math.log(1.0 * wmax / lmin) + 60.0 * math.log(2.0)) / tmin
    tail, floor = rw.dropped_tail(m, t, nodes, rw.window_starts(t, short, 0))
    assert np.any(tail > floor)


@pytest.mark.parametrize("right,stale", [("cache-slow", "cache-fast")])
def test_a_stale_cut_moves_the_loglikelihood(right, stale):
    case = rw.case_of(right)
    m, t, nodes, T = cr.model_of(case), case["times"], case["nodes"], case["T"]
    assert np.array_equal(t, rw.case_of(stale)["times"]) and np.array_equal(m.theta, rw.case_of(stale)["theta"] / 100.0)
    assert 0.2 < rw.cut_of(stale) < 0.25 and 20.0 < rw.cut_of(right) < 25.0
    want = rw.loglik_with_starts(m, t, nodes, T, rw.full_starts(t))
    _, res = rw.prepared(right)
    assert abs(want - float(res.ll)) <= 1e-15 * abs(want)               # the restatement with starts is the reference's recursive form
    kept = rw.loglik_with_starts(m, t, nodes, T, rw.window_starts(t, rw.cut_of(right), 3))
    assert abs(kept - want) <= 1e-15 * abs(want)
    got = rw.loglik_with_starts(m, t, nodes, T, rw.window_starts(t, rw.cut_of(stale), 3))
    assert abs(got - want) >= 1e-6 * abs(want), (got, want)
