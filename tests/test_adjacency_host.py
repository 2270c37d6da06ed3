"""tests/adjacency_ref.py tied to the oracle, and the inputs of tests/test_adjacency_edges_gpu.py shown to reach what they
are meant to reach.  CPU only.

Oracle agreement.  For every case and every one of its four sweeps (random u; adversarial u; a second adversarial sweep from
the matrix the first left; other W and impulse parameters on the same data) orc.resample_adjacency returns the matrix the
restatement returns -- with one qualification that the oracle's own arithmetic forces.  The oracle decides with
u <= exp(ll1 - Z), Z = logsumexp(ll0, ll1), where ll0 and ll1 are whole log-likelihoods of the column, |ll| = S ≈ 1e2..1e4.
A rounding of ll, 2⁻⁵³·S, moves exp(ll1 - Z) = 1/(1 + e^-d) by 2⁻⁵³·S·e^-d/(1 + e^-d)², which in log-odds is 2⁻⁵³·S·(1 + e^d):
negligible for d <= 0, but for an entry at d = 11 in a column of a thousand events (S ≈ 2e3) it is 2e-8, more than the
smallest adversarial offset 1e-9.  So where a column differs, its FIRST differing entry must lie within
4·2⁻⁵³·S·(1 + e^d) of the threshold (four roundings: ll0, ll1, Z, the exponential), S taken from the oracle's own
intensities; the entries after it were decided from another state and say nothing.  Seen here: A-lgcp one column (the hot
one) in its first adversarial sweep, E one, one and two columns in its three, every other case and sweep identical in every entry.

Reference agreement.  A float64 run of the same restatement takes the same decisions and agrees with the long-double one on
the data term Σ_k [log(l0_k + x_kp) - log l0_k] within B on every entry.  Largest |Δ64 - Δ| / B observed: A-exp 0.13,
A-logit 0.14, A-lgcp 0.18, B-64 0.16, B-65 0.14, C 0.0015, D 0.015, E 0.58.

Census (adjacency_ref.census, the grouping rules restated in integers), case A: 4570 lists of 2..16 entries, 228 of 17..64,
25 above 64 (longest 2403), 483 short lists that name a child twice, groups of 1 / 2 / 3 / 4 parents 352 / 618 / 585 / 3326,
253 general steps, 182 groups cut by a 64-chunk, step counts of all three residues mod 3, columns 1, 77 and 130 empty.
B-64 / B-65: 2104 short lists (longest 10), 262 folded, no general step, 0 / 53 chunk cuts, B-65's last column empty.
C: one list of 825 entries.  D: 25 lists above 64, the longest 10 918, 4025 children in one column.

Fallbacks (adversarial draws replaced by a random u): none in A, B, C, D; E 121, 95, 99 of 16 900 (0.72 %).
"""
import numpy as np
import pytest

import adjacency_ref as ar

CASES = list(ar.SHAPES)


def oracle_scale(orc, stage, data):
    """S[c]: the size of the column's log-likelihood as the oracle adds it up, from the oracle's own intensities."""
    case = stage.case
    times, nodes, T = data
    om = ar.oracle_model(orc, case, stage.A_start)
    lam = orc.total_intensity(om, times, nodes)
    N = case["N"]
    cnt = np.bincount(nodes - 1, minlength=N).astype(float)
    S = np.zeros(N)
    np.add.at(S, nodes - 1, np.abs(np.log(lam)))
    if case["grid_x"] is None:
        base = case["lam0"] * T
    else:
        base = ((case["lam0"][:, 1:] + case["lam0"][:, :-1]) / 2 * np.diff(case["grid_x"])[None, :]).sum(axis=1)
    return S + base + (case["W"] * cnt[:, None]).sum(axis=0)


def excused_columns(orc, stage, data, want):
    """Columns where the oracle differs; asserts that each one's first differing entry is inside the oracle's own resolution."""
    with np.errstate(divide="ignore", over="ignore"):
        margins = np.log(stage.u / (1.0 - stage.u)) - stage.d.astype(np.float64) if stage.margins is None else stage.margins
        cols = np.nonzero((want != stage.A).any(axis=0))[0]
        if len(cols) == 0:
            return 0
        S = oracle_scale(orc, stage, data)
        for c in cols:
            p = int(np.nonzero(want[:, c] != stage.A[:, c])[0][0])
            resolution = 4 * ar.EPS * S[c] * (1.0 + np.exp(float(stage.d[p, c])))
            assert abs(margins[p, c]) < resolution, (stage.name, p, c, margins[p, c], resolution, float(stage.d[p, c]))
    return len(cols)


@pytest.mark.parametrize("name", CASES)
def test_the_oracle_takes_the_restatements_decisions(orc, name):
    case, cs, stages = ar.prepared(name)
    excused = []
    for st in stages:
        om = ar.oracle_model(orc, st.case, st.A_start)
        want = orc.resample_adjacency(om, *case["data"], ar.RHO, st.u)
        excused.append(excused_columns(orc, st, case["data"], want))
        assert name == "C" or 0 < st.A.sum() < st.A.size             # a non-trivial draw
    if name == "C":                                                  # one entry: both outcomes over its four sweeps
        assert {float(st.A[0, 0]) for st in stages} == {0.0, 1.0}
    print(f"{name}: columns whose first difference lies inside the oracle's resolution, per sweep: {excused}")
    assert excused[0] == 0                                           # random u: margins of 1/N², far from any rounding


def test_the_oracle_takes_the_rho_matrix_decisions(orc):
    case, rho, u, A, d = ar.prepared_rho_matrix()
    want = orc.resample_adjacency(ar.oracle_model(orc, case, case["A0"]), *case["data"], rho, u)
    assert np.array_equal(want, A)
    # what the infinite log-odds must give: ρ = 0 -> 0 unless u = 0; ρ = 1 -> 1; u = 0 -> 1
    assert A[0, 0] == 1 and A[1, 0] == 0 and A[2, 1] == 1 and A[3, 1] == 1 and A[8, 1] == 0 and A[4, 2] == 1
    assert A[6, 3] == 1 and A[7, 3] == 0 and A[0, 8] == 1 and A[8, 8] == 1 and A[3, 5] == 1 and A[4, 5] == 0
    assert np.isneginf(float(d[0, 0])) and np.isposinf(float(d[2, 1]))
    assert 0 < A.sum() < A.size


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_within_the_bound(name):
    case, cs, stages = ar.prepared(name)
    worst = 0.0
    for st in stages[:2]:
        A64, d64, B64, D64 = ar.sweep(ar.model_of(st.case), *case["data"], ar.RHO, st.u, st.A_start, real=np.float64, parts=True)
        assert np.array_equal(A64, st.A)
        err = np.abs((D64.astype(np.longdouble) - st.delta).astype(np.float64))
        assert np.all(err <= st.B), (name, st.name, float((err / np.maximum(st.B, 1e-300)).max()))
        pos = st.B > 0
        worst = max(worst, float((err[pos] / st.B[pos]).max()))
        assert np.all(np.abs(B64 - st.B) <= 1e-6 * st.B)
    print(f"{name}: largest |delta64 - delta| / B = {worst:.2g}")


def test_mpmath_backend_is_the_same_restatement():
    case = ar.adjacency_case(N=4, M=60, T=12.0, bursts=3, seed=3, kind="logitnormal", lgcp=True)
    u = np.random.default_rng(5).uniform(size=(4, 4))
    A, d, B = ar.sweep(ar.model_of(case), *case["data"], ar.RHO, u, case["A0"], real=np.longdouble)
    Am, dm, Bm = ar.sweep(ar.model_of(case), *case["data"], ar.RHO, u, case["A0"], real="mpmath")
    assert np.array_equal(A, Am) and B.max() > 0
    tol = max(float(np.finfo(np.longdouble).eps), 1e-19) * 64 * (1.0 + np.abs(d.astype(np.float64)))
    assert np.all(np.abs(np.array([[float(v) for v in row] for row in dm - d.astype(object)])) <= tol)
    assert np.allclose(B, Bm, rtol=1e-9)


def test_census_case_a():
    # every one of the three A cases and E share these data
    for name in ("A-exp", "A-logit", "A-lgcp", "E"):
        s = ar.census_summary(ar.prepared(name)[1])
        assert s["short"] >= 100 and s["mid"] >= 100 and s["long"] >= 20
        assert s["folded"] >= 100
        assert all(g >= 1 for g in s["groups"])
        assert s["general"] == s["mid"] + s["long"] >= 100
        assert s["cuts"] >= 50
        assert s["residues"] == [0, 1, 2]
        assert s["empty_columns"] == [0, 76, 129]                    # first, middle and LAST column: base == total
    print("A:", s)


def test_census_case_b():
    for name, N in (("B-64", 64), ("B-65", 65)):
        case, cs, _ = ar.prepared(name)
        s = ar.census_summary(cs)
        assert case["N"] == N
        assert s["general"] == 0 and s["max_list"] <= 16               # group-only columns
        assert all(g >= 50 for g in s["groups"]) and s["folded"] >= 20 and s["short"] >= 500
        assert s["residues"] == [0, 1, 2]
        # 64: every column's last group ends at parent 63, no chunk rule applies; 65: the rule cuts groups at 64 and
        # parent 64 is a step of its own at the very end
        if N == 64:
            assert s["cuts"] == 0 and s["empty_columns"] == []
        else:
            assert s["cuts"] >= 20 and s["empty_columns"] == [64] and np.all(cs.codes[64, :] == 1)
        print(name, s)


def test_census_cases_c_d_f():
    case, cs, _ = ar.prepared("C")
    assert cs.lengths.shape == (1, 1) and cs.lengths[0, 0] > 64 * 4 and cs.codes[0, 0] == 255 and cs.steps[0] == 1
    case, cs, _ = ar.prepared("D")
    s = ar.census_summary(cs)
    children = int(np.bincount(case["nodes"]).max())
    assert 20 * children + 4 * (5 + 2) + 5 + 8 > 64 * 1024               # the sweep's column state, above 64 KiB
    assert 4 * (2 * 5 + 2 + 256 + children) < 64 * 1024 < 160 * 1024
    assert s["long"] == 25 and cs.lengths.min() > 64 and s["max_list"] > 5000
    print("D:", s, "children", children)
    case = ar.prepared_rho_matrix()[0]
    s = ar.census_summary(ar.census(case["N"], case["times"], case["nodes"], case["dt_max"]))
    assert s["general"] == 81                                             # every list long: the general step throughout


@pytest.mark.parametrize("name", CASES)
def test_fallback_cap(name):
    case, cs, stages = ar.prepared(name)
    for st in stages[1:]:
        kept = st.cls >= 0
        assert (~kept).sum() <= 0.01 * st.cls.size, (name, st.name, int((~kept).sum()))
        m = np.abs(st.margins[kept])
        mags = np.array([ar.OFFSETS[i // 2][0] for i in st.cls[kept]])
        assert np.all(m >= mags / 2) and np.all(m >= 64 * st.B[kept])
        if name.startswith("A") or name == "E":
            assert np.bincount(st.cls[kept], minlength=12).min() >= 50
    print(f"{name}: fallbacks {[int((st.cls < 0).sum()) for st in stages[1:]]}, smallest margin "
          f"{min(float(np.abs(st.margins[st.cls >= 0]).min()) for st in stages[1:]):.3g}")
