"""The continuous adjacency sweep (csrc/cont_adjacency.hip: k_adj_build, k_adj_eval, k_adj_sweep) held to an exact reference
at its edges.  The expected matrices come from tests/adjacency_ref.py (long double, λ from scratch at every entry);
tests/test_adjacency_host.py ties that restatement to the oracle and shows that the inputs reach the paths named here.

Every case is swept four times: with random u from A0; with ADVERSARIAL u from A0 (each u placed at a chosen distance from
the entry's own threshold: ±1e-9, ±1e-6, ±3e-4·(1+Δ) inside the kernel's fp32 band, ±1.1e-3·(1+Δ), ±2e-3·(1+Δ) just outside
it, ±0.1; Δ the entry's data term); again from the matrix that sweep left (k_adj_eval must start from the new matrix); and
with other W and impulse parameters on the same dataset (the cached pair lists and the cached logit(x) depend on the data
only).  adjacency_matrix is compared with np.array_equal, the returned link count with A.sum().

    A-exp, A-logit, A-lgcp   N=130 M=4000 T=500 Δtmax=1, a quarter of the events on one node, 40 bursts (t, t, t + 1e-3),
                             nodes 1, 77, 130 empty: three 64-chunks (64 + 64 + 2), groups of 1..4, folded repeats, general
                             steps below and above 64 entries, an empty first, middle and last column, step counts of all
                             residues mod 3; exponential, logit-normal, and exponential with the LGCP baseline
    B-64, B-65               N=64 / 65 (node 65 empty) M=1500 T=300, 10 bursts: group-only columns that end exactly on the
                             chunk boundary and one past it
    C                        N=1 M=300 T=100: one column whose only list (825 entries) is its own
    D                        N=5 M=6000 T=1500, 60 % of the events on one node, W·0.06: 4025 children in a column (sweep
                             LDS above 64 KiB), lists of up to 10 918 entries through the e += 64 loops
    E                        A's data, λ0·1e-4, W·13: x/λ0 reaches 1e4, the incremental λ update under cancellation; B
                             grows (up to 4.9e-10) and the offsets follow it through the 64·B rule
    F                        N=9 M=800 T=200: ρ as a MATRIX through nhp_cont_resample_adjacency by ctypes, entries exactly 0
                             and 1 mixed in, u exactly 0 and 1 - 2⁻⁵³ mixed in; against the oracle as well

Census of A: 4570 lists of 2..16 entries, 228 of 17..64, 25 above 64, 483 folded, groups 352 / 618 / 585 / 3326, 253 general
steps, 182 chunk cuts.  B: 2104 short lists, 262 folded, no general step, 0 / 53 chunk cuts.  A float64 run of the
restatement stays within 0.58·B of the long-double one (case E; 0.18·B elsewhere).  Smallest realised margin |logit(u) - d|
of an adversarial draw: 1e-9 in every case (E: 8.3e-10); fallbacks to a random u: none, E 0.72 % at most.

A node with more events than the 160 KiB column state holds (8191 with N = 2) is refused with NotImplementedError before any
kernel runs; 8190 events, the most that fit, are swept and compared.

Mistakes planted in scratch builds, and the cases that went red on an MI355X:
    decision from fp32 alone (`sure` forced true)      A-exp A-logit A-lgcp B-64 B-65 E   (at the ±1e-9 / ±1e-6 offsets)
    band narrowed to 1e-7                               A-exp A-logit A-lgcp B-64 B-65 E   (at the ±1e-9 offsets)
    no fold (`run` forced to 0 in k_adj_build)          A-exp A-logit A-lgcp B-64 B-65 E
    the `eb + 64 + lane` loops dropped                  A-exp A-logit A-lgcp C D E and the 8190-event case
    sign of the λ update in visit_group flipped         A-exp A-logit A-lgcp B-64 B-65 E
    k_adj_eval started from the previous sweep's input  every case, at its second sweep
    the `& 63` chunk rule removed                       none: 182 (A) and 53 (B-65) groups then cross a chunk boundary and every
                                                        decision stays the same -- the sweep fetches a step's constants per parent,
                                                        so the rule restricts the grouping without being needed for the result
                                                        (DESIGN.md 3.5); no case can tell it apart
"""
import ctypes as C

import numpy as np
import pytest

import adjacency_ref as ar

pytestmark = pytest.mark.gpu


def explain(st, cs, got):
    """The first differing entry of every column that differs: entry, step code, offset class, margin."""
    out = []
    for c in np.nonzero((got != st.A).any(axis=0))[0][:8]:
        p = int(np.nonzero(got[:, c] != st.A[:, c])[0][0])
        head = p
        while cs.codes[head, c] == 0:
            head -= 1
        off = "random u" if st.cls is None or st.cls[p, c] < 0 else \
            "%+g%s" % (ar.OFFSETS[st.cls[p, c] // 2][0] * (-1 if st.cls[p, c] & 1 else 1), "·(1+Δ)" if ar.OFFSETS[st.cls[p, c] // 2][1] else "")
        margin = float(st.margins[p, c]) if st.margins is not None else float("nan")
        out.append(f"[{p},{c}] got {got[p, c]:.0f} want {st.A[p, c]:.0f}: list of {cs.lengths[p, c]}, step code {cs.codes[head, c]} "
                   f"headed by {head}, offset {off}, margin {margin:.3g}, d {float(st.d[p, c]):.6g}, B {st.B[p, c]:.2g}")
    return "\n".join(out)


def set_parameters(proc, case):
    proc.weights.W = case["W"].copy()
    if case["kind"] == "exponential":
        proc.impulses.θ = case["theta"].copy()
    else:
        proc.impulses.μ, proc.impulses.τ = case["mu"].copy(), case["tau"].copy()


@pytest.mark.parametrize("name", list(ar.SHAPES))
def test_sweep_decisions_at_the_edges(nhp, orc, name):
    case, cs, stages = ar.prepared(name)
    proc = ar.process_of(nhp, case, case["A0"], ar.RHO)
    for st in stages:
        if st.name in ("random", "adversarial"):
            proc.adjacency_matrix = st.A_start.copy()
        else:                                                         # from what the sweep before left on the process
            assert np.array_equal(proc.adjacency_matrix, st.A_start)
        if st.name == "parameters":
            set_parameters(proc, st.case)
        links = nhp.resample_adjacency_matrix_(proc, case["data"], u=st.u)
        got = proc.adjacency_matrix
        if st.margins is not None:
            print(f"{name} {st.name}: smallest kept margin {np.abs(st.margins[st.cls >= 0]).min():.3g}, differing entries "
                  f"{int((got != st.A).sum())}")
        assert np.array_equal(got, st.A), f"{name}, {st.name} sweep:\n" + explain(st, cs, got)
        assert links == st.A.sum()


def test_rho_matrix_and_infinite_log_odds(nhp, orc):
    from nhp_amd import _lib, continuous
    case, rho, u, want, d = ar.prepared_rho_matrix()
    N = case["N"]
    assert np.array_equal(orc.resample_adjacency(ar.oracle_model(orc, case, case["A0"]), *case["data"], rho, u), want)
    proc = ar.process_of(nhp, case, case["A0"], 0.5)
    ctx = _lib.default_context()
    ds = continuous.device_dataset(proc, case["data"], ctx)
    model = proc.device_model(ctx)
    rho_c, u_c, A, nl = _lib.colmajor(rho), _lib.colmajor(u), np.empty(N * N), C.c_double()
    _lib.check(_lib.lib().nhp_cont_resample_adjacency(ctx.h, ds.h, model.h, _lib.dptr(rho_c), 0.5, _lib.dptr(u_c), 0, 0,
                                                      _lib.dptr(A), C.byref(nl)), ctx.h)
    got = A.reshape((N, N), order="F")
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(p), int(c), rho[p, c], u[p, c], float(d[p, c])) for p, c in bad]
    assert nl.value == want.sum()


def one_heavy_node(nhp, events):
    """N = 2, `events` events on node 1 and 40 on node 2, about one parent per child."""
    rng = np.random.default_rng(21)
    M = events + 40
    T = float(M)
    times = np.sort(rng.uniform(0.0, T, M))
    nodes = np.ones(M, dtype=np.int64)
    nodes[rng.choice(M, 40, replace=False)] = 2
    case = ar.adjacency_case(N=2, M=4, T=T, seed=22, kind="exponential", w_scale=0.001)
    case.update(times=times, nodes=nodes, data=(times, nodes, T))
    return case


def test_column_state_limit(nhp):
    # lds_sweep = 20·max_children + 4·(N + 2) + N + 8 bytes against 160 KiB (nhp_adj_enqueue); the build and eval kernels'
    # blocks, 4·(2N + 2 + 256 + max_children) and 24·N + 8·max_children, are far below it here
    N, limit = 2, 160 * 1024
    lds = lambda mc: 20 * mc + 4 * (N + 2) + N + 8
    assert lds(8190) <= limit < lds(8191) and 4 * (2 * N + 2 + 256 + 8191) < limit and 24 * N + 8 * 8191 < limit
    over = one_heavy_node(nhp, 8191)
    assert np.bincount(over["nodes"]).max() == 8191
    proc = ar.process_of(nhp, over, over["A0"], ar.RHO)
    u = np.random.default_rng(2).uniform(size=(N, N))
    with pytest.raises(NotImplementedError, match="160 KiB"):
        nhp.resample_adjacency_matrix_(proc, over["data"], u=u)
    assert np.array_equal(proc.adjacency_matrix, over["A0"])
    # the most that fits is swept, and the context goes on working: a small case afterwards
    for case in (one_heavy_node(nhp, 8190), ar.prepared("C")[0]):
        n = case["N"]
        u = np.random.default_rng(3).uniform(size=(n, n))
        want, _, _ = ar.sweep(ar.model_of(case), *case["data"], ar.RHO, u, case["A0"])
        proc = ar.process_of(nhp, case, case["A0"], ar.RHO)
        links = nhp.resample_adjacency_matrix_(proc, case["data"], u=u)
        assert np.array_equal(proc.adjacency_matrix, want) and links == want.sum()
