"""VB / SVI for the stochastic block network on the GPU (nhp_disc_sbmvb_run, nhp_disc_sbmsvi_run) against
tests/disc_sbmvb_ref.py.

Bounds.  The tables inherited from the dense step: rtol 1e-10 / atol 1e-12 after one step, rtol 1e-9 after six, as in
tests/test_disc_netvb_gpu.py.  The link layer: the reference logit at the device's own tables and at the network state the
device READ; ρv is held to nr.measured_logit_error() plus br.measured_net_error(), both the reference's own errors against
50-digit arithmetic.  The block tables against α + Σω ρv of the device's own ρv and m: a sum of at most N² non-negative
terms, rtol N² 2⁻⁵² (γv: N 2⁻⁵²).  The sweep node by node without extra outputs: the state before node n's step is
[m_after[0:n], m_before[n:]] and the reference update of node n from it must match m_after[n] to 1e-10 absolute, the
bound tests/test_sbm_gpu.py holds the Gibbs conditionals to (measured maximum over the six shapes: see the print of
test_one_and_six_steps).  network_bound at the device's states, with the ρv both states share, must not fall by more
than 4 x the reference's own error in it against 50 digits."""
import numpy as np
import pytest
from scipy.special import digamma, polygamma

import disc_netvb_ref as nr
import disc_sbmvb_ref as br
import disc_svi_ref as sr

pytestmark = pytest.mark.gpu

PRI, BPRI, WP = br.PRIORS, br.BPRI, br.PRIORS[2:6]
ULP = 2.0 ** -52


def setup(nhp, shape, bpri=BPRI):
    N, T, B, L, K = shape
    data, conv, params, blk = br.problem(*shape)
    proc = br.make_process(nhp, N, B, L, K, bpri=bpri, seed=N)
    return proc, data, conv, params, blk, nhp.convolve(proc, data)


_REF = {}


def reference(shape, data, conv, params, blk):
    if shape not in _REF:
        one = br.sbmvb_step(data, conv, 1.0, PRI, BPRI, params, blk)
        five = br.sbmvb_run(data, conv, 1.0, PRI, BPRI, one[0], one[1], 4)
        _REF[shape] = (one, br.sbmvb_step(data, conv, 1.0, PRI, BPRI, five[0], five[1]))
    return _REF[shape]


def check_step(before, after, label, links=True):
    """One device step: `before` = (params, blk) it read, `after` what it wrote.  Returns the sweep's largest difference.
    links=False leaves the link layer out (its bound is measured on br.SHAPES)."""
    (pb, bb), (pa, ba) = before, after
    N, K = bb[0].shape
    err = nr.measured_logit_error() + br.measured_net_error() if links else np.inf
    want = nr.sigmoid(nr.logit(br.net_term(bb[0], bb[1], bb[2]), WP, pa[2], pa[3], pa[5]))
    d = float(np.max(np.abs(pa[7] - want)))
    av, bv, gv = br.tables(BPRI, bb[0], pa[7])
    dt = max(float(np.max(np.abs(ba[1] - av) / av)), float(np.max(np.abs(ba[2] - bv) / bv)))
    dg = float(np.max(np.abs(ba[3] - gv) / gv))
    E = br.expectations(ba[1], ba[2], ba[3])
    cur, ds = bb[0].copy(), 0.0
    for n in range(N):
        ds = max(ds, float(np.max(np.abs(br.node_update(n, cur, pa[7], *E) - ba[0][n]))))
        cur[n] = ba[0][n]
    rows = float(np.max(np.abs(ba[0].sum(axis=1) - 1.0)))
    print(f"{label}: max |Δρv| {d:.2e} (bound {err:.2e}); block tables {dt:.2e} (bound {N * N * ULP:.2e}), γv {dg:.2e} "
          f"(bound {N * ULP:.2e}); sweep max |Δm| {ds:.2e} (bound 1e-10); rows off 1 by {rows:.2e} (bound {4 * ULP * K:.2e})")
    assert d <= err
    assert dt <= N * N * ULP and dg <= N * ULP
    assert ds <= 1e-10
    assert rows <= 4 * ULP * K and np.all(ba[0] >= 0.0) and np.all(np.isfinite(ba[0]))
    return ds


@pytest.mark.parametrize("shape", br.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_one_and_six_steps(nhp, shape):
    """(3,50,2,4,1); (5,700,3,7,2); (5,700,3,7,3): N < 2K; (130,300,2,3,5): N crosses the 128-column tile, 67 link workgroups,
    K no power of two; (300,120,2,3,2): more nodes than the sweep has threads; (70,120,2,3,64): the largest K.  Six calls
    of one step, so that every state the device read is known.  Measured over the six shapes: |Δρv| <= 3.3e-16
    (bound 9.8e-15), block tables 8.7e-16 relative, the sweep node by node 1.3e-13 at worst (bound 1e-10), rows of m within
    2 ulp of 1, smallest rise of network_bound 1.1e-7 against a margin of 1.2e-14."""
    N, T, B, L, K = shape
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    (want1, wblk1), (want6, wblk6) = reference(shape, data, conv, params, blk)
    br.put(proc, params, blk)
    states = [(params, blk)]
    for _ in range(6):
        v = nhp.update_(proc, data, ds)
        states.append(br.get(proc))
    assert len(v) == 2 * N + 4 * N * N + N * N * B + N * N + 2 * K * K + K + N * K
    for g, w in zip(states[1][0][:7], want1[:7]):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-12)
    for g, w in zip(states[6][0][:7], want6[:7]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    worst = max(check_step(states[0], states[1], "one step"), check_step(states[5], states[6], "sixth step"))
    print(f"{shape}: the sweep's largest |Δm| against the reference update, node by node: {worst:.2e}")
    # The network part of the bound over the six steps, each at the ρv the step wrote (both states share it).  The margin
    # is 4 x the LARGEST of the reference's own errors over the twelve evaluations compared, as on the host.  The maximum
    # only grows with every evaluation measured, so the evaluations are measured one by one and only while some step
    # still misses the margin reached so far: passing early is passing against the full maximum.
    steps = []
    for i in range(6):
        rho = states[i + 1][0][7]
        steps.append((br.network_bound(states[i][1], rho, BPRI), br.network_bound(states[i + 1][1], rho, BPRI)))
    mp_states = {}

    def err_at(j, i):                                  # state j at the ρv step i + 1 wrote
        if j not in mp_states:
            mp_states[j] = br.bound_mp_state(states[j][1], BPRI)
        return br.measured_bound_error(states[j][1], states[i + 1][0][7], BPRI, mp_states[j])

    todo = [(j, i) for i in range(6) for j in (i, i + 1)]
    err, measured = err_at(*todo.pop()), 1
    while todo and any(hi < lo - 4 * err for lo, hi in steps):
        err, measured = max(err, err_at(*todo.pop())), measured + 1
    for i, (lo, hi) in enumerate(steps):
        print(f"step {i + 1}: network_bound {lo:.9g} -> {hi:.9g}")
    print(f"the reference's own error, largest of the {measured} evaluation(s) measured: {err:.2e}")
    assert all(hi >= lo - 4 * err for lo, hi in steps)
    # against the reference's trajectory: ρv through the logit's slope, the block state at the tables' bound
    k0, n0, k1, n1 = want1[2], want1[3], want1[4], want1[5]
    slope = np.abs(digamma(k1) - digamma(k0) - np.log(n1 / n0))
    b = 0.25 * (slope * (1e-10 * k0 + 1e-12) + 4 * (nr.measured_logit_error() + br.measured_net_error()))
    assert np.all(np.abs(states[1][0][7] - want1[7]) <= b)
    assert np.allclose(states[1][1][0], wblk1[0], rtol=0.0, atol=1e-9)
    for g, w in zip(states[1][1][1:], wblk1[1:]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("shape", [(1100, 40, 2, 3, 8), (1120, 40, 2, 3, 16)], ids=lambda s: "-".join(map(str, s)))
def test_the_sweep_above_64_kib_of_lds(nhp, shape):
    """The launches that need the raised dynamic-LDS limit and 16 staged (row, column) pairs per thread (N > 1024).
    (1100,40,2,3,8): 89 280 bytes and the four tables (2 KiB) staged with them.  (1120,40,2,3,16): 163 840 bytes, the limit
    exactly; the tables (8 KiB) no longer fit and are read from global memory.  One step: the block tables and the sweep
    node by node, at the bounds of test_one_and_six_steps (the link layer's bound is measured on br.SHAPES and is left out)."""
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    N, K = shape[0], shape[4]
    Kp = 1 << (K - 1).bit_length()
    assert 8 * (N * K + 2 * N + 20 * Kp) in (89280, 163840)
    br.put(proc, params, blk)
    nhp.update_(proc, data, ds)
    after = br.get(proc)
    assert not np.array_equal(after[1][0], blk[0])
    worst = check_step((params, blk), after, f"{shape}", links=False)
    print(f"{shape}: the sweep's largest |Δm| against the reference update, node by node: {worst:.2e}")


@pytest.mark.parametrize("N,T,B,L", [(3, 50, 2, 4), (5, 700, 3, 7)])
def test_one_block_is_the_bernoulli_update(nhp, N, T, B, L):
    data, conv, start = nr.parity_problem(N, T, B, L)
    bern = nr.make_process(nhp, N, B, L, PRI, nr.PARITY_NET, seed=N)
    proc = br.make_process(nhp, N, B, L, 1, bpri=(nr.PARITY_NET[0], nr.PARITY_NET[1], 0.8), seed=N)
    ds = nhp.convolve(bern, data)
    for steps in (1, 3):
        nr.put(bern, start)
        br.put(proc, start[:8], (np.ones((N, 1)), np.array([[start[8]]]), np.array([[start[9]]]), np.array([1.4])))
        nhp.update_(bern, data, ds, n_steps=steps)
        nhp.update_(proc, data, ds, n_steps=steps)
        want, (got, blk) = nr.get(bern), br.get(proc)
        for g, w in zip(got, want[:8]):
            assert np.allclose(g, w, rtol=1e-13, atol=0.0)
        print(f"{steps} step(s): αv {blk[1][0, 0]!r} against {want[8]!r}, βv {blk[2][0, 0]!r} against {want[9]!r}")
        assert abs(blk[1][0, 0] - want[8]) <= N * N * ULP * want[8] and abs(blk[2][0, 0] - want[9]) <= N * N * ULP * want[9]
        assert np.all(blk[0] == 1.0) and np.isclose(blk[3][0], 0.8 + N, rtol=N * ULP, atol=0.0)


def test_reproducible_and_resident(nhp):
    shape = (130, 300, 2, 3, 5)
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    runs = []
    for _ in range(2):
        br.put(proc, params, blk)
        nhp.update_(proc, data, ds, n_steps=5)
        runs.append(br.get(proc))
    br.put(proc, params, blk)
    for _ in range(5):
        nhp.update_(proc, data, ds)
    runs.append(br.get(proc))
    for other in runs[1:]:
        for g, w in zip(other[0] + other[1], runs[0][0] + runs[0][1]):
            assert np.array_equal(g, w)
    assert not np.array_equal(runs[0][1][0], blk[0])


def test_labels_every_counts_global_steps(nhp):
    """labels_every = 2 with one step per call, the way vb_ keeps its trace and a loop over update_ runs: m changes at
    steps 2 and 4 only, and vb_(keep_trace=True), four calls of one step and one call of four steps are bit-equal."""
    shape = (5, 700, 3, 7, 3)
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    proc.network.labels_every = 2
    br.put(proc, params, blk)
    nhp.update_(proc, data, ds, n_steps=4)
    whole = br.get(proc)
    assert proc.network.vb_step == 4
    br.put(proc, params, blk)
    ms = []
    for i in range(4):
        nhp.update_(proc, data, ds)
        ms.append(br.get(proc)[1][0])
        assert proc.network.vb_step == i + 1
    single = br.get(proc)
    assert np.array_equal(ms[0], blk[0]) and not np.array_equal(ms[1], ms[0])
    assert np.array_equal(ms[2], ms[1]) and not np.array_equal(ms[3], ms[2])
    br.put(proc, params, blk)
    res = nhp.vb_(proc, data, max_steps=4)                                    # keep_trace=True: one step per call
    traced = br.get(proc)
    NK = shape[0] * shape[4]
    assert res.step == 4 and len(res.trace) == 4
    assert np.array_equal(res.trace[0][-NK:], blk[0].ravel(order="F")) and np.array_equal(res.trace[1][-NK:], ms[1].ravel(order="F"))
    for other in (single, traced):
        for g, w in zip(other[0] + other[1], whole[0] + whole[1]):
            assert np.array_equal(g, w)
    want_p, want_b = br.sbmvb_run(data, conv, 1.0, PRI, BPRI, params, blk, 4, labels_every=2)
    assert np.allclose(whole[1][0], want_b[0], rtol=0.0, atol=1e-9)
    # a fit that goes on: steps 5 and 6 of a second call sweep at 6, and step0 says where a call stands
    nhp.update_(proc, data, ds, n_steps=2)
    six = br.get(proc)
    br.put(proc, params, blk)
    nhp.update_(proc, data, ds, n_steps=5)
    five = br.get(proc)[1][0]
    nhp.update_(proc, data, ds, step0=5)
    assert proc.network.vb_step == 6 and not np.array_equal(br.get(proc)[1][0], five)
    for g, w in zip(br.get(proc)[0] + br.get(proc)[1], six[0] + six[1]):
        assert np.array_equal(g, w)


def test_labels_every(nhp):
    """labels_every = 2: m changes at steps 2 and 4 only; the tables and ρv move at every step."""
    shape = (5, 700, 3, 7, 3)
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    proc.network.labels_every = 2
    got = []
    for steps in (1, 2, 3, 4):
        br.put(proc, params, blk)
        nhp.update_(proc, data, ds, n_steps=steps)
        got.append(br.get(proc))
    m = [g[1][0] for g in got]
    assert np.array_equal(m[0], blk[0]) and not np.array_equal(m[1], m[0])
    assert np.array_equal(m[2], m[1]) and not np.array_equal(m[3], m[2])
    assert not np.array_equal(got[2][1][1], got[1][1][1]) and not np.array_equal(got[0][0][7], params[7])
    want_p, want_b = br.sbmvb_run(data, conv, 1.0, PRI, BPRI, params, blk, 4, labels_every=2)
    assert np.allclose(m[3], want_b[0], rtol=0.0, atol=1e-9)
    # SVI counts its own global steps: a step without a sweep leaves m bit for bit (the blend skips it) and moves the tables
    kw = dict(batch_bins=256, delay=1.0, forgetting=0.6, blocks=np.array([0, 2, 1], dtype=np.int32))
    br.put(proc, params, blk)
    nhp.svi_(proc, ds, nsteps=1, **kw)
    one = br.get(proc)
    assert np.array_equal(one[1][0], blk[0]) and not np.array_equal(one[1][1], blk[1])
    nhp.svi_(proc, ds, nsteps=1, step0=1, **{**kw, "blocks": kw["blocks"][1:]})
    two = br.get(proc)
    assert not np.array_equal(two[1][0], blk[0])
    nhp.svi_(proc, ds, nsteps=1, step0=2, **{**kw, "blocks": kw["blocks"][2:]})
    assert np.array_equal(br.get(proc)[1][0], two[1][0])
    want_p, want_b = br.sbmsvi_run(data, conv, 1.0, PRI, BPRI, params, blk, kw["blocks"], 256, 1.0, 0.6, labels_every=2)
    assert np.allclose(br.get(proc)[1][0], want_b[0], rtol=0.0, atol=1e-9)
    for g, w in zip(br.get(proc)[1][1:], want_b[1:]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    with pytest.raises(Exception, match="labels_every"):
        proc.network.labels_every = 0
        nhp.update_(proc, data, ds)


def test_svi_one_block_and_no_delay_is_update(nhp):
    shape = (130, 300, 2, 3, 5)
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    br.put(proc, params, blk)
    nhp.update_(proc, data, ds)
    want = br.get(proc)
    br.put(proc, params, blk)
    res = nhp.svi_(proc, ds, nsteps=1, batch_bins=shape[1], delay=0.0, forgetting=1.0)
    got = br.get(proc)
    assert res.step == 1 and len(res.trace[0]) == len(proc.variational_params())
    for g, w in zip(got[0] + got[1], want[0] + want[1]):
        assert np.allclose(g, w, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("shape,Tb", [((5, 700, 3, 7, 2), 256), ((130, 300, 2, 3, 5), 112)])
def test_svi_three_blocks_simplex_and_resume(nhp, shape, Tb):
    """Six steps over three blocks against the reference at the bounds of the netvb SVI test (tables rtol 1e-9; ρv through
    the logit's slope at that rtol plus the link layer's own bound; m to 1e-9 absolute, the block tables to rtol 1e-9); every
    row of m stays on the simplex; streamed equals resident; a run cut at step 2 and resumed with step0 is bit-equal."""
    N, T, B, L, K = shape
    proc, data, conv, params, blk, ds = setup(nhp, shape)
    nb = sr.n_blocks(T, Tb)
    assert nb == 3
    blocks = np.array([0, nb - 1, 1, nb - 1, 0, 0], dtype=np.int32)
    kw = dict(batch_bins=Tb, delay=1.0, forgetting=0.6)
    br.put(proc, params, blk)
    res = nhp.svi_(proc, ds, nsteps=6, blocks=blocks, **kw)
    got, gblk = br.get(proc)
    want5 = br.sbmsvi_run(data, conv, 1.0, PRI, BPRI, params, blk, blocks[:5], Tb, 1.0, 0.6)
    want, wblk = br.sbmsvi_run(data, conv, 1.0, PRI, BPRI, want5[0], want5[1], blocks[5:], Tb, 1.0, 0.6, step0=5)
    assert res.step == 6
    for g, w in zip(got[:7], want[:7]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    hat, hblk = br.sbmsvi_step(data, conv, 1.0, PRI, BPRI, want5[0], want5[1], int(blocks[5]), Tb, 1, 0.0, 1.0)
    slope = np.abs(digamma(hat[4]) - digamma(hat[2]) - np.log(hat[5] / hat[3]))
    av, bv = want5[1][1], want5[1][2]
    dnet = float(np.max(polygamma(1, av) * av + polygamma(1, bv) * bv)) * 1e-9 + 2 * K * float(np.max(np.abs(digamma(av) - digamma(bv)))) * 1e-9
    b = 0.25 * (slope * 1e-9 * hat[2] + dnet + 4 * (nr.measured_logit_error() + br.measured_net_error())) + 1e-9 * want[7]
    print(f"six SVI steps: max |Δρv| {float(np.max(np.abs(got[7] - want[7]))):.2e} (bound up to {float(b.max()):.2e}); "
          f"max |Δm| {float(np.max(np.abs(gblk[0] - wblk[0]))):.2e}")
    assert np.all(np.abs(got[7] - want[7]) <= b)
    assert np.allclose(gblk[0], wblk[0], rtol=0.0, atol=1e-9)
    for g, w in zip(gblk[1:], wblk[1:]):
        assert np.allclose(g, w, rtol=1e-9, atol=0.0)
    assert np.all(gblk[0] >= 0.0) and np.max(np.abs(gblk[0].sum(axis=1) - 1.0)) <= 8 * ULP * K
    br.put(proc, params, blk)
    nhp.svi_(proc, data, nsteps=6, blocks=blocks, streamed=True, **kw)
    sgot, sblk = br.get(proc)
    for g, w in zip(sgot + sblk, got + gblk):
        assert np.allclose(g, w, rtol=1e-12, atol=1e-15)
    br.put(proc, params, blk)
    first = nhp.svi_(proc, ds, nsteps=2, seed=3, **kw)
    nhp.svi_(proc, ds, nsteps=4, seed=3, step0=first.step, trace_every=2, **kw)
    cut = br.get(proc)
    br.put(proc, params, blk)
    nhp.svi_(proc, ds, nsteps=6, seed=3, **kw)
    whole = br.get(proc)
    for g, w in zip(whole[0] + whole[1], cut[0] + cut[1]):
        assert np.array_equal(g, w)


def test_the_lds_limit_is_reported_before_any_launch(nhp):
    N, T, B, L, K = 400, 32, 1, 2, 64
    data = nr.counts(N, T, 3)
    proc = br.make_process(nhp, N, B, L, K, seed=1)
    blk = br.random_blocks(N, K)
    start = nr.random_start(N, B)[:8]
    br.put(proc, start, blk)
    ds = nhp.convolve(proc, data)
    need = 8 * (N * K + 2 * N + 20 * 64)
    for call in (lambda: nhp.update_(proc, data, ds), lambda: nhp.svi_(proc, ds, nsteps=1, batch_bins=16)):
        with pytest.raises(NotImplementedError, match=str(need)):
            call()
        after = br.get(proc)
        for g, w in zip(after[0] + after[1], tuple(start) + tuple(blk)):
            assert np.array_equal(g, w)
    bad = (blk[0] * 1.001,) + blk[1:]
    br.put(proc, start, bad)
    with pytest.raises(Exception, match="sums to"):
        nhp.update_(proc, data, ds)


def test_recovery_labels_as_the_reference(nhp):
    """The planted two-block problem of the host test: the device's argmax mv is the reference's for every node, and after
    variational_mean_ the log-likelihood of the fit is finite."""
    r = br.RECOVERY
    data, A, z, start, params, blk = br.recovery_reference()
    proc = br.make_process(nhp, r["N"], r["B"], r["L"], 2, priors=r["priors"], bpri=r["bpri"], seed=1)
    proc.network.variational_init_(seed=r["init_seed"], sharpness=r["sharpness"], labels_every=r["labels_every"])
    assert np.array_equal(proc.network.mv, start[0])
    nr.put(proc, nr.ones_start(r["N"], r["B"])[:8] + (1.0, 1.0))
    proc.network.αv, proc.network.βv = start[1].copy(), start[2].copy()
    res = nhp.vb_(proc, data, max_steps=r["steps"], keep_trace=False)
    got = np.argmax(proc.network.mv, axis=1)
    print(got, np.round(np.max(proc.network.mv, axis=1), 3), f"max |Δm| against the reference {float(np.max(np.abs(proc.network.mv - blk[0]))):.2e}")
    assert res.step == r["steps"]
    assert np.array_equal(got, np.argmax(blk[0], axis=1)) and br.same_partition(got, z)
    nhp.variational_mean_(proc)
    net = proc.network
    assert np.array_equal(net.z, got) and np.isclose(net.π.sum(), 1.0) and np.allclose(net.ρ, net.αv / (net.αv + net.βv))
    assert np.array_equal(proc.adjacency_matrix, (proc.weights.ρv > 0.5).astype(np.float64))
    ll = nhp.loglikelihood(proc, data)
    assert np.isfinite(ll)
