"""numpy/scipy restatement of the mean-field variational fit of the continuous network process under a STOCHASTIC BLOCK
network, written from its definition (include/nhp.h, nhp_cont_sbmvb_step / nhp_cont_sbmvb_run), not from the kernels, on top
of tests/cnetvb_ref.py (the process, its factors and pieces) and tests/disc_sbmvb_ref.py (the block model: net_term, tables,
sweep, network_bound and their brute-force and 50-digit twins).  Nothing here is copied from either: both are imported.

A state is cnetvb_ref's dict (kappa, nu the slab's; kappa0, nu0; rho; na, nb unused) plus "blk" = (m [N,K], αv [K,K], βv [K,K],
γv [K]).  Priors are cnetvb_ref.priors(net=None) plus "bpri" = (α, β, γ).

One step, numbered i:  the factors of cnetvb_ref.update;  logit ρv = disc_netvb_ref.logit at net = net_term(OLD m, αv, βv);
tables from the NEW ρv and the current m;  the sweep where i % labels_every == 0.

    KL_net = Σ [ρv ln ρv + (1-ρv) ln(1-ρv)] - (links + labels - KL_Dir - ΣKL_Beta)          (network_pieces, = network_bound)

`logit_mp` and `network_pieces_mp` are 50-digit twins of the link logit and of the five network pieces;
`measured_logit_error()` / `measured_piece_errors()` are this file's own rounding errors against them on the shapes of the
GPU tests.  Test code only."""
import math

import numpy as np
from scipy.special import betaln, digamma, gammaln

import cnetvb_ref as cr
import disc_netvb_ref as dn
import disc_sbmvb_ref as sb
import em_ref as er
import vb_ref as vr

BPRI = (1.5, 2.5, 1.2)                                              # (α, β, γ): tests/disc_sbmvb_ref.py's
# (N, M, T, K) of the one-step GPU test; the last one for exponential impulses only
SHAPES = [(3, 300, 30.0, 2), (70, 2000, 100.0, 3), (70, 2000, 100.0, 5), (300, 3000, 100.0, 2)]


def priors(bpri=BPRI, spike=cr.SPIKE, base=None):
    return dict(cr.priors(net=None, spike=spike, base=base), bpri=tuple(float(v) for v in bpri))


def logit(state_new, blk, q):
    """logit ρv at the NEW (κv, νv) and the OLD block state."""
    return dn.logit(sb.net_term(blk[0], blk[1], blk[2]), cr.wpri(q), state_new["kappa0"], state_new["nu0"], state_new["nu"])


def logit_mp(state_new, blk, q):
    """The same from 50-digit arithmetic: the network term and the rest each taken at 50 digits (disc_netvb_ref.logit_mp with
    ψ(1) - ψ(1) = 0 for its scalar), rounded to doubles and added -- one more rounding than a single 50-digit expression."""
    return sb.net_term_mp(blk[0], blk[1], blk[2]) + dn.logit_mp(1.0, 1.0, cr.wpri(q), state_new["kappa0"], state_new["nu0"])


def update(model, stats, cnt, T, q, blk, do_sweep):
    """The update of every factor from the statistics taken at `model`, with `blk` the block state stepped from."""
    st = cr.update(model, stats, cnt, T, q, 1.0, 1.0)               # (q["net"] is None: every factor but ρv and the network)
    rho = dn.sigmoid(logit(st, blk, q))
    st["rho"] = rho
    st["blk"] = sb.network_update(q["bpri"], blk, rho, do_sweep)
    return st


def network_pieces(blk, rho, bpri):
    """(Σ entropy of ρv, links, labels, KL_Dir, ΣKL_Beta), each one math.fsum over its terms, T1 and T0 at blk's own m."""
    m, av, bv, gv = blk
    a, b, g = bpri
    K = len(gv)
    E1, E0, Epi = sb.expectations(av, bv, gv)
    ent = math.fsum((cr._xlogx(rho) + cr._xlogx(1.0 - rho)).ravel())
    links = math.fsum((sb.omega_sum(m, rho) * E1 + sb.omega_sum(m, 1.0 - rho) * E0).ravel())
    labels = math.fsum((m * Epi[None, :] - cr._xlogx(m)).ravel())
    kl_dir = (gammaln(gv.sum()) - math.fsum(gammaln(gv))) - (gammaln(K * g) - K * gammaln(g)) + math.fsum((gv - g) * Epi)
    kl_beta = math.fsum((betaln(a, b) - betaln(av, bv) + (av - a) * E1 + (bv - b) * E0).ravel())
    return ent, links, labels, float(kl_dir), kl_beta


def network_piece_terms(blk, rho, bpri):
    """Σ of the magnitudes of the terms each network piece is added up from (the rounded-terms allowance of the GPU tests)."""
    m, av, bv, gv = blk
    a, b, g = bpri
    K = len(gv)
    E1, E0, Epi = sb.expectations(av, bv, gv)
    ent = float(np.sum(np.abs(cr._xlogx(rho)) + np.abs(cr._xlogx(1.0 - rho))))
    links = float(np.sum(sb.omega_sum(m, rho) * np.abs(E1) + sb.omega_sum(m, 1.0 - rho) * np.abs(E0)))
    labels = float(np.sum(np.abs(m * Epi[None, :]) + np.abs(cr._xlogx(m))))
    kl_dir = float(abs(gammaln(gv.sum())) + np.sum(np.abs(gammaln(gv))) + abs(gammaln(K * g) - K * gammaln(g)) + np.sum(np.abs((gv - g) * Epi)))
    kl_beta = float(np.sum(np.abs(gammaln(av + bv)) + np.abs(gammaln(av)) + np.abs(gammaln(bv)) + abs(betaln(a, b))
                           + np.abs((av - a) * E1) + np.abs((bv - b) * E0)))
    return ent, links, labels, kl_dir, kl_beta


def kl_net(blk, rho, bpri):
    ent, links, labels, kl_dir, kl_beta = network_pieces(blk, rho, bpri)
    return ent - (links + labels - kl_dir - kl_beta)


def pieces(state, cnt, T, q):
    """(E_q[compensator], KL_λ0, KL_W, KL_imp, KL_net) of a state."""
    return cr.pieces(state, cnt, T, q)[:4] + (kl_net(state["blk"], state["rho"], q["bpri"]),)


def step(model, pr, q, blk, do_sweep, exact=True):
    """One update from the surrogate (or guess) `model`: (new state, Σ log λ̃ at `model`, the E-step's statistics)."""
    stats = er.statistics(model, pr, exact)
    return update(model, stats, pr.cnt, pr.T, q, blk, do_sweep), vr.loglam(model, stats, pr), stats


def run(model, pr, q, steps, blk, labels_every=1, step0=0, exact=True):
    """`steps` updates from the guess `model` and the block state `blk`: (final state, [L_1 .. L_steps])."""
    dt_max = model.dt_max
    trace, state = [], None
    for k in range(steps + 1):
        stats = er.statistics(model, pr, exact)
        if state is not None:
            trace.append(vr.loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q)))
        if k == steps:
            break
        state = update(model, stats, pr.cnt, pr.T, q, blk, (step0 + k + 1) % labels_every == 0)
        blk = state["blk"]
        model = cr.surrogate(state, dt_max)
    return state, np.array(trace)


def planes(state):
    """(S, R, Q, B): cnetvb_ref's planes without the Bernoulli pair, and B = [vec αv; vec βv; γv; vec m], column-major."""
    S, R, Q = cr.planes(dict(state, na=1.0, nb=1.0))
    m, av, bv, gv = state["blk"]
    f = lambda v: np.asarray(v, float).ravel(order="F")             # noqa: E731
    return S, R, Q[:-2], np.concatenate([f(av), f(bv), f(gv), f(m)])


def blk_from_B(B, N, K):
    B = np.asarray(B, float)
    KK = K * K
    return (B[2 * KK + K:].reshape((N, K), order="F"), B[:KK].reshape((K, K), order="F"), B[KK:2 * KK].reshape((K, K), order="F"),
            B[2 * KK:2 * KK + K].copy())


def from_planes(S, R, Q, B, N, K, kind):
    st = cr.from_planes(S, R, np.concatenate([np.asarray(Q, float), [1.0, 1.0]]), N, kind)
    st["blk"] = blk_from_B(B, N, K)
    return st


def random_state(N, K, kind, seed):
    """cnetvb_ref's random state (ρv uniform in [0.05, 0.95]) with disc_sbmvb_ref's random block state."""
    st = cr.random_state(N, kind, seed)
    st["blk"] = sb.random_blocks(N, K, seed=11 + K)
    return st


def parity_problem(N, M, T, K, kind, dt_max, recursive=False, seed=1):
    """The one-step problem of the GPU tests: helpers.random_case(seed=3)'s events, a random state, its surrogate and the
    restated step WITH a sweep from it.  Returns (state, pairs, new state, Σ log λ̃, statistics)."""
    from helpers import random_case
    c = random_case(N, M, T, kind, dt_max, seed=3)
    state = random_state(N, K, kind, seed)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive and kind == "exponential")
    new, loglam, stats = step(cr.surrogate(state, dt_max), pr, priors(), state["blk"], True)
    return state, pr, new, loglam, stats


# ---- 50-digit twins of the five network pieces -----------------------------------------------------------------------------

def network_pieces_mp(blk, rho, bpri):
    """network_pieces in 50-digit arithmetic (mpmath numbers throughout: N²K products, so for small shapes), floats out."""
    mp = sb._mp()
    m, av, bv, gv = blk
    N, K = m.shape
    a, b, g = (mp.mpf(float(v)) for v in bpri)
    f = lambda x: mp.mpf(float(x))                                  # noqa: E731
    xlx = lambda x: x * mp.log(x) if x > 0 else mp.mpf(0)           # noqa: E731
    ent = mp.fsum(xlx(f(r)) + xlx(1 - f(r)) for r in rho.ravel())
    M = [[f(m[n, k]) for k in range(K)] for n in range(N)]
    R = [[f(rho[p, c]) for c in range(N)] for p in range(N)]
    U1 = [[mp.fsum(R[p][c] * M[c][l] for c in range(N) if c != p) for l in range(K)] for p in range(N)]
    U0 = [[mp.fsum((1 - R[p][c]) * M[c][l] for c in range(N) if c != p) for l in range(K)] for p in range(N)]
    links = kl_beta = mp.mpf(0)
    lnB = lambda x, y: mp.loggamma(x) + mp.loggamma(y) - mp.loggamma(x + y)      # noqa: E731
    for k in range(K):
        for l in range(K):
            x, y = f(av[k, l]), f(bv[k, l])
            ds = mp.digamma(x + y)
            e1, e0 = mp.digamma(x) - ds, mp.digamma(y) - ds
            t1 = mp.fsum(M[p][k] * (U1[p][l] + (R[p][p] if k == l else 0)) for p in range(N))
            t0 = mp.fsum(M[p][k] * (U0[p][l] + ((1 - R[p][p]) if k == l else 0)) for p in range(N))
            links += t1 * e1 + t0 * e0
            kl_beta += lnB(a, b) - lnB(x, y) + (x - a) * e1 + (y - b) * e0
    GV = [f(v) for v in gv]
    gs = mp.fsum(GV)
    Epi = [mp.digamma(v) - mp.digamma(gs) for v in GV]
    labels = mp.fsum(M[n][k] * Epi[k] - xlx(M[n][k]) for n in range(N) for k in range(K))
    kl_dir = (mp.loggamma(gs) - mp.fsum(mp.loggamma(v) for v in GV)) - (mp.loggamma(K * g) - K * mp.loggamma(g)) \
        + mp.fsum((GV[k] - g) * Epi[k] for k in range(K))
    return tuple(float(v) for v in (ent, links, labels, kl_dir, kl_beta))


_LOGIT_ERR, _PIECE_ERR = [], []


def measured_logit_error():
    """max |logit - logit_mp| over every link of SHAPES' first three, at the tables the restated step writes from the parity
    start and the random block state it reads (both impulse families, Δtmax = 1.5).  Once per process."""
    if not _LOGIT_ERR:
        worst, q = 0.0, priors()
        for N, M, T, K in SHAPES[:3]:
            for kind in ("exponential", "logitnormal"):
                state, _, new, _, _ = parity_problem(N, M, T, K, kind, 1.5)
                worst = max(worst, float(np.max(np.abs(logit(new, state["blk"], q) - logit_mp(new, state["blk"], q)))))
        _LOGIT_ERR.append(worst)
    return _LOGIT_ERR[0]


def measured_piece_errors():
    """max over SHAPES' first three of |network_pieces - network_pieces_mp| relative to max(1, |piece|), per piece, at the
    parity start and at the restated step from it (exponential impulses, Δtmax = 1.5).  Once per process."""
    if not _PIECE_ERR:
        worst, q = np.zeros(5), priors()
        for N, M, T, K in SHAPES[:3]:
            state, _, new, _, _ = parity_problem(N, M, T, K, "exponential", 1.5)
            for st in (state, new):
                got, want = network_pieces(st["blk"], st["rho"], q["bpri"]), network_pieces_mp(st["blk"], st["rho"], q["bpri"])
                worst = np.maximum(worst, [abs(g - w) / max(1.0, abs(w)) for g, w in zip(got, want)])
        _PIECE_ERR.append(worst)
    return _PIECE_ERR[0]


# ---- recovery: a planted two-block network ------------------------------------------------------------------------------------
# Dense inside a block (0.9), sparse across (0.05), every present link of weight 0.12 (branching ratio about 0.7).  The sweep
# runs at EVERY step: in continuous time this much data separates the links within some twenty steps, and from then on each
# sweep sharpens the labels -- by step 22 they are the planted halves.  With sweeps only every 2nd to 10th step the same inputs
# drift into one block instead (every node's m moves the same way before the halves part), so the schedule is part of the
# inputs.  The start labels alternate (the constructor's default) and say nothing about the planted halves.
RECOVERY = dict(N=12, T=1500.0, seed=5, steps=60, p_in=0.9, p_out=0.05, w=0.12, lam0=0.25, theta=2.0, dt_max=3.0, w_guess=0.05,
                bpri=(1.0, 1.0, 1.0), spike=(0.3, 100.0), init_seed=2, sharpness=0.3, labels_every=1)


def recovery_problem():
    """(times, nodes (1-based), T, A, planted labels): the cluster representation of the process -- immigrants at rate λ0 per
    node, every event of node p with Poisson(W[p,c]) children on node c at Exponential(θ) lags below Δtmax.  About 15 000 events."""
    r = RECOVERY
    rng = np.random.default_rng(r["seed"])
    N, T = r["N"], r["T"]
    z = sb.planted_labels(N)
    A = (rng.uniform(size=(N, N)) < np.where(z[:, None] == z[None, :], r["p_in"], r["p_out"])).astype(np.float64)
    W = r["w"] * A
    assert np.max(np.abs(np.linalg.eigvals(W))) < 0.9              # subcritical: the generations below die out
    times, nodes = [], []
    gen = [(t, n) for n in range(N) for t in rng.uniform(0.0, T, rng.poisson(r["lam0"] * T))]
    while gen:
        times += [t for t, _ in gen]
        nodes += [n for _, n in gen]
        nxt = []
        for t, p in gen:
            for c in np.nonzero(W[p])[0]:
                for _ in range(rng.poisson(W[p, c])):
                    lag = rng.exponential(1.0 / r["theta"])
                    if lag < r["dt_max"] and t + lag < T:
                        nxt.append((t + lag, int(c)))
        gen = nxt
    order = np.argsort(times, kind="stable")
    return np.asarray(times)[order], np.asarray(nodes, dtype=np.int64)[order] + 1, T, A, z


def recovery_start():
    r = RECOVERY
    return sb.init_blocks(np.arange(r["N"]) % 2, 2, r["bpri"], r["sharpness"], r["init_seed"])


def recovery_guess():
    """The guess in the device order [λ0; θ; W]."""
    r = RECOVERY
    NN = r["N"] ** 2
    return np.concatenate([np.full(r["N"], r["lam0"]), np.full(NN, r["theta"]), np.full(NN, r["w_guess"])])


_RECOVERY = []


def recovery_reference():
    """(times, nodes, T, A, planted labels, fitted state) of RECOVERY under the restatement; once per process (3 s)."""
    if not _RECOVERY:
        r = RECOVERY
        times, nodes, T, A, z = recovery_problem()
        pr = er.Pairs(times, nodes, T, r["N"], r["dt_max"])
        model = er.from_vector(recovery_guess(), r["N"], "exponential", r["dt_max"])
        state, _ = run(model, pr, priors(r["bpri"], r["spike"]), r["steps"], recovery_start(), r["labels_every"], exact=False)
        _RECOVERY.append((times, nodes, T, A, z, state))
    return _RECOVERY[0]


def recovered(m, rho, A, z):
    """(labels equal the planted partition up to relabelling, share of planted links with ρv > ½, share of absent ones with ρv < ½)"""
    return sb.same_partition(np.argmax(m, axis=1), z), float(np.mean(rho[A == 1.0] > 0.5)), float(np.mean(rho[A == 0.0] < 0.5))
