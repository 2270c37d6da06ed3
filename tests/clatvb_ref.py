"""numpy/scipy restatement of the variational fit of the continuous network process under a LATENT DISTANCE network, written
from its definition (include/nhp.h, nhp_cont_latvb_step / nhp_cont_latvb_run), not from the kernels, on top of
tests/cnetvb_ref.py (the process, its factors and pieces), which is imported and not copied.

A state is cnetvb_ref's dict (kappa, nu the slab's; kappa0, nu0; rho; na, nb unused) plus "lat" = (zv [N, D], bv) and, where a
step made it, "rungs" (the rung each ascent iteration took, -1: it stayed).  Priors are cnetvb_ref.priors(net=None) plus
"lpri" = (σ, μb, σb).

One step:  the factors of cnetvb_ref.update;  logit ρv = disc_netvb_ref.logit at net = η of the OLD (zv, bv);  J iterations of
the ascent of F at the NEW ρv, each taking the gradient, the ladder t_r = τ·4^(1-r) along it through the quadratic-in-t form of
the definition, and the best rung if it exceeds F at t = 0.

    KL_net = Σ [ρv ln ρv + (1-ρv) ln(1-ρv)] - (links + ln p(zv) + ln p(bv))                          (network_pieces)

`F_mp` and `logit_mp` are 50-digit twins of F and of the link logit; `measured_logit_error()` / `measured_F_error()` are this
file's own rounding errors against them on the shapes of the GPU tests.  Test code only."""
import math

import numpy as np

import cnetvb_ref as cr
import disc_netvb_ref as dn
import em_ref as er
import vb_ref as vr

LPRI = (1.3, 0.2, 1.5)                                              # (σ, μb, σb)
RUNGS = 8
# (N, M, T, D) of the one-step GPU test; the last one for exponential impulses only
SHAPES = [(3, 300, 30.0, 1), (70, 2000, 100.0, 3), (70, 2000, 100.0, 8), (300, 3000, 100.0, 2)]
EPS = 2.0 ** -52


def priors(lpri=LPRI, spike=cr.SPIKE, base=None):
    return dict(cr.priors(net=None, spike=spike, base=base), lpri=tuple(float(v) for v in lpri))


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def dist2(z):
    d = z[:, None, :] - z[None, :, :]
    return np.sum(d * d, axis=2)


def eta(z, b):
    """η[p, c] = b - ‖z_p - z_c‖² (symmetric; the diagonal is b)."""
    return b - dist2(z)


def link_terms(z, b, rho):
    return rho * eta(z, b) - softplus(eta(z, b))


def F(z, b, rho, lpri):
    """F(z, b) = Σ_pc [ρ η - softplus(η)] - ‖z‖²/(2σ²) - (b - μb)²/(2σb²), evaluated directly; math.fsum over the links."""
    s, mu, sb = lpri
    return math.fsum(link_terms(z, b, rho).ravel()) - math.fsum((z * z).ravel()) / (2.0 * s * s) - (b - mu) ** 2 / (2.0 * sb * sb)


def F_terms(z, b, rho, lpri):
    """Σ of the magnitudes of the terms F is added up from, η's own terms included (b and ‖Δz‖² cancel in it)."""
    s, mu, sb = lpri
    return float(np.sum(rho * (abs(b) + dist2(z)) + softplus(eta(z, b))) + np.sum(z * z) / (2.0 * s * s) + (b - mu) ** 2 / (2.0 * sb * sb))


def grad(z, b, rho, lpri):
    """(∂F/∂z [N, D], ∂F/∂b) by the formulas of the definition, C = ρ + ρᵀ."""
    s, mu, sb = lpri
    w = (rho + rho.T) - 2.0 * dn.sigmoid(eta(z, b))                 # w[n, j] = C[j, n] - 2 s(η_nj)
    gz = -2.0 * (np.sum(w, axis=1)[:, None] * z - w @ z) - z / (s * s)
    return gz, 0.5 * float(np.sum(w)) - (b - mu) / (sb * sb)


def ladder(N, sigma):
    tau = 1.0 / (N + 1.0 / (sigma * sigma))
    return np.array([tau * 4.0 ** (1 - r) for r in range(RUNGS)])


def ray(z, b, rho, lpri, gz, gb, ts):
    """(F at (z, b) + t·G for every t of ts, the magnitudes of the terms of each) through the quadratic-in-t form of the
    definition: one (a, bb, c) per pair."""
    s, mu, sb = lpri
    C = rho + rho.T
    dz, dg = z[:, None, :] - z[None, :, :], gz[:, None, :] - gz[None, :, :]
    a, bb, c = np.sum(dz * dz, axis=2), np.sum(dz * dg, axis=2), np.sum(dg * dg, axis=2)
    zz, zg, gg = float(np.sum(z * z)), float(np.sum(z * gz)), float(np.sum(gz * gz))
    out, mags = [], []
    for t in ts:
        bt = b + t * gb
        e = bt - (a + t * (2.0 * bb + t * c))
        quad = (zz + t * (2.0 * zg + t * gg)) / (2.0 * s * s)
        out.append(0.5 * math.fsum((C * e - 2.0 * softplus(e)).ravel()) - quad - (bt - mu) ** 2 / (2.0 * sb * sb))
        mags.append(0.5 * float(np.sum(C * (abs(b) + abs(t * gb) + a + abs(t) * 2.0 * np.abs(bb) + t * t * c) + 2.0 * softplus(e)))
                    + (zz + abs(t) * 2.0 * abs(zg) + t * t * gg) / (2.0 * s * s) + (bt - mu) ** 2 / (2.0 * sb * sb))
    return np.array(out), np.array(mags)


def ascent_iteration(z, b, rho, lpri, rung=None):
    """One iteration from (z, b): (z', b', rung taken, F at the 8 rungs and at t = 0, the terms' magnitudes of each).  With `rung`
    given that rung is taken instead of the best one (-1: stay): a replay."""
    gz, gb = grad(z, b, rho, lpri)
    ts = np.concatenate([ladder(z.shape[0], lpri[0]), [0.0]])
    Fs, mags = ray(z, b, rho, lpri, gz, gb, ts)
    if rung is None:
        best = int(np.argmax(Fs[:RUNGS]))                           # (argmax: the lowest index on ties)
        rung = best if Fs[best] > Fs[RUNGS] else -1
    if rung < 0:
        return z, b, -1, Fs, mags
    t = ts[rung]
    return z + t * gz, b + t * gb, int(rung), Fs, mags


def ascent(z, b, rho, lpri, J, rungs=None):
    """J iterations: (z', b', rungs taken, [F at t = 0 of every iteration])."""
    taken, cur = [], []
    for j in range(J):
        z, b, r, Fs, _ = ascent_iteration(z, b, rho, lpri, None if rungs is None else int(rungs[j]))
        taken.append(r)
        cur.append(Fs[RUNGS])
    return z, b, taken, cur


def logit(state_new, lat, q):
    """logit ρv at the NEW (κv, νv) and the OLD (zv, bv)."""
    return dn.logit(eta(*lat), cr.wpri(q), state_new["kappa0"], state_new["nu0"], state_new["nu"])


def update(model, stats, cnt, T, q, lat, J, rungs=None):
    """The update of every factor from the statistics taken at `model`, with `lat` the (zv, bv) of the state stepped from."""
    st = cr.update(model, stats, cnt, T, q, 1.0, 1.0)               # (q["net"] is None: every factor but ρv and the network)
    st["rho"] = dn.sigmoid(logit(st, lat, q))
    z, b, taken, _ = ascent(lat[0], lat[1], st["rho"], q["lpri"], J, rungs)
    st["lat"], st["rungs"] = (z, b), taken
    return st


def _xlogx(v):
    return cr._xlogx(v)


def network_pieces(lat, rho, lpri):
    """(Σ entropy of ρv, links, ln p(zv), ln p(bv)), the Gaussian log-densities with their normalising constants."""
    z, b = lat
    s, mu, sb = lpri
    ent = math.fsum((_xlogx(rho) + _xlogx(1.0 - rho)).ravel())
    links = math.fsum(link_terms(z, b, rho).ravel())
    lnz = -math.fsum((z * z).ravel()) / (2.0 * s * s) - 0.5 * z.size * math.log(2.0 * math.pi * s * s)
    lnb = -(b - mu) ** 2 / (2.0 * sb * sb) - 0.5 * math.log(2.0 * math.pi * sb * sb)
    return ent, links, lnz, lnb


def network_piece_terms(lat, rho, lpri):
    """Σ of the magnitudes of the terms each network piece is added up from (the rounded-terms allowance of the GPU tests)."""
    z, b = lat
    s, mu, sb = lpri
    ent = float(np.sum(np.abs(_xlogx(rho)) + np.abs(_xlogx(1.0 - rho))))
    links = float(np.sum(rho * (abs(b) + dist2(z)) + softplus(eta(z, b))))
    lnz = float(np.sum(z * z)) / (2.0 * s * s) + abs(0.5 * z.size * math.log(2.0 * math.pi * s * s))
    lnb = (b - mu) ** 2 / (2.0 * sb * sb) + abs(0.5 * math.log(2.0 * math.pi * sb * sb))
    return ent, links, lnz, lnb


def kl_net(lat, rho, lpri):
    ent, links, lnz, lnb = network_pieces(lat, rho, lpri)
    return ent - (links + lnz + lnb)


def pieces(state, cnt, T, q):
    """(E_q[compensator], KL_λ0, KL_W, KL_imp, KL_net) of a state."""
    return cr.pieces(state, cnt, T, q)[:4] + (kl_net(state["lat"], state["rho"], q["lpri"]),)


def step(model, pr, q, lat, J, exact=True):
    """One update from the surrogate (or guess) `model`: (new state, Σ log λ̃ at `model`, the E-step's statistics)."""
    stats = er.statistics(model, pr, exact)
    return update(model, stats, pr.cnt, pr.T, q, lat, J), vr.loglam(model, stats, pr), stats


def run(model, pr, q, steps, lat, J, exact=True):
    """`steps` updates from the guess `model` and the point estimate `lat`: (final state, [L_1 .. L_steps], [F at every state])."""
    dt_max = model.dt_max
    trace, Fs, state = [], [], None
    for k in range(steps + 1):
        stats = er.statistics(model, pr, exact)
        if state is not None:
            trace.append(vr.loglam(model, stats, pr) - math.fsum(pieces(state, pr.cnt, pr.T, q)))
            Fs.append(F(state["lat"][0], state["lat"][1], state["rho"], q["lpri"]))
        if k == steps:
            break
        state = update(model, stats, pr.cnt, pr.T, q, lat, J)
        lat = state["lat"]
        model = cr.surrogate(state, dt_max)
    return state, np.array(trace), np.array(Fs)


def z_vector(lat):
    return np.concatenate([np.asarray(lat[0], float).ravel(order="F"), [float(lat[1])]])


def lat_from_Z(Z, N, D):
    Z = np.asarray(Z, float)
    return Z[:-1].reshape((N, D), order="F").copy(), float(Z[-1])


def planes(state):
    """(S, R, Q, Z): cnetvb_ref's planes without the Bernoulli pair, and Z = [vec zv; bv], column-major."""
    S, R, Q = cr.planes(dict(state, na=1.0, nb=1.0))
    return S, R, Q[:-2], z_vector(state["lat"])


def from_planes(S, R, Q, Z, N, D, kind):
    st = cr.from_planes(S, R, np.concatenate([np.asarray(Q, float), [1.0, 1.0]]), N, kind)
    st["lat"] = lat_from_Z(Z, N, D)
    return st


def random_lat(N, D, seed):
    rng = np.random.default_rng(seed + 77)
    return 0.6 * rng.standard_normal((N, D)) / math.sqrt(D), 0.4


def random_state(N, D, kind, seed):
    """cnetvb_ref's random state (ρv uniform in [0.05, 0.95]) with random positions (‖z_p - z_c‖² of order 1 for every D) and
    bv = 0.4."""
    st = cr.random_state(N, kind, seed)
    st["lat"] = random_lat(N, D, seed)
    return st


def parity_problem(N, M, T, D, kind, dt_max, recursive=False, seed=1, J=3):
    """The one-step problem of the GPU tests: helpers.random_case(seed=3)'s events, a random state, its surrogate and the
    restated step with J ascent iterations from it.  Returns (state, pairs, new state, Σ log λ̃, statistics)."""
    from helpers import random_case
    c = random_case(N, M, T, kind, dt_max, seed=3)
    state = random_state(N, D, kind, seed)
    pr = er.Pairs(c["times"], c["nodes"], c["T"], N, dt_max, recursive=recursive and kind == "exponential")
    new, loglam, stats = step(cr.surrogate(state, dt_max), pr, priors(), state["lat"], J, exact=N <= 70)
    return state, pr, new, loglam, stats


# ---- 50-digit twins ------------------------------------------------------------------------------------------------------------

def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def eta_mp(z, b):
    """η in 50-digit arithmetic, float64 array out."""
    mp = _mp()
    N, D = z.shape
    Zm = [[mp.mpf(float(z[n, d])) for d in range(D)] for n in range(N)]
    out = np.empty((N, N))
    for p in range(N):
        for c in range(N):
            out[p, c] = float(mp.mpf(float(b)) - mp.fsum((Zm[p][d] - Zm[c][d]) ** 2 for d in range(D)))
    return out


def logit_mp(state_new, lat, q):
    """The link logit from 50-digit arithmetic: η and the rest each taken at 50 digits (disc_netvb_ref.logit_mp with
    ψ(1) - ψ(1) = 0 for its scalar), rounded to doubles and added -- one more rounding than a single 50-digit expression."""
    return eta_mp(*lat) + dn.logit_mp(1.0, 1.0, cr.wpri(q), state_new["kappa0"], state_new["nu0"])


def F_mp(z, b, rho, lpri):
    """F in 50-digit arithmetic (mpmath numbers throughout: N²·D products, so for small shapes), a float out."""
    mp = _mp()
    N, D = z.shape
    s, mu, sb = (mp.mpf(float(v)) for v in lpri)
    bm = mp.mpf(float(b))
    Zm = [[mp.mpf(float(z[n, d])) for d in range(D)] for n in range(N)]
    tot = mp.mpf(0)
    for p in range(N):
        for c in range(N):
            e = bm - mp.fsum((Zm[p][d] - Zm[c][d]) ** 2 for d in range(D))
            sp = (e if e > 0 else mp.mpf(0)) + mp.log1p(mp.exp(-abs(e)))
            tot += mp.mpf(float(rho[p, c])) * e - sp
    zz = mp.fsum(v * v for row in Zm for v in row)
    return float(tot - zz / (2 * s * s) - (bm - mu) ** 2 / (2 * sb * sb))


_LOGIT_ERR, _F_ERR = [], []


def measured_logit_error():
    """max |logit - logit_mp| over every link of SHAPES' first three, at the tables the restated step writes from the parity
    start and the positions it reads (both impulse families, Δtmax = 1.5).  Once per process."""
    if not _LOGIT_ERR:
        worst, q = 0.0, priors()
        for N, M, T, D in SHAPES[:3]:
            for kind in ("exponential", "logitnormal"):
                state, _, new, _, _ = parity_problem(N, M, T, D, kind, 1.5, J=0)
                worst = max(worst, float(np.max(np.abs(logit(new, state["lat"], q) - logit_mp(new, state["lat"], q)))))
        _LOGIT_ERR.append(worst)
    return _LOGIT_ERR[0]


def measured_F_error():
    """max over SHAPES' first three of |F - F_mp| / max(1, |F_mp|) at the parity start (exponential impulses).  Once per process."""
    if not _F_ERR:
        worst, q = 0.0, priors()
        for N, M, T, D in SHAPES[:3]:
            st = random_state(N, D, "exponential", 1)
            got, want = F(st["lat"][0], st["lat"][1], st["rho"], q["lpri"]), F_mp(st["lat"][0], st["lat"][1], st["rho"], q["lpri"])
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
        _F_ERR.append(worst)
    return _F_ERR[0]


# ---- recovery: a planted 12-node latent network ----------------------------------------------------------------------------------
# Three groups of four nodes at the corners of a triangle of side 2.2 in the plane, spread 0.25 inside a group, offset b = 1.5: a
# link inside a group has probability about 0.8, one across about 0.03.  Every present link has weight 0.12 (branching ratio
# below 0.6).  The start is the zero positions plus variational_init_'s 0.1·N(0, I) and says nothing about the planted groups.
RECOVERY = dict(N=12, D=2, T=1500.0, seed=7, steps=40, J=4, side=2.2, spread=0.25, b=1.5, w=0.12, lam0=0.25, theta=2.0, dt_max=3.0,
                w_guess=0.05, lpri=(1.5, 0.0, 2.0), spike=(0.3, 100.0), init_seed=0, scale=0.1)


def recovery_problem():
    """(times, nodes (1-based), T, A, planted link probabilities): the cluster representation of the process -- immigrants at
    rate λ0 per node, every event of node p with Poisson(W[p,c]) children on node c at Exponential(θ) lags below Δtmax."""
    r = RECOVERY
    rng = np.random.default_rng(r["seed"])
    N, T = r["N"], r["T"]
    corners = r["side"] * np.array([[0.0, 0.0], [1.0, 0.0], [0.5, math.sqrt(0.75)]])
    z = corners[np.arange(N) % 3] + r["spread"] * rng.standard_normal((N, 2))
    P = dn.sigmoid(eta(z, r["b"]))
    A = (rng.uniform(size=(N, N)) < P).astype(np.float64)
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
    return np.asarray(times)[order], np.asarray(nodes, dtype=np.int64)[order] + 1, T, A, P


def recovery_start():
    """variational_init_(seed, scale) from zero positions and b = 0: (zv, bv)."""
    r = RECOVERY
    return r["scale"] * np.random.default_rng(r["init_seed"]).standard_normal((r["N"], r["D"])), 0.0


def recovery_guess():
    """The guess in the device order [λ0; θ; W]."""
    r = RECOVERY
    NN = r["N"] ** 2
    return np.concatenate([np.full(r["N"], r["lam0"]), np.full(NN, r["theta"]), np.full(NN, r["w_guess"])])


_RECOVERY = []


def recovery_reference():
    """(times, nodes, T, A, planted probabilities, fitted state) of RECOVERY under the restatement; once per process."""
    if not _RECOVERY:
        r = RECOVERY
        times, nodes, T, A, P = recovery_problem()
        pr = er.Pairs(times, nodes, T, r["N"], r["dt_max"])
        model = er.from_vector(recovery_guess(), r["N"], "exponential", r["dt_max"])
        state, _, _ = run(model, pr, priors(r["lpri"], r["spike"]), r["steps"], recovery_start(), r["J"], exact=False)
        _RECOVERY.append((times, nodes, T, A, P, state))
    return _RECOVERY[0]


def recovered(rho, net_p, A, P):
    """(mean ρv over planted links, mean ρv over absent ones, correlation of the network's link probabilities with the planted)"""
    return float(np.mean(rho[A == 1.0])), float(np.mean(rho[A == 0.0])), float(np.corrcoef(net_p.ravel(), P.ravel())[0, 1])
