"""The latent distance network model restated in plain numpy, for tests/test_latent_host.py (which holds it to brute force)
and tests/test_latent_gpu.py (which replays the device's slice steps against it).

    z_n ~ N(0, σ² I_D),  b ~ N(μb, σb²),  η[p,c] = b - ‖z_p - z_c‖²,  A[p,c] ~ Bernoulli(1 / (1 + exp(-η[p,c])))

A slice step reads its draws as [normals; u0; u1..u100] and follows the reference's elliptical_slice
(src/baselines.jl:287-326)."""
import math

import numpy as np

MAX_ATTEMPTS = 100
TWO_PI = 2 * np.pi


def softplus(eta):
    return max(eta, 0.0) + math.log1p(math.exp(-abs(eta)))


def loglik(A, z, b):
    """Σ_{p,c} A[p,c]·η[p,c] - softplus(η[p,c]) over all N² entries, in loops."""
    N = len(z)
    total = 0.0
    for p in range(N):
        for c in range(N):
            eta = b - sum((z[p][d] - z[c][d]) ** 2 for d in range(len(z[p])))
            total += A[p, c] * eta - softplus(eta)
    return total


def conditional(A, z, b, n, zn=None):
    """L_n(zn) = Σ_{j≠n} s_nj·η_j - 2·softplus(η_j), η_j = b - ‖zn - z_j‖², s_nj = A[n,j] + A[j,n], in loops."""
    zn = z[n] if zn is None else zn
    total = 0.0
    for j in range(len(z)):
        if j == n:
            continue
        eta = b - sum((zn[d] - z[j][d]) ** 2 for d in range(len(zn)))
        total += (A[n, j] + A[j, n]) * eta - 2.0 * softplus(eta)
    return total


def conditional_vec(A, z, b, n, zn=None):
    """conditional() with the loop over j as array operations (the host test holds the two together)."""
    zn = z[n] if zn is None else zn
    keep = np.arange(len(z)) != n
    eta = b - np.sum((zn[None, :] - z[keep]) ** 2, axis=1)
    s = (A[n] + A[:, n])[keep]
    return float(np.sum(s * eta - 2.0 * (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))))


def loglik_vec(A, z, b):
    eta = b - np.sum((z[:, None, :] - z[None, :, :]) ** 2, axis=2)
    return float(np.sum(A * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))))


def angles(us):
    """θ_1..θ_100 from u_1..u_100: a function of the uniforms alone (the bracket moves by the sign of the rejected angle)."""
    out = []
    th = TWO_PI * us[0]
    lo, hi = th - TWO_PI, th
    out.append(th)
    for u in us[1:]:
        if th < 0.0:
            lo = th
        else:
            hi = th
        th = lo + (hi - lo) * u
        out.append(th)
    return out


def ess_step(L, x, nu, u0, us):
    """One slice step on the log-likelihood L from the value x with the prior draw nu.  -> (new x, attempts, trace,
    margin): attempts = index 1..100 of the accepted candidate, 101 when all failed (x is kept); trace = [threshold,
    L(candidate 1), ..., L(candidate attempts)]; margin = the smallest |L - threshold| among them."""
    with np.errstate(divide="ignore"):
        thr = L(x) + (math.log(u0) if u0 > 0.0 else -math.inf)
    trace, margin = [thr], math.inf
    for k, th in enumerate(angles(us), start=1):
        cand = x * math.cos(th) + nu * math.sin(th)
        l = L(cand)
        trace.append(l)
        margin = min(margin, abs(l - thr))
        if l >= thr:
            return cand, k, trace, margin
    return x, MAX_ATTEMPTS + 1, trace, margin


def node_draws(draws, N, D, sweep, n):
    """The draws of node n's step (n = N: the offset's) in sweep `sweep` of a stream: (normals, u0, u[1..100])."""
    rs = N * (D + 101) + 102
    at = sweep * rs + n * (D + 101)
    dims = D if n < N else 1
    return draws[at:at + dims], draws[at + dims], draws[at + dims + 1:at + dims + 101]


def position_step(A, z, b, sigma, n, normals, u0, us, fast=True):
    cond = conditional_vec if fast else conditional
    return ess_step(lambda zn: cond(A, z, b, n, zn), z[n].copy(), sigma * np.asarray(normals), u0, us)


def offset_step(A, z, b, mu_b, sigma_b, normal, u0, us, fast=True):
    ll = loglik_vec if fast else loglik
    x, k, trace, margin = ess_step(lambda x: ll(A, z, mu_b + x), b - mu_b, sigma_b * normal, u0, us)
    return (mu_b + x if k <= MAX_ATTEMPTS else b), k, trace, margin


def sweep(A, z, b, sigma, mu_b, sigma_b, draws, sweep_index=0, do_offset=True, fast=True):
    """One resample: nodes 0..N-1 in order, then the offset.  -> (z, b, attempts [N+1], traces, margins)."""
    N, D = z.shape
    z = z.copy()
    att, traces, margins = [], [], []
    for n in range(N):
        z[n], k, t, m = position_step(A, z, b, sigma, n, *node_draws(draws, N, D, sweep_index, n), fast=fast)
        att.append(k); traces.append(t); margins.append(m)
    if do_offset:
        nrm, u0, us = node_draws(draws, N, D, sweep_index, N)
        b, k, t, m = offset_step(A, z, b, mu_b, sigma_b, nrm[0], u0, us, fast=fast)
        att.append(k); traces.append(t); margins.append(m)
    return z, b, att, traces, margins


def replay(A, z_old, z_new, b_old, case, draws, sweep_index=0, do_offset=True):
    """Every step of one device sweep against the reference at the state the device was in: the device's new positions
    for the nodes already visited, the old ones for the rest -- so one near-tie cannot cascade.
    -> (expected positions per node, expected b, attempts, traces, margins)."""
    N, D = z_old.shape
    want_z, att, traces, margins = np.empty_like(z_old), [], [], []
    for n in range(N):
        state = np.vstack([z_new[:n], z_old[n:]])
        want_z[n], k, t, m = position_step(A, state, b_old, case["sigma"], n, *node_draws(draws, N, D, sweep_index, n))
        att.append(k); traces.append(t); margins.append(m)
    want_b = b_old
    if do_offset:
        nrm, u0, us = node_draws(draws, N, D, sweep_index, N)
        want_b, k, t, m = offset_step(A, z_new, b_old, case["mu_b"], case["sigma_b"], nrm[0], u0, us)
        att.append(k); traces.append(t); margins.append(m)
    return want_z, want_b, att, traces, margins


# ---- the cases of tests/test_latent_gpu.py (the host test runs them all through this reference) ----------------------
def make_draws(rng, N, D, n_sweeps=1):
    out = []
    for _ in range(n_sweeps):
        for n in range(N + 1):
            out += [rng.standard_normal(D if n < N else 1), rng.uniform(size=101)]
    return np.concatenate(out)


def make_case(N, D, seed, A="random", b=0.5, z="random", diag=None, n_sweeps=1, sigma=1.0, mu_b=0.0, sigma_b=1.0):
    rng = np.random.default_rng(seed)
    if A == "random":
        Am = (rng.uniform(size=(N, N)) < 0.3).astype(np.float64)
    elif A == "upper":
        Am = np.triu(np.ones((N, N)), 1)
    else:
        Am = np.full((N, N), 1.0 if A == "ones" else 0.0)
    if diag is not None:
        Am[np.arange(N), np.arange(N)] = diag
    z0 = rng.standard_normal((N, D))
    if z == "far":                                                # two groups 100 apart: softplus underflows, links are present
        z0[:, 0] += np.where(np.arange(N) % 2 == 0, -50.0, 50.0)
    return {"N": N, "D": D, "A": Am, "z0": z0, "b0": float(b), "sigma": sigma, "mu_b": mu_b, "sigma_b": sigma_b,
            "draws": make_draws(rng, N, D, n_sweeps), "n_sweeps": n_sweeps}


SHAPES = [(1, 1), (2, 1), (3, 2), (31, 2), (33, 3), (63, 2), (65, 8), (255, 2), (257, 3)]


def decision_cases():
    out = {f"{N}x{D}": make_case(N, D, 7000 + 13 * N + D) for N, D in SHAPES}
    out["65x2-zeros"] = make_case(65, 2, 7101, A="zeros")
    out["65x2-ones"] = make_case(65, 2, 7102, A="ones")
    out["65x2-upper"] = make_case(65, 2, 7103, A="upper")
    out["33x2-diag0"] = make_case(33, 2, 7104, diag=0.0)
    out["33x2-diag1"] = make_case(33, 2, 7104, diag=1.0)          # the same case but for the diagonal
    out["33x2-far"] = make_case(33, 2, 7105, z="far")
    out["33x2-b+30"] = make_case(33, 2, 7106, b=30.0)
    out["33x2-b-30"] = make_case(33, 2, 7107, b=-30.0)
    return out


def stale_case():
    """Three sweeps in one call; a wide prior ellipse against positions near 0, so nearly every node moves far."""
    return make_case(65, 2, 7201, n_sweeps=3, sigma=2.0)


# ---- streams that steer a slice step (tests 3 and 4) --------------------------------------------------------------------
def steering_uniforms(fail):
    """u_1..u_100 whose first `fail` angles stay far from 0 (θ1 = π, then alternately near the lower and the upper end
    of the bracket, which loses a share `spread` of its width per step and keeps more than a fifth of it over all of
    them, so |θ| > 0.6) and whose next angle is ~0."""
    if fail == 0:
        return np.array([0.0] + [0.5] * (MAX_ATTEMPTS - 1))
    spread = min(0.05, 1.5 / fail)
    us = [0.5]
    while len(us) < fail:
        us.append(spread if len(us) % 2 == 1 else 1.0 - spread)
    if fail < MAX_ATTEMPTS:
        th = angles(us)
        lo, hi = th[0] - TWO_PI, th[0]
        for t in th:
            if t < 0.0:
                lo = t
            else:
                hi = t
        us.append(-lo / (hi - lo))
        us += [0.5] * (MAX_ATTEMPTS - len(us))
    return np.array(us[:MAX_ATTEMPTS])


def steered_case(fails_by_sweep, N=5, D=2):
    """All nodes at (1, .., 1), every link present, b = 1, prior draws 0 and u0 = 0.999: every candidate is the current value
    scaled by cos θ, which is strictly worse than the current value (the maximum of its conditional) by far more than
    -log u0 unless θ ~ 0.  fails_by_sweep[s][n] candidates fail at step n of sweep s (n = N: the offset's; 100: all)."""
    draws = []
    for fails in fails_by_sweep:
        for n in range(N + 1):
            draws += [np.zeros(D if n < N else 1), [0.999], steering_uniforms(fails[n])]
    return {"N": N, "D": D, "A": np.ones((N, N)), "z0": np.ones((N, D)), "b0": 1.0, "sigma": 1.0, "mu_b": 0.0, "sigma_b": 1.0,
            "draws": np.concatenate(draws), "n_sweeps": len(fails_by_sweep)}


def fallback_case():
    """Acceptances on either side of the batch edges: a position step's first batch holds candidates 1..7 and the later
    ones eight each, the offset step's 1..15 and sixteen each."""
    return steered_case([[6, 7, 8, 15, 16, 14], [23, 0, 40, 99, 1, 15], [2, 3, 4, 5, 6, 16], [0, 0, 0, 0, 0, 99]])


def exhaustion_case():
    return steered_case([[100, 0, 3, 100, 0, 100]])


# ---- test 6: the exact posterior at N = 2, D = 1 (and of b at N = 3) ----------------------------------------------------
POSTERIOR_SAMPLES = 1000
POSTERIOR_THIN = 20             # sweeps between kept samples of z0 - z1
OFFSET_THIN = 5                 # offset updates between kept samples of b
P_MIN = 1e-4                    # the threshold of tests/test_device_draws_gpu.py


def delta_cdf(s01, b, sigma, x):
    """CDF at x of δ = z0 - z1 | A under N(δ; 0, 2σ²)·exp(s01·η - 2·softplus(η)), η = b - δ², by quadrature."""
    grid = np.linspace(-12 * sigma, 12 * sigma, 200001)
    eta = b - grid ** 2
    dens = np.exp(-grid ** 2 / (4 * sigma ** 2) + s01 * eta - 2.0 * (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))))
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]))])
    return np.interp(x, grid, cdf / cdf[-1])


def offset_cdf(A, z, mu_b, sigma_b, x):
    """CDF at x of b | A, z under N(b; μb, σb²)·exp(loglik), by quadrature."""
    grid = np.linspace(mu_b - 12 * sigma_b, mu_b + 12 * sigma_b, 20001)
    d2 = np.sum((z[:, None, :] - z[None, :, :]) ** 2, axis=2)
    eta = grid[:, None, None] - d2[None]
    ll = np.sum(A[None] * eta - (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))), axis=(1, 2))
    logd = ll - (grid - mu_b) ** 2 / (2 * sigma_b ** 2)
    dens = np.exp(logd - logd.max())
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]))])
    return np.interp(x, grid, cdf / cdf[-1])


def posterior_cases():
    return {"linked": np.array([[0.0, 1.0], [1.0, 0.0]]), "unlinked": np.zeros((2, 2))}


def offset_posterior_case():
    rng = np.random.default_rng(77)
    z = rng.standard_normal((3, 2))
    A = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    return A, z, 0.3, 1.5                                          # A, z, μb, σb


# ---- test 7: two planted clusters --------------------------------------------------------------------------------------------
RECOVERY_SWEEPS = 150
RECOVERY_BURN = 50


def planted_case(seed=12, N=40, D=2, b=1.0):
    rng = np.random.default_rng(seed)
    truth = np.arange(N) % 2
    zt = 0.3 * rng.standard_normal((N, D))
    zt[:, 0] += np.where(truth == 0, -1.5, 1.5)
    eta = b - np.sum((zt[:, None, :] - zt[None, :, :]) ** 2, axis=2)
    A = (rng.uniform(size=(N, N)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return {"N": N, "D": D, "A": A, "truth": truth, "z_true": zt, "b_true": b, "z0": 0.1 * rng.standard_normal((N, D)), "b0": 0.0,
            "sigma": 2.0, "mu_b": 0.0, "sigma_b": 2.0}


def link_probability(z, b):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(np.sum((z[:, None, :] - z[None, :, :]) ** 2, axis=2) - b))


def cluster_gap(P, truth):
    """Mean link probability of within-cluster pairs minus that of between-cluster pairs (diagonal left out)."""
    same = truth[:, None] == truth[None, :]
    off = ~np.eye(len(truth), dtype=bool)
    return float(P[same & off].mean() - P[~same].mean())


def reference_recovery_gap(case, seed=5):
    """The numpy chain on the planted case: the gap of its posterior mean link-probability matrix."""
    rng = np.random.default_rng(seed)
    z, b = case["z0"].copy(), case["b0"]
    acc = np.zeros((case["N"], case["N"]))
    for s in range(RECOVERY_SWEEPS):
        z, b, _, _, _ = sweep(case["A"], z, b, case["sigma"], case["mu_b"], case["sigma_b"], make_draws(rng, case["N"], case["D"]))
        if s >= RECOVERY_BURN:
            acc += link_probability(z, b)
    return cluster_gap(acc / (RECOVERY_SWEEPS - RECOVERY_BURN), case["truth"])
