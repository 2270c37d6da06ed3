"""Plain numpy restatement of the stochastic block network model's resample (csrc/sbm.hip): block counts, the label
conditionals and the sequential label sweep, plus the cases the host and the GPU tests share.

    z_n ~ Categorical(π), π ~ Dirichlet(γ), ρ[k,l] ~ Beta(α, β), A[p,c] ~ Bernoulli(ρ[z_p, z_c]) (diagonal included)

Conditional of z_n given every other label (out_l, in_l, cnt_l over m != n at their current labels):

    s_k = log π_k + Σ_l [out_l log ρ[k,l] + (cnt_l - out_l) log(1 - ρ[k,l])]
                  + Σ_l [in_l log ρ[l,k] + (cnt_l - in_l) log(1 - ρ[l,k])] + (A[n,n] ? log ρ[k,k] : log(1 - ρ[k,k]))
    p_k = exp(s_k - max s) / Σ;   z_n = first k with u_n <= p_0 + ... + p_k (the last block catches rounding)
"""
import itertools

import numpy as np


def counts(A, z, K):
    """L[k,l] = Σ A[p,c]·[z_p = k][z_c = l] (diagonal included) and the block sizes, as integers."""
    Z = np.zeros((len(z), K), dtype=np.int64)
    Z[np.arange(len(z)), z] = 1
    return Z.T @ (np.asarray(A) != 0).astype(np.int64) @ Z, Z.sum(axis=0)


def counts_loops(A, z, K):
    L, n = np.zeros((K, K), dtype=np.int64), np.zeros(K, dtype=np.int64)
    for p in range(len(z)):
        n[z[p]] += 1
        for c in range(len(z)):
            if A[p, c] != 0:
                L[z[p], z[c]] += 1
    return L, n


def conditional(A, z, n, rho, pi):
    """p(z_n = k | z_-n, A, ρ, π) for k = 0..K-1."""
    N, K = len(z), len(pi)
    lr, l1r = np.log(rho), np.log(1.0 - rho)
    other = np.arange(N) != n
    zo = z[other]
    out = np.bincount(zo, weights=(A[n, other] != 0), minlength=K)
    inn = np.bincount(zo, weights=(A[other, n] != 0), minlength=K)
    cnt = np.bincount(zo, minlength=K).astype(np.float64)
    s = np.log(pi) + lr @ out + l1r @ (cnt - out) + lr.T @ inn + l1r.T @ (cnt - inn)
    s = s + np.where(A[n, n] != 0, np.diag(lr), np.diag(l1r))
    p = np.exp(s - s.max())
    return p / p.sum()


def decide(p, u):
    """(block, margin): first k with u <= cumsum(p)_k, else the last; margin = distance of u to the nearest boundary that
    separates two blocks (the last block's upper boundary separates nothing)."""
    cum = np.cumsum(p)
    hit = np.nonzero(u <= cum)[0]
    k = int(hit[0]) if len(hit) else len(p) - 1
    margin = np.min(np.abs(u - cum[:-1])) if len(p) > 1 else np.inf
    return k, margin


def sweep(A, z, rho, pi, u):
    """One sequential sweep over n = 0..N-1; returns (new labels, conditionals [N, K], margins [N])."""
    z = np.array(z, dtype=np.int64)
    N, K = len(z), len(pi)
    probs, margins = np.empty((N, K)), np.empty(N)
    for n in range(N):
        probs[n] = conditional(A, z, n, rho, pi)
        z[n], margins[n] = decide(probs[n], u[n])
    return z, probs, margins


def replay(A, z_old, z_new, rho, pi, u):
    """The sweep's steps recomputed from the labels a sampler reports: only z_n changes at step n, so the state before it
    is z_new[:n] ++ z_old[n:].  Returns (conditionals, decisions, margins) of the reference at those states."""
    N, K = len(z_old), len(pi)
    probs, dec, margins = np.empty((N, K)), np.empty(N, dtype=np.int64), np.empty(N)
    for n in range(N):
        state = np.concatenate([z_new[:n], z_old[n:]]).astype(np.int64)
        probs[n] = conditional(A, state, n, rho, pi)
        dec[n], margins[n] = decide(probs[n], u[n])
    return probs, dec, margins


def log_joint(A, z, rho, pi):
    P = rho[np.ix_(z, z)]
    return np.sum(np.log(pi[z])) + np.sum(np.where(A != 0, np.log(P), np.log(1.0 - P)))


def conditional_by_enumeration(A, z, n, rho, pi):
    lj = np.array([log_joint(A, np.concatenate([z[:n], [k], z[n + 1:]]).astype(np.int64), rho, pi) for k in range(len(pi))])
    p = np.exp(lj - lj.max())
    return p / p.sum()


def all_labelings(N, K):
    return (np.array(t, dtype=np.int64) for t in itertools.product(range(K), repeat=N))


# ---- the cases of tests/test_sbm_gpu.py (the host test sweeps them all with this reference) -------------------------
SHAPES = [(1, 1), (2, 2), (3, 8), (63, 3), (64, 2), (65, 5), (130, 7), (96, 64), (257, 1)]
# beyond the issue's list: K = 20, 33 and 49 put live lanes in two, three and four rows of 16 (the cross-row halves of the
# sweep's wave maximum and prefix sum), and (189, 64) is the largest N at K = 64 whose tables fit the 160 KiB of LDS
# (8·N·K + 16·K·(K|1) + 16·ceil(N/32) + N + 16 = 163 629 of 163 840 bytes; N = 190 is refused)
SHAPES += [(40, 20), (40, 33), (50, 49), (189, 64)]


def make_case(N, K, seed, A="random", z="random", n_sweeps=1, assortative=False):
    rng = np.random.default_rng(seed)
    if A == "random":
        Am = (rng.uniform(size=(N, N)) < 0.3).astype(np.float64)
        Am[np.arange(N), np.arange(N)] = (rng.uniform(size=N) < 0.5).astype(np.float64)      # a non-trivial diagonal
    else:
        Am = np.full((N, N), 1.0 if A == "ones" else 0.0)
    z0 = rng.integers(0, K, N).astype(np.int32) if z == "random" else np.zeros(N, dtype=np.int32)
    if assortative:
        rho = np.full((K, K), 0.05) + 0.85 * np.eye(K)
        zt = rng.integers(0, K, N)
        Am = (rng.uniform(size=(N, N)) < rho[np.ix_(zt, zt)]).astype(np.float64)
        rho = rho * rng.uniform(0.9, 1.1, (K, K))
    else:
        rho = rng.uniform(1e-3, 1.0 - 1e-3, (K, K))
    pi = rng.dirichlet(np.full(K, 2.0))
    pi = pi / pi.sum()
    u = rng.uniform(size=n_sweeps * N)
    return {"N": N, "K": K, "A": Am, "z0": z0, "rho": rho, "pi": pi, "u": u, "n_sweeps": n_sweeps}


def decision_cases():
    """name -> case: the shapes of test 1, the all-zero / all-one matrices and the empty blocks at (65, 5)."""
    out = {f"{N}x{K}": make_case(N, K, 1000 + 17 * N + K) for N, K in SHAPES}
    out["65x5-zeros"] = make_case(65, 5, 2001, A="zeros")
    out["65x5-ones"] = make_case(65, 5, 2002, A="ones")
    out["65x5-block0"] = make_case(65, 5, 2003, z="zero")
    return out


def stale_case():
    """test 2: three sweeps in one call, strongly assortative ρ, random starting labels -- most nodes move."""
    return make_case(65, 5, 3001, n_sweeps=3, assortative=True)


def run_sweeps(case):
    """The reference over all of the case's sweeps: (labels after each sweep, conditionals, margins)."""
    N = case["N"]
    z, zs, probs, margins = case["z0"].astype(np.int64), [], [], []
    for s in range(case["n_sweeps"]):
        z, p, m = sweep(case["A"], z, case["rho"], case["pi"], case["u"][s * N:(s + 1) * N])
        zs.append(z.copy()); probs.append(p); margins.append(m)
    return zs, np.concatenate(probs), np.concatenate(margins)


# ---- test 6: recovery of a planted partition -------------------------------------------------------------------------
RECOVERY_SEED = 4
RECOVERY_ITERS = 60


def planted_case(seed=RECOVERY_SEED, N=60, K=3, rho_in=0.7, rho_out=0.05):
    rng = np.random.default_rng(seed)
    truth = np.repeat(np.arange(K), N // K)
    rho = np.full((K, K), rho_out) + (rho_in - rho_out) * np.eye(K)
    A = (rng.uniform(size=(N, N)) < rho[np.ix_(truth, truth)]).astype(np.float64)
    z0 = rng.integers(0, K, N).astype(np.int32)
    return {"N": N, "K": K, "A": A, "truth": truth, "z0": z0, "rng": rng}


def recovery_draws(case, z, rng, alpha=1.0, beta=1.0, gamma=1.0):
    """ρ | counts, π | sizes and the sweep's uniforms, drawn with numpy (handed to the reference and to the device alike)."""
    K = case["K"]
    L, n = counts(case["A"], z, K)
    rho = rng.beta(alpha + L, beta + np.outer(n, n) - L)
    rho = np.clip(rho, 1e-12, 1.0 - 1e-12)
    pi = rng.dirichlet(gamma + n)
    pi = pi / pi.sum()
    return rho, pi, rng.uniform(size=case["N"])


def same_partition(z, truth):
    """Equal up to a relabelling of the blocks."""
    fwd, back = {}, {}
    for a, b in zip(z, truth):
        if fwd.setdefault(int(a), int(b)) != int(b) or back.setdefault(int(b), int(a)) != int(a):
            return False
    return True
