"""Reference for mean-field VB and SVI on a discrete network Hawkes process whose network is a stochastic block model
(DESIGN §3.21), on top of tests/disc_netvb_ref.py (everything about the process itself is imported from there).

Model: z_n ~ Categorical(π), π ~ Dirichlet(γ 1_K), ρ[k,l] ~ Beta(α, β), A[p,c] ~ Bernoulli(ρ[z_p, z_c]), diagonal included.
Family: q(z_n) = Categorical(m[n,:]), q(π) = Dirichlet(γv), q(ρ[k,l]) = Beta(αv[k,l], βv[k,l]), q(A[p,c] = 1) = ρv[p,c].

    E1 = ψ(αv) - ψ(αv + βv),  E0 = ψ(βv) - ψ(αv + βv),  D = E1 - E0 = ψ(αv) - ψ(βv),  Eπ = ψ(γv) - ψ(Σγv)
    ω[p,c,k,l] = m[p,k] m[c,l] (p ≠ c),   ω[p,p,k,l] = m[p,k] δ_kl          (a node has ONE label)

One step is the step of disc_netvb_ref with (1) net[p,c] = Σ_kl ω D from the OLD m and tables in place of the scalar
ψ(αv) - ψ(βv); (2) αv = α + Σ_pc ω ρv, βv = β + Σ_pc ω (1 - ρv), γv = γ + Σ_n m from the NEW ρv and the current m;
(3) a sweep, node 0 .. N-1, m[n,:] = softmax(s) with the score of the issue, each node reading the current m of the others.

`blk` = (m [N,K], αv [K,K], βv [K,K], γv [K]); `bpri` = (α, β, γ); `params` = the first eight of disc_netvb_ref.
`net_term` is written as the library writes it (m·D first, then K products per link, the diagonal apart); `net_term_mp`
is the same in 50-digit arithmetic from (m, αv, βv), and `measured_net_error()` is this file's own error against it on the
GPU shapes (8.9e-16 where it was written).  The `_brute` functions loop over p, c, k, l.
"""
import numpy as np
from scipy.special import betaln, digamma, gammaln

import disc_netvb_ref as nr
import disc_svi_ref as sr


def expectations(av, bv, gv):
    s = digamma(av + bv)
    return digamma(av) - s, digamma(bv) - s, digamma(gv) - digamma(np.sum(gv))


def net_term(m, av, bv):
    D = digamma(av) - digamma(bv)
    net = (m @ D) @ m.T
    net[np.diag_indices_from(net)] = m @ np.diag(D)
    return net


def omega_sum(m, X):
    """Σ_pc ω[p,c,k,l] X[p,c] as a K x K matrix."""
    off = X - np.diag(np.diag(X))
    return m.T @ (off @ m) + np.diag(np.diag(X) @ m)


def tables(bpri, m, rho):
    return bpri[0] + omega_sum(m, rho), bpri[1] + omega_sum(m, 1.0 - rho), bpri[2] + m.sum(axis=0)


def softmax(s):
    e = np.exp(s - np.max(s))
    return e / e.sum()


def node_score(n, m, rho, E1, E0, Epi):
    mo = m.copy()
    mo[n] = 0.0
    r, q = rho[n, :], rho[:, n]
    return (Epi + rho[n, n] * np.diag(E1) + (1.0 - rho[n, n]) * np.diag(E0)
            + E1 @ (r @ mo) + E0 @ ((1.0 - r) @ mo) + E1.T @ (q @ mo) + E0.T @ ((1.0 - q) @ mo))


def node_update(n, m, rho, E1, E0, Epi):
    return softmax(node_score(n, m, rho, E1, E0, Epi))


def sweep(m, rho, av, bv, gv):
    E1, E0, Epi = expectations(av, bv, gv)
    m = m.copy()
    for n in range(m.shape[0]):
        m[n] = node_update(n, m, rho, E1, E0, Epi)
    return m


def simultaneous(m, rho, av, bv, gv):
    """All nodes at once from the old m: NOT coordinate ascent (the host test shows it can lower the bound)."""
    E1, E0, Epi = expectations(av, bv, gv)
    return np.array([node_update(n, m, rho, E1, E0, Epi) for n in range(m.shape[0])])


def network_update(bpri, blk, rho, do_sweep=True):
    """Items 2 and 3 of the step at a given ρv."""
    av, bv, gv = tables(bpri, blk[0], rho)
    return (sweep(blk[0], rho, av, bv, gv) if do_sweep else blk[0].copy()), av, bv, gv


def rho_hat(priors, blk, hats):
    return nr.sigmoid(nr.logit(net_term(blk[0], blk[1], blk[2]), priors[2:6], hats[2], hats[3], hats[5]))


def _finish(data, dt, priors, bpri, params, blk, ah, gh, r, do_sweep):
    hats = nr._finish(data, dt, priors, None, tuple(params[:8]) + (1.0, 1.0), ah, gh, None)
    rh = rho_hat(priors, blk, hats)
    bh = network_update(bpri, blk, rh, do_sweep)
    new = hats[:7] + (rh,)
    if r is None:
        return new, bh
    out = tuple(sr.blend(x, xh, r) for x, xh in zip(blk, bh))
    if not do_sweep:                                   # no sweep, no m̂: m stays as it is, bit for bit
        out = (blk[0].copy(),) + out[1:]
    return tuple(sr.blend(x, xh, r) for x, xh in zip(params[:8], new)), out


def sbmvb_step(data, conv, dt, priors, bpri, params, blk, do_sweep=True):
    a_stat, G = nr.block_stats(data, conv, params, 0, data.shape[1])
    return _finish(data, dt, priors, bpri, params, blk, priors[0] + a_stat, priors[6] + G, None, do_sweep)


def sbmvb_run(data, conv, dt, priors, bpri, params, blk, n, labels_every=1, step0=0):
    for i in range(step0 + 1, step0 + n + 1):
        params, blk = sbmvb_step(data, conv, dt, priors, bpri, params, blk, i % labels_every == 0)
    return params, blk


def sbmsvi_step(data, conv, dt, priors, bpri, params, blk, j, Tb, i, delay, forgetting, labels_every=1):
    T = data.shape[1]
    nblk = sr.n_blocks(T, Tb)
    t0, t1 = sr.block_bounds(T, Tb, j)
    a_stat, G = nr.block_stats(data, conv, params, t0, t1)
    a0, g = priors[0], priors[6]
    ah = a0 + nblk * ((a0 + a_stat) - a0)
    gh = g + nblk * ((g + G) - g)
    return _finish(data, dt, priors, bpri, params, blk, ah, gh, sr.rho(i, delay, forgetting), i % labels_every == 0)


def sbmsvi_run(data, conv, dt, priors, bpri, params, blk, blocks, Tb, delay, forgetting, step0=0, labels_every=1):
    for k, j in enumerate(blocks):
        params, blk = sbmsvi_step(data, conv, dt, priors, bpri, params, blk, int(j), Tb, step0 + k + 1, delay, forgetting, labels_every)
    return params, blk


def network_bound(blk, rho, bpri):
    """The network part of the ELBO at fixed ρv:  Σ_pc Σ_kl ω (ρv E1 + (1 - ρv) E0) + Σ_nk m (Eπ - ln m)
    - KL(Dir(γv) ‖ Dir(γ)) - Σ_kl KL(Beta(αv, βv) ‖ Beta(α, β)),  0 ln 0 = 0."""
    m, av, bv, gv = blk
    a, b, g = bpri
    K = len(gv)
    E1, E0, Epi = expectations(av, bv, gv)
    links = np.sum(omega_sum(m, rho) * E1 + omega_sum(m, 1.0 - rho) * E0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(m > 0.0, m * np.log(m), 0.0)
    labels = np.sum(m * Epi[None, :]) - np.sum(ent)
    kl_dir = (gammaln(gv.sum()) - gammaln(gv).sum()) - (gammaln(K * g) - K * gammaln(g)) + np.sum((gv - g) * Epi)
    kl_beta = np.sum(betaln(a, b) - betaln(av, bv) + (av - a) * digamma(av) + (bv - b) * digamma(bv) + (a - av + b - bv) * digamma(av + bv))
    return float(links + labels - kl_dir - kl_beta)


# ---- 50-digit twins ------------------------------------------------------------------------------------------------------

def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def net_term_mp(m, av, bv):
    """net[p,c] in 50-digit arithmetic from (m, αv, βv); float64 array out."""
    mp = _mp()
    N, K = m.shape
    D = [[mp.digamma(mp.mpf(float(av[k, l]))) - mp.digamma(mp.mpf(float(bv[k, l]))) for l in range(K)] for k in range(K)]
    M = [[mp.mpf(float(m[n, k])) for k in range(K)] for n in range(N)]
    MD = [[mp.fsum(M[n][k] * D[k][l] for k in range(K)) for l in range(K)] for n in range(N)]
    out = np.empty((N, N))
    for p in range(N):
        for c in range(N):
            if p == c:
                out[p, c] = float(mp.fsum(M[p][k] * D[k][k] for k in range(K)))
            else:
                out[p, c] = float(mp.fsum(MD[p][l] * M[c][l] for l in range(K)))
    return out


_FIX = 400                                             # bits of the fixed point the link sums are taken in (120 digits)


def _fixed(x):
    """Doubles as integers x·2^400 (object array): exact down to 2^-400, below that truncated."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.size, dtype=object)
    for i, v in enumerate(x.ravel()):
        n, d = float(v).as_integer_ratio()
        out[i] = (n << _FIX) // d
    return out.reshape(x.shape)


def bound_mp_state(blk, bpri):
    """What network_bound_mp needs of a state whatever ρv is: E1, E0 and the terms without ρv in 50-digit arithmetic, m in
    fixed point.  The O(K²) special functions are the slow part (0.7 s at K = 64), so a caller that evaluates one state at
    several ρv computes this once."""
    mp = _mp()
    m, av, bv, gv = blk
    N, K = m.shape
    a, b, g = (mp.mpf(float(v)) for v in bpri)
    f = lambda x: mp.mpf(float(x))                                                # noqa: E731
    AV = [[f(av[k, l]) for l in range(K)] for k in range(K)]
    BV = [[f(bv[k, l]) for l in range(K)] for k in range(K)]
    GV = [f(v) for v in gv]
    gs = mp.fsum(GV)
    ds = [[mp.digamma(AV[k][l] + BV[k][l]) for l in range(K)] for k in range(K)]
    da = [[mp.digamma(AV[k][l]) for l in range(K)] for k in range(K)]
    db = [[mp.digamma(BV[k][l]) for l in range(K)] for k in range(K)]
    Epi = [mp.digamma(GV[k]) - mp.digamma(gs) for k in range(K)]
    rest = mp.mpf(0)
    for n in range(N):
        for k in range(K):
            x = f(m[n, k])
            rest += x * Epi[k] - (x * mp.log(x) if x > 0 else 0)
    rest -= (mp.loggamma(gs) - mp.fsum(mp.loggamma(v) for v in GV)) - (mp.loggamma(K * g) - K * mp.loggamma(g))
    rest -= mp.fsum((GV[k] - g) * Epi[k] for k in range(K))
    lnB = lambda x, y: mp.loggamma(x) + mp.loggamma(y) - mp.loggamma(x + y)      # noqa: E731
    for k in range(K):
        for l in range(K):
            x, y = AV[k][l], BV[k][l]
            rest -= lnB(a, b) - lnB(x, y) + (x - a) * da[k][l] + (y - b) * db[k][l] + (a - x + b - y) * ds[k][l]
    E1 = [[da[k][l] - ds[k][l] for l in range(K)] for k in range(K)]
    E0 = [[db[k][l] - ds[k][l] for l in range(K)] for k in range(K)]
    return E1, E0, rest, _fixed(m)


def network_bound_mp(blk, rho, bpri, state=None):
    """network_bound in 50-digit arithmetic.  Σ_pc ω ρv and Σ_pc ω (1 - ρv) are taken in integers (fixed point, 2^-400),
    where N²·K products cost a fraction of what they cost in mpmath numbers; the K x K tables and the rest are mpmath."""
    mp = _mp()
    E1, E0, rest, Mi = state if state is not None else bound_mp_state(blk, bpri)
    K = Mi.shape[1]
    one = 1 << _FIX

    def omega_sum_fixed(Xi):                           # scale 2^(3·400)
        off = Xi.copy()
        dg = np.array([Xi[i, i] for i in range(Xi.shape[0])], dtype=object)
        for i in range(Xi.shape[0]):
            off[i, i] = 0
        out = Mi.T.dot(off.dot(Mi))
        d = dg.dot(Mi)
        for k in range(K):
            out[k, k] += d[k] * one
        return out

    Ri = _fixed(rho)
    S1, S0 = omega_sum_fixed(Ri), omega_sum_fixed(one - Ri)
    links = mp.fsum(mp.mpf(int(S1[k, l])) * E1[k][l] + mp.mpf(int(S0[k, l])) * E0[k][l] for k in range(K) for l in range(K))
    return mp.ldexp(links, -3 * _FIX) + rest


# ---- brute force: explicit loops over p, c, k, l -------------------------------------------------------------------------

def omega(m, p, c, k, l):
    return m[p, k] * m[c, l] if p != c else (m[p, k] if k == l else 0.0)


def net_term_brute(m, av, bv):
    N, K = m.shape
    out = np.zeros((N, N))
    for p in range(N):
        for c in range(N):
            for k in range(K):
                for l in range(K):
                    out[p, c] += omega(m, p, c, k, l) * ((digamma(av[k, l]) - digamma(av[k, l] + bv[k, l]))
                                                         - (digamma(bv[k, l]) - digamma(av[k, l] + bv[k, l])))
    return out


def tables_brute(bpri, m, rho):
    N, K = m.shape
    av, bv, gv = np.full((K, K), float(bpri[0])), np.full((K, K), float(bpri[1])), np.full(K, float(bpri[2]))
    for p in range(N):
        for c in range(N):
            for k in range(K):
                for l in range(K):
                    av[k, l] += omega(m, p, c, k, l) * rho[p, c]
                    bv[k, l] += omega(m, p, c, k, l) * (1.0 - rho[p, c])
    for n in range(N):
        for k in range(K):
            gv[k] += m[n, k]
    return av, bv, gv


def node_score_brute(n, m, rho, av, bv, gv):
    N, K = m.shape
    s = np.zeros(K)
    for k in range(K):
        e1 = lambda i, j: digamma(av[i, j]) - digamma(av[i, j] + bv[i, j])           # noqa: E731
        e0 = lambda i, j: digamma(bv[i, j]) - digamma(av[i, j] + bv[i, j])           # noqa: E731
        s[k] = digamma(gv[k]) - digamma(sum(gv)) + rho[n, n] * e1(k, k) + (1.0 - rho[n, n]) * e0(k, k)
        for c in range(N):
            if c == n:
                continue
            for l in range(K):
                s[k] += m[c, l] * (rho[n, c] * e1(k, l) + (1.0 - rho[n, c]) * e0(k, l))
                s[k] += m[c, l] * (rho[c, n] * e1(l, k) + (1.0 - rho[c, n]) * e0(l, k))
    return s


def network_bound_brute(blk, rho, bpri):
    m, av, bv, gv = blk
    N, K = m.shape
    a, b, g = bpri
    tot = 0.0
    for p in range(N):
        for c in range(N):
            for k in range(K):
                for l in range(K):
                    s = digamma(av[k, l] + bv[k, l])
                    tot += omega(m, p, c, k, l) * (rho[p, c] * (digamma(av[k, l]) - s) + (1.0 - rho[p, c]) * (digamma(bv[k, l]) - s))
    for n in range(N):
        for k in range(K):
            tot += m[n, k] * (digamma(gv[k]) - digamma(sum(gv))) - (m[n, k] * np.log(m[n, k]) if m[n, k] > 0 else 0.0)
    tot -= gammaln(sum(gv)) - sum(gammaln(v) for v in gv) - gammaln(K * g) + K * gammaln(g)
    tot -= sum((gv[k] - g) * (digamma(gv[k]) - digamma(sum(gv))) for k in range(K))
    for k in range(K):
        for l in range(K):
            x, y = av[k, l], bv[k, l]
            tot -= betaln(a, b) - betaln(x, y) + (x - a) * digamma(x) + (y - b) * digamma(y) + (a - x + b - y) * digamma(x + y)
    return float(tot)


# ---- starts, shapes and measured errors ----------------------------------------------------------------------------------

def random_blocks(N, K, seed=11):
    """A random block state: Dirichlet rows of m, tables in (0.5, 3)."""
    rng = np.random.default_rng(seed)
    m = rng.dirichlet(np.ones(K), N)
    return m, rng.uniform(0.5, 3.0, (K, K)), rng.uniform(0.5, 3.0, (K, K)), rng.uniform(0.5, 3.0, K)


# the shapes of tests/test_disc_sbmvb_gpu.py: (N, T, B, L, K)
SHAPES = [(3, 50, 2, 4, 1), (5, 700, 3, 7, 2), (5, 700, 3, 7, 3), (130, 300, 2, 3, 5), (300, 120, 2, 3, 2), (70, 120, 2, 3, 64)]
PRIORS = nr.PARITY_PRIORS
BPRI = (1.5, 2.5, 1.2)


def problem(N, T, B, L, K):
    data, conv, start = nr.parity_problem(N, T, B, L)
    return data, conv, start[:8], random_blocks(N, K, seed=11 + K)


_NET_ERR, _BOUND_ERR = [], {}


def measured_net_error():
    """max |net_term - net_term_mp| over every link of SHAPES at the random block state the first step reads.  Computed
    once per process (2.6 s: 1.1e5 links at 50 digits)."""
    if not _NET_ERR:
        worst = 0.0
        for (N, T, B, L, K) in SHAPES:
            m, av, bv, gv = random_blocks(N, K, seed=11 + K)
            worst = max(worst, float(np.max(np.abs(net_term(m, av, bv) - net_term_mp(m, av, bv)))))
        _NET_ERR.append(worst)
    return _NET_ERR[0]


def measured_bound_error(blk, rho, bpri, state=None):
    """|network_bound - network_bound_mp| at one state and one ρv: the reference's own rounding error there (`state`:
    bound_mp_state(blk, bpri), when the caller has it)."""
    return abs(float(network_bound_mp(blk, rho, bpri, state) - _mp().mpf(network_bound(blk, rho, bpri))))


# ---- recovery: a planted two-block network --------------------------------------------------------------------------------
# The sweep runs at every 10th step: from the all-ones start the links take some 40 steps to separate, and a sweep over
# labels while ρv is still flat collapses every node into one block, which no later step leaves (measured here: with
# labels_every = 1 all twelve nodes share a label after 10 steps, for every start tried).
RECOVERY = dict(N=12, T=20000, B=3, L=8, seed=3, steps=100, priors=(1.0, 1.0, 0.5, 100.0, 2.0, 20.0, 1.0), bpri=(1.0, 1.0, 1.0),
                p_in=0.9, p_out=0.05, init_seed=2, sharpness=0.3, labels_every=10)


def planted_labels(N):
    return (np.arange(N) >= N // 2).astype(np.int32)


def simulate_blocks(N=12, T=20000, B=3, L=8, seed=3, p_in=0.9, p_out=0.05, dt=1.0):
    """disc_netvb_ref.simulate_sparse with A drawn from two planted blocks: dense inside a block, sparse across."""
    rng = np.random.default_rng(seed)
    z = planted_labels(N)
    lam0 = rng.uniform(0.05, 0.15, N)
    P = np.where(z[:, None] == z[None, :], p_in, p_out)
    A = (rng.uniform(size=(N, N)) < P).astype(np.float64)
    W = rng.uniform(0.04, 0.12, (N, N)) * A
    theta = rng.dirichlet(np.ones(B), (N, N))
    phi = sr.basis_brute(L, B, dt)
    h = np.einsum("pc,pcb,lb->lpc", W, theta, phi) * dt
    data = np.zeros((N, T), dtype=np.int64)
    for t in range(T):
        lam = lam0 * dt
        for l in range(1, min(L, t) + 1):
            lam = lam + data[:, t - l] @ h[l - 1]
        data[:, t] = rng.poisson(lam)
    return data, A, z


def init_blocks(z, K, bpri, sharpness, seed):
    """StochasticBlockNetworkModel.variational_init_ in numpy."""
    N = len(z)
    m = np.full((N, K), (1.0 - sharpness) / K)
    m[np.arange(N), z] += sharpness
    if seed is not None:
        m = 0.9 * m + 0.1 * np.random.default_rng(seed).dirichlet(np.ones(K), N)
    m = m / m.sum(axis=1, keepdims=True)
    return m, np.full((K, K), float(bpri[0])), np.full((K, K), float(bpri[1])), np.full(K, float(bpri[2]))


_RECOVERY = []


def recovery_reference():
    """(data, A, planted labels, start blk, fitted params, fitted blk) of RECOVERY; computed once per process (9 s).  The
    start labels alternate (the constructor's default), so the start says nothing about the planted halves."""
    if not _RECOVERY:
        r = RECOVERY
        data, A, z = simulate_blocks(r["N"], r["T"], r["B"], r["L"], r["seed"], r["p_in"], r["p_out"])
        conv = nr.convolve(data, sr.basis_brute(r["L"], r["B"], 1.0))
        start = init_blocks(np.arange(r["N"]) % 2, 2, r["bpri"], r["sharpness"], r["init_seed"])
        params, blk = sbmvb_run(data, conv, 1.0, r["priors"], r["bpri"], nr.ones_start(r["N"], r["B"])[:8], start, r["steps"],
                                r["labels_every"])
        _RECOVERY.append((data, A, z, start, params, blk))
    return _RECOVERY[0]


def same_partition(z, want):
    """Equal up to the swap of the two labels."""
    return np.array_equal(z, want) or np.array_equal(1 - z, want)


# ---- the package's objects ---------------------------------------------------------------------------------------------------

def make_process(nhp, N, B, L, K, priors=PRIORS, bpri=BPRI, seed=0, z=None):
    proc = nr.make_process(nhp, N, B, L, priors, nr.PARITY_NET, seed=seed)
    proc.network = nhp.StochasticBlockNetworkModel(N, K, z=z, α=bpri[0], β=bpri[1], γ=bpri[2])
    return proc


def put(proc, params, blk):
    nr.put(proc, tuple(params[:8]) + (1.0, 1.0))
    net = proc.network
    net.mv, net.αv, net.βv, net.γv = (np.array(x, dtype=np.float64) for x in blk)
    net.vb_step = 0                                    # a fresh start: the sweep's schedule counts from here
    return proc


def get(proc):
    net = proc.network
    cp = lambda x: np.array(x, dtype=np.float64, copy=True)                       # noqa: E731
    return tuple(cp(x) for x in nr.get(proc)[:8]), (cp(net.mv), cp(net.αv), cp(net.βv), cp(net.γv))
