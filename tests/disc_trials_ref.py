"""Independent trials of one discrete process, restated on the host: the trials stacked along time, and Ŝ of the stack as the
concatenation of every trial convolved ALONE by the oracle -- the definition nhp_disc_dataset_set_trials gives the device
convolution.  Everything downstream of Ŝ is a function of rows, so the existing references are fed the stacked counts and
this Ŝ (or, where a reference convolves for itself, are evaluated per trial and added: the log-likelihood, its gradient,
the information blocks and their bin counts are sums over rows).

make_trials() draws the counts the way `make` of tests/test_discrete_gpu.py does and then puts at least one count into the
LAST bin of every trial, so that a convolution that runs across a boundary changes the first bins of the next trial."""
import numpy as np

import disc_grad_ref as gr
import disc_information_ref as ir


def stack(trials):
    """(counts [N, ΣT_r] int64, offsets int64 [R + 1])."""
    trials = [np.asarray(x, dtype=np.int64) for x in trials]
    offsets = np.concatenate([[0], np.cumsum([x.shape[1] for x in trials])]).astype(np.int64)
    return np.concatenate(trials, axis=1), offsets


def convolve(orc, trials, phi):
    """Ŝ [ΣT_r, N, B]: oracle.disc_convolve of every trial alone, one after the other."""
    return np.concatenate([orc.disc_convolve(np.asarray(x, dtype=np.int64), phi) for x in trials], axis=0)


def convolve_naive(orc, trials, phi):
    """What np.concatenate of the trials gives: the last bins of a trial excite the first bins of the next."""
    return orc.disc_convolve(stack(trials)[0], phi)


def convsum(conv):
    """Σ_t Ŝ[t, n, b] as [N, B].  The device adds in an order of its own (per thread, wave, workgroup, then the workgroups
    in turn), so the sum is compared bit for bit where every order gives the same bits: with the dyadic basis below."""
    return conv.sum(axis=0)


def _wave_sums(v):
    """nhp_wave_sum over [..., 64] lanes: inside a row of 16 the four DPP steps are a pairwise tree (lanes, quads, halves of
    8, the row); the four row sums are then added in turn.  Every + is one IEEE addition of two arrays."""
    v = v.reshape(v.shape[:-1] + (4, 4, 4))                       # [..., row, quad, lane]
    q = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])          # a quad
    r = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])          # a row of 16
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def convsum_device_order(conv, sparse):
    """Σ_t Ŝ[t, n, b] as [N, B] in the order the device adds, from the bits of Ŝ [T, N, B].

    sparse (k_disc_convolve[_trials] + k_disc_convsum_blocks): a workgroup owns 2048 bins; thread tid adds its four pairs
    (bins 2·(tid + 256·pp), + 1), pp in turn, each pair summed first; nhp_wave_sum; the four waves as (w0 + w1) + (w2 + w3);
    the workgroups in turn from 0.0.  dense (k_disc_convsum): thread tid adds the bins tid, tid + 256, … in turn from 0.0;
    nhp_wave_sum; the four waves in turn from 0.0.  Bins past T add +0.0, which changes no bit of a non-negative sum."""
    T, N, B = conv.shape
    x = np.ascontiguousarray(conv.transpose(1, 2, 0))             # [N, B, T]
    if sparse:
        nblk = -(-T // 2048)
        x = np.concatenate([x, np.zeros((N, B, nblk * 2048 - T))], axis=2).reshape(N, B, nblk, 4, 256, 2)
        pair = x[..., 0] + x[..., 1]                               # [N, B, blk, pp, tid]
        cs = ((pair[..., 0, :] + pair[..., 1, :]) + pair[..., 2, :]) + pair[..., 3, :]
        w = _wave_sums(cs.reshape(N, B, nblk, 4, 64))              # [N, B, blk, wave]
        part = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
        s = np.zeros((N, B))
        for k in range(nblk):
            s = s + part[..., k]
        return s
    rounds = -(-T // 256)
    x = np.concatenate([x, np.zeros((N, B, rounds * 256 - T))], axis=2).reshape(N, B, rounds, 256)
    cs = np.zeros((N, B, 256))
    for k in range(rounds):
        cs = cs + x[:, :, k, :]
    w = _wave_sums(cs.reshape(N, B, 4, 64))
    s = np.zeros((N, B))
    for k in range(4):
        s = s + w[..., k]
    return s


def dyadic_basis(L, B):
    """An L x B basis of small multiples of 2⁻⁶: with integer counts every Ŝ and every partial sum of them is a multiple of
    2⁻⁶ far below 2⁵³·2⁻⁶, hence exact, and Σ_t Ŝ has the same bits in any order of summation."""
    l, b = np.arange(1, L + 1)[:, None], np.arange(B)[None, :]
    return (1 + (3 * l + 5 * b) % 61) / 64.0


def make_trials(nhp, N, lengths, B, L, seed=0, rate=0.3, dt=1.0, network=False, zero=(), big=None):
    """-> (process, trials, lam0, W, theta, A or None).  `zero`: trials left without a single count; `big`: a trial that gets a
    count above 255 (the device then keeps no byte copy of the counts)."""
    rng = np.random.default_rng(seed)
    T = int(sum(lengths))
    data = rng.poisson(rate, (N, T)).astype(np.int64)
    W = rng.uniform(0.05, 0.3, (N, N)) / max(1, N // 4)
    th = rng.dirichlet(np.ones(B), (N, N)) if B > 1 else np.ones((N, N, 1))
    th[:, :, -1] = 1.0 - th[:, :, :-1].sum(axis=2)
    lam0 = rng.uniform(0.2, 1.0, N)
    A = (rng.uniform(size=(N, N)) < 0.6).astype(float)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    trials = []
    for r, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        x = data[:, a:b].copy()
        if r in zero:
            x[:] = 0
        else:
            x[r % N, -1] += 1 + r % 2                # the count a leak across the boundary carries into the next trial
            if big == r:
                x[(r + 1) % N, x.shape[1] // 2] = 300
        trials.append(x)
    base = nhp.DiscreteHomogeneousProcess(lam0, dt)
    imp = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    imp.θ, imp.γ, imp.γv, imp.nlags, imp.dt, imp.ϕ = th, 1.0, np.ones_like(th), L, dt, None
    wts = nhp.DenseWeightModel(W)
    if network:
        proc = nhp.DiscreteNetworkHawkesProcess(base, imp, wts, A, nhp.BernoulliNetworkModel(0.6, N), dt)
    else:
        proc = nhp.DiscreteStandardHawkesProcess(base, imp, wts, dt)
    return proc, trials, lam0, W, th, (A if network else None)


# The convolution cases of tests/test_disc_trials_gpu.py: name -> (N, lengths, B, L, rate, zero, big).  Every case but
# "dense_by_rule" (L > 64) is sparse enough for the bitmap kernel (tests/test_disc_trials_host.py checks the occupancy), and
# every one runs a second time with NHP_CONV_DENSE=1.
CONV_CASES = {
    "around_the_lags":   (6, [1, 1, 2, 6, 7, 8], 3, 7, 0.03, (), None),          # [1, 1, 2, L − 1, L, L + 1]; odd total
    "word_edges":        (2, [63, 64, 65, 127, 129], 2, 32, 0.05, (), None),     # boundaries around the bitmap's 64-bin words
    "tile_edges":        (2, [2047, 2048, 2049, 5], 2, 8, 0.05, (), None),       # a boundary before, on and after a 2048-bin tile edge
    "pair_straddles":    (4, [5, 7, 9, 11], 3, 4, 0.05, (), None),               # odd lengths, even total: a 16-byte pair over a boundary
    "odd_total":         (3, [10, 11, 12], 2, 4, 0.05, (), None),                # 8-byte stores
    "full_lag_mask":     (2, [70, 64, 66, 130], 3, 64, 0.04, (), None),          # L = 64: the mask is a whole word
    "dense_by_rule":     (2, [80, 70, 71, 150], 2, 70, 0.05, (), None),          # L = 70 takes the dense kernel
    "two_basis_passes":  (3, [20, 33, 47], 11, 9, 0.05, (), None),               # B = 11
    "no_byte_copy":      (3, [30, 41, 29], 2, 5, 0.05, (), 1),                   # a count above 255
    "an_empty_trial":    (3, [25, 30, 21], 2, 5, 0.05, (2,), None),              # the last trial holds no count at all
    "one_trial":         (3, [257], 2, 5, 0.05, (), None),                       # R = 1: the plain dataset
}


def conv_case(nhp, name):
    N, lengths, B, L, rate, zero, big = CONV_CASES[name]
    proc, trials, *_ = make_trials(nhp, N, lengths, B, L, seed=len(name) + N, rate=rate, zero=zero, big=big)
    return proc, trials


def leak_rows(lengths, L):
    """Per trial after the first: (first bin, bins the previous trial can reach) in stacked bins."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [(int(off[r]), int(min(L, lengths[r]))) for r in range(1, len(lengths))]


# ---- references that convolve for themselves: evaluated per trial, added over the trials ------------------------------------
class Sum:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def grad_reference(trials, phi, W, theta, dt, lam0):
    """disc_grad_ref.evaluate over the trials: λ stacked, ll, gradient and gradient scale added."""
    parts = [gr.evaluate(np.asarray(x), phi, W, theta, dt, lam0=lam0) for x in trials]
    return Sum(lam=np.concatenate([p.lam for p in parts], axis=0), conv=np.concatenate([p.conv for p in parts], axis=0),
               ll=sum(p.ll for p in parts), grad=sum(p.grad for p in parts), scale=sum(p.scale for p in parts))


def information_reference(trials, phi, W, theta, dt, lam0, kind, columns=None):
    """disc_information_ref.evaluate over the trials: blocks and their bin counts added (what check_blocks reads)."""
    parts = [ir.evaluate(dict(data=np.asarray(x), phi=phi, W=W, theta=theta, dt=dt, lam0=lam0), kind, columns=columns) for x in trials]
    return Sum(columns=parts[0].columns, blocks=sum(p.blocks for p in parts), n_t=sum(p.n_t for p in parts))
