"""The streaming quantiles' definition (include/nhp.h: nhp_cont_model_quantiles_*) restated in numpy, vectorised over the
entries: the extended P² algorithm with K = 2m + 3 markers per entry.  Every expression is written operation by operation
as the header writes it -- IEEE fp64 + − × ÷ and int32 → fp64 conversions, each rounded on its own -- so that the GPU tests
can ask the kernel for the same bits."""
import numpy as np


def marker_probs(probs):
    """d_0 … d_{K−1}: d_{2j} = p_j, d_{2j+1} = (p_j + p_{j+1})/2 with p_0 = 0 and p_{m+1} = 1."""
    p = np.concatenate([[0.0], np.asarray(probs, dtype=np.float64), [1.0]])
    d = np.empty(2 * len(probs) + 3)
    d[0::2] = p
    d[1::2] = (p[:-1] + p[1:]) / 2.0
    return d


class P2:
    """Markers of `entries` independent series.  q [K, entries] fp64; pos [K, entries] int32 with pos[0] = 1 and
    pos[K − 1] = n kept explicitly; n values seen."""

    def __init__(self, probs, entries):
        self.probs = np.asarray(probs, dtype=np.float64)
        self.m = len(self.probs)
        self.K = 2 * self.m + 3
        self.d = marker_probs(self.probs)
        self.q = np.zeros((self.K, entries))
        self.pos = np.zeros((self.K, entries), dtype=np.int32)
        self.n = 0

    def add(self, x):
        x = np.asarray(x, dtype=np.float64)
        q, pos, K, n = self.q, self.pos, self.K, self.n
        if n < K:
            # into the sorted prefix q_0 … q_{n−1}, after equal values
            j = np.sum(q[:n] <= x, axis=0)
            for i in range(n, 0, -1):
                q[i] = np.where(i > j, q[i - 1], np.where(i == j, x, q[i]))
            q[0] = np.where(j == 0, x, q[0])
            self.n = n + 1
            if self.n == K:
                pos[:] = (np.arange(K, dtype=np.int32) + 1)[:, None]
            return
        lo = x < q[0]
        hi = ~lo & (x >= q[K - 1])
        k = np.zeros(x.shape[0], dtype=np.int64)
        for i in range(1, K - 1):
            k = np.where(q[i] <= x, i, k)
        k = np.where(lo, 0, np.where(hi, K - 2, k))
        q[0] = np.where(lo, x, q[0])
        q[K - 1] = np.where(hi, x, q[K - 1])
        for i in range(1, K - 1):
            pos[i] += (i > k).astype(np.int32)
        n += 1
        pos[K - 1] = n
        self.n = n
        nm1 = np.float64(n - 1)
        with np.errstate(all="ignore"):
            for i in range(1, K - 1):
                delta = (1.0 + nm1 * self.d[i]) - pos[i].astype(np.float64)
                up = (delta >= 1.0) & (pos[i + 1] - pos[i] > 1)
                dn = ~up & (delta <= -1.0) & (pos[i - 1] - pos[i] < -1)
                s = up.astype(np.int32) - dn.astype(np.int32)
                move = s != 0
                sd = s.astype(np.float64)
                a = (pos[i] - pos[i - 1]).astype(np.float64)
                b = (pos[i + 1] - pos[i]).astype(np.float64)
                c = (pos[i + 1] - pos[i - 1]).astype(np.float64)
                t1 = ((a + sd) * (q[i + 1] - q[i])) / b
                t2 = ((b - sd) * (q[i] - q[i - 1])) / a
                qn = q[i] + (sd / c) * (t1 + t2)
                qs = np.where(s > 0, q[i + 1], q[i - 1])
                ps = np.where(s > 0, pos[i + 1], pos[i - 1])
                den = np.where(move, ps - pos[i], 1).astype(np.float64)
                lin = q[i] + (sd * (qs - q[i])) / den
                inside = (q[i - 1] < qn) & (qn < q[i + 1])
                q[i] = np.where(move, np.where(inside, qn, lin), q[i])
                pos[i] += s

    def values(self):
        """[m, entries]: the estimate of p_j is q_{2j}; NaN while n < K."""
        if self.n < self.K:
            return np.full((self.m, self.q.shape[1]), np.nan)
        return self.q[2:self.K - 1:2].copy()

    def min(self):
        return self.q[0].copy() if self.n >= 1 else np.full(self.q.shape[1], np.nan)

    def max(self):
        return self.q[min(self.n, self.K) - 1].copy() if self.n >= 1 else np.full(self.q.shape[1], np.nan)

    def check_invariants(self):
        """Heights non-decreasing, positions strictly increasing from 1 to n (once the warm-up is over)."""
        top = min(self.n, self.K)
        assert np.all(np.diff(self.q[:top], axis=0) >= 0.0)
        if self.n >= self.K:
            assert np.all(self.pos[0] == 1) and np.all(self.pos[self.K - 1] == self.n)
            assert np.all(np.diff(self.pos, axis=0) >= 1)


def feed(probs, series, every=1):
    """P2 over series [steps, entries], every `every`-th row."""
    series = np.asarray(series, dtype=np.float64)
    if series.ndim == 1:
        series = series[:, None]
    p = P2(probs, series.shape[1])
    for x in series[::every]:
        p.add(x)
    return p


def prototype_series(n, entries=2000, seed=0):
    """The series the definition was tried on: AR(1) log-normal values, half of the entries multiplied by a 0/1 mask, plus
    a constant entry (the last)."""
    rng = np.random.default_rng(seed)
    phi = 0.8
    z = np.empty((n, entries))
    z[0] = rng.standard_normal(entries)
    for t in range(1, n):
        z[t] = phi * z[t - 1] + np.sqrt(1.0 - phi * phi) * rng.standard_normal(entries)
    x = np.exp(0.5 * z)
    mask = rng.integers(0, 2, (n, entries // 2)).astype(np.float64)
    x[:, :entries // 2] *= mask
    return np.concatenate([x, np.full((n, 1), 0.375)], axis=1)


def rank_error(series, estimates, probs):
    """|F̂_n(q̂) − p| per probability and entry, F̂_n the empirical distribution of the series, taken at the closest of its two
    one-sided values (a q̂ on an atom -- the exact zeros -- has every rank from P(x < q̂) to P(x <= q̂))."""
    series = np.asarray(series)
    out = np.empty(estimates.shape)
    for j, p in enumerate(probs):
        le = np.mean(series <= estimates[j], axis=0)
        lt = np.mean(series < estimates[j], axis=0)
        out[j] = np.where((lt <= p) & (p <= le), 0.0, np.minimum(np.abs(le - p), np.abs(lt - p)))
    return out
