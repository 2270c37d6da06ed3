"""Streaming convergence diagnostics, restated in numpy from the definitions in include/nhp.h (nhp_cont_model_diagnostics_*):
the same running planes, updated step by step in the header's order, and the same formulas at fetch, operation by operation.
Nothing here knows the library; the tests hold the library to it (and it to known answers: test_chain_diagnostics_host.py)."""
import numpy as np

FIELDS = ("entries", "undefined", "min_ess", "min_ess_index", "max_rhat", "max_rhat_index", "ess_below", "rhat_above", "max_mcse")


def pos(v):
    """pos(v) = v if v > 0, else 0 (so a NaN gives 0)."""
    return np.where(v > 0.0, v, 0.0)


class Accumulator:
    """The planes of one chain over `length` entries: S1, S2, B, SB, QB and the snapshots of (S1, S2)."""

    def __init__(self, length, batch_len, n_planned):
        assert batch_len >= 1 and n_planned >= 0
        self.b, self.planned, self.h, self.n = int(batch_len), int(n_planned), int(n_planned) // 2, 0
        self.S1, self.S2, self.B, self.SB, self.QB = (np.zeros(length) for _ in range(5))
        self.snapA = self.snapB = None

    def add(self, x):
        x = np.asarray(x, dtype=np.float64)
        self.S1 += x
        self.S2 += x * x
        self.B += x
        self.n += 1
        if self.n % self.b == 0:
            m = self.B / self.b
            self.SB += m
            self.QB += m * m
            self.B[:] = 0.0
        if self.n == self.h:
            self.snapA = (self.S1.copy(), self.S2.copy())
        if self.n == self.planned - self.h:
            self.snapB = (self.S1.copy(), self.S2.copy())
        return self

    def fetch(self):
        """-> dict: ess, mcse, rhat, undefined (bool) per entry, n, a, and the conditions of the three raw-sum subtractions
        (cond_s2, cond_bm, cond_w: the minuend over the difference) with the half means m1, m2 and W, for tolerances."""
        n, b, h = float(self.n), float(self.b), float(self.h)
        assert self.n >= 1
        a = float(self.n // self.b)
        nan = np.full(len(self.S1), np.nan)
        with np.errstate(divide="ignore", invalid="ignore"):
            d_s = pos(self.S2 - self.S1 * self.S1 / n)
            s2 = d_s / (n - 1.0)
            d_b = pos(self.QB - self.SB * self.SB / a) if a >= 2 else nan
            sbm = b * d_b / (a - 1.0) if a >= 2 else nan
            mcse = np.sqrt(sbm / n)
            ess = np.where(s2 == 0.0, np.nan, n * s2 / sbm)
            out = {"n": self.n, "a": int(a), "undefined": s2 == 0.0, "ess": ess, "mcse": mcse, "rhat": nan.copy(),
                   "cond_s2": self.S2 / d_s, "cond_bm": self.QB / d_b}
            if self.n == self.planned and self.h >= 2:
                A1, A2 = self.snapA
                B1, B2 = self.snapB
                m1, d1 = A1 / h, pos(A2 - A1 * A1 / h)
                v1 = d1 / (h - 1.0)
                c1, c2 = self.S1 - B1, self.S2 - B2
                m2, d2 = c1 / h, pos(c2 - c1 * c1 / h)
                v2 = d2 / (h - 1.0)
                W, dm = (v1 + v2) / 2.0, m1 - m2
                out["rhat"] = np.where(W == 0.0, np.nan, np.sqrt((h - 1.0) / h + dm * dm / (2.0 * W)))
                out.update(m1=m1, m2=m2, W=W, cond_w=(A2 + c2) / (d1 + d2))
        return out


def diagnose(samples, batch_len, n_planned=None):
    """Accumulate the rows of `samples` [n, length] one by one and fetch."""
    samples = np.asarray(samples, dtype=np.float64)
    if samples.ndim == 1:
        samples = samples[:, None]
    acc = Accumulator(samples.shape[1], batch_len, len(samples) if n_planned is None else n_planned)
    for x in samples:
        acc.add(x)
    return acc.fetch()


def summarize(d, ess_below, rhat_above, sl=slice(None)):
    """The summary of one group (entries `sl` of a fetch): undefined entries are counted and take no part in anything else,
    NaNs are excluded, ties go to the lower index, an extreme nobody defines is NaN with index -1."""
    ess, mcse, rhat, und = d["ess"][sl], d["mcse"][sl], d["rhat"][sl], d["undefined"][sl]
    s = dict.fromkeys(FIELDS, 0)
    s.update(entries=len(ess), undefined=int(und.sum()), min_ess=np.nan, min_ess_index=-1, max_rhat=np.nan, max_rhat_index=-1,
             max_mcse=np.nan)
    e = np.where(und, np.nan, ess)
    r = np.where(und, np.nan, rhat)
    m = np.where(und, np.nan, mcse)
    if np.any(~np.isnan(e)):
        s["min_ess_index"] = int(np.nanargmin(e))           # first occurrence: the lower index
        s["min_ess"] = float(e[s["min_ess_index"]])
        s["ess_below"] = int(np.sum(e[~np.isnan(e)] < ess_below))
    if np.any(~np.isnan(r)):
        s["max_rhat_index"] = int(np.nanargmax(r))
        s["max_rhat"] = float(r[s["max_rhat_index"]])
        s["rhat_above"] = int(np.sum(r[~np.isnan(r)] > rhat_above))
    if np.any(~np.isnan(m)):
        s["max_mcse"] = float(np.nanmax(m))
    return s


def tolerances(d, eps=np.finfo(np.float64).eps):
    """Relative tolerances per entry for ess, mcse and rhat of a fetch `d` against another evaluation of the same sums in
    another order or with fused operations: 16·n·ε·κ for a raw-sum difference of condition κ (a sum of n terms carries up to
    n·ε relative error in each operand; 16 covers the two operands, the division inside and the few operations behind).
      ess  = n·s²/σ²_bm          -> κ(s²) + κ(σ²_bm)
      mcse = √(σ²_bm/n)          -> κ(σ²_bm)/2
      rhat = √(c + dm²/(2W))     -> [t·κ(W) + dm·(|m1| + |m2|)/W] / (2·rhat²) with t = dm²/(2W): W's error and the
                                    difference of the half means (each a sum), propagated through the square root."""
    k = 16.0 * d["n"] * eps
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"ess": k * (d["cond_s2"] + d["cond_bm"]), "mcse": k * d["cond_bm"] / 2.0}
        if "W" in d:
            dm, W = d["m1"] - d["m2"], d["W"]
            t = dm * dm / (2.0 * W)
            out["rhat"] = k * (t * d["cond_w"] + np.abs(dm) * (np.abs(d["m1"]) + np.abs(d["m2"])) / W) / (2.0 * d["rhat"] ** 2)
        else:
            out["rhat"] = np.full(len(d["ess"]), np.nan)
    return out
