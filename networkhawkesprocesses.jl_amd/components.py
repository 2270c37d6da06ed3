"""Plug-in components: the reference's Baseline / ImpulseResponse / Weights / Network types
with the same names, fields and constructor defaults, as plain parameter holders.

The reference dispatches a scalar method per (parent, child) pair on these types inside its
innermost loops; here they only carry arrays, which `lower()` in
continuous.py turns into the nhp_cont_model_desc blob the HIP kernels read.  Field names
keep the reference's Unicode spelling (θ, λ, Δtmax ...) so code written against the Julia
package reads the same.  Matrices are indexed [parent, child] (src/continuous.jl:303).

Host-side random draws (Gibbs conjugate updates, src/baselines.jl:72-77,
src/weights.jl:59-64, src/impulses.jl:68-73,204-214, src/networks.jl:65-78) use numpy's
Generator: statistically, not bitwise, the same as Julia's samplers.
"""
import collections

import numpy as np

from . import _lib
from ._lib import DomainError


def _fillna(x, value):
    """fillna!(X, value): src/utils/helpers.jl:18-25"""
    x = np.array(x, dtype=np.float64)
    x[np.isnan(x)] = value
    return x


# ------------------------------------------------------------------------------ baselines
class Baseline:
    pass


class HomogeneousProcess(Baseline):
    """HomogeneousProcess(λ[, α0, β0]) -- src/baselines.jl:27-39."""

    def __init__(self, λ, α0=1.0, β0=1.0):
        λ = np.array(λ, dtype=np.float64)
        if np.any(λ < 0):
            raise DomainError("HomogeneousProcess: intensity parameter λ must be non-negative")
        if not α0 > 0:
            raise DomainError("HomogeneousProcess: shape parameter α0 must be positive")
        if not β0 > 0:
            raise DomainError("HomogeneousProcess: rate parameter β0 must be positive")
        self.λ, self.α0, self.β0 = λ, float(α0), float(β0)

    def ndims(self):
        return len(self.λ)

    def params(self):
        return self.λ.copy()

    def params_(self, x):
        """params!: src/baselines.jl:44-50"""
        if len(x) != len(self.λ):
            raise ValueError("Parameter vector length does not match model parameter length.")
        self.λ[:] = x

    def intensity(self, node=None, time=0.0):
        """src/baselines.jl:110-118"""
        if time < 0:
            raise DomainError("time must be non-negative")
        return self.λ.copy() if node is None else self.λ[node - 1]

    def integrated_intensity(self, duration, node=None):
        """src/baselines.jl:98-108"""
        if duration < 0:
            raise DomainError("duration must be non-negative")
        return self.λ * duration if node is None else self.λ[node - 1] * duration

    def resample_(self, cnt0, duration, rng):
        """resample!: λ ~ Gamma(α0 + counts, 1/(β0 + T)) -- src/baselines.jl:72-77"""
        self.λ = rng.gamma(self.α0 + cnt0, 1.0 / (self.β0 + duration))
        return self.λ


# ---- Gaussian-process plumbing of the LGCP baseline (src/utils/gaussian.jl, src/utils/helpers.jl:1-11)
def posdef_(sigma, maxiter=3):
    """posdef!: shift the diagonal until the smallest eigenvalue is positive -- src/utils/helpers.jl:1-11"""
    sigma = np.array(sigma, dtype=np.float64)
    for _ in range(maxiter):
        eps = 2 * np.min(np.linalg.eigvalsh(sigma))
        if eps > 0.0:
            return sigma
        sigma[np.diag_indices_from(sigma)] -= eps
    print("WARNING: failed to make sigma positive definite")
    return sigma


class Kernel:
    def __call__(self, x, y=None):
        """kernel(x, y) on scalars; kernel(x::Vector) -> posdef!(Σ) -- src/utils/gaussian.jl:8-17"""
        if y is not None:
            return self.k(x, y)
        x = np.asarray(x, dtype=np.float64)
        return posdef_(self.k(x[:, None], x[None, :]))


class SquaredExponentialKernel(Kernel):
    """σ² exp(-((x-y)/η)²/2) -- src/utils/gaussian.jl:19-24"""

    def __init__(self, σ, η):
        self.σ, self.η = σ, η

    def k(self, x, y):
        return self.σ ** 2 * np.exp(-((x - y) / self.η) ** 2 / 2)


class OrnsteinUhlenbeckKernel(Kernel):
    """σ² exp(-|x-y|/η) -- src/utils/gaussian.jl:26-31"""

    def __init__(self, σ, η):
        self.σ, self.η = σ, η

    def k(self, x, y):
        return self.σ ** 2 * np.exp(-np.abs(x - y) / self.η)


class PeriodicKernel(Kernel):
    """σ² exp(-2 (sin(π|x-y|/θ)/η)²) -- src/utils/gaussian.jl:33-39"""

    def __init__(self, σ, η, θ):
        self.σ, self.η, self.θ = σ, η, θ

    def k(self, x, y):
        return self.σ ** 2 * np.exp(-2 * (np.sin(np.pi * np.abs(x - y) / self.θ) / self.η) ** 2)


class GaussianProcess:
    """GaussianProcess(kernel) / GaussianProcess(mu, kernel) -- src/utils/gaussian.jl:60-83"""

    def __init__(self, *args):
        self.mu, self.kernel = (np.zeros_like, args[0]) if len(args) == 1 else args

    def cov(self, x):
        return self.kernel(np.asarray(x, dtype=np.float64))

    def rand(self, x, rng, sigma=None):
        x = np.asarray(x, dtype=np.float64)
        sigma = self.cov(x) if sigma is None else sigma
        return np.asarray(self.mu(x), dtype=np.float64) + np.linalg.cholesky(sigma) @ rng.standard_normal(len(x))


def host_array(x, dtype):
    """A host numpy array of `x`: an array, a list or a torch tensor on any device (copied to the host)."""
    if type(x).__module__.startswith("torch") and hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def split_extract(data, parents, nnodes):
    """Events attributed to the baseline (parent node 0), split by node -- src/baselines.jl:227-238.  events / nodes may
    be torch tensors (copied to the host)."""
    events, nodes, duration = data
    events, nodes = host_array(events, np.float64), host_array(nodes, np.int64)
    parentnodes = np.asarray(parents[1], dtype=np.int64)
    out = []
    for node in range(1, nnodes + 1):
        idx = np.flatnonzero((nodes == node) & (parentnodes == 0)) if len(nodes) else np.array([], dtype=np.int64)
        out.append((events[idx], nodes[idx], duration))
    return out


class LogGaussianCoxProcess(Baseline):
    """LogGaussianCoxProcess(x, λ, Σ | kernel, m) -- src/baselines.jl:148-173: piecewise-linear
    intensity through (x, λ[k]) per node (src/utils/interpolation.jl), λ = exp(m + y), y ~ N(0, Σ)."""

    def __init__(self, x, λ, Σ=None, m=0.0):
        x = np.asarray(x, dtype=np.float64)
        if x[0] != 0.0:
            raise DomainError("Grid points x must start at 0.")
        self.x = x
        self.λ = [np.asarray(v, dtype=np.float64) for v in λ]
        for v in self.λ:
            if len(v) != len(x):
                raise ValueError("intensity vectors must match the grid")
        self.Σ = Σ(x) if isinstance(Σ, Kernel) else (None if Σ is None else np.asarray(Σ, dtype=np.float64))
        self.m = float(m)

    @classmethod
    def from_gp(cls, gp, m, T, n, k, rng):
        """LogGaussianCoxProcess(gp, m, T, n, k): random intensities on n+1 grid points -- src/baselines.jl:164-171"""
        x = np.linspace(0.0, T, n + 1)
        Σ = gp.cov(x)
        return cls(x, [np.exp(m + gp.rand(x, rng, sigma=Σ)) for _ in range(k)], Σ, m)

    def ndims(self):
        return len(self.λ)

    def length(self):
        """length(process) = x[end], the longest duration the process supports -- src/baselines.jl:173"""
        return float(self.x[-1])

    def params(self):
        return np.concatenate(self.λ)

    def params_(self, x):
        """params!: src/baselines.jl:175-188"""
        if len(x) != sum(len(v) for v in self.λ):
            raise ValueError("Parameter vector length does not match model parameter length.")
        G = len(self.x)
        self.λ = [np.array(x[k * G:(k + 1) * G], dtype=np.float64) for k in range(len(self.λ))]

    def integrated_intensity(self, duration=None):
        """integrate.(LinearInterpolator) -- src/baselines.jl:336; ignores duration"""
        dx = np.diff(self.x)
        return np.array([np.sum(0.5 * (y[:-1] + y[1:]) * dx) for y in self.λ])

    def candidate_loglikelihood(self, ds, Y, parentnodes=None):
        """loglikelihood(process, data, node, y) (src/baselines.jl:247-254) of latent curves Y [N, G],
        one per node, in a single GPU call.  The baseline-attributed events are those the latest
        parent sweep left on the device with `ds`, unless `parentnodes` is given."""
        from . import _lib
        lam = _lib.f64(np.exp(self.m + np.asarray(Y, dtype=np.float64)).ravel())
        pn = None if parentnodes is None else np.ascontiguousarray(parentnodes, dtype=np.int64)
        out = np.empty(self.ndims())
        _lib.check(_lib.lib().nhp_cont_lgcp_loglik(ds.ctx.h, ds.h, _lib.iptr(pn), _lib.dptr(self.x), len(self.x),
                                                   _lib.dptr(lam), _lib.dptr(out)), ds.ctx.h)
        return out

    def resample_(self, ds, rng, parentnodes=None, max_attempts=100):
        """resample!(process, data, parents; sampler=elliptical_slice) -- src/baselines.jl:212-245,287-326
        (Murray et al. 2010).  The reference runs one slice loop per node; the loops are independent,
        so they advance in lock step here and each round scores the pending candidates of all nodes
        with one GPU call."""
        if self.Σ is None:
            raise ValueError("LogGaussianCoxProcess needs Σ to be resampled")
        N, G = self.ndims(), len(self.x)
        L = np.linalg.cholesky(self.Σ)
        Y = np.log(np.vstack(self.λ)) - self.m                      # init_y: :241
        V = rng.standard_normal((N, G)) @ L.T                       # v ~ N(0, Σ)
        lly = self.candidate_loglikelihood(ds, Y, parentnodes) + np.log(rng.uniform(size=N))
        θ = 2 * np.pi * rng.uniform(size=N)
        θmin, θmax = θ - 2 * np.pi, θ.copy()
        Ynew = Y * np.cos(θ)[:, None] + V * np.sin(θ)[:, None]
        done = self.candidate_loglikelihood(ds, Ynew) >= lly
        attempts = 1
        while not done.all():
            if attempts >= max_attempts:
                raise RuntimeError("Elliptical slice sampling reached maximum attempts.")
            attempts += 1
            todo = ~done
            neg = θ < 0.0
            θmin = np.where(todo & neg, θ, θmin)
            θmax = np.where(todo & ~neg, θ, θmax)
            θ = np.where(todo, θmin + (θmax - θmin) * rng.uniform(size=N), θ)
            cand = Y * np.cos(θ)[:, None] + V * np.sin(θ)[:, None]
            Ynew = np.where(todo[:, None], cand, Ynew)              # accepted nodes keep their draw
            done = done | (todo & (self.candidate_loglikelihood(ds, Ynew) >= lly))
        self.λ = [np.exp(self.m + Ynew[k]) for k in range(N)]       # resample_node!: :242-244
        return [v.copy() for v in self.λ]


# ------------------------------------------------------------------------------ impulses
class ImpulseResponse:
    pass


class ExponentialImpulseResponse(ImpulseResponse):
    """ExponentialImpulseResponse(θ[, α, β, Δtmax]); 1-arg default Δtmax = Inf -- src/impulses.jl:30-37."""

    def __init__(self, θ, α=1.0, β=1.0, Δtmax=np.inf):
        self.θ = np.array(θ, dtype=np.float64)
        self.α, self.β, self.Δtmax = float(α), float(β), float(Δtmax)

    def size(self):
        return self.θ.shape[0]

    def params(self):
        return self.θ.ravel(order="F").copy()

    def params_(self, x):
        """params!: src/impulses.jl:43-51"""
        if len(x) != self.θ.size:
            raise ValueError("Parameter vector length does not match model parameter length.")
        n = self.size()
        self.θ = np.asarray(x, dtype=np.float64).reshape((n, n), order="F").copy(order="F")   # (column-major like the vector: a plain copy)

    def resample_(self, Mnm, Xnm, rng):
        """resample!: θ ~ Gamma(α + Mnm, 1/(β + Mnm·Xnm)) -- src/impulses.jl:68-73"""
        self.θ = rng.gamma(self.α + Mnm, 1.0 / (self.β + Mnm * Xnm))
        return self.θ


class LogitNormalImpulseResponse(ImpulseResponse):
    """LogitNormalImpulseResponse(μ, τ, [μμ, κμ, α0, β0,] Δtmax) -- src/impulses.jl:138-148."""

    def __init__(self, μ, τ, *args):
        if len(args) == 1:
            μμ, κμ, α0, β0, Δtmax = 1.0, 1.0, 1.0, 1.0, args[0]
        elif len(args) == 5:
            μμ, κμ, α0, β0, Δtmax = args
        else:
            raise TypeError("LogitNormalImpulseResponse(μ, τ, Δtmax) or (μ, τ, μμ, κμ, α0, β0, Δtmax)")
        self.μ = np.array(μ, dtype=np.float64)
        self.τ = np.array(τ, dtype=np.float64)
        self.μμ, self.κμ, self.α0, self.β0, self.Δtmax = float(μμ), float(κμ), float(α0), float(β0), float(Δtmax)

    def size(self):
        return self.μ.shape[0]

    def params(self):
        return np.concatenate([self.μ.ravel(order="F"), self.τ.ravel(order="F")])

    def params_(self, x):
        """params!: src/impulses.jl:154-162"""
        if len(x) != self.μ.size + self.τ.size:
            raise ValueError("Parameter vector length does not match model parameter length.")
        n = self.size()
        x = np.asarray(x, dtype=np.float64)
        self.μ = x[: n * n].reshape((n, n), order="F").copy(order="F")
        self.τ = x[n * n:].reshape((n, n), order="F").copy(order="F")

    def resample_(self, Mnm, Xnm, Vnm, rng):
        """resample!: normal-gamma conjugate draw -- src/impulses.jl:204-214"""
        with np.errstate(invalid="ignore", divide="ignore"):
            αnm = self.α0 + Mnm / 2
            βnm = _fillna(Vnm / 2 + Mnm * self.κμ / (Mnm + self.κμ) * (Xnm - self.μμ) ** 2 / 2, self.β0)
            self.τ = rng.gamma(αnm, 1.0 / βnm)
            κnm = self.κμ + Mnm
            μnm = _fillna((self.κμ * self.μμ + Mnm * Xnm) / (self.κμ + Mnm), self.μμ)
            σ = (1.0 / (κnm * self.τ)) ** 0.5
            self.μ = rng.normal(μnm, σ)
        return self.μ.copy(), self.τ.copy()


# ------------------------------------------------------------------------------ weights
class Weights:
    pass


class DenseWeightModel(Weights):
    """DenseWeightModel(W[, κ, ν, κv, νv]) -- src/weights.jl:47-55."""

    def __init__(self, W, κ=1.0, ν=1.0, κv=None, νv=None):
        self.W = np.array(W, dtype=np.float64, order="K")
        self.κ, self.ν = float(κ), float(ν)
        self.κv = np.ones_like(self.W) if κv is None else np.array(κv, dtype=np.float64)
        self.νv = np.ones_like(self.W) if νv is None else np.array(νv, dtype=np.float64)

    def size(self):
        return self.W.shape[0]

    def params(self):
        return self.W.ravel(order="F").copy()

    def params_(self, x):
        """params!: src/weights.jl:9-15"""
        if len(x) != self.W.size:
            raise ValueError("Parameter vector length does not match model parameter length.")
        self.W = np.asarray(x, dtype=np.float64).reshape(self.W.shape, order="F").copy(order="F")

    def resample_(self, Mn, Mnm, rng):
        """resample!: W ~ Gamma(κ + Mnm, 1/(ν + Mn[p])) -- src/weights.jl:59-64"""
        self.W = rng.gamma(self.κ + Mnm, 1.0 / (self.ν + Mn)[:, None] * np.ones_like(Mnm))
        return self.W

    def variational_params(self):
        return np.concatenate([self.κv.ravel(order="F"), self.νv.ravel(order="F")])


class SparseWeightModel(DenseWeightModel):
    """SparseWeightModel(W) -- src/weights.jl:104-127: the weights of a network process, with separate Gamma priors
    for absent (κ0, ν0) and present (κ1, ν1) links.  Its Gibbs update (src/weights.jl:133-139) is the dense one under
    the present-link prior -- W ~ Gamma(κ1 + Mnm, 1/(ν1 + Mn[p])) -- so every Gibbs kernel sees it as a DenseWeightModel
    with (κ, ν) = (κ1, ν1).  The variational methods of the reference throw on their wiring (undefined `p`, `ν1`, `ρ`,
    field-name mismatches: src/weights.jl:141-173); their intended semantics run on the GPU for a network
    process (update_): q(W | A = a) = Gamma(κv_a, νv_a) and q(A = 1) = ρv, an N x N matrix that starts as
    None, meaning "start from network.link_probability()"."""

    def __init__(self, W, κ0=1.0, ν0=1.0, κ1=1.0, ν1=1.0):
        super().__init__(W, κ1, ν1)
        self.κ0, self.ν0, self.κ1, self.ν1 = float(κ0), float(ν0), float(κ1), float(ν1)
        self.κv0, self.νv0 = np.ones_like(self.W), np.ones_like(self.W)
        self.κv1, self.νv1 = np.ones_like(self.W), np.ones_like(self.W)
        self.ρv = None

    def variational_params(self):
        """src/weights.jl:131"""
        return np.concatenate([v.ravel(order="F") for v in (self.κv0, self.νv0, self.κv1, self.νv1)])


# ------------------------------------------------------------------------------ networks
class Network:
    pass


class DenseNetworkModel(Network):
    """src/networks.jl:13-31: every link present."""

    def __init__(self, nnodes):
        self.nnodes = int(nnodes)

    def params(self):
        return np.array([])

    def link_probability(self):
        return np.ones((self.nnodes, self.nnodes))

    def rand(self, rng):
        return np.ones((self.nnodes, self.nnodes))

    def resample_(self, A, rng):
        return None

    def resample_links_(self, nlinks, size, rng):
        return None


class BernoulliNetworkModel(Network):
    """BernoulliNetworkModel(ρ, N) with Beta(α, β) prior -- src/networks.jl:34-78; (αv, βv) are the parameters of the
    variational Beta of ρ (src/networks.jl:54: both start at 1)."""

    def __init__(self, ρ, nnodes, α=1.0, β=1.0, αv=1.0, βv=1.0):
        self.ρ, self.α, self.β, self.nnodes = float(ρ), float(α), float(β), int(nnodes)
        self.αv, self.βv = float(αv), float(βv)

    def params(self):
        return np.array([self.ρ])

    def link_probability(self):
        return self.ρ * np.ones((self.nnodes, self.nnodes))

    def rand(self, rng):
        return (rng.uniform(size=(self.nnodes, self.nnodes)) < self.ρ).astype(np.float64)

    def resample_(self, A, rng):
        """resample!: ρ ~ Beta(α + ΣA, β + N² - ΣA) -- src/networks.jl:70-78"""
        return self.resample_links_(float(np.sum(A)), A.size, rng)

    def resample_links_(self, nlinks, size, rng):
        self.ρ = rng.beta(self.α + nlinks, self.β + size - nlinks)
        return self.ρ


class StochasticBlockNetworkModel(Network):
    """StochasticBlockNetworkModel(nnodes, nblocks, ρ, π, z; α, β, γ) -- the reference names the model and leaves it an
    empty stub (src/networks.jl, last lines).  Nodes belong to latent blocks and a link p → c exists with the
    probability of its pair of blocks:

        z_n ~ Categorical(π),  π ~ Dirichlet(γ·1_K),  ρ[k,l] ~ Beta(α, β),  A[p,c] ~ Bernoulli(ρ[z_p, z_c])

    for all N² entries (the diagonal is counted, as BernoulliNetworkModel counts it).  Labels are 0-based.  With one
    block this is BernoulliNetworkModel.  params() is [vec(ρ) column-major; π]; the labels are latent state, not
    parameters.  Block labels are identified only up to a permutation, so a chain can switch them: summaries of ρ, π
    and the labels over a chain are meaningful only as long as it did not.  The variational state (mv, αv, βv, γv) of
    update_ / vb_ / svi_ on a discrete network process is None until variational_init_ creates it."""

    def __init__(self, nnodes, nblocks, ρ=None, π=None, z=None, α=1.0, β=1.0, γ=1.0):
        self.nnodes, self.nblocks = int(nnodes), int(nblocks)
        K = self.nblocks
        if K < 1 or K > 64:
            raise ValueError("nblocks must lie in 1..64")
        self.α, self.β, self.γ = float(α), float(β), float(γ)
        if not (self.α > 0 and self.β > 0 and self.γ > 0):
            raise _lib.DomainError("the priors need α, β, γ > 0")
        self.ρ = np.full((K, K), 0.5) if ρ is None else np.array(ρ, dtype=np.float64).reshape((K, K))
        self.π = np.full(K, 1.0 / K) if π is None else np.array(π, dtype=np.float64).reshape(K)
        self.z = (np.arange(self.nnodes) % K).astype(np.int32) if z is None else np.array(z, dtype=np.int32).reshape(self.nnodes)
        if np.any(self.z < 0) or np.any(self.z >= K):
            raise _lib.DomainError(f"labels must lie in 0..{K - 1}")
        if not np.all((self.ρ > 0) & (self.ρ < 1)):
            raise _lib.DomainError("ρ must lie in the open interval (0, 1)")
        if not (np.all(self.π > 0) and abs(self.π.sum() - 1.0) <= 1e-12):
            raise _lib.DomainError("π must be positive and sum to 1")
        # the variational state: None until variational_init_ creates it
        self.mv = self.αv = self.βv = self.γv = None
        self.labels_every, self.vb_step = 1, 0

    def variational_init_(self, seed=None, sharpness=0.5, labels_every=1):
        """Create the variational state of update_ / vb_ / svi_: q(z_n) = Categorical(mv[n,:]), q(ρ[k,l]) = Beta(αv, βv),
        q(π) = Dirichlet(γv), with mv = sharpness·onehot(z) + (1 - sharpness)/K around the current labels, αv = α, βv = β,
        γv = γ.  With a seed every row of mv is mixed with a Dirichlet(1) draw (weight 0.1), which breaks ties between
        nodes that share a label.  Mean-field over labels has the uniform state as a fixed point: from mv ≡ 1/K every node
        sees the same blocks, every label scores the same and nothing ever moves.  sharpness = 0 is that state and is
        refused; nothing creates this state implicitly, which is why a freshly constructed model has no variational
        update.  The sweep over the labels runs at the steps whose global number is a multiple of labels_every, as in
        mcmc_: vb_step counts the steps update_ / vb_ have taken since this call (0 here), whether they came one per call
        or many, and svi_ counts with its own step0."""
        K, N = self.nblocks, self.nnodes
        if not 0.0 < sharpness <= 1.0:
            raise ValueError("variational_init!: sharpness must lie in (0, 1]; 0 is the symmetric fixed point of the label "
                             "update, from which no step moves")
        if int(labels_every) < 1:
            raise ValueError("labels_every must be a positive integer")
        m = np.full((N, K), (1.0 - sharpness) / K)
        m[np.arange(N), self.z] += sharpness
        if seed is not None:
            m = 0.9 * m + 0.1 * np.random.default_rng(seed).dirichlet(np.ones(K), N)
        self.mv = m / m.sum(axis=1, keepdims=True)
        self.αv, self.βv = np.full((K, K), self.α), np.full((K, K), self.β)
        self.γv = np.full(K, self.γ)
        self.labels_every, self.vb_step = int(labels_every), 0
        return self

    def has_variational_state(self):
        return self.mv is not None

    def variational_params(self):
        """[vec(αv); vec(βv); γv; vec(mv)], column-major"""
        return np.concatenate([np.asarray(self.αv).ravel(order="F"), np.asarray(self.βv).ravel(order="F"), np.asarray(self.γv),
                               np.asarray(self.mv).ravel(order="F")])

    def params(self):
        return np.concatenate([self.ρ.ravel(order="F"), self.π])

    def link_probability(self):
        return self.ρ[np.ix_(self.z, self.z)]

    def rand(self, rng):
        """Labels from π, then A from ρ[z_p, z_c]."""
        self.z = rng.choice(self.nblocks, size=self.nnodes, p=self.π).astype(np.int32)
        return (rng.uniform(size=(self.nnodes, self.nnodes)) < self.link_probability()).astype(np.float64)

    def block_counts(self, A, ctx=None):
        """(L, n): L[k,l] = Σ A[p,c]·[z_p = k][z_c = l] and the block sizes, from the GPU (exact integers)."""
        ctx = ctx or _lib.default_context()
        K, N = self.nblocks, self.nnodes
        Af = _lib.colmajor(A)
        z = np.ascontiguousarray(self.z, dtype=np.int32)
        L, n = np.empty(K * K, dtype=np.int64), np.empty(K, dtype=np.int64)
        _lib.check(_lib.lib().nhp_sbm_block_counts(ctx.h, _lib.dptr(Af), N, K, z.ctypes.data, L.ctypes.data, n.ctypes.data), ctx.h)
        return L.reshape((K, K), order="F"), n

    def resample_(self, A, rng, seed=None, step=0, ctx=None, labels=True):
        """resample!(network, A): block counts, ρ[k,l] ~ Beta(α + L, β + n_k n_l - L), π ~ Dirichlet(γ + n), then one
        collapsed-Gibbs sweep over the labels (node after node, each given the current labels of all others) -- all
        on the GPU (csrc/sbm.hip), keyed (seed, step).  Without a seed one is drawn from `rng`."""
        ctx = ctx or _lib.default_context()
        if seed is None:
            seed = int(rng.integers(0, 2 ** 63))
        K, N = self.nblocks, self.nnodes
        lib = _lib.lib()
        Af = _lib.colmajor(A)
        L, n = self.block_counts(A, ctx)
        Lf = np.ascontiguousarray(L.ravel(order="F"))
        rho, pi = np.empty(K * K), np.empty(K)
        _lib.check(lib.nhp_sbm_draw(ctx.h, K, Lf.ctypes.data, n.ctypes.data, self.α, self.β, self.γ, seed, step, _lib.dptr(rho),
                                    _lib.dptr(pi)), ctx.h)
        self.ρ, self.π = rho.reshape((K, K), order="F"), pi
        if labels:
            z = np.ascontiguousarray(self.z, dtype=np.int32).copy()
            _lib.check(lib.nhp_sbm_resample_blocks(ctx.h, _lib.dptr(Af), N, K, z.ctypes.data, _lib.dptr(rho), _lib.dptr(pi), None, seed,
                                                   step, 1, None, None), ctx.h)
            self.z = z
        return self.params()


class LatentDistanceNetworkModel(Network):
    """LatentDistanceNetworkModel(nnodes, ndims, z, b; σ, μb, σb) -- the reference names the model and leaves it an empty
    stub (src/networks.jl, last lines).  Nodes have positions in a latent space and a link is the likelier the closer
    its two nodes are:

        z_n ~ N(0, σ² I_D),  b ~ N(μb, σb²),  A[p,c] ~ Bernoulli(1 / (1 + exp(-(b - ‖z_p - z_c‖²))))

    for all N² entries (the diagonal is counted, with the logit b).  params() is [b]; the positions `z` (N x D) are
    latent state, not parameters.  Positions are identified only up to rotation, reflection and sign, so over a chain
    the link-probability matrix is the summary to average, not the positions."""

    MAX_DIMS = 8

    def __init__(self, nnodes, ndims=2, z=None, b=0.0, σ=1.0, μb=0.0, σb=1.0):
        self.nnodes, self.ndims = int(nnodes), int(ndims)
        if self.nnodes < 1:
            raise ValueError("nnodes must be positive")
        if self.ndims < 1 or self.ndims > self.MAX_DIMS:
            raise ValueError(f"ndims must lie in 1..{self.MAX_DIMS}")
        self.σ, self.μb, self.σb, self.b = float(σ), float(μb), float(σb), float(b)
        if not (self.σ > 0 and self.σb > 0 and np.isfinite([self.σ, self.σb, self.μb]).all()):
            raise _lib.DomainError("the priors need σ, σb > 0 and a finite μb")
        self.z = (np.zeros((self.nnodes, self.ndims)) if z is None
                  else np.array(z, dtype=np.float64).reshape((self.nnodes, self.ndims)))
        if not (np.all(np.isfinite(self.z)) and np.isfinite(self.b)):
            raise _lib.DomainError("positions and offset must be finite")
        # the variational state: None until variational_init_ creates it
        self.zv = self.bv = None
        self.ascent_steps = 4

    def variational_init_(self, seed=0, scale=0.1, ascent_steps=4):
        """Create the variational state of update_ / vb_ on a continuous network process: the point estimate (zv, bv) the fit
        moves, zv = the current z plus scale·N(0, I) (seeded), bv = b; `ascent_steps` (0..64) iterations of the ascent run per
        step (0 holds the network fixed).  All positions equal is a saddle of the ascent -- the position gradient is -z/σ² and
        nothing separates the nodes --, so scale = 0 with all rows of z equal is refused, and nothing creates this state
        implicitly."""
        if not (np.isfinite(scale) and scale >= 0.0):
            raise ValueError("variational_init!: scale must be finite and >= 0")
        if not 0 <= int(ascent_steps) <= 64:
            raise ValueError("variational_init!: ascent_steps must lie in 0..64")
        z = np.array(self.z, dtype=np.float64).reshape((self.nnodes, self.ndims))
        if scale == 0.0 and self.nnodes > 1 and np.all(z == z[0]):
            raise ValueError("variational_init!: scale = 0 with all positions equal is a saddle of the ascent, from which no "
                             "step separates the nodes")
        if scale > 0.0:
            z = z + scale * np.random.default_rng(seed).standard_normal(z.shape)
        self.zv, self.bv, self.ascent_steps = z, float(self.b), int(ascent_steps)
        return self

    def has_variational_state(self):
        return getattr(self, "zv", None) is not None

    def variational_params(self):
        """Z = [vec(zv) column-major; bv]"""
        return np.concatenate([np.asarray(self.zv, dtype=np.float64).ravel(order="F"), [float(self.bv)]])

    def expected_loglikelihood(self, rho, gradient=False, ctx=None):
        """F(z, b) = Σ rho·η - softplus(η) - ‖z‖²/(2σ²) - (b - μb)²/(2σb²) at the current (z, b) for link probabilities rho
        (N x N, each in [0, 1]), from the GPU: the soft-link counterpart of loglikelihood plus the priors' quadratics, the
        objective the variational fit climbs.  With `gradient` also (∂F/∂z [N x D], ∂F/∂b)."""
        N, D = self.nnodes, self.ndims
        rho = np.asarray(rho, dtype=np.float64)
        if rho.shape != (N, N) or not np.all((rho >= 0.0) & (rho <= 1.0)):
            raise ValueError("rho must be an N x N matrix of probabilities")
        ctx = ctx or _lib.default_context()
        out = np.empty(N * D + 2)
        lat = np.array([self.σ, self.μb, self.σb], dtype=np.float64)
        _lib.check(_lib.lib().nhp_latent_expected_loglik(ctx.h, _lib.dptr(_lib.colmajor(rho)), N, D, _lib.dptr(_lib.colmajor(self.z)),
                                                         float(self.b), _lib.dptr(lat), _lib.dptr(out)), ctx.h)
        if not gradient:
            return float(out[0])
        return float(out[0]), out[1:1 + N * D].reshape((N, D), order="F").copy(), float(out[-1])

    def params(self):
        return np.array([self.b])

    def link_probability(self):
        diff = self.z[:, None, :] - self.z[None, :, :]
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(np.sum(diff * diff, axis=2) - self.b))

    def rand(self, rng):
        """Positions from their prior, then A from the link probabilities (b stays)."""
        self.z = self.σ * rng.standard_normal((self.nnodes, self.ndims))
        return (rng.uniform(size=(self.nnodes, self.nnodes)) < self.link_probability()).astype(np.float64)

    def loglikelihood(self, A, ctx=None, conditionals=False):
        """log p(A | z, b) = Σ A·η - softplus(η) over all N² entries, from the GPU; with `conditionals` also the N terms
        L_n = Σ_{j≠n} (A[n,j] + A[j,n])·η_nj - 2·softplus(η_nj) the position sweep slices on."""
        ctx = ctx or _lib.default_context()
        out = np.empty(self.nnodes + 1)
        z = _lib.colmajor(self.z)
        _lib.check(_lib.lib().nhp_latent_loglik(ctx.h, _lib.dptr(_lib.colmajor(A)), self.nnodes, self.ndims, _lib.dptr(z), self.b,
                                                _lib.dptr(out)), ctx.h)
        return (float(out[0]), out[1:]) if conditionals else float(out[0])

    def resample_(self, A, rng, seed=None, step=0, ctx=None, positions=True):
        """resample!(network, A): one elliptical-slice sweep over the positions (node after node, each given the current
        positions of all others; skipped with positions=False), then an elliptical-slice update of b -- all on the GPU
        (csrc/latent.hip), keyed (seed, step).  Without a seed one is drawn from `rng`.  `self.exhausted` counts the
        slice steps of this call that used up their 100 attempts and kept their value."""
        import ctypes as C
        ctx = ctx or _lib.default_context()
        if seed is None:
            seed = int(rng.integers(0, 2 ** 63))
        z = _lib.colmajor(self.z).copy()
        b, ex = C.c_double(self.b), C.c_int64(0)
        _lib.check(_lib.lib().nhp_latent_resample(ctx.h, _lib.dptr(_lib.colmajor(A)), self.nnodes, self.ndims, _lib.dptr(z), C.byref(b),
                                                  self.σ, self.μb, self.σb, None, seed, step, 1 if positions else 0, 1, None, None,
                                                  None, C.byref(ex)), ctx.h)
        self.z, self.b, self.exhausted = z.reshape((self.nnodes, self.ndims), order="F"), b.value, int(ex.value)
        return self.params()


# ------------------------------------------------------------------------------ parameter vector
ParamLayout = collections.namedtuple("ParamLayout", "baseline impulses weights adjacency")


def param_layout(process, network=False):
    """Where the blocks of a continuous process sit in a parameter vector, as slices.

    Device order (default): params(process) of the standard process, [λ0; θ | μ; τ; W] -- the
    order of params!, the gradient, the device-resident block and its running moments, which put
    vec(A) behind it when the model has one; `weights.stop` is len(params) of the standard process.
    network=True: params(process) of a ContinuousNetworkHawkesProcess,
    [ρ; λ0; W; impulses; vec(A)] (src/continuous.jl:325-333)."""
    N = process.ndims()
    lengths = {"baseline": N if isinstance(process.baseline, HomogeneousProcess) else N * len(process.baseline.x),
               "impulses": N * N * (1 if isinstance(process.impulses, ExponentialImpulseResponse) else 2),
               "weights": N * N, "adjacency": N * N if hasattr(process, "network") else 0}
    order = ("baseline", "weights", "impulses", "adjacency") if network else ParamLayout._fields
    at = len(process.network.params()) if network else 0
    where = {}
    for name in order:
        where[name] = slice(at, at + lengths[name])
        at += lengths[name]
    return ParamLayout(**where)
