"""Discrete-time process models: host mirror of src/discrete.jl (+ the discrete components of
src/baselines.jl:358-456 and src/impulses.jl:272-375) on top of libnhp.so.

`data` is the reference's N x T Int64 count matrix (src/discrete.jl:18,80); `convolved` is the
T x N x B array of basis-filtered counts, kept on the device inside a DiscreteDataset handle.
"""
import collections
import ctypes as C
import time
import weakref

import numpy as np

from . import _lib
from ._lib import DomainError
from .components import DenseWeightModel
from .continuous import HawkesProcess


class DiscreteBaseline:
    pass


class DiscreteHomogeneousProcess(DiscreteBaseline):
    """DiscreteHomogeneousProcess(λ[, dt]) or (λ, α0, β0, αv, βv, dt) -- src/baselines.jl:358-382."""

    def __init__(self, λ, *args):
        λ = np.array(λ, dtype=np.float64)
        if len(args) <= 1:
            α0, β0, αv, βv, dt = 1.0, 1.0, np.ones_like(λ), np.ones_like(λ), (args[0] if args else 1.0)
        elif len(args) == 5:
            α0, β0, αv, βv, dt = args
        else:
            raise TypeError("DiscreteHomogeneousProcess(λ[, dt]) or (λ, α0, β0, αv, βv, dt)")
        αv, βv = np.array(αv, dtype=np.float64), np.array(βv, dtype=np.float64)
        if np.any(λ < 0):
            raise DomainError("DiscreteHomogeneousProcess: intensity parameter λ must be non-negative")
        if not α0 > 0:
            raise DomainError("DiscreteHomogeneousProcess: shape parameter α0 must be positive")
        if not β0 > 0:
            raise DomainError("DiscreteHomogeneousProcess: rate parameter β0 must be positive")
        if not np.all(αv > 0):
            raise DomainError("DiscreteHomogeneousProcess: shape parameter αv must be positive")
        if not np.all(βv > 0):
            raise DomainError("DiscreteHomogeneousProcess: rate parameter βv must be positive")
        if not dt > 0.0:
            raise DomainError("DiscreteHomogeneousProcess: time step dt must be non-negative")
        self.λ, self.α0, self.β0, self.αv, self.βv, self.dt = λ, float(α0), float(β0), αv, βv, float(dt)

    def ndims(self):
        return len(self.λ)

    def params(self):
        return self.λ.copy()

    def variational_params(self):
        return np.concatenate([self.αv, self.βv])

    def intensity(self, *args):
        """intensity(p, ts) -> len(ts) x N, or intensity(p, node, time) -- src/baselines.jl:402-411"""
        if len(args) == 1:
            ts = np.atleast_1d(np.asarray(args[0], dtype=np.float64))
            if np.any(ts < 0.0):
                raise DomainError("intensity: times ts must be non-negative")
            return np.tile(self.λ, (len(ts), 1)) * self.dt
        node, t = args
        if node < 1 or node > self.ndims():
            raise DomainError("intensity: node must be between one and ndims")
        if t < 0.0:
            raise DomainError("intensity: time must be non-negative")
        return self.λ[node - 1] * self.dt

    def sufficient_statistics(self, data):
        """src/baselines.jl:421-425 (pinned by test/baselines.jl:77-78); a list of trials counts as its stacked matrix"""
        data = np.asarray(_trials(data))
        return data.sum(axis=1), data.shape[1]

    def integrated_intensity(self, *args):
        """src/baselines.jl:427-439"""
        if len(args) == 1:
            (duration,) = args
            if duration < 0.0:
                raise DomainError("intensity: duration must be non-negative")
            return self.λ * self.dt * duration
        node, duration = args
        if node < 1 or node > self.ndims():
            raise DomainError("intensity: node must be between one and ndims")
        if duration < 0.0:
            raise DomainError("intensity: duration must be non-negative")
        return self.λ[node - 1] * self.dt * duration

    def update_(self, data, parents):
        """The reference's argument check (src/baselines.jl:447, test/baselines.jl:88); the update
        itself is fused into the GPU VB step."""
        data, parents = np.asarray(_trials(data)), np.asarray(parents)
        if data.shape != (parents.shape[1], parents.shape[0]):
            raise ValueError("update!: data and parent dimensions do not conform")
        N, T = data.shape
        self.αv = self.α0 + np.sum(parents[:, :, 0] * data.T, axis=0)
        self.βv = 1.0 / self.β0 + T * self.dt * np.ones(N)
        return self.αv.copy(), self.βv.copy()


class DiscreteLogGaussianCoxProcess(DiscreteBaseline):
    """DiscreteLogGaussianCoxProcess(x, λ, Σ | kernel, m, dt) -- src/baselines.jl:461-509: λ is G x N
    (λ[i, n] = λ_n(x[i])), intensity = linear interpolation of (x, λ[:, n]·dt)."""

    def __init__(self, x, λ, Σ, m, dt):
        from .components import Kernel
        x = np.asarray(x, dtype=np.float64)
        if isinstance(Σ, Kernel):
            if x[0] != 0.0:
                raise ValueError("Grid points must start at 0.")            # src/baselines.jl:493
            Σ = Σ(x)
        self.x = x
        self.λ = np.array(λ, dtype=np.float64)
        if self.λ.ndim != 2 or self.λ.shape[0] != len(x):
            raise ValueError("λ must be a (grid points) x (nodes) matrix")
        self.Σ = None if Σ is None else np.asarray(Σ, dtype=np.float64)
        self.m, self.dt = float(m), float(dt)

    @classmethod
    def from_gp(cls, gp, m, T, n, k, dt, rng):
        """DiscreteLogGaussianCoxProcess(gp, m, T, n, k, dt) -- src/baselines.jl:497-505"""
        if T % n != 0:
            raise ValueError("Duration must be divisible by number of steps.")
        x = np.linspace(0.0, T, n + 1)
        Σ = gp.cov(x)
        return cls(x, np.column_stack([np.exp(m + gp.rand(x, rng, sigma=Σ)) for _ in range(k)]), Σ, m, dt)

    def ndims(self):
        return self.λ.shape[1]

    def range(self):
        """range(p) = x[1] : dt : x[end] - dt  -- src/baselines.jl:509"""
        return self.x[0] + self.dt * np.arange(self.nsteps())

    def nsteps(self):
        return int(np.floor((self.x[-1] - self.dt - self.x[0]) / self.dt + 1e-9)) + 1

    def params(self):
        return self.λ.ravel(order="F").copy()

    def params_(self, x):
        """params!: src/baselines.jl:514-520"""
        if len(x) != self.λ.size:
            raise ValueError("Parameter vector length does not match model parameter length.")
        self.λ = np.asarray(x, dtype=np.float64).reshape(self.λ.shape, order="F").copy()

    def intensity(self, *args):
        """intensity(p, times) -> len(times) x N, intensity(p, node, times): src/baselines.jl:523-541
        (piecewise-linear through (x, λ[:, n]·dt); DomainError outside the grid, last value at x[end])"""
        if len(args) == 2:
            node, ts = args
            return self.intensity(ts)[:, node - 1] if np.ndim(ts) else self.intensity(np.array([ts]))[0, node - 1]
        ts = np.atleast_1d(np.asarray(args[0], dtype=np.float64))
        if np.any(ts < self.x[0]) or np.any(ts > self.x[-1]):
            raise DomainError("Value is outside interpolation support")
        return np.column_stack([np.interp(ts, self.x, self.λ[:, n] * self.dt) for n in range(self.ndims())])

    def integrated_intensity(self, duration=None):
        """src/baselines.jl:543"""
        return self.intensity(self.range()).sum(axis=0)

    def attach(self, ds):
        """Put intensity(p, 1:T) on the device with the dataset (calls then pass lambda0 = NULL)."""
        lam = np.asfortranarray(self.λ).ravel(order="K")
        _lib.check(_lib.lib().nhp_disc_set_lgcp_baseline(ds.ctx.h, ds.h, _lib.dptr(self.x), len(self.x), _lib.dptr(lam), self.dt),
                   ds.ctx.h)

    def candidate_loglikelihood(self, ds, Y):
        """loglikelihood(p, data, node, y) (src/baselines.jl:571-584) of latent curves Y [G, N], one per node, in
        one GPU call, on the baseline counts parents[:, :, 1] the latest parent sweep left on the device."""
        cand = np.asfortranarray(np.exp(self.m + np.asarray(Y, dtype=np.float64))).ravel(order="K")
        out = np.empty(self.ndims())
        _lib.check(_lib.lib().nhp_disc_lgcp_loglik(ds.ctx.h, ds.h, _lib.dptr(cand), self.dt, _lib.dptr(out)), ds.ctx.h)
        return out

    def resample_(self, ds, rng, max_attempts=100):
        """resample!(process, parents; sampler=elliptical_slice) -- src/baselines.jl:589-609,640-679; the N slice
        loops advance in lock step, one GPU likelihood call per round (as for the continuous LGCP)."""
        if self.Σ is None:
            raise ValueError("DiscreteLogGaussianCoxProcess needs Σ to be resampled")
        G, N = self.λ.shape
        L = np.linalg.cholesky(self.Σ)
        Y = np.log(self.λ) - self.m
        V = L @ rng.standard_normal((G, N))
        lly = self.candidate_loglikelihood(ds, Y) + np.log(rng.uniform(size=N))
        θ = 2 * np.pi * rng.uniform(size=N)
        θmin, θmax = θ - 2 * np.pi, θ.copy()
        Ynew = Y * np.cos(θ)[None, :] + V * np.sin(θ)[None, :]
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
            cand = Y * np.cos(θ)[None, :] + V * np.sin(θ)[None, :]
            Ynew = np.where(todo[None, :], cand, Ynew)
            done = done | (todo & (self.candidate_loglikelihood(ds, Ynew) >= lly))
        self.λ = np.exp(self.m + Ynew)
        return self.λ.copy()


class DiscreteImpulseResponse:
    pass


class DiscreteGaussianImpulseResponse(DiscreteImpulseResponse):
    """DiscreteGaussianImpulseResponse(θ, nlags[, dt]) -- src/impulses.jl:272-288; θ is N x N x B
    with Σ_b θ[p,c,·] = 1."""

    def __init__(self, θ, nlags, dt=1.0):
        θ = np.array(θ, dtype=np.float64, order="K")
        if not np.all(θ.sum(axis=2) == 1.0):
            raise ValueError("Invalid discrete basis parameter.")
        self.θ, self.γ, self.γv, self.nlags, self.dt = θ, 1.0, np.ones_like(θ), int(nlags), float(dt)
        self.ϕ = None

    def ndims(self):
        return self.θ.shape[0]

    def nbasis(self):
        return self.θ.shape[2]

    def params(self):
        return self.θ.ravel(order="F").copy()

    def variational_params(self):
        return self.γv.ravel(order="F").copy()

    def basis(self):
        """basis(impulse) -> L x B matrix (column b = ϕ_b) -- src/impulses.jl:321-335"""
        L, B = self.nlags, self.nbasis()
        phi = np.empty((B, L))
        _lib.check(_lib.lib().nhp_disc_basis(L, B, self.dt, _lib.dptr(phi)))
        return phi.T.copy()


def stack_trials(trials):
    """Independent trials of one system -- a list or tuple of N x T_r count matrices with the same N -- stacked along time:
    returns (counts [N, ΣT_r] int64, offsets int64 [R + 1]); trial r holds the stacked bins offsets[r] <= t < offsets[r + 1].
    Host code only.  ValueError for an empty list, a non-2-D entry, a trial with zero bins or differing N; DomainError for
    a negative count."""
    if isinstance(trials, StackedTrials):
        return trials.counts, trials.offsets
    if not isinstance(trials, (list, tuple)):
        raise ValueError("trials must be a list or tuple of N x T count matrices")
    if len(trials) == 0:
        raise ValueError("trials is empty: at least one N x T count matrix is needed")
    mats = []
    for r, x in enumerate(trials):
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError(f"trial {r} is not an N x T matrix (it has {x.ndim} dimensions)")
        if x.shape[1] < 1:
            raise ValueError(f"trial {r} holds no bins")
        if mats and x.shape[0] != mats[0].shape[0]:
            raise ValueError(f"trial {r} has {x.shape[0]} nodes, trial 0 has {mats[0].shape[0]}")
        if x.size and x.min() < 0:
            raise DomainError(f"trial {r}: counts must be non-negative")
        mats.append(x.astype(np.int64, copy=False))
    offsets = np.zeros(len(mats) + 1, dtype=np.int64)
    np.cumsum([m.shape[1] for m in mats], out=offsets[1:])
    return np.concatenate(mats, axis=1), offsets


class StackedTrials:
    """What a list of trials becomes at the entry of a discrete call: the stacked count matrix and the trial offsets.
    np.asarray / np.shape of it give the stacked matrix."""

    def __init__(self, counts, offsets):
        self.counts, self.offsets = counts, offsets
        self.shape = counts.shape

    def __array__(self, dtype=None, copy=None):
        return self.counts if dtype is None else self.counts.astype(dtype)


def _is_trials(data):
    """A list or tuple whose first entry is a matrix is a list of trials (a nested list of numbers stays one matrix)."""
    return isinstance(data, StackedTrials) or (isinstance(data, (list, tuple)) and len(data) > 0 and np.ndim(data[0]) == 2)


def _trials(data):
    """Normalise `data` once at the entry of a call: a list or tuple of trial matrices becomes StackedTrials (every check of
    stack_trials runs here, before any device work); anything else is returned as it is."""
    if isinstance(data, (list, tuple)) and _is_trials(data):
        return StackedTrials(*stack_trials(data))
    return data


def _has_trials(data):
    return (isinstance(data, StackedTrials) and len(data.offsets) > 2) or (isinstance(data, DiscreteDataset) and data.ntrials > 1)


class DiscreteDataset:
    """nhp_disc_dataset handle: the count matrix (uploaded once, transposed on the device) and,
    after convolve(), the T x N x B basis-filtered counts.

    DiscreteDataset(ctx, data, trial_offsets=None): `data` is an N x T matrix, or a list or tuple of N x T_r matrices --
    independent trials, stacked along time (stack_trials).  `trial_offsets` (int64 [R + 1]: 0, strictly increasing, ending at
    T) cuts a stacked matrix into trials.  convolve() stops at the trial boundaries; everything downstream works on rows of Ŝ
    and takes the dataset as it is, with bin ranges in stacked bins (trial_bins)."""

    def __init__(self, ctx, data, trial_offsets=None):
        data = _trials(data)
        if isinstance(data, StackedTrials):
            if trial_offsets is not None:
                raise ValueError("trial_offsets comes with one stacked matrix, not with a list of trials")
            data, trial_offsets = data.counts, data.offsets
        data = np.asarray(data)
        if data.ndim != 2:
            raise ValueError("data must be an N x T matrix")
        if data.size and data.min() < 0:              # any entry (a node's total may still be positive); nhp_disc_dataset_create
            raise DomainError("counts must be non-negative")        # refuses the same, this one before any device work
        self.N, self.T = data.shape
        self.ctx = ctx
        self.node_counts = data.sum(axis=1).astype(np.float64)    # node_counts(data): src/parents.jl:118-121
        d = np.asfortranarray(data.astype(np.int64, copy=False)).ravel(order="K")
        h = C.c_void_p()
        _lib.check(_lib.lib().nhp_disc_dataset_create(ctx.h, _lib.iptr(d), self.N, self.T, C.byref(h)), ctx.h)
        self.h = h
        self.B = 0
        self._fin = weakref.finalize(self, _lib.lib().nhp_disc_dataset_destroy, h)
        self.trial_offsets = np.array([0, self.T], dtype=np.int64)
        if trial_offsets is not None:
            self.set_trials(trial_offsets)

    def set_trials(self, offsets):
        """nhp_disc_dataset_set_trials: cut the T bins into trials at `offsets` (R + 1 entries).  An existing convolution is
        dropped: convolve() must run again."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or len(offsets) < 2:
            raise ValueError("trial offsets must hold R + 1 >= 2 entries")
        _lib.check(_lib.lib().nhp_disc_dataset_set_trials(self.ctx.h, self.h, _lib.iptr(offsets), len(offsets) - 1), self.ctx.h)
        self.B = 0
        n = C.c_int32()
        _lib.check(_lib.lib().nhp_disc_dataset_get_trials(self.h, C.byref(n), None), self.ctx.h)
        out = np.empty(n.value + 1, dtype=np.int64)
        _lib.check(_lib.lib().nhp_disc_dataset_get_trials(self.h, C.byref(n), _lib.iptr(out)), self.ctx.h)
        self.trial_offsets = out

    def convsum(self):
        """Σ_t Ŝ[t, n, b] as the convolution left it on the device -> [N, B]."""
        out = np.empty(self.N * self.B)
        _lib.check(_lib.lib().nhp_disc_dataset_get_convsum(self.ctx.h, self.h, _lib.dptr(out)), self.ctx.h)
        return out.reshape((self.N, self.B), order="F")

    @property
    def ntrials(self):
        return len(self.trial_offsets) - 1

    def trial_bins(self, r):
        """(start, stop) of trial r in stacked bins; negative r counts from the last trial."""
        R = self.ntrials
        if not -R <= r < R:
            raise IndexError(f"trial {r} of {R}")
        r = int(r) % R
        return int(self.trial_offsets[r]), int(self.trial_offsets[r + 1])


class DiscreteHawkesProcess(HawkesProcess):
    def ndims(self):
        return self.baseline.ndims()

    def nlags(self):
        return self.impulses.nlags

    def _lowered(self):
        A = getattr(self, "adjacency_matrix", None)
        l0 = None if isinstance(self.baseline, DiscreteLogGaussianCoxProcess) else _lib.f64(self.baseline.λ)
        return (l0, _lib.colmajor(self.weights.W), _lib.colmajor(self.impulses.θ),
                None if A is None else _lib.colmajor(A))


class DiscreteStandardHawkesProcess(DiscreteHawkesProcess):
    """DiscreteStandardHawkesProcess(baseline, impulses, weights, dt) -- src/discrete.jl:161-170."""

    def __init__(self, baseline, impulses, weights, dt):
        if baseline.dt != dt or impulses.dt != dt:
            raise ValueError("Baseline and impulse response time step must match process time step.")
        self.baseline, self.impulses, self.weights, self.dt = baseline, impulses, weights, float(dt)

    def isstable(self):
        return np.max(np.abs(np.linalg.eigvals(self.weights.W))) < 1.0

    def params(self):
        """[λ0; vec(W .* θ)] -- src/discrete.jl:174-182"""
        return np.concatenate([self.baseline.params(), (self.weights.W[:, :, None] * self.impulses.θ).ravel(order="F")])

    def variational_params(self):
        """src/discrete.jl:204-209"""
        return np.concatenate([self.baseline.variational_params(), self.impulses.variational_params(),
                               self.weights.variational_params()])


class DiscreteNetworkHawkesProcess(DiscreteHawkesProcess):
    """DiscreteNetworkHawkesProcess(baseline, impulses, weights, adjacency_matrix, network, dt)
    -- src/discrete.jl:395-402."""

    def __init__(self, baseline, impulses, weights, adjacency_matrix, network, dt):
        self.baseline, self.impulses, self.weights = baseline, impulses, weights
        self.adjacency_matrix, self.network, self.dt = np.array(adjacency_matrix, dtype=np.float64), network, float(dt)

    def isstable(self):
        return np.max(np.abs(np.linalg.eigvals(self.adjacency_matrix * self.weights.W))) < 1.0

    def params(self):
        """[ρ; λ0; W; θ; vec(A)] -- src/discrete.jl:406-414"""
        return np.concatenate([self.network.params(), self.baseline.params(), self.weights.params(),
                               self.impulses.params(), self.adjacency_matrix.ravel(order="F")])

    def link_probabilities(self):
        """q(A = 1): the weights' ρv, or link_probability(network) while no update has run."""
        ρv = getattr(self.weights, "ρv", None)
        return self.network.link_probability() if ρv is None else ρv

    def variational_params(self):
        """[baseline; κv0; νv0; κv1; νv1; γv; vec(ρv); αv; βv] -- the last two for a Bernoulli network only; a block
        network appends [vec(αv); vec(βv); γv; vec(mv)] instead"""
        from .components import StochasticBlockNetworkModel
        if isinstance(self.network, StochasticBlockNetworkModel):
            net = [self.network.variational_params()] if self.network.has_variational_state() else []
        else:
            net = [np.array([self.network.αv, self.network.βv])] if hasattr(self.network, "αv") else []
        return np.concatenate([self.baseline.variational_params(), self.weights.variational_params(),
                               self.impulses.variational_params(), self.link_probabilities().ravel(order="F")] + net)


def convolve(process, data, ctx=None, fetch=False):
    """convolve(process, data) -- src/discrete.jl:146-151.  Returns a DiscreteDataset whose device
    copy holds Ŝ (T x N x B); with fetch=True also returns the array itself.  `data` may be a list or tuple of N x T_r
    matrices, independent trials (or a DiscreteDataset cut into trials): they are stacked along time, T = ΣT_r, and the
    convolution stops at every trial's first bin -- the rows of a trial are those of the trial convolved alone."""
    data = _trials(data)
    _refuse_lgcp_trials(process, data)
    ctx = ctx or _lib.default_context()
    ds = data if isinstance(data, DiscreteDataset) else DiscreteDataset(ctx, data)
    phi = process.impulses.basis()
    L, B = phi.shape
    ph = np.asfortranarray(phi).ravel(order="K")
    out = np.empty(ds.T * ds.N * B) if fetch else None
    _lib.check(_lib.lib().nhp_disc_convolve(ctx.h, ds.h, _lib.dptr(ph), L, B, _lib.dptr(out)), ctx.h)
    ds.B = B
    if fetch:
        return ds, out.reshape((ds.T, ds.N, B), order="F")
    return ds


def _refuse_lgcp_trials(process, data):
    if _has_trials(data) and isinstance(process.baseline, DiscreteLogGaussianCoxProcess):
        raise NotImplementedError("a DiscreteLogGaussianCoxProcess baseline is a function of time across the recording and is "
                                  "not defined for several trials; fit the trials with a DiscreteHomogeneousProcess baseline")


def _enter(process, data, convolved=None):
    """The head of every discrete call that takes `data`: a trial list normalised once, and the one refusal that needs
    no device -- before a context is opened."""
    data = _trials(data)
    _refuse_lgcp_trials(process, convolved if convolved is not None else data)
    return data


def _convolved(process, data, convolved, ctx):
    if convolved is not None:
        _refuse_lgcp_trials(process, convolved)
    ds = convolved if convolved is not None else convolve(process, data, ctx)
    if isinstance(process.baseline, DiscreteLogGaussianCoxProcess):
        process.baseline.attach(ds)           # intensity(baseline, 1:T) follows the current grid values
    return ds


def disc_rand(process, steps, seed=0, *, ctx=None, max_events=50_000_000, return_background=False, device=False):
    """rand(process::DiscreteHawkesProcess, steps) on the GPU (nhp_disc_simulate) -- the device route for discrete
    processes; `rand(process, steps)` is the host simulator and keeps refusing device=True for them.

    Returns the N x steps int64 count matrix of src/discrete.jl:20-38 as a numpy array, or with device=True as a torch
    tensor on the context's device; with return_background=True the pair (counts, background), background the immigrants
    alone (parents[:, :, 1] of the reference's augmented model, as N x steps).  Works for DiscreteStandardHawkesProcess and
    DiscreteNetworkHawkesProcess with either baseline; for a DiscreteLogGaussianCoxProcess the per-bin means are
    baseline.intensity(1:steps), and bins outside its grid raise "Sample duration does not match process duration." (where
    the host simulator's intensity(baseline, 1:steps) fails).  The draws come from counter-based Philox streams
    (include/nhp.h has the scheme): the same law as the host simulator, not the same sample; the result depends on the
    parameters, steps and seed only.  More than `max_events` events raise RuntimeError ("branching process exploded")."""
    out = _disc_simulate(process, steps, seed, ctx, max_events, return_background, device)
    return out[:2] if return_background else out[0]


def _disc_simulate(process, steps, seed, ctx, max_events, return_background, device):
    """disc_rand's call of nhp_disc_simulate -> (counts, background | None, events, generations)."""
    if not isinstance(process, DiscreteHawkesProcess):
        raise TypeError("disc_rand simulates discrete processes; rand(process, duration, device=True) is the device route "
                        "for continuous ones")
    if int(steps) != steps or steps < 1:
        raise ValueError(f"steps = {steps} must be a positive integer")
    steps, max_events = int(steps), int(max_events)
    if not 0 <= max_events < 2 ** 31:
        raise ValueError(f"max_events = {max_events} outside [0, 2^31)")
    N = process.ndims()
    l0, W, th, A = process._lowered()
    base = None
    if l0 is None:
        b = process.baseline
        if steps > b.x[-1] or 1 < b.x[0]:
            raise ValueError("Sample duration does not match process duration.")
        base = np.asfortranarray(b.intensity(np.arange(1, steps + 1, dtype=np.float64))).ravel(order="K")      # T x N, t fastest
    phi = np.asfortranarray(process.impulses.basis())
    L, B = phi.shape
    ph = phi.ravel(order="K")
    ctx = ctx or _lib.default_context()
    n, gens = C.c_int64(), C.c_int32()
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        out = torch.empty((steps, N), dtype=torch.int64, device=dev)               # node fastest: the transpose is N x T
        bg = torch.empty((steps, N), dtype=torch.int64, device=dev) if return_background else None
        torch.cuda.current_stream(dev).synchronize()      # earlier users of the buffers' memory are done before the library writes
        po, pb = out.data_ptr(), (bg.data_ptr() if return_background else None)
    else:
        out = np.empty((steps, N), dtype=np.int64)
        bg = np.empty((steps, N), dtype=np.int64) if return_background else None
        po, pb = out.ctypes.data, (bg.ctypes.data if return_background else None)
    _lib.check(_lib.lib().nhp_disc_simulate(ctx.h, _lib.dptr(l0), _lib.dptr(base), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                            _lib.dptr(ph), L, B, process.dt, N, steps, int(seed) & (2 ** 64 - 1), max_events,
                                            1 if device else 0, po, pb, C.byref(n), C.byref(gens)), ctx.h)
    tr = (lambda x: None if x is None else x.t()) if device else (lambda x: None if x is None else x.T)
    return tr(out), tr(bg), n.value, gens.value


class DiscreteForecast:
    """Result of disc_forecast(): totals [S, N] int64 (events of node c over the horizon in replica r), mean [N, H] (the
    ensemble mean per cell, cell_sum / S), expected [N, H] (the exact predictive mean, no sampling), carry [N, H] (the expected
    carry-over children of the observed events per cell, 0 beyond nlags bins), paths = None or [S, N, H] int64 (the count matrix
    of every replica), cell_sum [N, H] int64, events (of all replicas) and generations.  numpy arrays, or torch tensors on the
    context's device."""

    def __init__(self, totals, cell_sum, expected, carry, paths, events, generations):
        self.totals, self.cell_sum, self.expected, self.carry, self.paths = totals, cell_sum, expected, carry, paths
        if hasattr(cell_sum, "new_full"):             # a tensor divisor: an IEEE division, as numpy's (a scalar one multiplies by 1/S)
            self.mean = cell_sum.double() / cell_sum.new_full((), totals.shape[0]).double()
        else:
            self.mean = cell_sum / float(totals.shape[0])
        self.events, self.generations = events, generations

    def __repr__(self):
        return (f"DiscreteForecast(nsamples={self.totals.shape[0]}, nodes={self.totals.shape[1]}, horizon={self.mean.shape[1]}, "
                f"paths={self.paths is not None})")


def _history_tail(data, N, L):
    """The last min(L, T0) bins of an N x T0 count matrix as [bins, N] int64, node fastest -> (tail, T0, on_device)."""
    if _is_trials(data):
        raise NotImplementedError("disc_forecast continues one recording, not a list of trials: pass the count matrix of the "
                                  "trial to continue")
    if isinstance(data, DiscreteDataset):
        raise TypeError("disc_forecast: a DiscreteDataset keeps no host copy of its counts; pass the N x T count matrix "
                        "(a numpy array or a device tensor)")
    if type(data).__module__.split(".")[0] == "torch":
        import torch
        if data.dim() != 2 or data.shape[0] != N or data.shape[1] < 1:
            raise ValueError(f"data must be an N x T matrix with N = {N} rows and at least one bin, got {tuple(data.shape)}")
        if data.dtype.is_floating_point or data.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise TypeError("data must be an integer count matrix")
        T0 = int(data.shape[1])
        tu = min(L, T0)
        if data.is_cuda:
            return data[:, T0 - tu:].t().to(torch.int64).contiguous(), T0, True
        data = data.numpy()
    data = np.asarray(data)
    if data.ndim != 2 or data.shape[0] != N or data.shape[1] < 1:
        raise ValueError(f"data must be an N x T matrix with N = {N} rows and at least one bin, got {data.shape}")
    if data.dtype.kind not in "iu":
        raise TypeError("data must be an integer count matrix")
    T0 = data.shape[1]
    if data.dtype.kind == "i" and np.any(data < 0):                 # the whole host matrix; of a device matrix the tail, on the device
        raise DomainError("disc_forecast: counts must be non-negative")
    tail = np.ascontiguousarray(data[:, T0 - min(L, T0):].T.astype(np.int64))
    return tail, T0, False


def disc_forecast(process, data, horizon, nsamples=1000, seed=0, *, return_paths=False, device=False, max_events=50_000_000,
                  ctx=None):
    """`nsamples` independent continuations of the N x T0 count matrix `data` over the next `horizon` bins, conditional on
    the observed counts (nhp_disc_forecast) -- the forecast for discrete processes; `forecast(process, data, horizon)` is
    the one for continuous processes and keeps refusing discrete ones.  A continuation is the union of the children the
    observed events still have beyond T0 (the carry-over: a process restarted at T0 would lose them), new immigrants, and
    the descendants of both, under the law disc_rand samples.

    Returns DiscreteForecast(totals [S, N], mean [N, H], expected [N, H], carry [N, H], paths None | [S, N, H], events,
    generations); `expected` is the exact predictive mean (a linear recursion, no sampling), `mean` the ensemble's.
    device=False: numpy arrays; device=True: torch tensors on the context's device.  `data`: a numpy integer matrix or a
    torch tensor (for instance disc_rand(..., device=True)); only its last nlags bins are uploaded or read (negative counts
    raise DomainError: anywhere in a host matrix, before any device work; in the last nlags bins of a device tensor).  For a
    DiscreteLogGaussianCoxProcess the grid must reach T0 + horizon ("Sample duration does not match process duration."
    otherwise).  The sample depends on (process, the last nlags bins of data, horizon, nsamples, seed) only; replica r's
    draws are not the same for different nsamples.  More than `max_events` events in all replicas together raise
    RuntimeError ("branching process exploded").  A replica's path appended to the data is data for loglikelihood."""
    if not isinstance(process, DiscreteHawkesProcess):
        raise TypeError("disc_forecast forecasts discrete processes; forecast(process, data, horizon) is the route for "
                        "continuous ones")
    for name, v in (("horizon", horizon), ("nsamples", nsamples)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or v < 1:
            raise ValueError(f"{name} = {v} must be a positive integer")
    H, S, max_events = int(horizon), int(nsamples), int(max_events)
    if not 0 <= max_events < 2 ** 31:
        raise ValueError(f"max_events = {max_events} outside [0, 2^31)")
    N = process.ndims()
    L = process.nlags()
    tail, T0, on_device = _history_tail(data, N, L)
    l0, W, th, A = process._lowered()
    base = None
    if l0 is None:
        b = process.baseline
        if T0 + H > b.x[-1] or T0 + 1 < b.x[0]:
            raise ValueError("Sample duration does not match process duration.")
        base = np.asfortranarray(b.intensity(np.arange(T0 + 1, T0 + H + 1, dtype=np.float64))).ravel(order="K")  # H x N, k fastest
    phi = np.asfortranarray(process.impulses.basis())
    L, B = phi.shape
    ph = phi.ravel(order="K")
    ctx = ctx or _lib.default_context()
    n, gens = C.c_int64(), C.c_int32()
    if on_device and tail.device.index != ctx.device:
        raise ValueError(f"data lives on {tail.device}, the context on device {ctx.device}")
    if device or on_device:
        import torch
        dev = torch.device("cuda", ctx.device)
    if device:
        tot = torch.empty((S, N), dtype=torch.int64, device=dev)
        cell = torch.empty((H, N), dtype=torch.int64, device=dev)
        mu, carry = (torch.empty((H, N), dtype=torch.float64, device=dev) for _ in range(2))
        paths = torch.empty((S, H, N), dtype=torch.int64, device=dev) if return_paths else None
        ptr = [x.data_ptr() if x is not None else None for x in (tot, cell, paths, carry, mu)]
    else:
        tot, cell = np.empty((S, N), dtype=np.int64), np.empty((H, N), dtype=np.int64)
        mu, carry = np.empty((H, N)), np.empty((H, N))
        paths = np.empty((S, H, N), dtype=np.int64) if return_paths else None
        ptr = [x.ctypes.data if x is not None else None for x in (tot, cell, paths, carry, mu)]
    if device or on_device:
        torch.cuda.current_stream(dev).synchronize()      # the tail is written and the buffers' earlier users are done
    hp = tail.data_ptr() if on_device else tail.ctypes.data
    _lib.check(_lib.lib().nhp_disc_forecast(ctx.h, _lib.dptr(l0), _lib.dptr(base), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                            _lib.dptr(ph), L, B, process.dt, N, hp, tail.shape[0], 1 if on_device else 0, H, S,
                                            int(seed) & (2 ** 64 - 1), max_events, 1 if device else 0, *ptr, C.byref(n),
                                            C.byref(gens)), ctx.h)
    if device:
        return DiscreteForecast(tot, cell.t(), mu.t(), carry.t(), None if paths is None else paths.transpose(1, 2), n.value,
                                gens.value)
    return DiscreteForecast(tot, cell.T, mu.T, carry.T, None if paths is None else paths.transpose(0, 2, 1), n.value, gens.value)


class DiscreteResiduals:
    """Result of disc_residuals(): per cell pit, pearson, cumulative [N, T] (None when not requested); per node expected
    (Σ_t μ), observed (Σ_t s, int64), chi2 (Σ_t (s-μ)²/μ), deviance [N] and histogram [N, nbins] int64 (cells per bin of pit);
    impossible: the cells with μ = 0 and a positive count; bins = T.  numpy arrays, or torch tensors on the context's device."""

    def __init__(self, pit, pearson, cumulative, expected, observed, chi2, deviance, histogram, impossible, bins):
        self.pit, self.pearson, self.cumulative = pit, pearson, cumulative
        self.expected, self.observed, self.chi2, self.deviance, self.histogram = expected, observed, chi2, deviance, histogram
        self.impossible, self.bins = impossible, bins
        self.pass_ms = None                           # the residual kernel's device time, ms (tools/residuals_discrete.py)

    def __repr__(self):
        planes = [k for k in ("pit", "pearson", "cumulative") if getattr(self, k) is not None]
        return (f"DiscreteResiduals(nodes={self.histogram.shape[0]}, bins={self.bins}, nbins={self.histogram.shape[1]}, "
                f"planes={planes}, impossible={self.impossible})")


def disc_residuals(process, data=None, convolved=None, seed=0, nbins=20, *, pit=True, pearson=False, cumulative=False,
                   device=False, ctx=None):
    """Residuals of a discrete process on its N x T count matrix (nhp_disc_residuals): cell (t, c) is Poisson(μ[t,c]) with
    μ = intensity(process, data), and one pass on the GPU makes of every cell its randomized probability integral transform
    pit = F(s-1) + v·p(s), v uniform -- exactly uniform on [0, 1) under the model, whatever the means --, its Pearson residual
    (s-μ)/√μ, and of every node Σμ against Σs, χ² = Σ(s-μ)²/μ, the deviance and the histogram of its pit values over `nbins`
    equal bins; `cumulative` is the compensator Σ_{t' <= t} μ[t',c].  The T x N intensity never leaves the device.  For a list
    of trials every plane is [N, ΣT_r] in stacked bins, and `cumulative` runs on over the stacked bins: it does not restart
    at a trial's first bin.

    Returns DiscreteResiduals; the planes pit, pearson, cumulative are [N, T] or None when not requested (an absent plane is
    not computed).  device=False: numpy arrays; device=True: torch tensors on the context's device.  `data`: the count matrix,
    or pass `convolved` (a DiscreteDataset after convolve()).  A cell with μ = 0 and a positive count is impossible under the
    model: pit = 1, pearson = inf (so chi2 of its node is inf), counted in `impossible`.  The uniforms come from a
    counter-based Philox stream of their own (include/nhp.h): the result depends on (process, data, seed, nbins) only, and
    the seed changes pit and the histogram alone.  Raises TypeError for a continuous process (compensator /
    time_rescaling_test are its route), ValueError for nbins outside [1, 4096], DomainError for a negative or non-finite
    mean, NotImplementedError for a mean or a count above 2^20."""
    if not isinstance(process, DiscreteHawkesProcess):
        raise TypeError("disc_residuals takes discrete processes; compensator(process, data) and time_rescaling_test are the "
                        "route for continuous ones")
    if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)) or not 1 <= nbins <= 4096:
        raise ValueError(f"nbins = {nbins} must be an integer in [1, 4096]")
    nbins = int(nbins)
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, A = process._lowered()
    N, T = ds.N, ds.T
    want = (pit, pearson, cumulative)
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        planes = [torch.empty((N, T), dtype=torch.float64, device=dev) if w else None for w in want]
        ex, chi, dv = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
        ob = torch.empty(N, dtype=torch.int64, device=dev)
        hist = torch.empty((N, nbins), dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # earlier users of the buffers' memory are done before the library writes
        ptr = [x.data_ptr() if x is not None else None for x in (*planes, ex, ob, chi, dv, hist)]
    else:
        planes = [np.empty((N, T)) if w else None for w in want]
        ex, chi, dv = np.empty(N), np.empty(N), np.empty(N)
        ob, hist = np.empty(N, dtype=np.int64), np.empty((N, nbins), dtype=np.int64)
        ptr = [x.ctypes.data if x is not None else None for x in (*planes, ex, ob, chi, dv, hist)]
    imp, ms = C.c_int64(), C.c_double()
    _lib.check(_lib.lib().nhp_disc_residuals(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A), process.dt,
                                             int(seed) & (2 ** 64 - 1), nbins, 1 if device else 0, *ptr, C.byref(imp),
                                             C.byref(ms)), ctx.h)
    res = DiscreteResiduals(*planes, ex, ob, chi, dv, hist, imp.value, T)
    res.pass_ms = ms.value
    return res


class DiscreteFitTest:
    """Result of disc_goodness_of_fit(): `statistic` / `pvalue`: the Kolmogorov-Smirnov test of all pit values against
    U(0, 1); `node_statistic` / `node_pvalue` [N]: the same per node; `histogram_chi2` / `histogram_pvalue`: the χ² test of
    the pooled pit histogram against equal bins (nbins - 1 degrees of freedom); `dispersion` [N] = chi2 / T, near 1 under the
    model (above it: overdispersed counts); `expected`, `observed` [N]: Σμ against Σs per node; `impossible`: cells the model
    gives probability 0."""

    def __init__(self, statistic, pvalue, node_statistic, node_pvalue, histogram_chi2, histogram_pvalue, dispersion, expected,
                 observed, impossible):
        self.statistic, self.pvalue, self.node_statistic, self.node_pvalue = statistic, pvalue, node_statistic, node_pvalue
        self.histogram_chi2, self.histogram_pvalue = histogram_chi2, histogram_pvalue
        self.dispersion, self.expected, self.observed, self.impossible = dispersion, expected, observed, impossible

    def __repr__(self):
        return (f"DiscreteFitTest(statistic={self.statistic:.4g}, pvalue={self.pvalue:.4g}, "
                f"histogram_pvalue={self.histogram_pvalue:.4g}, nodes={len(self.dispersion)}, impossible={self.impossible})")


def disc_goodness_of_fit(process, data=None, convolved=None, residuals=None, seed=0, nbins=20, *, device=False, ctx=None):
    """Does the process describe the count matrix?  The pit values of disc_residuals() are uniform on [0, 1) under the model:
    returns their Kolmogorov-Smirnov statistic and p-value, pooled and per node, the χ² uniformity test of the pooled pit
    histogram, the per-node dispersion chi2 / T and Σμ against Σs (DiscreteFitTest).  `residuals` reuses an earlier
    disc_residuals() result (it must hold the pit plane); with device=True (or residuals that live on the device) the values
    are sorted with torch on the GPU, otherwise with numpy on the host."""
    from scipy.special import gammaincc
    from .continuous import _is_tensor, _ks_sorted, kolmogorov_pvalue
    if residuals is None:
        residuals = disc_residuals(process, data, convolved, seed, nbins, pit=True, device=device, ctx=ctx)
    elif not isinstance(process, DiscreteHawkesProcess):
        raise TypeError("disc_goodness_of_fit takes discrete processes; time_rescaling_test is the route for continuous ones")
    r = residuals
    if r.pit is None:
        raise ValueError("disc_goodness_of_fit: the residuals hold no pit plane (disc_residuals(..., pit=True))")
    N, T = r.pit.shape
    if _is_tensor(r.pit):
        import torch
        rows = torch.sort(r.pit, dim=1).values
        pooled = _ks_sorted(torch.sort(r.pit.reshape(-1)).values)
        host = lambda x: x.cpu().numpy()
    else:
        rows = np.sort(r.pit, axis=1)
        pooled = _ks_sorted(np.sort(r.pit, axis=None))
        host = np.asarray
    stats = np.array([_ks_sorted(rows[c]) for c in range(N)])
    pvals = np.array([kolmogorov_pvalue(s, T) for s in stats])
    h = host(r.histogram).sum(axis=0).astype(np.float64)
    k = len(h)
    x2 = float(np.sum((h - h.sum() / k) ** 2 / (h.sum() / k)))
    hp = float(gammaincc(0.5 * (k - 1), 0.5 * x2)) if k > 1 else float("nan")
    return DiscreteFitTest(pooled, kolmogorov_pvalue(pooled, N * T), stats, pvals, x2, hp, host(r.chi2) / T, host(r.expected),
                           host(r.observed), r.impossible)


def disc_intensity(process, data=None, convolved=None, ctx=None):
    """intensity(process, convolved) / intensity(process, data) -> T x N -- src/discrete.jl:115-131"""
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, A = process._lowered()
    out = np.empty(ds.T * ds.N)
    _lib.check(_lib.lib().nhp_disc_intensity(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                             process.dt, _lib.dptr(out)), ctx.h)
    return out.reshape((ds.T, ds.N), order="F")


def disc_loglikelihood(process, data=None, convolved=None, ctx=None):
    """loglikelihood(process, data[, convolved]) -- src/discrete.jl:86-102"""
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, A = process._lowered()
    ll = C.c_double()
    _lib.check(_lib.lib().nhp_disc_loglik(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                          process.dt, C.byref(ll)), ctx.h)
    return ll.value


def disc_loglikelihood_gradient(process, data=None, convolved=None, ctx=None):
    """(ll, ∂ll/∂[λ0; vec(W .* θ)]) in one GPU call: the analytic gradient of mle!'s objective
    (src/discrete.jl:211-296 uses finite differences of loglikelihood, 2P calls per gradient)."""
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, _ = process._lowered()
    P = len(process.baseline.params()) + ds.N * ds.N * ds.B
    g = np.empty(P)
    ll = C.c_double()
    _lib.check(_lib.lib().nhp_disc_loglik_grad(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), process.dt,
                                               C.byref(ll), _lib.dptr(g), P), ctx.h)
    return ll.value, g


def disc_params_(process, x):
    """params!(process::DiscreteStandardHawkesProcess, x): x = [λ0; vec(W .* θ)], W = Σ_b η, θ = η ./ W
    -- src/discrete.jl:183-201"""
    N, B = process.ndims(), process.impulses.nbasis()
    nb = len(process.baseline.params())
    if len(x) != nb + N * N * B:
        raise ValueError("Parameter vector length does not match model parameter length.")
    η = np.asarray(x[nb:], dtype=np.float64).reshape((N, N, B), order="F")
    W = η.sum(axis=2)
    if isinstance(process.baseline, DiscreteLogGaussianCoxProcess):
        process.baseline.params_(x[:nb])
    else:
        process.baseline.λ = np.array(x[:nb], dtype=np.float64)
    process.weights.W = np.asfortranarray(W)
    process.impulses.θ = np.asfortranarray(η / W[:, :, None])
    return process.params()


def disc_mle_(process, data, optimizer="L-BFGS-B", verbose=False, f_abstol=1e-6, regularize=False, guess=None,
              seed=None, max_steps=1000, ctx=None):
    """mle!(process::DiscreteStandardHawkesProcess, data) -- src/discrete.jl:211-296: same objective
    (-loglikelihood(process, data, convolved)), same parameter vector [λ0; vec(W .* θ)], same box [1e-6, 10],
    same stable random start (:346-360) and |f - f_prev| < f_abstol stopping rule.  The reference runs
    Optim's Fminbox(BFGS) on finite differences; here scipy's L-BFGS-B gets the analytic gradient from the GPU
    (three fp64-MFMA GEMMs per objective + gradient)."""
    import time
    from scipy import optimize
    from .inference import MaximumLikelihood
    if not isinstance(process, DiscreteStandardHawkesProcess):
        raise TypeError("mle! is defined for DiscreteStandardHawkesProcess (src/discrete.jl:211)")
    if regularize:
        raise NotImplementedError("logprior(::DiscreteStandardHawkesProcess) reads fields that do not exist "
                                  "(src/discrete.jl:316-322, SURVEY D5)")
    data = _enter(process, data)
    ctx = ctx or _lib.default_context()
    ds = convolve(process, data, ctx)
    N = process.ndims()
    rng = np.random.default_rng(seed)
    if guess is None:                                    # _rand_init_: src/discrete.jl:346-360
        for _ in range(100):
            x0 = rng.uniform(size=len(process.params()))
            nb = len(process.baseline.params())
            x0[nb:] /= 10
            W0 = x0[nb:].reshape((N, N, -1), order="F").sum(axis=2)
            if np.max(np.abs(np.linalg.eigvals(W0))) < 1.0:
                break
        else:
            raise RuntimeError("Random initialization reached max attempts.")
    else:
        x0 = np.array(guess, dtype=np.float64)
    lower, upper = 1e-6, 1e1
    state = {"minloss": np.inf, "steps": 0, "converged": False, "last": None}
    start = time.time()

    if optimizer in ("device", "LBFGS-device"):
        # the optimizer's state on the device (nhp_disc_mle_run: projected L-BFGS in HBM; params!'s split of x into W and θ
        # redone on the device per evaluation): no parameter upload, gradient download or host-side update per objective call
        if isinstance(process.baseline, DiscreteLogGaussianCoxProcess):
            raise NotImplementedError("optimizer='device' takes the homogeneous baseline; use the host optimizer with an LGCP baseline")
        x = np.ascontiguousarray(np.clip(x0, lower, upper), dtype=np.float64)
        loss, steps, conv, evals = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().nhp_disc_mle_run(ctx.h, ds.h, process.dt, lower, upper, float(f_abstol), int(max_steps), _lib.dptr(x), len(x),
                                               C.byref(loss), C.byref(steps), C.byref(conv), C.byref(evals)), ctx.h)
        if verbose:
            print(f" > steps: {steps.value}, objective evaluations: {evals.value}, loss: {loss.value}, elapsed: {time.time() - start}")
        disc_params_(process, x)
        res = MaximumLikelihood(x.copy(), -float(loss.value), int(steps.value), time.time() - start, "success" if conv.value else "failure")
        res.evaluations = int(evals.value)
        return res

    def fg(x):
        disc_params_(process, x)
        ll, g = disc_loglikelihood_gradient(process, convolved=ds, ctx=ctx)
        state["last"] = -ll
        return -ll, -g

    def status_update(xk):
        state["steps"] += 1
        value = state["last"]
        if verbose:
            print(f" > step: {state['steps']}, loss: {value}, elapsed: {time.time() - start}")
        if abs(value - state["minloss"]) < f_abstol:
            state["converged"] = True
            raise StopIteration
        state["minloss"] = value

    options = {"maxiter": max_steps}
    if optimizer == "L-BFGS-B":       # scipy's own relative-decrease test off, as in inference.mle_ (Optim's g_tol = 1e-8 kept)
        options.update(ftol=0.0, gtol=1e-8, maxfun=20 * max_steps + 1000)
    res = optimize.minimize(fg, np.clip(x0, lower, upper), jac=True, method=optimizer,
                            bounds=[(lower, upper)] * len(x0), callback=status_update, options=options)
    disc_params_(process, res.x)
    return MaximumLikelihood(res.x.copy(), -float(res.fun), state["steps"], time.time() - start,
                             "success" if (state["converged"] or res.success) else "failure")


DiscreteInformation = collections.namedtuple("DiscreteInformation", "ll columns blocks names kind")
DiscreteStandardErrors = collections.namedtuple("DiscreteStandardErrors", "se lower_ci upper_ci free pd se_W se_theta")
_INFORMATION_KINDS = {"observed": 0, "fisher": 1}


def _disc_information_check(process, what):
    if not isinstance(process, DiscreteStandardHawkesProcess):
        raise TypeError(f"{what} is defined for DiscreteStandardHawkesProcess, the process mle! fits (src/discrete.jl:211)")
    if isinstance(process.baseline, DiscreteLogGaussianCoxProcess):
        raise NotImplementedError(f"{what} takes the homogeneous baseline (the LGCP baseline is not covered)")


def _disc_kind(kind):
    if kind not in _INFORMATION_KINDS:
        raise ValueError("kind must be 'observed' or 'fisher'")
    return _INFORMATION_KINDS[kind]


def disc_block_index(N, B, c):
    """Positions in [λ0; vec(η)] of the rows of column c's block: λ0[c], then η[p,c,b] at row 1 + b·N + p."""
    return np.concatenate([[c], N + (np.arange(B)[:, None] * N * N + np.arange(N)[None, :] + c * N).ravel()])


def disc_observed_information(process, data=None, convolved=None, columns=None, kind="observed", device=False, tile_rows=0,
                              slab_bins=0, ctx=None):
    """The information of the discrete log-likelihood in mle_'s parameters [λ0; vec(η)], η = W∘θ, at the process's current
    parameters (nhp_disc_information).

    The intensity is linear in these parameters, so the information is block diagonal by child node: `blocks[k]` is the
    D x D block, D = 1 + N·B, of column c = columns[k] (all columns in order by default) over [λ0[c]; η[:,c,:]] -- row 0 is
    λ0[c], row 1 + b·N + p is η[p,c,b]; `names[r]` = ("λ0", None, None) or ("η", p, b).  kind="observed": minus the
    Hessian, dt²·Σ_t (s/λ²)·x xᵀ; kind="fisher": its expectation under the model, dt²·Σ_t (1/λ)·x xᵀ.  Both are positive
    semi-definite, exactly symmetric and bit-reproducible.  tile_rows (a multiple of 16 up to 96) and slab_bins force the
    tiling of a block and of the time axis (0: automatic).  device=False: numpy [n_columns, D, D]; device=True: a float64
    torch tensor view of the buffer the kernels wrote.  Returns DiscreteInformation(ll, columns, blocks, names, kind)."""
    from .inference import _check_columns
    _disc_information_check(process, "disc_observed_information")
    code = _disc_kind(kind)
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    N, B = ds.N, ds.B
    cols = _check_columns(columns, N)
    for name, v in (("tile_rows", tile_rows), ("slab_bins", slab_bins)):
        if not (isinstance(v, (int, np.integer)) and v >= 0):
            raise ValueError(f"{name} must be a non-negative integer (0: automatic)")
    D = 1 + N * B
    l0, W, th, _ = process._lowered()
    ll = C.c_double()
    fn = _lib.lib().nhp_disc_information
    args = (ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), process.dt, code, cols.ctypes.data_as(C.POINTER(C.c_int32)),
            len(cols), int(tile_rows), int(slab_bins), C.byref(ll))
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        out = torch.empty((len(cols), D, D), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffer's memory are done before the library writes
        _lib.check(fn(*args, out.data_ptr()), ctx.h)
        blocks = out.transpose(1, 2)                           # column-major blocks (symmetric: the same numbers)
    else:
        out = np.empty((len(cols), D, D))
        _lib.check(fn(*args, out.ctypes.data), ctx.h)
        blocks = out.transpose(0, 2, 1)
    names = [("λ0", None, None)] + [("η", p, b) for b in range(B) for p in range(N)]
    return DiscreteInformation(ll.value, cols.copy(), blocks, names, kind)


def disc_hessian_vector_product(process, data=None, convolved=None, v=None, kind="observed", device=False, ctx=None):
    """J·v for the information J of the given kind (disc_observed_information: MINUS the Hessian of the log-likelihood for
    kind="observed", positive semi-definite sign), v and the result full-length vectors in mle_'s order [λ0; vec(η)]
    (nhp_disc_hessian_vec: two intensity launches and the gradient's Gᵀ·R, no block is stored).  device=False: numpy in and
    out; device=True: float64 torch tensors on the context's device."""
    _disc_information_check(process, "disc_hessian_vector_product")
    code = _disc_kind(kind)
    if v is None:
        raise ValueError("v is required")
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    P = ds.N + ds.N * ds.N * ds.B
    if device:
        import torch
        if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (P,)):
            raise ValueError(f"device=True takes a float64 tensor of length {P} on the context's device")
    else:
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (P,):
            raise ValueError("Parameter vector length does not match model parameter length.")
    l0, W, th, _ = process._lowered()
    fn = _lib.lib().nhp_disc_hessian_vec
    args = (ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), process.dt, code)
    if device:
        dev = torch.device("cuda", ctx.device)
        v = v.contiguous()
        out = torch.empty(P, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(fn(*args, v.data_ptr(), out.data_ptr()), ctx.h)
        return out
    out = np.empty(P)
    _lib.check(fn(*args, v.ctypes.data, out.ctypes.data), ctx.h)
    return out


def _disc_standard_errors_from_blocks(blocks, cols, x, N, B, lower, upper, level):
    """disc_standard_errors' host part: free sets, Cholesky inverses of the free sub-blocks, Wald intervals, and the
    standard errors of W = Σ_b η (exact) and θ = η/W (delta method) from each link's B x B covariance."""
    from scipy.linalg import solve_triangular
    from scipy.stats import norm
    P = len(x)
    se = np.full(P, np.nan)
    free = np.zeros(P, dtype=bool)
    pd = np.zeros(len(cols), dtype=bool)
    se_W = np.full((N, N), np.nan)
    se_theta = np.full((N, N, B), np.nan)
    for k, c in enumerate(cols):
        idx = disc_block_index(N, B, int(c))
        J = np.asarray(blocks[k], dtype=np.float64)
        inside = (x[idx] > lower) & (x[idx] < upper)
        f = inside & np.any(J != 0.0, axis=1)
        sub = J[np.ix_(f, f)]
        ok = bool(f.any() and np.all(np.isfinite(sub)))
        if ok:
            try:
                L = np.linalg.cholesky(sub)
                Li = solve_triangular(L, np.eye(len(L)), lower=True)
                cov = Li.T @ Li
                var = np.diag(cov)
                ok = bool(np.all(np.isfinite(var)) and np.all(var > 0.0))
            except np.linalg.LinAlgError:
                ok = False
        pd[k] = ok
        if not ok:
            continue
        free[idx[f]] = True
        se[idx[f]] = np.sqrt(var)
        pos = np.full(len(idx), -1)
        pos[f] = np.arange(int(f.sum()))
        for p in range(N):
            rows = 1 + np.arange(B) * N + p                        # η[p,c,·] in the block
            fr = f[rows]
            if not fr.any():
                continue
            S = cov[np.ix_(pos[rows[fr]], pos[rows[fr]])]          # a bound or unidentified η[p,c,b] is held fixed
            se_W[p, c] = np.sqrt(S.sum())
            eta = x[idx[rows]]
            w = eta.sum()
            G = (np.eye(B) - (eta / w)[:, None]) / w               # ∂θ_b/∂η_b' = (δ_bb' - θ_b)/W
            Gf = G[:, fr]
            se_theta[p, c] = np.sqrt(np.maximum(np.einsum("ij,jk,ik->i", Gf, S, Gf), 0.0))
    z = norm.ppf(0.5 + 0.5 * level)
    return DiscreteStandardErrors(se, x - z * se, x + z * se, free, pd, se_W, se_theta)


def disc_standard_errors(process, data=None, convolved=None, columns=None, kind="observed", lower=1e-6, upper=10.0, level=0.95,
                         ctx=None):
    """Standard errors and Wald intervals of a fitted DiscreteStandardHawkesProcess from the inverse information
    (disc_observed_information; the blocks are Cholesky-inverted on the host).

    se, lower_ci, upper_ci [P] in mle_'s order [λ0; vec(η)], NaN for the parameters that are not free and the columns not
    asked for; free [P]: the parameters the inverse was taken over -- those strictly inside the box (lower, upper) whose
    row of the column's block is not identically zero; pd [n_columns]: the free sub-block of column columns[k] is positive
    definite (a column that is not gets NaNs, no exception).  se_W [N, N]: sqrt(1ᵀ Cov(η[p,c,·]) 1), exact because
    W = Σ_b η; se_theta [N, N, B]: the delta method for θ = η/W.  There is no `regularize`."""
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie in (0, 1)")
    if not lower < upper:
        raise ValueError("lower must be below upper")
    info = disc_observed_information(process, data, convolved, columns=columns, kind=kind, ctx=ctx)
    N, B = process.ndims(), process.impulses.nbasis()
    return _disc_standard_errors_from_blocks(info.blocks, info.columns, process.params(), N, B, lower, upper, level)


def resample_parent_counts(process, data=None, convolved=None, seed=0, step=0, ctx=None):
    """Σ_t resample_parents(process, data, convolved)[t, :, :] -> N x (1 + N·B) integer counts
    (src/parents.jl:82-116): column 0 the baseline, column 1 + p·B + b parent node p through basis b
    (0-based p, b) -- the reduction every discrete resample! applies to the T x N x (1+NB) array, which is
    never materialised here.  Draws are keyed (seed, step), reproducible, and equal to the oracle."""
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, A = process._lowered()
    N, B = ds.N, ds.B
    out = np.empty(N * (1 + N * B), dtype=np.int64)
    _lib.check(_lib.lib().nhp_disc_resample_parents(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                                    process.dt, seed, step, _lib.iptr(out)), ctx.h)
    return out.reshape((N, 1 + N * B), order="F")


def disc_parent_counts(counts, ndims, nbasis):
    """parent_counts(parents, ndims, nbasis) on the time-reduced array -- src/parents.jl:123-134"""
    return counts[:, 1:].reshape((ndims, ndims, nbasis)).sum(axis=2).T.astype(np.float64)      # [parent, child]


def disc_resample_adjacency_matrix_(process, data=None, convolved=None, u=None, seed=0, step=0, ctx=None):
    """resample_adjacency_matrix!(process, data, convolved) -- src/discrete.jl:424-480: one Gibbs sweep of
    the adjacency matrix on the GPU.  `u` (N x N, [parent, child]) supplies the Bernoulli uniforms
    explicitly; otherwise Philox keyed (seed, step).  Updates process.adjacency_matrix, returns ΣA."""
    from .components import BernoulliNetworkModel, DenseNetworkModel
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    l0, W, th, _ = process._lowered()
    N = ds.N
    if isinstance(process.network, BernoulliNetworkModel):
        scalar, rho_m = float(process.network.ρ), None
    elif isinstance(process.network, DenseNetworkModel):
        scalar, rho_m = 1.0, None
    else:
        scalar, rho_m = 0.5, _lib.colmajor(np.asarray(process.network.link_probability(), dtype=np.float64))
    A = _lib.colmajor(process.adjacency_matrix).copy()
    uu = None if u is None else _lib.colmajor(np.asarray(u, dtype=np.float64))
    nl = C.c_double()
    _lib.check(_lib.lib().nhp_disc_resample_adjacency(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A),
                                                      process.dt, _lib.dptr(rho_m), scalar, _lib.dptr(uu), seed, step,
                                                      C.byref(nl)), ctx.h)
    process.adjacency_matrix = A.reshape((N, N), order="F")
    return nl.value


def _resample_network(process, links, N, rng, seed, step, ctx):
    """resample!(network, A) after the adjacency sweep: the block and the latent distance model need the swept matrix, the
    others its link count."""
    from .components import LatentDistanceNetworkModel, StochasticBlockNetworkModel
    if isinstance(process.network, (StochasticBlockNetworkModel, LatentDistanceNetworkModel)):
        process.network.resample_(process.adjacency_matrix, rng, seed=seed, step=step, ctx=ctx)
    else:
        process.network.resample_links_(links, N * N, rng)


def disc_resample_(process, data, convolved, rng, seed=0, step=0, ctx=None, device_draws=True):
    """resample!(process::DiscreteStandardHawkesProcess, data, convolved) -- src/discrete.jl:362-368, and the
    network twin :416-424 (adds the adjacency sweep and the network's ρ).

    Parent counts come from the GPU; the conjugate draws are numpy (statistical, not bitwise, parity with
    Julia's samplers).  The reference's baseline update is broken for the homogeneous process (it passes
    the T x N slice to a helper that expects N x T: SURVEY D2); the intended update is applied:
    λ ~ Gamma(α0 + Σ_t parents[t, c, 1], 1 / (β0 + T·dt))  (src/baselines.jl:413-419)."""
    if not isinstance(process.weights, DenseWeightModel):
        raise NotImplementedError("discrete Gibbs is built for DenseWeightModel (SparseWeightModel: SURVEY 2.1)")
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    N, B = ds.N, ds.B
    b, w, imp = process.baseline, process.weights, process.impulses
    if device_draws and isinstance(b, DiscreteHomogeneousProcess):
        # parents and conjugate draws in one GPU call (nhp_disc_gibbs_step): only the new parameters come back
        l0, W, th, A = process._lowered()
        l0, W, th = l0.copy(), W.copy(), th.copy()
        _lib.check(_lib.lib().nhp_disc_gibbs_step(ctx.h, ds.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A), process.dt,
                                                  b.α0, b.β0, w.κ, w.ν, imp.γ, seed, step), ctx.h)
        b.λ, w.W, imp.θ = l0, W.reshape((N, N), order="F"), th.reshape((N, N, B), order="F")
        if isinstance(process, DiscreteNetworkHawkesProcess):
            links = disc_resample_adjacency_matrix_(process, convolved=ds, seed=seed, step=step, ctx=ctx)
            _resample_network(process, links, N, rng, seed, step, ctx)
        return process.params()
    counts = resample_parent_counts(process, convolved=ds, seed=seed, step=step, ctx=ctx)
    if isinstance(b, DiscreteLogGaussianCoxProcess):
        b.resample_(ds, rng)              # elliptical slice on parents[:, :, 1], left on the device by the sweep above
    else:
        b.λ = rng.gamma(b.α0 + counts[:, 0], 1.0 / (b.β0 + ds.T * b.dt))
    Mnm = disc_parent_counts(counts, N, B)
    w.W = rng.gamma(w.κ + Mnm, 1.0 / (w.ν + ds.node_counts)[:, None] * np.ones((N, N)))        # src/weights.jl:59-64
    γ = imp.γ + counts[:, 1:].reshape((N, N, B)).transpose(1, 0, 2)                                  # [parent, child, basis]
    g = rng.gamma(γ, 1.0)
    imp.θ = g / g.sum(axis=2, keepdims=True)                                                         # Dirichlet: src/impulses.jl:337-353
    if isinstance(process, DiscreteNetworkHawkesProcess):
        links = disc_resample_adjacency_matrix_(process, convolved=ds, seed=seed, step=step, ctx=ctx)
        _resample_network(process, links, N, rng, seed, step, ctx)
    return process.params()


class DiscreteDeviceModel:
    """nhp_disc_model handle: the state of a discrete chain in one device block, [λ0; vec(W); vec(θ); vec(A) of a network
    process], with the network's scalar ρ beside it (csrc/disc_chain.hip)."""

    def __init__(self, ctx, process):
        self.ctx, self.N, self.B = ctx, process.ndims(), process.impulses.nbasis()
        self.network = isinstance(process, DiscreteNetworkHawkesProcess)
        self.h = C.c_void_p()
        _lib.check(_lib.lib().nhp_disc_model_create(ctx.h, self.N, self.B, int(self.network), process.dt, C.byref(self.h)), ctx.h)
        self.push(process)

    def push(self, process):
        """The process's λ0, W, θ (A, ρ) onto the device."""
        from .components import BernoulliNetworkModel
        l0, W, th, A = process._lowered()
        _lib.check(_lib.lib().nhp_disc_model_set(self.ctx.h, self.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A)), self.ctx.h)
        if self.network:
            rho = float(process.network.ρ) if isinstance(process.network, BernoulliNetworkModel) else 1.0
            _lib.check(_lib.lib().nhp_disc_model_set_rho(self.ctx.h, self.h, rho), self.ctx.h)

    def pull(self, process):
        """The device state into the process's components; returns {ρ, Σρ, Σρ²} (zeros without a Bernoulli network)."""
        from .components import BernoulliNetworkModel
        N, B = self.N, self.B
        l0, W, th = np.empty(N), np.empty(N * N), np.empty(N * N * B)
        A = np.empty(N * N) if self.network else None
        _lib.check(_lib.lib().nhp_disc_model_get(self.ctx.h, self.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A)), self.ctx.h)
        process.baseline.λ, process.weights.W = l0, W.reshape((N, N), order="F")
        process.impulses.θ = th.reshape((N, N, B), order="F")
        r3 = np.zeros(3)
        if self.network:
            process.adjacency_matrix = A.reshape((N, N), order="F")
            if isinstance(process.network, BernoulliNetworkModel):
                _lib.check(_lib.lib().nhp_disc_model_get_rho(self.ctx.h, self.h, _lib.dptr(r3)), self.ctx.h)
                process.network.ρ = float(r3[0])
        return r3

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().nhp_disc_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def disc_moments_length(process):
    """Length of the device-side running sums of nhp_disc_model_moments_*: params(process) without the network's ρ."""
    N, B = process.ndims(), process.impulses.nbasis()
    return N + N * N * B + (2 * N * N if isinstance(process, DiscreteNetworkHawkesProcess) else 0)


def _check_resident(process, device_draws):
    """NotImplementedError naming what the device-resident discrete chain (nhp_disc_model) is not built for."""
    from .components import BernoulliNetworkModel, DenseNetworkModel, SparseWeightModel
    route = "the default route (keep_samples=True, moments=False) takes it"
    if not isinstance(process.baseline, DiscreteHomogeneousProcess):
        raise NotImplementedError(f"the device-resident discrete chain draws a homogeneous baseline (baseline: "
                                  f"{type(process.baseline).__name__}); {route}")
    if isinstance(process.weights, SparseWeightModel) or not isinstance(process.weights, DenseWeightModel):
        raise NotImplementedError(f"the device-resident discrete chain is built for DenseWeightModel (weights: "
                                  f"{type(process.weights).__name__}); {route}")
    if not device_draws:
        raise NotImplementedError(f"the device-resident discrete chain draws on the device (device_draws=False draws with numpy); {route}")
    if isinstance(process, DiscreteNetworkHawkesProcess) and not isinstance(process.network, (DenseNetworkModel, BernoulliNetworkModel)):
        raise NotImplementedError(f"the device-resident discrete chain holds a DenseNetworkModel or a BernoulliNetworkModel (network: "
                                  f"{type(process.network).__name__} keeps its state on the host); {route}")


def _disc_fetch_diagnostics(process, model, ctx, full, ess_below, rhat_above):
    """nhp_disc_model_diagnostics_fetch -> {"summary"[, "ess", "mcse", "rhat"]}; the per-entry arrays in params(process) order
    (the network's ρ first: its single entry is its group's extreme)."""
    from .components import BernoulliNetworkModel
    from .inference import DIAGNOSTIC_FIELDS
    L = disc_moments_length(process)
    summary = np.empty(_lib.DIAG_GROUPS * _lib.DIAG_FIELDS)
    planes = [np.empty(L) for _ in range(3)] if full else [None] * 3
    _lib.check(_lib.lib().nhp_disc_model_diagnostics_fetch(ctx.h, model.h, float(ess_below), float(rhat_above), _lib.dptr(summary),
                                                          *[_lib.dptr(v) for v in planes], L), ctx.h)
    summary = summary.reshape(_lib.DIAG_GROUPS, _lib.DIAG_FIELDS)
    network = model.network
    bernoulli = network and isinstance(process.network, BernoulliNetworkModel)
    names = ["baseline", "impulses.θ" if network else "weights∘impulses", None, "weights" if network else None,
             "adjacency" if network else None, "network.ρ" if bernoulli else None]
    ints = ("entries", "undefined", "min_ess_index", "max_rhat_index", "ess_below", "rhat_above")
    out = {"summary": {name: {f: (int(v) if f in ints else float(v)) for f, v in zip(DIAGNOSTIC_FIELDS, row)}
                       for name, row in zip(names, summary) if name is not None}}
    if full:
        if bernoulli:
            planes = [np.concatenate([[r], v]) for v, r in zip(planes, summary[5, [2, 8, 4]])]
        out["ess"], out["mcse"], out["rhat"] = planes
    return out


def _disc_fetch_quantiles(process, model, ctx, probs, every, effective):
    """nhp_disc_model_quantiles_fetch -> inference.ChainQuantiles in params(process) order (the network's ρ first; only a
    BernoulliNetworkModel's has a state)."""
    from .components import BernoulliNetworkModel
    from .inference import ChainQuantiles
    L, m = disc_moments_length(process), len(probs)
    values, lo, hi, rho = np.empty((m, L)), np.empty(L), np.empty(L), np.empty(m + 2)
    cnt = C.c_int64()
    _lib.check(_lib.lib().nhp_disc_model_quantiles_fetch(ctx.h, model.h, _lib.dptr(values), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(rho), L,
                                                        C.byref(cnt)), ctx.h)
    if model.network:
        k = len(process.network.params())
        if not isinstance(process.network, BernoulliNetworkModel):
            rho = np.full(m + 2, np.nan)
        values = np.concatenate([np.repeat(rho[:m, None], k, axis=1), values], axis=1)
        lo, hi = np.concatenate([np.full(k, rho[m]), lo]), np.concatenate([np.full(k, rho[m + 1]), hi])
    return ChainQuantiles(probs, values, lo, hi, cnt.value, every, effective)


# ---- scoring a chain: held-out predictive log-likelihood and WAIC (csrc/disc_score.hip) ---------------------------------------
SCORE_FIELDS = ("n", "cells", "lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "joint_lpd", "joint_mean", "joint_sd")


class DiscreteScore:
    """What nhp_disc_score_fetch returns for the cells of bins [t0, t1), all nodes, over `n` kept draws (definitions:
    include/nhp.h).  `lppd`, `p_waic`, `elpd_waic`, `waic` = −2·elpd_waic and `se_elpd` are the pointwise scores summed over
    the cells; `joint_lpd` = log mean_s p(all scored cells | θ_s) is the predictive log-likelihood of the bins as a whole (the
    number to report for held-out bins), `joint_mean` and `joint_sd` the mean and spread of the draws' log-likelihoods.
    `per_node` is a 3 x N array (lppd, p_waic, elpd_waic per node), `pointwise` -- when asked for -- the R x N array of
    elpd_i that compare_scores needs."""

    def __init__(self, summary, per_node, pointwise, bins):
        for name, v in zip(SCORE_FIELDS, summary):
            setattr(self, name, int(v) if name in ("n", "cells") else float(v))
        self.per_node, self.pointwise, self.bins = per_node, pointwise, (int(bins[0]), int(bins[1]))

    def __repr__(self):
        return (f"DiscreteScore(bins={self.bins}, n={self.n}, waic={self.waic:.6g}, elpd_waic={self.elpd_waic:.6g} ± {self.se_elpd:.3g}, "
                f"p_waic={self.p_waic:.4g}, joint_lpd={self.joint_lpd:.6g})")


class ScoreComparison:
    """compare_scores(a, b): elpd_diff = Σ_i (elpd_a,i − elpd_b,i) (positive: a predicts better) and its standard error."""

    def __init__(self, elpd_diff, se_diff, cells):
        self.elpd_diff, self.se_diff, self.cells = float(elpd_diff), float(se_diff), int(cells)

    def __repr__(self):
        return f"ScoreComparison(elpd_diff={self.elpd_diff:.6g} ± {self.se_diff:.3g}, cells={self.cells})"


def compare_scores(a, b):
    """The difference of two models' elpd_waic over the same cells, with the standard error of the paired difference,
    sqrt(cells · var_i(elpd_a,i − elpd_b,i)) (sample variance): plain numpy on the two `pointwise` arrays."""
    for s in (a, b):
        if getattr(s, "pointwise", None) is None:
            raise ValueError("compare_scores needs scores with pointwise values (pointwise=True)")
    pa, pb = np.asarray(a.pointwise, dtype=np.float64), np.asarray(b.pointwise, dtype=np.float64)
    if pa.shape != pb.shape:
        raise ValueError(f"the scores cover different cells: {pa.shape} and {pb.shape}")
    if tuple(a.bins) != tuple(b.bins):
        raise ValueError(f"the scores cover different bins: {tuple(a.bins)} and {tuple(b.bins)}")
    d = (pa - pb).ravel()
    se = np.sqrt(d.size * np.var(d, ddof=1)) if d.size > 1 else np.nan
    return ScoreComparison(d.sum(), se, d.size)


class _DeviceScore:
    """nhp_disc_score handle on a convolved dataset (kept alive with it)."""

    def __init__(self, ctx, ds, bins):
        self.ctx, self.ds, self.bins = ctx, ds, bins
        self.h = C.c_void_p()
        _lib.check(_lib.lib().nhp_disc_score_create(ctx.h, ds.h, int(bins[0]), int(bins[1]), C.byref(self.h)), ctx.h)

    def accumulate(self, model):
        _lib.check(_lib.lib().nhp_disc_score_accumulate(self.ctx.h, self.h, model.h), self.ctx.h)

    def fetch(self, pointwise=False):
        N, R = self.ds.N, self.bins[1] - self.bins[0]
        summary, per_node = np.empty(len(SCORE_FIELDS)), np.empty(3 * N)
        pw = np.empty(R * N) if pointwise else None
        _lib.check(_lib.lib().nhp_disc_score_fetch(self.ctx.h, self.h, _lib.dptr(summary), _lib.dptr(per_node), _lib.dptr(pw)), self.ctx.h)
        return DiscreteScore(summary, per_node.reshape(3, N), pw.reshape((R, N), order="F") if pointwise else None, self.bins)

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().nhp_disc_score_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _data_shape(data):
    if isinstance(data, DiscreteDataset):
        return data.N, data.T
    if _is_trials(data):
        return _trials(data).shape
    shape = np.shape(data)
    if len(shape) != 2:
        raise ValueError("data must be an N x T matrix")
    return shape


def _check_bins(bins, T, what):
    try:
        t0, t1 = bins
        t0, t1 = int(t0), int(t1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bins must be a pair (t0, t1)") from None
    if not 0 <= t0 < t1 <= T:
        raise ValueError(f"{what}: bins [{t0}, {t1}) must satisfy 0 <= t0 < t1 <= T = {T}")
    return t0, t1


def _score_plan(process, data, waic, heldout, score_every, burn):
    """The scorers a chain was asked for, as [(name, data or None for the chain's own, (t0, t1))]; every argument is checked here,
    before the library is touched."""
    if not waic and heldout is None:
        return []
    if int(score_every) != score_every or int(score_every) < 1:
        raise ValueError("score_every must be a positive integer")
    if int(burn) < 0:
        raise ValueError("burn must be non-negative when the chain is scored")
    if not isinstance(process.baseline, DiscreteHomogeneousProcess):
        raise NotImplementedError(f"scoring a discrete chain needs a homogeneous baseline (baseline: {type(process.baseline).__name__}: "
                                  f"its draws are not part of the device model)")
    N, T = _data_shape(data)
    plan = []
    if waic:
        plan.append(("waic", None, (0, int(T))))
    if heldout is not None:
        # (data_full, (t0, t1)) has a pair of bins second; any other tuple of matrices is a tuple of trials
        with_bins = isinstance(heldout, tuple) and len(heldout) == 2 and np.ndim(heldout[1]) < 2
        if with_bins or (isinstance(heldout, tuple) and not _is_trials(heldout)):
            if len(heldout) != 2:
                raise ValueError("heldout must be (data_full, (t0, t1)) or a count matrix")
            hd, bins = heldout
        else:
            hd, bins = heldout, None
        hN, hT = _data_shape(hd)
        if hN != N:
            raise ValueError(f"heldout data has {hN} nodes, the chain's data {N}")
        plan.append(("heldout", hd, _check_bins(bins if bins is not None else (0, hT), hT, "heldout")))
    return plan


def _open_scorers(ctx, process, ds, plan):
    out = []
    for name, data, bins in plan:
        out.append((name, _DeviceScore(ctx, ds if data is None else convolve(process, data, ctx), bins)))
    return out


def _close_scorers(res, scorers, pointwise):
    """Fetch every scorer into res.<name> (a chain that kept no step leaves None) and release it."""
    try:
        for name, s in scorers:
            setattr(res, name, None)
        for name, s in scorers:
            try:
                setattr(res, name, s.fetch(pointwise))
            except _lib.NhpError as e:
                if "nothing accumulated" not in str(e):
                    raise
    finally:
        for _, s in scorers:
            s.close()


def _sample_arrays(process, x):
    """(λ0, W, θ, A) that reproduce the intensity of the draw x = params(process).  A network process's sample holds the four
    arrays themselves.  A standard process's holds η = W∘θ, which is all the intensity depends on: (W, θ) = (1, η) gives the
    chain's bump table entry (W·θ)·dt bit for bit, where params!'s split W = Σ_b η, θ = η / W multiplies back to a neighbour."""
    N, B = process.ndims(), process.impulses.nbasis()
    NN = N * N
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (len(process.params()),):
        raise ValueError("Parameter vector length does not match model parameter length.")
    if isinstance(process, DiscreteNetworkHawkesProcess):
        l0, W, th, A = np.split(x[len(x) - (N + 2 * NN + NN * B):], [N, N + NN, N + NN + NN * B])
        return l0.copy(), W.copy(), th.copy(), A.copy()
    return x[:N].copy(), np.ones(NN), x[N:].copy(), None


def disc_score_samples(process, samples, data, bins=None, burn=0, every=1, pointwise=False, ctx=None):
    """Score the draws of a finished chain: samples[burn], samples[burn + every], … (each a params(process) vector, as
    res.samples holds them) on bins [t0, t1) of `data` (all of it by default).  Every draw is set into a device model through
    params! and accumulated as the chain itself would have (nhp_disc_score_accumulate): for the same draws the result is
    the in-chain score bit for bit.  The process supplies the shapes, the basis and dt; it is not changed."""
    if int(every) != every or int(every) < 1:
        raise ValueError("every must be a positive integer")
    if int(burn) != burn or int(burn) < 0:
        raise ValueError("burn must be a non-negative integer")
    samples = list(samples)
    if int(burn) >= len(samples):
        raise ValueError(f"no draws left: {len(samples)} samples, burn = {burn}")
    if not isinstance(process.baseline, DiscreteHomogeneousProcess):
        raise NotImplementedError(f"scoring needs a homogeneous baseline (baseline: {type(process.baseline).__name__})")
    data = _trials(data)
    N, T = _data_shape(data)
    if N != process.ndims():
        raise ValueError(f"data has {N} nodes, the process {process.ndims()}")
    bins = _check_bins(bins if bins is not None else (0, T), T, "disc_score_samples")
    draws = [_sample_arrays(process, x) for x in samples[int(burn)::int(every)]]
    ctx = ctx or _lib.default_context()
    ds = data if isinstance(data, DiscreteDataset) and data.B else convolve(process, data, ctx)
    model, scorer = DiscreteDeviceModel(ctx, process), None
    try:
        scorer = _DeviceScore(ctx, ds, bins)
        for l0, W, th, A in draws:
            _lib.check(_lib.lib().nhp_disc_model_set(ctx.h, model.h, _lib.dptr(l0), _lib.dptr(W), _lib.dptr(th), _lib.dptr(A)), ctx.h)
            scorer.accumulate(model)
        return scorer.fetch(pointwise)
    finally:
        if scorer is not None:
            scorer.close()
        model.close()


def _disc_mcmc_resident(process, data, nsteps, log_freq, verbose, seed, ctx, keep_samples, moments, burn, diagnostics, batch_len,
                        ess_below, rhat_above, plan=(), score_every=1, pointwise=False, qprobs=None, quantiles_every=1,
                        effective_weights=False):
    """The chain with its state on the device (nhp_disc_model): nothing is uploaded after the start; with keep_samples the
    state comes back once per step, without it the whole chain is nhp_disc_mcmc_run."""
    import math
    import time
    from .components import BernoulliNetworkModel
    from .inference import MarkovChainMonteCarlo
    ctx = ctx or _lib.default_context()
    ds = convolve(process, data, ctx)
    lib = _lib.lib()
    model = DiscreteDeviceModel(ctx, process)
    b, w, imp = process.baseline, process.weights, process.impulses
    pri = (b.α0, b.β0, w.κ, w.ν, imp.γ)
    net = process.network if model.network else None
    net_a, net_b = (net.α, net.β) if isinstance(net, BernoulliNetworkModel) else (0.0, 0.0)
    if diagnostics:
        n_planned = max(0, int(nsteps) - int(burn))
        diag_b = int(batch_len) if batch_len is not None else max(1, math.isqrt(n_planned))
        _lib.check(lib.nhp_disc_model_diagnostics_configure(ctx.h, model.h, diag_b, n_planned), ctx.h)
    if qprobs is not None:
        _lib.check(lib.nhp_disc_model_quantiles_configure(ctx.h, model.h, _lib.dptr(qprobs), len(qprobs), int(quantiles_every),
                                                          1 if effective_weights else 0), ctx.h)
    if moments:
        _lib.check(lib.nhp_disc_model_moments_reset(ctx.h, model.h), ctx.h)
    res = MarkovChainMonteCarlo()
    start = time.time()
    scorers, kept, qkept = [], 0, 0
    try:
        scorers = _open_scorers(ctx, process, ds, plan)
        if not keep_samples:
            for _, s in scorers:                 # nhp_disc_mcmc_run scores the kept steps itself
                _lib.check(lib.nhp_disc_model_attach_score(ctx.h, model.h, s.h, int(score_every)), ctx.h)
        # the driver's kept steps without moments: from −(burn + 1) on (include/nhp.h)
        run_burn = burn if moments else (-1 - int(burn) if scorers else -1)
        while res.steps < nsteps:
            if keep_samples:
                _lib.check(lib.nhp_disc_model_gibbs_step(ctx.h, ds.h, model.h, *pri, seed, res.steps), ctx.h)
                if model.network:
                    _lib.check(lib.nhp_disc_model_network_step(ctx.h, ds.h, model.h, net_a, net_b, seed, res.steps), ctx.h)
                if moments and res.steps >= burn:
                    _lib.check(lib.nhp_disc_model_moments_accumulate(ctx.h, model.h), ctx.h)
                    if qprobs is not None:
                        if qkept % int(quantiles_every) == 0:
                            _lib.check(lib.nhp_disc_model_quantiles_accumulate(ctx.h, model.h), ctx.h)
                        qkept += 1
                if scorers and res.steps >= burn:
                    if kept % int(score_every) == 0:
                        for _, s in scorers:
                            s.accumulate(model)
                    kept += 1
                model.pull(process)
                res.samples.append(process.params())
                n = 1
            else:
                n = min(nsteps - res.steps, log_freq if verbose else nsteps)
                _lib.check(lib.nhp_disc_mcmc_run(ctx.h, ds.h, model.h, *pri, net_a, net_b, seed, res.steps, n, run_burn), ctx.h)
            res.steps += n
            if res.steps % log_freq == 0 and verbose:
                res.elapsed = time.time() - start
                print(f" > step: {res.steps}, elapsed: {res.elapsed}")
        r3 = model.pull(process)
        res.elapsed = time.time() - start
        res.status = "complete"
        if not keep_samples:
            res.samples.append(process.params())
        if moments:
            L = disc_moments_length(process)
            s, q, cnt = np.empty(L), np.empty(L), C.c_int64()
            _lib.check(lib.nhp_disc_model_moments_fetch(ctx.h, model.h, _lib.dptr(s), _lib.dptr(q), L, C.byref(cnt)), ctx.h)
            res.n = cnt.value
            n = max(1, res.n)
            k = len(net.params()) if model.network else 0                 # params(process) = [ρ; λ0; W; θ; vec(A)]
            res.mean, res.m2 = np.concatenate([np.full(k, r3[1] / n), s / n]), np.concatenate([np.full(k, r3[2] / n), q / n])
            if diagnostics and res.n < 1:
                res.diagnostics = {"summary": {}}               # no kept step: nothing to diagnose
            elif diagnostics:
                res.diagnostics = _disc_fetch_diagnostics(process, model, ctx, diagnostics == "full", ess_below, rhat_above)
            if diagnostics:
                res.diagnostics.update(n=res.n, batch_len=diag_b, nbatches=res.n // diag_b)
            if qprobs is not None:
                res.quantiles = _disc_fetch_quantiles(process, model, ctx, qprobs, int(quantiles_every), effective_weights)
        _close_scorers(res, scorers, pointwise)
    finally:
        for _, s in scorers:
            s.close()
        model.close()
    return res


def disc_mcmc_(process, data, nsteps=1000, log_freq=100, verbose=False, seed=0, ctx=None, device_draws=True, keep_samples=True,
               moments=False, burn=0, diagnostics=False, batch_len=None, ess_below=100.0, rhat_above=1.01, waic=False,
               heldout=None, score_every=1, pointwise=False, quantiles=False, quantiles_every=1, effective_weights=False):
    """mcmc!(process::DiscreteHawkesProcess, data) -- src/inference.jl:49-70: convolve once, then
    resample!(process, data, convolved) per step.

    By default every step takes the process's arrays to the device and back and `res.samples` holds params(process) of every
    step.  `moments=True` or `keep_samples=False` keeps the chain's state on the device instead (nhp_disc_model,
    csrc/disc_chain.hip: the same kernels on the same bits, so λ0, W, θ and A are those of the default route step for step;
    the network's ρ is drawn on the device, as the continuous chain draws it).  With keep_samples=True the state comes back
    once per step and nothing is uploaded; with keep_samples=False the whole chain runs inside the library
    (nhp_disc_mcmc_run, cut at `log_freq` only when `verbose`) and res.samples holds the final params(process) alone.
    Either way the process holds the final state afterwards.

    `moments`, `burn`, `diagnostics`, `batch_len`, `ess_below`, `rhat_above` are those of the continuous mcmc_
    (inference.mcmc_): res.mean and res.m2 over the steps >= burn in params(process) order, res.diagnostics with `n`,
    `batch_len`, `nbatches` and `summary` per group -- "baseline", "weights∘impulses" for a standard process, and
    "weights", "impulses.θ", "adjacency", "network.ρ" (a BernoulliNetworkModel's) for a network process -- and with
    diagnostics="full" `ess`, `mcse`, `rhat` per entry.  Definitions: include/nhp.h.

    The device-resident route needs a homogeneous baseline, a DenseWeightModel, device_draws=True and a DenseNetworkModel or
    BernoulliNetworkModel: anything else is NotImplementedError (the default route takes it).

    Scoring (csrc/disc_score.hip; definitions in include/nhp.h, results as DiscreteScore): `waic=True` scores the chain's own
    bins, `heldout=(data_full, (t0, t1))` bins [t0, t1) of another count matrix with the same draws -- fit on
    data_full[:, :t0] and pass the full matrix, so that the history before t0 stays in the convolution -- or
    `heldout=data_test` every bin of a matrix of its own.  Every `score_every`-th step from `burn` on is scored, on the
    device, as the step is kept: nothing is stored per draw.  The results are res.waic and res.heldout (None when no step
    was kept), with `pointwise=True` including the per-cell elpd that compare_scores takes.  On the resident routes the
    chain's device model is scored in place; on the default route -- every model it takes -- each scored step's state is set
    into a device model kept for scoring.  A baseline other than DiscreteHomogeneousProcess is NotImplementedError.

    `quantiles`, `quantiles_every`, `effective_weights` are those of the continuous mcmc_ too (csrc/chain_quantiles.hip;
    definition in include/nhp.h): with `moments=True`, res.quantiles is a ChainQuantiles over params(process) -- for a standard
    process the quantiles of the products W∘θ the sums take, for a network process those of W (or A·W), θ and a
    BernoulliNetworkModel's ρ, NaN at vec(A).  They live next to the device-resident model, so whatever that route refuses
    (above) is NotImplementedError here as well.

    `data` (and the data of `heldout`) may be a list or tuple of N x T_r matrices, independent trials, or a DiscreteDataset
    cut into trials: every route runs on the stacked bins, and bin ranges are in stacked bins --
    heldout=(trials, ds.trial_bins(-1)) holds out the last trial.  A 2-tuple whose second entry is a pair of bins (or None, for
    all bins) is read as (data, bins); any other tuple of matrices -- one of exactly two trial matrices too -- as trials."""
    import time
    from .inference import MarkovChainMonteCarlo
    if diagnostics not in (False, True, "full"):
        raise ValueError('diagnostics must be False, True or "full"')
    if diagnostics and not moments:
        raise ValueError("diagnostics need the device-side running sums (moments=True)")
    if batch_len is not None and int(batch_len) < 1:
        raise ValueError("batch_len must be a positive integer")
    from .inference import _check_quantiles
    qprobs = _check_quantiles(quantiles, quantiles_every, moments)
    data = _enter(process, data)
    plan = _score_plan(process, data, waic, heldout, score_every, burn)
    if moments or not keep_samples:
        _check_resident(process, device_draws)
        return _disc_mcmc_resident(process, data, nsteps, log_freq, verbose, seed, ctx, keep_samples, moments, burn, diagnostics,
                                   batch_len, ess_below, rhat_above, plan, score_every, pointwise, qprobs, quantiles_every,
                                   effective_weights)
    ctx = ctx or _lib.default_context()
    ds = convolve(process, data, ctx)
    rng = np.random.default_rng(seed)
    res = MarkovChainMonteCarlo()
    start = time.time()
    scorers, smodel, kept = [], None, 0
    try:
        if plan:
            scorers = _open_scorers(ctx, process, ds, plan)
            smodel = DiscreteDeviceModel(ctx, process)           # holds the scored step's state; the chain does not read it
        while res.steps < nsteps:
            res.samples.append(disc_resample_(process, None, ds, rng, seed=seed, step=res.steps, ctx=ctx, device_draws=device_draws))
            if scorers and res.steps >= burn:
                if kept % int(score_every) == 0:
                    smodel.push(process)
                    for _, s in scorers:
                        s.accumulate(smodel)
                kept += 1
            res.steps += 1
            if res.steps % log_freq == 0 and verbose:
                res.elapsed = time.time() - start
                print(f" > step: {res.steps}, elapsed: {res.elapsed}")
        res.elapsed = time.time() - start
        res.status = "complete"
        _close_scorers(res, scorers, pointwise)
    finally:
        for _, s in scorers:
            s.close()
        if smodel is not None:
            smodel.close()
    return res


def _vb_kind(process, what):
    """'standard' or 'network' for the models the variational drivers are built for; NotImplementedError naming the
    part that is not."""
    from .components import BernoulliNetworkModel, DenseNetworkModel, SparseWeightModel, StochasticBlockNetworkModel
    if isinstance(process, DiscreteNetworkHawkesProcess):
        if not isinstance(process.weights, SparseWeightModel):
            raise NotImplementedError(f"{what}: a DiscreteNetworkHawkesProcess needs a SparseWeightModel (weights: "
                                      f"{type(process.weights).__name__} has no spike-and-slab parameters)")
        if isinstance(process.network, StochasticBlockNetworkModel):
            if not process.network.has_variational_state():
                raise NotImplementedError(f"{what}: the network (StochasticBlockNetworkModel) has no variational state: mean-field "
                                          "over labels cannot leave the uniform state, so none is created implicitly -- call "
                                          "network.variational_init_() first")
        elif not isinstance(process.network, (DenseNetworkModel, BernoulliNetworkModel)):
            raise NotImplementedError(f"{what}: network VB is built for DenseNetworkModel, BernoulliNetworkModel and "
                                      f"StochasticBlockNetworkModel (network: {type(process.network).__name__} has no variational update)")
        kind = "network"
    elif (isinstance(process, DiscreteStandardHawkesProcess) and isinstance(process.weights, DenseWeightModel)
          and not isinstance(process.weights, SparseWeightModel)):
        kind = "standard"
    else:
        raise NotImplementedError(f"{what} exists for DiscreteStandardHawkesProcess + DenseWeightModel and for "
                                  "DiscreteNetworkHawkesProcess + SparseWeightModel (sparse weights on a standard process "
                                  "have no network to draw links from: SURVEY D6)")
    if not isinstance(process.baseline, DiscreteHomogeneousProcess):
        raise NotImplementedError(f"{what} is defined for DiscreteHomogeneousProcess baselines only (baseline: "
                                  "src/baselines.jl:444-456)")
    return kind


class _DenseVB:
    """The buffers nhp_disc_vb_run / nhp_disc_svi_run update in place, and the way back into the process."""
    VB_RUN, SVI_RUN = "nhp_disc_vb_run", "nhp_disc_svi_run"

    def __init__(self, process):
        b, w, imp = process.baseline, process.weights, process.impulses
        self.process, self.N, self.B = process, process.ndims(), imp.nbasis()
        self.av, self.bv = _lib.f64(b.αv).copy(), _lib.f64(b.βv).copy()
        self.kv, self.nv, self.gv = _lib.colmajor(w.κv).copy(), _lib.colmajor(w.νv).copy(), _lib.colmajor(imp.γv).copy()

    def priors(self):
        b, w, imp = self.process.baseline, self.process.weights, self.process.impulses
        return (b.α0, b.β0, w.κ, w.ν, imp.γ)

    def pointers(self):
        return tuple(_lib.dptr(x) for x in (self.av, self.bv, self.kv, self.nv, self.gv))

    def store(self):                              # column-major views of the library's buffers: no transposing copy here or
        p, N, B = self.process, self.N, self.B    # at the next call (a later chunk of svi_ updates them in place)
        p.baseline.αv, p.baseline.βv = self.av, self.bv
        p.weights.κv, p.weights.νv = self.kv.reshape((N, N), order="F"), self.nv.reshape((N, N), order="F")
        p.impulses.γv = self.gv.reshape((N, N, B), order="F")


class _NetVB:
    """The buffers nhp_disc_netvb_run / nhp_disc_netsvi_run update in place, and the way back into the process."""
    VB_RUN, SVI_RUN = "nhp_disc_netvb_run", "nhp_disc_netsvi_run"

    def __init__(self, process):
        from .components import BernoulliNetworkModel
        b, w, imp, net = process.baseline, process.weights, process.impulses, process.network
        self.process, self.N, self.B = process, process.ndims(), imp.nbasis()
        self.kind = 1 if isinstance(net, BernoulliNetworkModel) else 0
        self.av, self.bv = _lib.f64(b.αv).copy(), _lib.f64(b.βv).copy()
        self.k0, self.n0 = _lib.colmajor(w.κv0).copy(), _lib.colmajor(w.νv0).copy()
        self.k1, self.n1 = _lib.colmajor(w.κv1).copy(), _lib.colmajor(w.νv1).copy()
        self.gv = _lib.colmajor(imp.γv).copy()
        self.rho = _lib.colmajor(np.asarray(process.link_probabilities(), dtype=np.float64)).copy()
        if self.rho.size != self.N * self.N:
            raise ValueError("ρv must be an N x N matrix")
        if self.kind and not np.all((self.rho >= 0.0) & (self.rho <= 1.0)):
            raise DomainError("ρv: link probabilities must lie in [0, 1]")
        self.na = C.c_double(net.αv if self.kind else 1.0)
        self.nb = C.c_double(net.βv if self.kind else 1.0)
        self.prior = (net.α, net.β) if self.kind else (1.0, 1.0)

    def priors(self):
        b, w, imp = self.process.baseline, self.process.weights, self.process.impulses
        return (b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, self.kind, self.prior[0], self.prior[1])

    def pointers(self):
        return tuple(_lib.dptr(x) for x in (self.av, self.bv, self.k0, self.n0, self.k1, self.n1, self.gv, self.rho)) + (
            C.cast(C.byref(self.na), C.POINTER(C.c_double)), C.cast(C.byref(self.nb), C.POINTER(C.c_double)))

    def store(self):
        p, N, B = self.process, self.N, self.B
        b, w, imp = p.baseline, p.weights, p.impulses
        b.αv, b.βv = self.av, self.bv
        w.κv0, w.νv0 = self.k0.reshape((N, N), order="F"), self.n0.reshape((N, N), order="F")
        w.κv1, w.νv1 = self.k1.reshape((N, N), order="F"), self.n1.reshape((N, N), order="F")
        w.ρv = self.rho.reshape((N, N), order="F")
        imp.γv = self.gv.reshape((N, N, B), order="F")
        if self.kind:
            p.network.αv, p.network.βv = self.na.value, self.nb.value


class _BlockVB(_NetVB):
    """The same for a StochasticBlockNetworkModel with a variational state (nhp_disc_sbmvb_run / nhp_disc_sbmsvi_run):
    mv [n, k] and the K x K tables column-major, in place of the Bernoulli network's two scalars."""
    VB_RUN, SVI_RUN = "nhp_disc_sbmvb_run", "nhp_disc_sbmsvi_run"

    def __init__(self, process):
        super().__init__(process)
        net = process.network
        K = self.K = net.nblocks
        self.m = _lib.colmajor(np.asarray(net.mv, dtype=np.float64)).copy()
        self.na, self.nb = _lib.colmajor(np.asarray(net.αv, dtype=np.float64)).copy(), _lib.colmajor(np.asarray(net.βv, dtype=np.float64)).copy()
        self.ng = _lib.f64(net.γv).copy()
        if self.m.size != self.N * K or self.na.size != K * K or self.nb.size != K * K or self.ng.size != K:
            raise ValueError("the block network's mv must be N x K, αv and βv K x K and γv of length K")
        if not np.all((self.rho >= 0.0) & (self.rho <= 1.0)):
            raise DomainError("ρv: link probabilities must lie in [0, 1]")

    def priors(self):
        b, w, imp, net = self.process.baseline, self.process.weights, self.process.impulses, self.process.network
        return (b.α0, b.β0, w.κ0, w.ν0, w.κ1, w.ν1, imp.γ, self.K, net.α, net.β, net.γ, int(net.labels_every))

    def pointers(self):
        return tuple(_lib.dptr(x) for x in (self.av, self.bv, self.k0, self.n0, self.k1, self.n1, self.gv, self.rho, self.m, self.na,
                                            self.nb, self.ng))

    def store(self):
        super().store()                                # kind is 0 there: no scalars to write back
        net, N, K = self.process.network, self.N, self.K
        net.mv = self.m.reshape((N, K), order="F")
        net.αv, net.βv, net.γv = self.na.reshape((K, K), order="F"), self.nb.reshape((K, K), order="F"), self.ng


def _vb_holder(process, kind):
    """The holder of the fit _vb_kind found; its type picks the library's entry points (VB_RUN, SVI_RUN)."""
    from .components import StochasticBlockNetworkModel
    if kind != "network":
        return _DenseVB(process)
    return _BlockVB(process) if isinstance(process.network, StochasticBlockNetworkModel) else _NetVB(process)


def update_(process, data, convolved, ctx=None, n_steps=1, step0=None):
    """update!(process, data, convolved) -- src/discrete.jl:369-375: one mean-field step (or n_steps
    of them with the parameters resident on the device in between); the variational parameters of
    baseline, weights and impulses are overwritten in place.  For a DiscreteNetworkHawkesProcess with a
    SparseWeightModel (src/discrete.jl:494-501, intended semantics: DESIGN §3.19) also weights.ρv and the Bernoulli
    network's (αv, βv), or the (mv, αv, βv, γv) of a StochasticBlockNetworkModel that carries a variational state
    (network.variational_init_()); process.adjacency_matrix is not touched.  The block network's label
    sweep runs at the steps whose GLOBAL number is a multiple of network.labels_every: the network counts the steps it has
    taken (network.vb_step, 0 after variational_init_, advanced here), so a loop of one-step calls -- vb_ with its trace --
    keeps the schedule of one call of n steps; step0 overrides the count."""
    kind = _vb_kind(process, "update!")
    data = _enter(process, data, convolved)
    ctx = ctx or _lib.default_context()
    ds = _convolved(process, data, convolved, ctx)
    st = _vb_holder(process, kind)
    first = ()
    if isinstance(st, _BlockVB):                      # the sweep's schedule counts steps across calls: network.vb_step
        first = (int(process.network.vb_step if step0 is None else step0),)
        if first[0] < 0:
            raise ValueError("update!: step0 must be non-negative")
    _lib.check(getattr(_lib.lib(), st.VB_RUN)(ctx.h, ds.h, process.dt, *st.priors(), *first, n_steps, *st.pointers()), ctx.h)
    if first:
        process.network.vb_step = first[0] + int(n_steps)
    st.store()
    return process.variational_params()


def variational_mean_(process):
    """Set the process's parameters to the means of its variational factors: λ0 = αv/βv, θ = γv/Σ_b γv, W = κv/νv; for a
    network process W = κv1/νv1 (the slab), A = (ρv > 0.5) and, for a Bernoulli network, ρ = αv/(αv + βv); for a block
    network ρ = αv/(αv + βv) per pair of blocks, π = γv/Σγv and z = argmax_k mv.  After it
    disc_loglikelihood, disc_forecast and disc_residuals run on a VB fit."""
    b, w, imp = process.baseline, process.weights, process.impulses
    b.λ = np.asarray(b.αv, dtype=np.float64) / np.asarray(b.βv, dtype=np.float64)
    g = np.asarray(imp.γv, dtype=np.float64)
    imp.θ = g / g.sum(axis=2, keepdims=True)
    if isinstance(process, DiscreteNetworkHawkesProcess):
        _vb_kind(process, "variational_mean!")
        w.W = np.asarray(w.κv1, dtype=np.float64) / np.asarray(w.νv1, dtype=np.float64)
        process.adjacency_matrix = (np.asarray(process.link_probabilities()) > 0.5).astype(np.float64)
        net = process.network
        if hasattr(net, "mv"):                        # a block network: ρ = αv/(αv + βv) per pair, π = γv/Σγv, z = argmax_k mv
            net.ρ = np.asarray(net.αv) / (np.asarray(net.αv) + np.asarray(net.βv))
            net.π = np.asarray(net.γv) / np.sum(net.γv)
            net.z = np.argmax(net.mv, axis=1).astype(np.int32)
        elif hasattr(net, "αv"):
            net.ρ = net.αv / (net.αv + net.βv)
    else:
        w.W = np.asarray(w.κv, dtype=np.float64) / np.asarray(w.νv, dtype=np.float64)
    return process


class VariationalInference:
    """src/inference.jl:78-92"""

    def __init__(self):
        self.trace, self.step, self.elapsed, self.status = [], 0, 0.0, "incomplete"

    def __repr__(self):
        return f"\n* Status: {self.status}\n    step: {self.step}\n    elapsed: {self.elapsed}"


def svi_blocks(seed, step0, n, nblocks):
    """The blocks svi_ draws for global steps step0 + 1 .. step0 + n (nhp_disc_svi_blocks): a function of (seed, step)
    alone, computed on the host."""
    out = np.empty(int(n), dtype=np.int32)
    rc = _lib.lib().nhp_disc_svi_blocks(int(seed), int(step0), int(n), int(nblocks), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != _lib.OK:
        raise ValueError("svi_blocks: seed, step0 >= 0, n >= 0 and nblocks >= 1 are required")
    return out


def svi_(process, data, nsteps=1000, batch_bins=4096, delay=1.0, forgetting=0.6, seed=0, blocks=None, streamed=False,
         trace_every=0, step0=0, ctx=None):
    """svi!(process, data; ...) -- a stub in the reference (src/inference.jl:190): stochastic variational inference for the
    models update_ accepts.  The T bins are cut into nb = ceil(T / batch_bins) consecutive blocks; step i (global, 1-based:
    step0 + 1, ...) takes one block -- blocks[k] for the k-th step of this call, or a draw that depends on (seed, i) alone
    (svi_blocks) -- computes the mean-field update! on that block alone, scales the block statistics by nb and blends the
    result into the variational parameters with weight ρ_i = (i + delay)^(-forgetting).  batch_bins >= T gives one block;
    otherwise it must be a multiple of 16.  streamed=True convolves each block on the fly instead of keeping the T x N x B
    convolution on the device (the same numbers).  trace_every = k runs chunks of k steps and appends
    variational_params(process) after each; 0 keeps only the final parameters.  svi_(..., step0=res.step) resumes a run
    exactly.  Returns a VariationalInference whose `step` counts steps (step0 included)."""
    kind = _vb_kind(process, "svi!")
    data = _trials(data)
    if streamed and _has_trials(data):
        raise NotImplementedError("svi!: streamed=True convolves each block on the fly, across the boundaries of the trials; "
                                  "use the resident mode (streamed=False) for trials")
    _refuse_lgcp_trials(process, data)
    T = data.T if isinstance(data, DiscreteDataset) else np.asarray(data).shape[1]
    nsteps, batch_bins, step0, trace_every = int(nsteps), int(batch_bins), int(step0), int(trace_every)
    if nsteps < 0 or step0 < 0 or trace_every < 0:
        raise ValueError("svi!: nsteps, step0 and trace_every must be non-negative")
    if batch_bins < T and (batch_bins < 16 or batch_bins % 16 != 0):
        raise ValueError(f"svi!: batch_bins = {batch_bins} must be a multiple of 16 (>= 16), or >= the {T} bins of the data")
    if not delay >= 0.0:
        raise ValueError("svi!: delay must be >= 0")
    if not 0.5 < forgetting <= 1.0:
        raise ValueError("svi!: forgetting must lie in (0.5, 1]")
    Tb = min(batch_bins, T)
    nb = -(-T // Tb)
    if blocks is not None:
        blocks = np.ascontiguousarray(blocks, dtype=np.int32)
        if blocks.ndim != 1 or len(blocks) < nsteps:
            raise ValueError(f"svi!: blocks holds {blocks.size} entries for {nsteps} steps")
        if blocks.size and (blocks.min() < 0 or blocks.max() >= nb):
            raise ValueError(f"svi!: block indices must lie in [0, {nb})")
    ctx = ctx or _lib.default_context()
    start = time.time()
    imp = process.impulses
    B = imp.nbasis()
    if streamed:
        ds = data if isinstance(data, DiscreteDataset) else DiscreteDataset(ctx, data)
        phi = imp.basis()
        L = phi.shape[0]
        ph = np.asfortranarray(phi).ravel(order="K")
    else:
        ds = data if isinstance(data, DiscreteDataset) and data.B == B else convolve(process, data, ctx)
        ph, L = None, 0
    st = _vb_holder(process, kind)                # the same loop for every fit: the holder's buffers, its entry point
    run = getattr(_lib.lib(), st.SVI_RUN)
    res = VariationalInference()
    res.step = step0
    done = 0
    while done < nsteps:
        n = min(trace_every, nsteps - done) if trace_every else nsteps
        blk = None if blocks is None else blocks[done:done + n].ctypes.data_as(C.POINTER(C.c_int32))
        _lib.check(run(ctx.h, ds.h, process.dt, *st.priors(), batch_bins, float(delay), float(forgetting), int(seed), step0 + done, n,
                       blk, _lib.dptr(ph), L, B, *st.pointers()), ctx.h)
        done += n
        res.step = step0 + done
        st.store()
        if trace_every:
            res.trace.append(process.variational_params())
    if not trace_every:
        res.trace.append(process.variational_params())
    res.elapsed = time.time() - start
    res.status = "complete"
    return res


def vb_(process, data, max_steps=1000, Δx_thresh=1e-6, Δq_thresh=1e-2, verbose=False, keep_trace=True, ctx=None):
    """vb!(process, data; max_steps, Δx_thresh, Δq_thresh, verbose) -- src/inference.jl:153-181.
    Like the reference (whose convergence test is commented out, :163-176) it runs max_steps updates.
    keep_trace=False runs them back to back on the device and records only the final parameters
    (the reference's per-step trace is 2N + N²B + 2N² doubles a step)."""
    _vb_kind(process, "vb!")
    data = _enter(process, data)
    ctx = ctx or _lib.default_context()
    start = time.time()
    convolved = convolve(process, data, ctx)
    res = VariationalInference()
    if not keep_trace and max_steps > 0:
        update_(process, data, convolved, ctx, n_steps=max_steps)
        res.trace.append(process.variational_params())
        res.step = max_steps
    while res.step < max_steps:
        update_(process, data, convolved, ctx)
        res.trace.append(process.variational_params())
        res.step += 1
    res.elapsed = time.time() - start
    if verbose:
        print(" ** maximum steps reached **")
    return res
