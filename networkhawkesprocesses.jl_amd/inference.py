"""Inference drivers: host mirror of src/inference.jl and of the mle! / resample! bodies in
src/continuous.jl:144-208,350-358.  Every O(M·K̄) or O(M·N) loop runs on the GPU; what stays
on the host is O(N²) bookkeeping and the conjugate random draws (out of scope).

Result containers keep the reference's field names (src/inference.jl:6-12,24-29,78-83).
"""
import collections
import math
import time

import numpy as np
from scipy import optimize
from scipy.special import gammaln

from . import _lib
from .components import (ExponentialImpulseResponse, HomogeneousProcess, LogitNormalImpulseResponse, param_layout)
from .continuous import (ContinuousNetworkHawkesProcess, ContinuousStandardHawkesProcess,
                         as_data, device_dataset, loglikelihood, loglikelihood_gradient)
from .parents import resample_parents


class MaximumLikelihood:
    """src/inference.jl:6-12"""

    def __init__(self, maximizer, maximum, steps, elapsed, status):
        self.maximizer, self.maximum, self.steps, self.elapsed, self.status = maximizer, maximum, steps, elapsed, status

    def __repr__(self):
        return f"\n* Status: {self.status}\n    steps: {self.steps}\n    elapsed: {self.elapsed}\n    loss: {self.maximum}"


class MarkovChainMonteCarlo:
    """src/inference.jl:24-37"""

    def __init__(self):
        self.samples, self.steps, self.elapsed, self.status = [], 0, 0.0, "incomplete"

    def __repr__(self):
        return f"\n* Status: complete\n    steps: {self.steps}\n    elapsed: {self.elapsed}"


# ---- log priors and their gradients (host, O(N²)) ---------------------------------------------
def _gamma_logpdf(x, shape, rate):
    return shape * np.log(rate) - gammaln(shape) + (shape - 1.0) * np.log(x) - rate * x


def logprior(process):
    """logprior(process) -- src/continuous.jl:278-284: Gamma(α0, 1/β0) on λ (src/baselines.jl:120-122),
    Gamma(κ, 1/ν) on W (src/weights.jl:66-68), Gamma(α, 1/β) on θ (src/impulses.jl:110-112) or
    normal-gamma on (μ, τ) (src/impulses.jl:254-259)."""
    b, w, imp = process.baseline, process.weights, process.impulses
    lp = np.sum(_gamma_logpdf(b.λ, b.α0, b.β0)) + np.sum(_gamma_logpdf(w.W, w.κ, w.ν))
    if isinstance(imp, ExponentialImpulseResponse):
        lp += np.sum(_gamma_logpdf(imp.θ, imp.α, imp.β))
    else:
        lp += np.sum(_gamma_logpdf(imp.τ, imp.α0, imp.β0))
        prec = imp.κμ * imp.τ
        lp += np.sum(0.5 * np.log(prec / (2 * np.pi)) - 0.5 * prec * (imp.μ - imp.μμ) ** 2)
    return float(lp)


def _logprior_gradient(process):
    b, w, imp = process.baseline, process.weights, process.impulses
    g = [(b.α0 - 1.0) / b.λ - b.β0]
    if isinstance(imp, ExponentialImpulseResponse):
        g.append(((imp.α - 1.0) / imp.θ - imp.β).ravel(order="F"))
    else:
        g.append((-imp.κμ * imp.τ * (imp.μ - imp.μμ)).ravel(order="F"))
        g.append(((imp.α0 - 1.0) / imp.τ - imp.β0 + 0.5 / imp.τ - 0.5 * imp.κμ * (imp.μ - imp.μμ) ** 2).ravel(order="F"))
    g.append(((w.κ - 1.0) / w.W - w.ν).ravel(order="F"))
    return np.concatenate(g)


def _rand_init_(process, rng):
    """src/continuous.jl:200: rand(length(params(process)))"""
    return rng.uniform(size=len(process.params()))


def mle_(process, data, optimizer="L-BFGS-B", verbose=False, f_abstol=1e-6, regularize=False, guess=None,
         recursive=True, seed=None, max_steps=1000, ctx=None):
    """mle!(process, data; optimizer, verbose, f_abstol, regularize, guess) -- src/continuous.jl:144-198.

    Same objective (-loglikelihood [- logprior]), same box [1e-6, 10] on every coordinate, same
    random start and the same |f - f_prev| < f_abstol stopping rule; `process` is overwritten with
    the estimate.  The reference runs Optim's Fminbox(BFGS) on finite differences (2P objective
    calls per gradient); here a box-constrained quasi-Newton method (scipy L-BFGS-B) is fed the
    analytic gradient computed on the GPU, so iterates differ while the optimum is the same.
    optimizer="device": the whole iteration on the GPU (nhp_cont_mle_run, projected L-BFGS with its state in HBM) -- at
    2.1e6 parameters the host route spends its time moving x and ∇ll over PCIe and in the host-side update."""
    if not isinstance(process, ContinuousStandardHawkesProcess):
        raise TypeError("mle! is defined for ContinuousStandardHawkesProcess (src/continuous.jl:144)")
    if regularize and not isinstance(process.baseline, HomogeneousProcess):
        raise NotImplementedError("logprior is not defined for LogGaussianCoxProcess in the reference (src/baselines.jl)")
    from .sharded import ShardedDataset, _all_reduce_sum
    shard = data if isinstance(data, ShardedDataset) else None       # every rank runs the same optimizer on all-reduced values
    ctx = (shard.ctx if shard else ctx) or _lib.default_context()
    ds = shard.local if shard else device_dataset(process, data, ctx)
    rng = np.random.default_rng(seed)
    x0 = _rand_init_(process, rng) if guess is None else np.asarray(guess, dtype=np.float64)
    if shard is not None and shard.world > 1:                        # rank 0's start everywhere
        x0 = _all_reduce_sum(x0 if shard.rank == 0 else np.zeros_like(x0), ctx)
    lower, upper = 1e-6, 1e1
    state = {"minloss": np.inf, "steps": 0, "converged": False, "last": None}
    start = time.time()

    import ctypes as C
    from .continuous import _check_recursive
    flags = _check_recursive(process, recursive)
    P = len(x0)
    comm = _lib.comm_for(ctx) if shard is not None else None

    if optimizer in ("device", "LBFGS-device"):
        # the optimizer's state on the device (nhp_cont_mle_run: projected L-BFGS in HBM, the host reads scalars): no
        # parameter upload, gradient download or host-side quasi-Newton update per objective call
        if regularize:
            raise NotImplementedError("optimizer='device' minimises -loglikelihood only; use the host optimizer with regularize=True")
        if shard is not None and shard.world > 1 and comm is None:
            raise NotImplementedError("optimizer='device' on a sharded dataset needs an RCCL clique (one GPU per rank)")
        x = np.clip(x0, lower, upper)                               # (a new float64 vector: the caller's guess is not written to)
        # mle! overwrites the process anyway: taking the start into it first leaves its tables column-major like the
        # vector, so lowering them to the device model is a plain copy (a fresh process holds row-major numpy arrays, whose
        # lowering transposes 16 MB at N = 1024); a wrong-length guess raises the reference's error here
        process.params_(x)
        model = process.device_model(ctx)
        loss, steps, conv, evals = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().nhp_cont_mle_run(ctx.h, comm.h if comm is not None else None, ds.h, model.h, flags, lower, upper,
                                               float(f_abstol), int(max_steps), _lib.dptr(x), P, C.byref(loss), C.byref(steps),
                                               C.byref(conv), C.byref(evals)), ctx.h)
        if verbose:
            print(f" > steps: {steps.value}, objective evaluations: {evals.value}, loss: {loss.value}, elapsed: {time.time() - start}")
        process.params_(x)
        res = MaximumLikelihood(x, -float(loss.value), int(steps.value), time.time() - start,
                                "success" if conv.value else "failure")
        res.evaluations = int(evals.value)
        return res

    model = process.device_model(ctx)

    def fg(x):
        # params!(process, x) straight into the device-resident model: x already is the reference's
        # column-major parameter vector, so nothing is re-packed on the host per objective call
        model.set_params(x)
        g = np.empty(P)
        ll_c = C.c_double()
        if comm is not None:           # the other ranks' columns: [ll; ∇ll] summed on the device over RCCL, one download
            _lib.check(_lib.lib().nhp_cont_loglik_grad_allreduce(ctx.h, comm.h, ds.h, model.h, flags, C.byref(ll_c), _lib.dptr(g), P), ctx.h)
            ll = ll_c.value
        else:
            _lib.check(_lib.lib().nhp_cont_loglik_grad(ctx.h, ds.h, model.h, flags, C.byref(ll_c), _lib.dptr(g), P), ctx.h)
            ll = ll_c.value
            if shard is not None:                                    # (gloo rehearsal) the other ranks' columns through the host
                tot = _all_reduce_sum(np.concatenate([[ll], g]), ctx)
                ll, g = float(tot[0]), tot[1:]
        if regularize:
            process.params_(x)
            ll += logprior(process)
            g = g + _logprior_gradient(process)
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
    if optimizer == "L-BFGS-B":
        # scipy's own tests would end the run long before the reference's rule does (its default is a RELATIVE decrease of
        # 2.2e-9, i.e. 2e-5 at |f| ~ 1e4): off, but for Optim's default gradient tolerance (g_tol = 1e-8)
        options.update(ftol=0.0, gtol=1e-8, maxfun=20 * max_steps + 1000)
    res = optimize.minimize(fg, np.clip(x0, lower, upper), jac=True, method=optimizer,
                            bounds=[(lower, upper)] * len(x0), callback=status_update,
                            options=options)
    process.params_(res.x)
    return MaximumLikelihood(res.x.copy(), -float(res.fun), state["steps"], time.time() - start,
                             "success" if (state["converged"] or res.success) else "failure")


ExpectedStatistics = collections.namedtuple("ExpectedStatistics", "ll bg EM S1 S2")


def _em_check(process, data, what):
    """The argument errors of em_ / expected_statistics, raised before any device work."""
    from .sharded import ShardedDataset
    if not isinstance(process, ContinuousStandardHawkesProcess):
        raise TypeError(f"{what} is defined for ContinuousStandardHawkesProcess")
    if not isinstance(process.baseline, HomogeneousProcess):
        raise NotImplementedError(f"{what}: the M-step of a LogGaussianCoxProcess baseline has no closed form")
    if isinstance(data, ShardedDataset):
        raise NotImplementedError(f"{what}: not available on a column shard (sharded.ShardedDataset)")


def expected_statistics(process, data, recursive=True, device=False, ctx=None):
    """The expected branching structure under the process's current parameters -- one E-step (nhp_cont_em_stats).

    With r_ij = W[n_j,c_i]·ħ(t_i - t_j)/λ_i over the pairs the objective's λ_i sums (`recursive` as in loglikelihood) and
    r_i0 = λ0[c_i]/λ_i:  ll, the log-likelihood;  bg[c] = Σ r_i0, the expected number of background events of node c;
    EM[p, c] = Σ r_ij, the expected number of events of node c that are children of node p;  S1[p, c] = Σ r_ij·Δt_ij
    (exponential) or Σ r_ij·z_ij, z = logit(Δt/Δtmax) (logit-normal);  S2[p, c] = Σ r_ij·(z_ij - μ[p, c])² (logit-normal, centred
    at the current μ; None for exponential impulses).  device=False: numpy arrays; device=True: float64 torch tensors on the
    context's device."""
    import ctypes as C
    from .continuous import _check_recursive
    _em_check(process, data, "expected_statistics")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    N = process.ndims()
    ln = not isinstance(process.impulses, ExponentialImpulseResponse)
    ll = C.c_double()
    fn = _lib.lib().nhp_cont_em_stats
    flags = _check_recursive(process, recursive)
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        bg = torch.empty(N, dtype=torch.float64, device=dev)
        mats = [torch.empty(N * N, dtype=torch.float64, device=dev) for _ in range(3 if ln else 2)]
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffers' memory are done before the library writes
        _lib.check(fn(ctx.h, ds.h, model.h, flags, 1, C.byref(ll), bg.data_ptr(), mats[0].data_ptr(), mats[1].data_ptr(),
                      mats[2].data_ptr() if ln else None), ctx.h)
        mats = [m.view(N, N).t() for m in mats]               # column-major [p + c·N] -> [p, c]
    else:
        bg = np.empty(N)
        mats = [np.empty(N * N) for _ in range(3 if ln else 2)]
        _lib.check(fn(ctx.h, ds.h, model.h, flags, 0, C.byref(ll), bg.ctypes.data, mats[0].ctypes.data, mats[1].ctypes.data,
                      mats[2].ctypes.data if ln else None), ctx.h)
        mats = [m.reshape((N, N), order="F") for m in mats]
    return ExpectedStatistics(ll.value, bg, mats[0], mats[1], mats[2] if ln else None)


def em_(process, data, max_steps=1000, f_abstol=1e-6, regularize=False, guess=None, recursive=True, seed=None,
        verbose=False, ctx=None, keep_trace=False):
    """Expectation-maximisation fit of a standard process with a homogeneous baseline, the whole iteration on the GPU
    (nhp_cont_em_run).

    The objective is mle_'s: loglikelihood(process, data; recursive) [+ logprior(process) with regularize], on the same box
    [1e-6, 10], from the same random start (or `guess`), stopped by the same |f - f_prev| < f_abstol rule; `process` is
    overwritten with the estimate.  Because the objective charges every event the full mass Σ_c W[n_i, c], the M-step has
    a closed form in every coordinate (with the reference's Gamma / normal-gamma priors too), so an iteration is one fused
    log-likelihood + gradient launch plus an O(P) pass, needs no line search and never decreases the objective.  Returns
    a MaximumLikelihood; keep_trace adds `.trace`, the objective at every iterate (steps + 1 values)."""
    import ctypes as C
    from .continuous import _check_recursive
    _em_check(process, data, "em!")
    P = len(process.params())
    rng = np.random.default_rng(seed)
    x0 = _rand_init_(process, rng) if guess is None else np.asarray(guess, dtype=np.float64)
    if x0.shape != (P,):
        raise ValueError("Parameter vector length does not match model parameter length.")
    lower, upper = 1e-6, 1e1
    priors = _priors(process) if regularize else None
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    start = time.time()
    x = np.clip(x0, lower, upper)                                   # (a new float64 vector: the caller's guess is not written to)
    process.params_(x)                                              # column-major tables, as in mle_(optimizer="device")
    model = process.device_model(ctx)
    loss, steps, conv = C.c_double(), C.c_int32(), C.c_int32()
    trace = np.full(int(max_steps) + 1, np.nan) if (keep_trace or verbose) else None
    _lib.check(_lib.lib().nhp_cont_em_run(ctx.h, ds.h, model.h, _check_recursive(process, recursive),
                                          C.byref(priors) if priors is not None else None, lower, upper, float(f_abstol),
                                          int(max_steps), _lib.dptr(x), P, C.byref(loss), C.byref(steps), C.byref(conv),
                                          _lib.dptr(trace)), ctx.h)
    if verbose:
        for k in range(steps.value + 1):
            print(f" > step: {k}, loss: {-trace[k]}")
        print(f" > steps: {steps.value}, loss: {loss.value}, elapsed: {time.time() - start}")
    process.params_(x)
    res = MaximumLikelihood(x, -float(loss.value), int(steps.value), time.time() - start, "success" if conv.value else "failure")
    if keep_trace:
        res.trace = trace[:steps.value + 1].copy()
    return res


# ---- mean-field variational inference for the continuous standard process (csrc/cont_vb.hip) -----------------------------
NHP_VB_RESUME, NHP_VB_FROM_MODEL = 256, 512


class ContinuousVariational:
    """The mean-field posterior of a continuous standard process (definition: include/nhp.h, nhp_cont_vb_run): one factor per
    entry, λ0[c] ~ Gamma(alpha, beta), W[p,c] ~ Gamma(kappa, nu), θ[p,c] ~ Gamma(a, b) or (μ, τ)[p,c] ~ NormalGamma(m, k, a, b)
    (rates, not scales).  `alpha`, `beta` are N-vectors, the other tables N×N arrays indexed [parent, child] (`m`, `k` None for
    exponential impulses); `S`, `R` are the same numbers as the two planes of the C entry points, in params(process) order.
    `elbo` is the evidence lower bound of the state, `trace` its value at every state the run passed (never falling),
    `steps` the updates made, `status` "success" when |ΔELBO| < f_abstol stopped the run, `pieces` the ELBO's terms where a
    single step returned them."""

    def __init__(self, kind, N, S, R, prior_kappa=0.0, elbo=float("nan"), trace=None, steps=0, status="incomplete", elapsed=0.0):
        if kind not in ("exponential", "logitnormal"):
            raise ValueError("kind must be 'exponential' or 'logitnormal'")
        self.kind, self.N = kind, int(N)
        N, NN = self.N, self.N * self.N
        self.S, self.R = np.array(S, dtype=np.float64), np.array(R, dtype=np.float64)
        P = N + NN * (2 if kind == "exponential" else 3)
        if self.S.shape != (P,) or self.R.shape != (P,):
            raise ValueError("Parameter vector length does not match model parameter length.")
        self.prior_kappa = float(prior_kappa)
        self.elbo, self.steps, self.status, self.elapsed = float(elbo), int(steps), status, float(elapsed)
        self.trace = np.empty(0) if trace is None else np.asarray(trace, dtype=np.float64)
        self.pieces = None

    def _table(self, plane, block):
        N, NN = self.N, self.N * self.N
        return plane[N + block * NN:N + (block + 1) * NN].reshape((N, N), order="F")

    @property
    def _mu_block(self):
        N, NN = self.N, self.N * self.N
        return slice(N, N + NN) if self.kind == "logitnormal" else slice(0, 0)

    alpha = property(lambda self: self.S[:self.N])
    beta = property(lambda self: self.R[:self.N])
    kappa = property(lambda self: self._table(self.S, 1 if self.kind == "exponential" else 2))
    nu = property(lambda self: self._table(self.R, 1 if self.kind == "exponential" else 2))
    a = property(lambda self: self._table(self.S, 0 if self.kind == "exponential" else 1))
    b = property(lambda self: self._table(self.R, 0 if self.kind == "exponential" else 1))
    m = property(lambda self: self._table(self.S, 0) if self.kind == "logitnormal" else None)
    k = property(lambda self: self._table(self.R, 0) if self.kind == "logitnormal" else None)

    def mean(self):
        """The posterior means in params(process) order: α'/β'; a'/b' | m', a'/b'; κ'/ν'."""
        out = self.S / self.R
        out[self._mu_block] = self.S[self._mu_block]
        return out

    def sd(self):
        """The posterior standard deviations in params(process) order: sqrt(shape)/rate for the Gamma factors; the marginal
        of μ is Student-t with 2a' degrees of freedom, sd = sqrt(b'/(k'(a' - 1))), inf for a' <= 1."""
        with np.errstate(invalid="ignore"):                   # (the μ block of S holds means of either sign: overwritten below)
            out = np.sqrt(self.S) / self.R
        if self.kind == "logitnormal":
            a, b, k = self.a.ravel(order="F"), self.b.ravel(order="F"), self.k.ravel(order="F")
            with np.errstate(divide="ignore", invalid="ignore"):
                out[self._mu_block] = np.where(a > 1.0, np.sqrt(b / (k * np.where(a > 1.0, a - 1.0, 1.0))), np.inf)
        return out

    def interval(self, level=0.95):
        """(lower, upper): the central credible interval of every parameter at `level`, in params(process) order, from the
        Gamma quantiles of the factors and the Student-t quantiles of μ's marginal (scipy, on the host)."""
        from scipy import stats
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie in (0, 1)")
        tail = 0.5 * (1.0 - level)
        lo, hi = (stats.gamma.ppf(q, self.S, scale=1.0 / self.R) for q in (tail, 1.0 - tail))
        if self.kind == "logitnormal":
            a, b, k = self.a.ravel(order="F"), self.b.ravel(order="F"), self.k.ravel(order="F")
            m, scale = self.S[self._mu_block], np.sqrt(b / (a * k))
            lo[self._mu_block], hi[self._mu_block] = (stats.t.ppf(q, 2.0 * a, loc=m, scale=scale) for q in (tail, 1.0 - tail))
        return lo, hi

    def expected_links(self):
        """EM[p, c]: the expected number of events of node c that are children of node p under q(z) -- κ' minus the prior's κ."""
        return self.kappa - self.prior_kappa

    def __repr__(self):
        return f"\n* Status: {self.status}\n    steps: {self.steps}\n    elapsed: {self.elapsed}\n    elbo: {self.elbo}"


def _hyper_check(what, label, values, mu_mu):
    """The hyper-parameters' argument errors: every named value positive and finite, the prior mean μμ finite."""
    for name, v in values:
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f"{what}: the {label} {name} = {v} must be positive and finite")
    if not math.isfinite(float(mu_mu)):
        raise ValueError(f"{what}: the prior mean mu_mu = {mu_mu} must be finite")


def _prior_values(pr, impulses):
    names = ["alpha0", "beta0", "kappa", "nu", "a", "b"] + ([] if isinstance(impulses, ExponentialImpulseResponse) else ["kappa_mu"])
    return [(n, float(getattr(pr, n))) for n in names]


def _vb_check(process, data, what):
    """_em_check's argument errors and the hyper-parameters' (positive and finite; μμ finite), before any device work."""
    _em_check(process, data, what)
    pr = _priors(process)
    _hyper_check(what, "prior hyper-parameter", _prior_values(pr, process.impulses), pr.mu_mu)
    return pr


def _vb_kind_of(process):
    return "exponential" if isinstance(process.impulses, ExponentialImpulseResponse) else "logitnormal"


def _vb_state(process, init, P):
    if not isinstance(init, ContinuousVariational):
        raise TypeError("init must be a ContinuousVariational (the result of an earlier vb_ or update_)")
    if init.kind != _vb_kind_of(process) or init.S.shape != (P,):
        raise ValueError("Parameter vector length does not match model parameter length.")
    return init.S.copy(), init.R.copy()


# One description per fit for the two helpers every continuous variational entry shares.  entry: nhp_cont_<entry>_step / _run;
# lead: the C arguments between the priors and the state; arrays(init, what) -> ([S, R, ...] as the entry takes them -- the state
# of `init`, or what a start without one reads --, step0 or None: the block fit's last lead argument); guess(): the default
# guess in device order; result(arrays, step0, taken, **kw) and write_back(x, res): the fit's result class and the overwrite
# of the process; npieces: ELBO pieces per state in stats (a block or latent fit's netpieces network pieces per state follow them,
# and with `rungs` the rung of every ascent iteration of a latent fit those).
_VBFit = collections.namedtuple("_VBFit", "entry pr P flags lead nstats npieces arrays guess result write_back netpieces rungs", defaults=(5, False))


def _vb_step(process, data, fit, init, recursive, ctx):
    """update_ of every continuous fit: one call of nhp_cont_<entry>_step on host planes; the result with its `pieces`."""
    import ctypes as C
    from .continuous import _check_recursive
    flags = _check_recursive(process, recursive) | fit.flags | (NHP_VB_FROM_MODEL if init is None else 0)
    arrays, step0 = fit.arrays(init, "update!")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    start = time.time()
    model = process.device_model(ctx)
    stats = np.empty(fit.nstats)
    lead = fit.lead + (() if step0 is None else (step0,))
    _lib.check(getattr(_lib.lib(), f"nhp_cont_{fit.entry}_step")(
        ctx.h, ds.h, model.h, flags, C.byref(fit.pr), *lead, arrays[0].ctypes.data, arrays[1].ctypes.data, fit.P,
        *(a.ctypes.data for a in arrays[2:]), 0, _lib.dptr(stats)), ctx.h)
    n = fit.npieces
    elbo = float("nan")
    if init is not None:
        elbo = stats[0]
        for j in range(1, n + 1):
            elbo = elbo - stats[j]
    res = fit.result(arrays, step0, 1, elbo=float(elbo), steps=1, elapsed=time.time() - start)
    res.pieces = {"loglam": float(stats[0]), "before": tuple(stats[1:1 + n]), "after": tuple(stats[1 + n:1 + 2 * n])}
    if fit.nstats > 1 + 2 * n:
        m = fit.netpieces
        res.pieces.update(network_before=tuple(stats[11:11 + m]), network_after=tuple(stats[11 + m:11 + 2 * m]))
        if fit.rungs:
            res.pieces["rungs"] = tuple(int(v) for v in stats[11 + 2 * m:])
    return res


def _vb_run(process, data, fit, max_steps, f_abstol, guess, recursive, init, keep_trace, verbose, ctx):
    """vb_ of every continuous fit: one call of nhp_cont_<entry>_run from a guess or from the state of `init`, the trace, the
    result and the overwrite of the process."""
    import ctypes as C
    from .continuous import _check_recursive
    P = fit.P
    flags = _check_recursive(process, recursive) | fit.flags
    max_steps = int(max_steps)
    if init is not None and guess is not None:
        raise ValueError("vb!: give a guess or a state to resume (init), not both")
    arrays, step0 = fit.arrays(init, "vb!")
    if init is not None:
        x = np.empty(P)
        flags |= NHP_VB_RESUME
    else:
        x = np.array(fit.guess() if guess is None else guess, dtype=np.float64)
        if x.shape != (P,):
            raise ValueError("Parameter vector length does not match model parameter length.")
    if max_steps < (0 if init is not None else 1):
        raise ValueError("vb!: max_steps must be at least 1 (0 with init)")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    start = time.time()
    if init is None and fit.entry == "vb":
        process.params_(x)                                          # column-major tables, as in em_
    model = process.device_model(ctx)
    elbo, steps, conv = C.c_double(), C.c_int32(), C.c_int32()
    trace = np.full(max_steps + 1, np.nan)
    lead = fit.lead + (() if step0 is None else (step0,))
    _lib.check(getattr(_lib.lib(), f"nhp_cont_{fit.entry}_run")(
        ctx.h, ds.h, model.h, flags, C.byref(fit.pr), *lead, float(f_abstol), max_steps, _lib.dptr(x), _lib.dptr(arrays[0]),
        _lib.dptr(arrays[1]), P, *(_lib.dptr(a) for a in arrays[2:]), C.byref(elbo), C.byref(steps), C.byref(conv), _lib.dptr(trace)), ctx.h)
    first = 0 if init is not None else 1
    if verbose:
        for k in range(first, steps.value + 1):
            print(f" > step: {k}, elbo: {trace[k]}")
        print(f" > steps: {steps.value}, elbo: {elbo.value}, elapsed: {time.time() - start}")
    res = fit.result(arrays, step0, steps.value, elbo=elbo.value, trace=trace[first:steps.value + 1].copy() if keep_trace else None,
                     steps=steps.value, status="success" if conv.value else "failure", elapsed=time.time() - start)
    fit.write_back(x, res)
    return res


def _standard_fit(process, pr):
    P = len(process.params())

    def arrays(init, what):
        return ([np.empty(P), np.empty(P)] if init is None else list(_vb_state(process, init, P))), None

    def result(arrays, step0, taken, **kw):
        return ContinuousVariational(_vb_kind_of(process), process.ndims(), *arrays, pr.kappa, **kw)
    return _VBFit("vb", pr, P, 0, (), 9, 4, arrays, process.params, result, lambda x, res: process.params_(x))


def vb_step_continuous(process, data, init=None, recursive=True, ctx=None):
    """One coordinate-ascent update of the mean-field posterior (nhp_cont_vb_step): from the state `init` (a
    ContinuousVariational), or with init=None from the process's current parameters used as if they were a surrogate
    (iteration 0 of vb_).  Returns the updated ContinuousVariational; its `pieces` is a dict with "loglam" = Σ_i log λ̃_i at the
    surrogate stepped from, "before" = (E_q[compensator], KL_λ0, KL_W, KL_imp) of the state stepped from (zeros for
    init=None) and "after" = the same of the state returned; `elbo` is that of the state stepped from (NaN for init=None).
    The process is not changed."""
    return _vb_step(process, data, _standard_fit(process, _vb_check(process, data, "update!")), init, recursive, ctx)


def vb_continuous(process, data, max_steps=1000, f_abstol=1e-6, guess=None, recursive=True, init=None, keep_trace=True,
                  verbose=False, ctx=None):
    """Mean-field variational fit of a standard process with a homogeneous baseline under its own priors, the whole
    iteration on the GPU (nhp_cont_vb_run; the definition is in include/nhp.h).

    Iteration 0 runs em_'s E-step at `guess` (default: the process's current parameters), used as if it were a surrogate
    vector; every later iteration at the surrogate of the current factors, followed by the conjugate update of every
    factor.  The ELBO never falls; the run stops when it changes by less than f_abstol or after max_steps updates.
    `init=res` resumes from an earlier result instead of a guess.  `data` as for em_ (a list of trials included; T is the
    summed duration).  Like mle_, `process` is overwritten with the posterior means.  Returns a ContinuousVariational; its
    trace (keep_trace) holds the ELBO of states 1 .. steps (of the resumed state too with `init`)."""
    fit = _standard_fit(process, _vb_check(process, data, "vb!"))
    return _vb_run(process, data, fit, max_steps, f_abstol, guess, recursive, init, keep_trace, verbose, ctx)


# ---- mean-field variational inference for the continuous network process (csrc/cont_netvb.hip) ---------------------------
NHP_VB_DENSE_NETWORK = 1024


class ContinuousNetworkVariational(ContinuousVariational):
    """The mean-field posterior of a continuous network process with spike-and-slab weights (definition: include/nhp.h,
    nhp_cont_netvb_run).  ContinuousVariational's factors, where `kappa`, `nu` (the W block of `S`, `R`) are the SLAB's
    q(W | A = 1) = Gamma(kappa, nu); in addition `kappa0`, `nu0` (the spike's q(W | A = 0)), `rho` = q(A = 1) (N×N, indexed
    [parent, child]) and `net_alpha`, `net_beta` of q(ρ) = Beta (the values given for a dense network, where rho ≡ 1).
    `pieces`, where a single step returned them: "loglam", and "before" / "after" = (E_q[compensator], KL_λ0, KL_W, KL_imp,
    KL_net) of the state stepped from / returned.

    mean() / sd() / interval() run over the planes S, R, in THEIR order [λ0; θ | μ, τ; W] with the slab for W -- the order of
    the standard process's params().  A network process's own params() is ordered [ρ; λ0; W; impulses; vec(A)], so index
    these summaries through the accessors (alpha, a, kappa, ...) rather than by position in process.params()."""

    def __init__(self, kind, N, S, R, Q, prior_kappa=0.0, dense=False, **kw):
        super().__init__(kind, N, S, R, prior_kappa, **kw)
        NN = self.N * self.N
        self.Q = np.array(Q, dtype=np.float64)
        if self.Q.shape != (3 * NN + 2,):
            raise ValueError("Q must hold 3·N² + 2 numbers: [κv0; νv0; ρv; αv; βv]")
        self.dense = bool(dense)

    def _qtable(self, block):
        NN = self.N * self.N
        return self.Q[block * NN:(block + 1) * NN].reshape((self.N, self.N), order="F")

    kappa0 = property(lambda self: self._qtable(0))
    nu0 = property(lambda self: self._qtable(1))
    rho = property(lambda self: self._qtable(2))
    net_alpha = property(lambda self: float(self.Q[-2]))
    net_beta = property(lambda self: float(self.Q[-1]))

    def link_probability(self):
        """q(A[p, c] = 1) = ρv."""
        return self.rho.copy()

    def effective_weight_mean(self):
        """E_q[W] with the link marginalised: (1 - ρv) κv0/νv0 + ρv κv1/νv1."""
        return (1.0 - self.rho) * (self.kappa0 / self.nu0) + self.rho * (self.kappa / self.nu)


def _netvb_check(process, data, what):
    """The argument errors of the network fit, raised before any device work; returns (priors, net [κ0, ν0, α, β], dense)."""
    from .components import (BernoulliNetworkModel, DenseNetworkModel, LatentDistanceNetworkModel, SparseWeightModel,
                             StochasticBlockNetworkModel)
    from .sharded import ShardedDataset
    if not isinstance(process.weights, SparseWeightModel):
        raise TypeError(f"{what} on a ContinuousNetworkHawkesProcess needs a SparseWeightModel (spike and slab); with other weights "
                        f"it is defined for ContinuousStandardHawkesProcess")
    block = isinstance(process.network, StochasticBlockNetworkModel)
    if block:
        if not process.network.has_variational_state():
            raise NotImplementedError(f"{what}: the network (StochasticBlockNetworkModel) has no variational state: mean-field "
                                      "over labels cannot leave the uniform state, so none is created implicitly -- call "
                                      "network.variational_init_() first")
    elif isinstance(process.network, LatentDistanceNetworkModel):
        if not process.network.has_variational_state():
            raise NotImplementedError(f"{what}: the network (LatentDistanceNetworkModel) has no variational state: with all "
                                      "positions equal the ascent is at a saddle, so none is created implicitly -- call "
                                      "network.variational_init_() first")
    elif not isinstance(process.network, (BernoulliNetworkModel, DenseNetworkModel)):
        raise NotImplementedError(f"{what}: a {type(process.network).__name__} is not implemented for continuous processes "
                                  f"(DenseNetworkModel, BernoulliNetworkModel, StochasticBlockNetworkModel and "
                                  f"LatentDistanceNetworkModel are)")
    if not isinstance(process.baseline, HomogeneousProcess):
        raise NotImplementedError(f"{what}: the update of a LogGaussianCoxProcess baseline has no closed form")
    if isinstance(data, ShardedDataset):
        raise NotImplementedError(f"{what}: not available on a column shard (sharded.ShardedDataset)")
    w, net = process.weights, process.network
    dense = isinstance(net, DenseNetworkModel)
    b, imp = process.baseline, process.impulses
    if isinstance(imp, ExponentialImpulseResponse):
        pr = _lib.GibbsPriors(b.α0, b.β0, w.κ1, w.ν1, imp.α, imp.β, 0.0, 1.0)
    else:
        pr = _lib.GibbsPriors(b.α0, b.β0, w.κ1, w.ν1, imp.α0, imp.β0, imp.μμ, imp.κμ)
    values = _prior_values(pr, imp) + [("kappa0", w.κ0), ("nu0", w.ν0)]
    latent = isinstance(net, LatentDistanceNetworkModel)
    if block:
        values += [("network alpha", net.α), ("network beta", net.β), ("network gamma", net.γ)]
    elif latent:
        values += [("network sigma", net.σ), ("network sigma_b", net.σb)]
    elif not dense:
        values += [("network alpha", net.α), ("network beta", net.β), ("network alpha_v", net.αv), ("network beta_v", net.βv)]
    _hyper_check(what, "hyper-parameter", values, pr.mu_mu)
    if latent:
        _latvb_check(process, what)
    plain = dense or block or latent
    netp = np.array([w.κ0, w.ν0, 1.0 if plain else net.α, 1.0 if plain else net.β], dtype=np.float64)
    return pr, netp, dense


def _netvb_start_Q(process, dense):
    """Q of a start without a state: ρv from weights.ρv (None: network.link_probability()), the network's own (αv, βv); the
    spike's tables are output only."""
    N = process.ndims()
    w, net = process.weights, process.network
    rho = net.link_probability() if w.ρv is None else np.asarray(w.ρv, dtype=np.float64)
    if rho.shape != (N, N) or not np.all((rho >= 0.0) & (rho <= 1.0)):
        raise ValueError("weights.ρv must be an N x N matrix of probabilities")
    if _is_block(process) or _is_latent(process):                   # (the block state travels in B, the latent one in Z)
        return np.concatenate([np.ones(2 * N * N), rho.ravel(order="F")])
    return np.concatenate([np.ones(2 * N * N), rho.ravel(order="F"), [1.0 if dense else net.αv, 1.0 if dense else net.βv]])


def _netvb_state(process, init, P):
    if not isinstance(init, ContinuousNetworkVariational):
        raise TypeError("init must be a ContinuousNetworkVariational (the result of an earlier vb_ or update_ of a network process)")
    if init.kind != _vb_kind_of(process) or init.S.shape != (P,):
        raise ValueError("Parameter vector length does not match model parameter length.")
    return init.S.copy(), init.R.copy(), init.Q.copy()


def _device_length(process):
    from .components import param_layout
    return param_layout(process).weights.stop


def _network_guess(process):
    return np.concatenate([process.baseline.params(), process.impulses.params(), process.weights.params()]).astype(np.float64)


def _network_fit(process, pr, netp, dense):
    """The fit of a network process for _vb_step / _vb_run: a Dense or Bernoulli network, a block network or a
    latent distance network."""
    P, kind, N = _device_length(process), _vb_kind_of(process), process.ndims()

    def write_back(x, res):
        _netvb_write_back(process, x, res)
    if _is_block(process):
        net = process.network

        def result(arrays, step0, taken, **kw):
            return ContinuousBlockNetworkVariational(kind, N, *arrays, net.nblocks, pr.kappa, step0 + taken, net.labels_every, **kw)
        lead = (_lib.dptr(netp), _lib.dptr(_sbmvb_priors(process)), net.nblocks, int(net.labels_every))
        return _VBFit("sbmvb", pr, P, 0, lead, 21, 5, lambda init, what: _sbmvb_inputs(process, init, P, what), lambda: _network_guess(process),
                      result, write_back)
    if _is_latent(process):
        net = process.network
        D, J = net.ndims, int(net.ascent_steps)

        def result(arrays, step0, taken, **kw):
            return ContinuousLatentNetworkVariational(kind, N, *arrays, D, pr.kappa, J, **kw)
        lead = (_lib.dptr(netp), _lib.dptr(_latvb_priors(process)), D, J)
        return _VBFit("latvb", pr, P, 0, lead, 19 + J, 5, lambda init, what: _latvb_inputs(process, init, P, what), lambda: _network_guess(process),
                      result, write_back, 4, True)

    def arrays(init, what):
        if init is None:
            return [np.empty(P), np.empty(P), _netvb_start_Q(process, dense)], None
        return list(_netvb_state(process, init, P)), None

    def result(arrays, step0, taken, **kw):
        return ContinuousNetworkVariational(kind, N, *arrays, pr.kappa, dense, **kw)
    return _VBFit("netvb", pr, P, NHP_VB_DENSE_NETWORK if dense else 0, (_lib.dptr(netp),), 11, 5, arrays, lambda: _network_guess(process), result,
                  write_back)


def vb_step_network_continuous(process, data, init=None, recursive=True, ctx=None):
    """One coordinate-ascent update of the network process's mean-field posterior (nhp_cont_netvb_step): from the state
    `init` (a ContinuousNetworkVariational), or with init=None from the process's current λ0, impulses and W used as if they
    were a surrogate (iteration 0 of vb_) and the network's (αv, βv).  Returns the updated ContinuousNetworkVariational with
    `pieces` (see the class); `elbo` is that of the state stepped from (NaN for init=None).  The process is not changed.

    Under a block network (nhp_cont_sbmvb_step): the step numbered init.vb_step + 1, or network.vb_step + 1 without a state;
    a ContinuousBlockNetworkVariational, and the network is not changed either.  Under a latent distance network
    (nhp_cont_latvb_step): a ContinuousLatentNetworkVariational, from init's (zv, bv) or the network's."""
    return _vb_step(process, data, _network_fit(process, *_netvb_check(process, data, "update!")), init, recursive, ctx)


def _netvb_write_back(process, x, res):
    """vb_'s overwrite of a network process: posterior means, W = κv1/νv1, A = (ρv > ½), the network's Beta and the tables."""
    from .components import param_layout
    L = param_layout(process)
    process.baseline.λ = x[L.baseline].copy()
    process.impulses.params_(x[L.impulses])
    process.weights.params_(x[L.weights])
    w, net = process.weights, process.network
    w.κv0, w.νv0, w.κv1, w.νv1, w.ρv = res.kappa0.copy(), res.nu0.copy(), res.kappa.copy(), res.nu.copy(), res.rho.copy()
    w.κv, w.νv = w.κv1, w.νv1
    process.adjacency_matrix = (res.rho > 0.5).astype(np.float64)
    if isinstance(res, ContinuousLatentNetworkVariational):
        net.zv, net.bv = res.positions(), res.offset()
        net.z, net.b = net.zv.copy(), net.bv
    elif isinstance(res, ContinuousBlockNetworkVariational):
        net.mv, net.αv, net.βv, net.γv = res.mv.copy(), res.alpha_v.copy(), res.beta_v.copy(), res.gamma_v.copy()
        net.ρ, net.π, net.z = res.block_link_probability(), net.γv / net.γv.sum(), res.labels()
        net.vb_step = res.vb_step
    elif not res.dense:
        net.αv, net.βv = res.net_alpha, res.net_beta
        net.ρ = net.αv / (net.αv + net.βv)


def vb_network_continuous(process, data, max_steps=1000, f_abstol=1e-6, guess=None, recursive=True, init=None, keep_trace=True,
                          verbose=False, ctx=None):
    """Mean-field variational fit of a ContinuousNetworkHawkesProcess with SparseWeightModel weights under a Dense or
    Bernoulli network, the whole iteration on the GPU (nhp_cont_netvb_run; the definition is in include/nhp.h).  It answers
    "which links are there" -- q(A[p, c] = 1) = ρv -- without running a chain.

    Arguments and stopping rule are vb_continuous's; `guess` is a vector in the device order [λ0; θ | μ, τ; W] (default: the
    process's current values), `init=res` resumes from an earlier ContinuousNetworkVariational.  The network's (αv, βv) start
    from the network's own.  The process is overwritten: λ0 and the impulses take their posterior means, weights.W = κv1/νv1,
    adjacency_matrix = (ρv > ½), network.ρ = αv/(αv + βv) with network.αv, network.βv, and the weights' variational tables and ρv.

    Under a block network (nhp_cont_sbmvb_run) the block state starts from the network's (variational_init_) or from `init`;
    the sweep over the labels runs at the steps whose number since variational_init_ is a multiple of network.labels_every.
    In addition network.mv, αv, βv, γv hold the state, network.ρ = αv/(αv + βv), network.π = γv/Σγv, network.z = labels() and
    network.vb_step advances by the steps taken.

    Under a latent distance network (nhp_cont_latvb_run) the point estimate (zv, bv) starts from the network's
    (variational_init_) or from `init`; every step runs network.ascent_steps iterations of the ascent.  In addition
    network.zv, network.bv hold the state and network.z, network.b are set to them."""
    fit = _network_fit(process, *_netvb_check(process, data, "vb!"))
    return _vb_run(process, data, fit, max_steps, f_abstol, guess, recursive, init, keep_trace, verbose, ctx)


# ---- ... under a stochastic block network (csrc/cont_netvb.hip) ---------------------------------------------

def _is_block(process):
    from .components import StochasticBlockNetworkModel
    return isinstance(process.network, StochasticBlockNetworkModel)


class ContinuousBlockNetworkVariational(ContinuousNetworkVariational):
    """The mean-field posterior of a continuous network process under a StochasticBlockNetworkModel (definition:
    include/nhp.h, nhp_cont_sbmvb_run).  ContinuousNetworkVariational's factors -- Q holds the three planes [κv0; νv0; ρv] -- and
    the block model's: `mv` (N×K, q(z_n) = Categorical(mv[n, :])), `alpha_v`, `beta_v` (K×K, q(ρ[k,l]) = Beta) and `gamma_v`
    (K, q(π) = Dirichlet), kept in `B` = [vec αv; vec βv; γv; vec mv] (StochasticBlockNetworkModel.variational_params()).
    `vb_step` is the number of steps taken since network.variational_init_() -- the label sweep runs at the steps whose
    number is a multiple of `labels_every` -- and travels with `init=res`.  `pieces`, where a single step returned them:
    ContinuousNetworkVariational's, and "network_before" / "network_after" = (Σ entropy of ρv, links, labels, KL_Dir, ΣKL_Beta)
    with KL_net = entropy - (links + labels - KL_Dir - ΣKL_Beta).  There is no single Beta: net_alpha, net_beta are None."""

    def __init__(self, kind, N, S, R, Q, B, nblocks, prior_kappa=0.0, vb_step=0, labels_every=1, **kw):
        ContinuousVariational.__init__(self, kind, N, S, R, prior_kappa, **kw)
        N, K = self.N, int(nblocks)
        self.Q, self.B = np.array(Q, dtype=np.float64), np.array(B, dtype=np.float64)
        if self.Q.shape != (3 * N * N,):
            raise ValueError("Q must hold 3·N² numbers: [κv0; νv0; ρv]")
        if K < 1 or self.B.shape != (2 * K * K + K + N * K,):
            raise ValueError("B must hold 2·K² + K + N·K numbers: [vec αv; vec βv; γv; vec mv]")
        self.nblocks, self.vb_step, self.labels_every, self.dense = K, int(vb_step), int(labels_every), False

    net_alpha = property(lambda self: None)
    net_beta = property(lambda self: None)
    alpha_v = property(lambda self: self.B[:self.nblocks ** 2].reshape((self.nblocks, self.nblocks), order="F"))
    beta_v = property(lambda self: self.B[self.nblocks ** 2:2 * self.nblocks ** 2].reshape((self.nblocks, self.nblocks), order="F"))
    gamma_v = property(lambda self: self.B[2 * self.nblocks ** 2:2 * self.nblocks ** 2 + self.nblocks])
    mv = property(lambda self: self.B[2 * self.nblocks ** 2 + self.nblocks:].reshape((self.N, self.nblocks), order="F"))

    def labels(self):
        """argmax_k mv[n, k], the lowest index on ties (0-based, as StochasticBlockNetworkModel.z)."""
        return np.argmax(self.mv, axis=1).astype(np.int32)

    def block_link_probability(self):
        """E_q ρ[k, l] = αv / (αv + βv)."""
        return self.alpha_v / (self.alpha_v + self.beta_v)


def _sbmvb_inputs(process, init, P, what):
    """([S, R, Q, B], step0) of a call: the state of `init`, or without one the network's own block state and step count."""
    net, N = process.network, process.ndims()
    K = net.nblocks
    if net.nnodes != N:
        raise ValueError(f"{what}: the network has {net.nnodes} nodes, the process {N}")
    if init is not None:
        if not isinstance(init, ContinuousBlockNetworkVariational):
            raise TypeError("init must be a ContinuousBlockNetworkVariational (the result of an earlier vb_ or update_ of this process)")
        if init.kind != _vb_kind_of(process) or init.S.shape != (P,) or init.nblocks != K:
            raise ValueError("Parameter vector length does not match model parameter length.")
        return [init.S.copy(), init.R.copy(), init.Q.copy(), init.B.copy()], init.vb_step
    shapes = ((net.mv, (N, K), "mv"), (net.αv, (K, K), "αv"), (net.βv, (K, K), "βv"), (net.γv, (K,), "γv"))
    for v, shape, name in shapes:
        if np.shape(v) != shape:
            raise ValueError(f"{what}: network.{name} must have shape {shape}")
    B = np.ascontiguousarray(net.variational_params(), dtype=np.float64)
    return [np.empty(P), np.empty(P), _netvb_start_Q(process, False), B], int(net.vb_step)


def _sbmvb_priors(process):
    net = process.network
    return np.array([net.α, net.β, net.γ], dtype=np.float64)


# ---- ... under a latent distance network (csrc/cont_netvb.hip, csrc/nhp_latvb_dev.h) -------------------------

def _is_latent(process):
    from .components import LatentDistanceNetworkModel
    return isinstance(process.network, LatentDistanceNetworkModel)


class ContinuousLatentNetworkVariational(ContinuousNetworkVariational):
    """The variational posterior of a continuous network process under a LatentDistanceNetworkModel (definition:
    include/nhp.h, nhp_cont_latvb_run).  ContinuousNetworkVariational's factors -- Q holds the three planes [κv0; νv0; ρv] -- and
    the network's point estimate (zv, bv), kept in `Z` = [vec zv; bv] (LatentDistanceNetworkModel.variational_params()):
    variational EM over the positions and the offset.  `ascent_steps` iterations of the ascent ran per step.  `pieces`, where a
    single step returned them: ContinuousNetworkVariational's, "network_before" / "network_after" = (Σ entropy of ρv, links,
    ln p(zv), ln p(bv)) with KL_net = entropy - (links + ln p(zv) + ln p(bv)), and "rungs" = the rung of the ladder each ascent
    iteration took (-1: it stayed).  There is no Beta: net_alpha, net_beta are None."""

    def __init__(self, kind, N, S, R, Q, Z, ndims, prior_kappa=0.0, ascent_steps=4, **kw):
        ContinuousVariational.__init__(self, kind, N, S, R, prior_kappa, **kw)
        N, D = self.N, int(ndims)
        self.Q, self.Z = np.array(Q, dtype=np.float64), np.array(Z, dtype=np.float64)
        if self.Q.shape != (3 * N * N,):
            raise ValueError("Q must hold 3·N² numbers: [κv0; νv0; ρv]")
        if D < 1 or D > 8 or self.Z.shape != (N * D + 1,):
            raise ValueError("Z must hold N·D + 1 numbers, D in 1..8: [vec zv; bv]")
        if not 0 <= int(ascent_steps) <= 64:
            raise ValueError("ascent_steps must lie in 0..64")
        self.ndims, self.ascent_steps, self.dense = D, int(ascent_steps), False

    net_alpha = property(lambda self: None)
    net_beta = property(lambda self: None)

    def positions(self):
        """zv (N x D)."""
        return self.Z[:-1].reshape((self.N, self.ndims), order="F").copy()

    def offset(self):
        """bv."""
        return float(self.Z[-1])

    def network_link_probability(self):
        """s(η[p, c]) at (zv, bv), η = bv - ‖zv_p - zv_c‖²: the network's own link probabilities (link_probability() is ρv)."""
        z = self.positions()
        diff = z[:, None, :] - z[None, :, :]
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(np.sum(diff * diff, axis=2) - self.offset()))


def _latvb_check(process, what):
    """The latent network's own argument errors: μb finite, the state's shape, finite entries, ascent_steps in 0..64."""
    net, N = process.network, process.ndims()
    if not math.isfinite(float(net.μb)):
        raise ValueError(f"{what}: the network's mu_b = {net.μb} must be finite")
    if net.nnodes != N:
        raise ValueError(f"{what}: the network has {net.nnodes} nodes, the process {N}")
    if not 1 <= int(net.ndims) <= 8:
        raise ValueError(f"{what}: network.ndims = {net.ndims} must lie in 1..8")
    if not 0 <= int(net.ascent_steps) <= 64:
        raise ValueError(f"{what}: network.ascent_steps = {net.ascent_steps} must lie in 0..64")
    if np.shape(net.zv) != (N, net.ndims):
        raise ValueError(f"{what}: network.zv must have shape {(N, net.ndims)}")
    if not (np.all(np.isfinite(net.zv)) and math.isfinite(float(net.bv))):
        raise ValueError(f"{what}: network.zv and network.bv must be finite")


def _latvb_inputs(process, init, P, what):
    """([S, R, Q, Z], None) of a call: the state of `init`, or without one the network's own (zv, bv)."""
    net, N = process.network, process.ndims()
    if init is not None:
        if not isinstance(init, ContinuousLatentNetworkVariational):
            raise TypeError("init must be a ContinuousLatentNetworkVariational (the result of an earlier vb_ or update_ of this process)")
        if init.kind != _vb_kind_of(process) or init.S.shape != (P,) or init.ndims != net.ndims:
            raise ValueError("Parameter vector length does not match model parameter length.")
        if not np.all(np.isfinite(init.Z)):
            raise ValueError(f"{what}: the state's zv and bv must be finite")
        return [init.S.copy(), init.R.copy(), init.Q.copy(), init.Z.copy()], None
    Z = np.ascontiguousarray(net.variational_params(), dtype=np.float64)
    return [np.empty(P), np.empty(P), _netvb_start_Q(process, False), Z], None


def _latvb_priors(process):
    net = process.network
    return np.array([net.σ, net.μb, net.σb], dtype=np.float64)


# ---- observed information, Hessian-vector products, standard errors ------------------------------------------------------
Information =collections.namedtuple("Information", "ll columns blocks names")
StandardErrors = collections.namedtuple("StandardErrors", "se lower_ci upper_ci free pd")


def _information_check(process, data, what):
    """_em_check's argument errors (a network process is admitted: its A multiplies the pair sums), before any device work."""
    from .sharded import ShardedDataset
    if not isinstance(process, (ContinuousStandardHawkesProcess, ContinuousNetworkHawkesProcess)):
        raise TypeError(f"{what} is defined for continuous Hawkes processes")
    if not isinstance(process.baseline, HomogeneousProcess):
        raise NotImplementedError(f"{what}: not available for a LogGaussianCoxProcess baseline")
    if isinstance(data, ShardedDataset):
        raise NotImplementedError(f"{what}: not available on a column shard (sharded.ShardedDataset)")


def _kinds(process):
    return ("θ", "W") if isinstance(process.impulses, ExponentialImpulseResponse) else ("μ", "τ", "W")


def _params_order(process):
    """[λ0; θ | μ; τ; W]: params! order, for a network process too (whose params() leads with ρ and ends with vec(A))."""
    return np.concatenate([process.baseline.params(), process.impulses.params(), process.weights.params()])


def block_index(N, kinds, c):
    """Positions in the params!-order vector of the rows of column c's block: λ0[c], then p fastest inside each kind."""
    k = np.arange(kinds)[:, None] * N * N + np.arange(N)[None, :] + c * N
    return np.concatenate([[c], N + k.ravel()])


def _check_columns(columns, N):
    if columns is None:
        return np.arange(N, dtype=np.int32)
    cols = np.asarray(columns)
    if cols.ndim != 1 or len(cols) == 0 or not np.issubdtype(cols.dtype, np.integer):
        raise ValueError("columns must be a non-empty list of 0-based node indices")
    if cols.min() < 0 or cols.max() >= N or len(np.unique(cols)) != len(cols):
        raise ValueError(f"columns must be distinct indices in [0, {N})")
    return np.ascontiguousarray(cols, dtype=np.int32)


def _prior_information(process, cols):
    """Minus the Hessian of logprior, column by column: (diag [n, D], the (μ, τ) entries [n, N] or None)."""
    b, w, imp = process.baseline, process.weights, process.impulses
    N = process.ndims()
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (N, N))
    parts = [((np.broadcast_to(b.α0, (N,)) - 1.0) / np.asarray(b.λ) ** 2)[cols][:, None]]
    off = None
    if isinstance(imp, ExponentialImpulseResponse):
        parts.append(((full(imp.α) - 1.0) / imp.θ ** 2)[:, cols].T)
    else:
        parts.append((full(imp.κμ) * imp.τ)[:, cols].T)
        parts.append(((full(imp.α0) - 1.0 + 0.5) / imp.τ ** 2)[:, cols].T)
        off = (full(imp.κμ) * (imp.μ - full(imp.μμ)))[:, cols].T
    parts.append(((full(w.κ) - 1.0) / w.W ** 2)[:, cols].T)
    return np.concatenate(parts, axis=1), off


def observed_information(process, data, columns=None, recursive=True, regularize=False, device=False, tile_nodes=0, ctx=None):
    """The observed information of the objective mle_ / em_ maximise, at the process's current parameters
    (nhp_cont_information).

    The objective separates by child node, so the information is block diagonal: `blocks[k]` is MINUS the Hessian over the
    D = 1 + kinds·N parameters [λ0[c]; θ[:,c] | μ[:,c]; τ[:,c]; W[:,c]] of column c = columns[k] (all columns in order by
    default), positive definite at a well-determined optimum; `names[r]` = (kind, parent) of row r (parent None for λ0).
    regularize adds minus the Hessian of logprior (and logprior to ll).  recursive as in loglikelihood; where the recursive objective has no
    truncated window the call raises NotImplementedError.  tile_nodes: parent nodes per LDS tile of a block (0: automatic).
    device=False: numpy [n_columns, D, D]; device=True: a float64 torch tensor on the context's device.  Returns
    Information(ll, columns, blocks, names)."""
    import ctypes as C
    from .continuous import _check_recursive
    _information_check(process, data, "observed_information")
    N = process.ndims()
    cols = _check_columns(columns, N)
    if not (isinstance(tile_nodes, (int, np.integer)) and 0 <= tile_nodes <= N):
        raise ValueError(f"tile_nodes must be an integer in [0, {N}] (0: automatic)")
    kinds = _kinds(process)
    D = 1 + len(kinds) * N
    prior = _prior_information(process, cols) if regularize else None
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    flags = _check_recursive(process, recursive)
    ll = C.c_double()
    fn = _lib.lib().nhp_cont_information
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        out = torch.empty((len(cols), D, D), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()          # earlier users of the buffer's memory are done before the library writes
        _lib.check(fn(ctx.h, ds.h, model.h, flags, cols.ctypes.data_as(C.POINTER(C.c_int32)), len(cols), int(tile_nodes), 1, C.byref(ll), out.data_ptr()), ctx.h)
        blocks = out.transpose(1, 2)                           # column-major blocks (symmetric: the same numbers)
    else:
        out = np.empty((len(cols), D, D))
        _lib.check(fn(ctx.h, ds.h, model.h, flags, cols.ctypes.data_as(C.POINTER(C.c_int32)), len(cols), int(tile_nodes), 0, C.byref(ll), out.ctypes.data), ctx.h)
        blocks = out.transpose(0, 2, 1)
    value = ll.value
    if prior is not None:
        diag, off = prior
        r = np.arange(D)
        if device:
            blocks = blocks.contiguous()
            blocks[:, r, r] += torch.as_tensor(diag, device=dev)
        else:
            blocks = np.ascontiguousarray(blocks)
            blocks[:, r, r] += diag
        if off is not None:
            mu, tau = 1 + np.arange(N), 1 + N + np.arange(N)
            o = torch.as_tensor(off, device=dev) if device else off
            blocks[:, mu, tau] += o
            blocks[:, tau, mu] += o
        value += logprior(process)
    names = [("λ0", None)] + [(k, p) for k in kinds[:-1] for p in range(N)] + [("W", p) for p in range(N)]
    return Information(value, cols.copy(), blocks, names)


def hessian_vector_product(process, data, v, recursive=True, device=False, ctx=None):
    """H·v for the Hessian H of loglikelihood(process, data; recursive) at the process's current parameters, v and the
    result in params! order [λ0; θ | μ; τ; W] (nhp_cont_hessian_vec: two window walks per event, no block is stored).  H is
    the Hessian itself, not minus it.  device=False: numpy in and out; device=True: float64 torch tensors on the
    context's device."""
    from .continuous import _check_recursive
    _information_check(process, data, "hessian_vector_product")
    N = process.ndims()
    P = N + len(_kinds(process)) * N * N
    if device:
        import torch
        if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (P,)):
            raise ValueError(f"device=True takes a float64 tensor of length {P} on the context's device")
    else:
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (P,):
            raise ValueError("Parameter vector length does not match model parameter length.")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = process.device_model(ctx)
    flags = _check_recursive(process, recursive)
    fn = _lib.lib().nhp_cont_hessian_vec
    if device:
        dev = torch.device("cuda", ctx.device)
        v = v.contiguous()
        out = torch.empty(P, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(fn(ctx.h, ds.h, model.h, flags, 1, v.data_ptr(), out.data_ptr(), P), ctx.h)
        return out
    out = np.empty(P)
    _lib.check(fn(ctx.h, ds.h, model.h, flags, 0, v.ctypes.data, out.ctypes.data, P), ctx.h)
    return out


def _standard_errors_from_blocks(blocks, cols, x, N, kinds, lower, upper, level):
    """standard_errors' host part: free sets, Cholesky of the free sub-blocks, Wald intervals."""
    from scipy.linalg import solve_triangular
    from scipy.stats import norm
    P = len(x)
    se = np.full(P, np.nan)
    free = np.zeros(P, dtype=bool)
    pd = np.zeros(len(cols), dtype=bool)
    for k, c in enumerate(cols):
        idx = block_index(N, kinds, int(c))
        B = np.asarray(blocks[k], dtype=np.float64)
        inside = (x[idx] > lower) & (x[idx] < upper)
        f = inside & np.any(B != 0.0, axis=1)
        sub = B[np.ix_(f, f)]
        ok = bool(np.all(np.isfinite(sub)))
        if ok and f.any():
            try:
                L = np.linalg.cholesky(sub)
                Li = solve_triangular(L, np.eye(len(L)), lower=True)
                var = (Li * Li).sum(axis=0)
                ok = bool(np.all(np.isfinite(var)) and np.all(var > 0.0))
            except np.linalg.LinAlgError:
                ok = False
        pd[k] = ok
        if ok:
            free[idx[f]] = True
            if f.any():
                se[idx[f]] = np.sqrt(var)
    z = norm.ppf(0.5 + 0.5 * level)
    return StandardErrors(se, x - z * se, x + z * se, free, pd)


def standard_errors(process, data, columns=None, recursive=True, regularize=False, lower=1e-6, upper=10.0, level=0.95, ctx=None):
    """Standard errors and Wald intervals of the fitted process's parameters from the inverse observed information.

    se, lower_ci, upper_ci [P] in params! order, NaN where undefined; free [P]: the parameters the inverse was taken over --
    those strictly inside the box (lower, upper) whose row of the column's block is not identically zero (a link with
    A = 0 or W = 0's impulse parameters, a parent no window joins to the column); pd [n_columns]: the free sub-block of
    column columns[k] is positive definite (Cholesky on the host).  A column that is not gets NaNs, no exception."""
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie in (0, 1)")
    if not lower < upper:
        raise ValueError("lower must be below upper")
    info = observed_information(process, data, columns=columns, recursive=recursive, regularize=regularize, ctx=ctx)
    return _standard_errors_from_blocks(info.blocks, info.columns, _params_order(process), process.ndims(), len(_kinds(process)),
                                        lower, upper, level)


def resample_adjacency_matrix_(process, data, u=None, seed=0, step=0, model=None, fetch=True, ctx=None):
    """resample_adjacency_matrix!(process, data) -- src/continuous.jl:444-470: one Gibbs sweep of the
    adjacency matrix, columns in parallel, entries of a column in sequence (resample_column! :472-487).
    `u` (N x N, [parent, child]) supplies the Bernoulli uniforms explicitly; otherwise they come from
    Philox keyed (seed, step).  Updates process.adjacency_matrix in place and returns the link count."""
    import ctypes as C
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model = model or process.device_model(ctx)
    N = process.ndims()
    from .components import BernoulliNetworkModel, DenseNetworkModel
    if isinstance(process.network, BernoulliNetworkModel):       # link_probability = ρ .* ones  (src/networks.jl:65-68)
        scalar, rho_m = float(process.network.ρ), None
    elif isinstance(process.network, DenseNetworkModel):
        scalar, rho_m = 1.0, None
    else:
        scalar, rho_m = None, _lib.colmajor(np.asarray(process.network.link_probability(), dtype=np.float64))
    uu = None if u is None else _lib.colmajor(np.asarray(u, dtype=np.float64))
    A = np.empty(N * N) if fetch else None
    nl = C.c_double()
    _lib.check(_lib.lib().nhp_cont_resample_adjacency(ctx.h, ds.h, model.h, _lib.dptr(rho_m), scalar if scalar is not None else 0.5,
                                                      _lib.dptr(uu), seed, step, _lib.dptr(A), C.byref(nl)), ctx.h)
    if fetch:
        process.adjacency_matrix = A.reshape((N, N), order="F")
    return nl.value


def resample_(process, data, rng, step=0, seed=0, ctx=None, labels_every=1, positions_every=1):
    """resample!(process, data) -- src/continuous.jl:202-208,350-358: one Gibbs sweep.

    Parents and every sufficient statistic come from one GPU call; the conjugate draws are host
    numpy; the network process then resamples its adjacency matrix on the GPU and redraws ρ."""
    data = as_data(data)                # (trials: stacked once; the stacked duration ΣT_r is the exposure)
    _, _, st = resample_parents(process, data, seed=seed, step=step, with_stats=True, want_parents=False, ctx=ctx)
    duration = data.duration if hasattr(data, "duration") else data[2]
    if isinstance(process.baseline, HomogeneousProcess):
        process.baseline.resample_(st["cnt0"], duration, rng)
    else:       # LGCP: elliptical slice on the events the sweep above attributed to the baseline
        process.baseline.resample_(device_dataset(process, data, ctx), rng)
    process.weights.resample_(st["Mn"], st["Mnm"], rng)
    if isinstance(process.impulses, ExponentialImpulseResponse):
        process.impulses.resample_(st["Mnm"], st["Xnm"], rng)
    else:
        process.impulses.resample_(st["Mnm"], st["Xnm"], st["Vnm"], rng)
    if isinstance(process, ContinuousNetworkHawkesProcess):
        resample_adjacency_matrix_(process, data, seed=seed, step=step, ctx=ctx)
        from .components import LatentDistanceNetworkModel, StochasticBlockNetworkModel
        if isinstance(process.network, StochasticBlockNetworkModel):      # on the GPU, keyed like the device-resident step
            process.network.resample_(process.adjacency_matrix, rng, seed=seed, step=step, ctx=ctx, labels=step % labels_every == 0)
        elif isinstance(process.network, LatentDistanceNetworkModel):
            process.network.resample_(process.adjacency_matrix, rng, seed=seed, step=step, ctx=ctx, positions=step % positions_every == 0)
        else:
            process.network.resample_(process.adjacency_matrix, rng)
    return process.params()


def _priors(process):
    b, w, imp = process.baseline, process.weights, process.impulses
    if isinstance(imp, ExponentialImpulseResponse):
        return _lib.GibbsPriors(b.α0, b.β0, w.κ, w.ν, imp.α, imp.β, 0.0, 1.0)
    return _lib.GibbsPriors(b.α0, b.β0, w.κ, w.ν, imp.α0, imp.β0, imp.μμ, imp.κμ)


def _pull_params(process, model, ctx):
    """Copy the device-resident parameters back into the component structs (in-place semantics of
    the reference: "all inference methods overwrite model parameters", docs/src/index.md:109-111)."""
    L = param_layout(process)
    x = np.empty(L.weights.stop)
    _lib.check(_lib.lib().nhp_cont_model_get_params(ctx.h, model.h, _lib.dptr(x), len(x)), ctx.h)
    process.baseline.λ = x[L.baseline].copy()
    process.impulses.params_(x[L.impulses])
    process.weights.params_(x[L.weights])


def _fetch_moments(process, model, ctx, network, rho_sum, rho_sq):
    """Mean and mean square of params(process) from the device-side running sums, in params(process) order."""
    import ctypes as C
    L = moments_length(process)
    s, q = np.empty(L), np.empty(L)
    cnt = C.c_int64()
    _lib.check(_lib.lib().nhp_cont_model_moments_fetch(ctx.h, model.h, _lib.dptr(s), _lib.dptr(q), L, C.byref(cnt)), ctx.h)
    mean, m2 = _moments_in_params_order(process, s, q, cnt.value, network, rho_sum, rho_sq)
    return mean, m2, cnt.value


def moments_length(process):
    """Length of the device-side running sums of nhp_cont_model_moments_*: [λ0; impulses; W; vec(A) if any]."""
    return param_layout(process).adjacency.stop


def _moments_in_params_order(process, s, q, count, network, rho_sum, rho_sq):
    """Σx, Σx² in the device order -> mean and mean square in params(process) order."""
    n = max(1, count)
    mean, m2 = s / n, q / n
    if network:        # device order [λ0; impulses; W; vec(A)] -> params(process) = [ρ; λ0; W; impulses; vec(A)] (src/continuous.jl:325-333)
        k = len(process.network.params())
        L = param_layout(process)

        def order(v, rho):
            return np.concatenate([np.full(k, rho), v[L.baseline], v[L.weights], v[L.impulses], v[L.adjacency]])
        mean, m2 = order(mean, rho_sum / n), order(m2, rho_sq / n)
    return mean, m2


DIAGNOSTIC_FIELDS = ("entries", "undefined", "min_ess", "min_ess_index", "max_rhat", "max_rhat_index", "ess_below", "rhat_above",
                     "max_mcse")


def _fetch_diagnostics(process, model, ctx, network, full, ess_below, rhat_above):
    """nhp_cont_model_diagnostics_fetch -> {"summary"[, "ess", "mcse", "rhat"]} (the caller adds n, batch_len, nbatches).
    The per-entry arrays take the reordering of _moments_in_params_order."""
    from .components import BernoulliNetworkModel
    L = moments_length(process)
    summary = np.empty(_lib.DIAG_GROUPS * _lib.DIAG_FIELDS)
    planes = [np.empty(L) for _ in range(3)] if full else [None] * 3
    _lib.check(_lib.lib().nhp_cont_model_diagnostics_fetch(ctx.h, model.h, float(ess_below), float(rhat_above), _lib.dptr(summary),
                                                          *[_lib.dptr(v) for v in planes], L), ctx.h)
    summary = summary.reshape(_lib.DIAG_GROUPS, _lib.DIAG_FIELDS)
    exponential = isinstance(process.impulses, ExponentialImpulseResponse)
    names = ["baseline", "impulses.θ" if exponential else "impulses.μ", None if exponential else "impulses.τ", "weights",
             "adjacency" if network else None,
             "network.ρ" if network and isinstance(process.network, BernoulliNetworkModel) else None]
    ints = ("entries", "undefined", "min_ess_index", "max_rhat_index", "ess_below", "rhat_above")
    out = {"summary": {name: {f: (int(v) if f in ints else float(v)) for f, v in zip(DIAGNOSTIC_FIELDS, row)}
                       for name, row in zip(names, summary) if name is not None}}
    if full:
        if network:    # [ρ-entries; λ0; W; impulses; vec(A)]; ρ's single entry is its group's extreme, anything else NaN
            k = len(process.network.params())
            lay = param_layout(process)
            rho = summary[5, [2, 8, 4]] if "network.ρ" in out["summary"] else [np.nan] * 3
            planes = [np.concatenate([np.full(k, r), v[lay.baseline], v[lay.weights], v[lay.impulses], v[lay.adjacency]])
                      for v, r in zip(planes, rho)]
        out["ess"], out["mcse"], out["rhat"] = planes
    return out


# ---- streaming quantiles of a chain that keeps no samples (csrc/chain_quantiles.hip) -----------------------------
DEFAULT_QUANTILES = (0.025, 0.5, 0.975)


class ChainQuantiles:
    """Streaming quantile estimates of params(process) over a chain's kept steps (extended P², definition: include/nhp.h).
    `probs` [m]; `values` [m, len(params(process))], row j the estimate of probs[j]; `min`, `max` the smallest and largest
    value seen, exact; `n` the values every entry was fed, one per `every`-th kept step.  NaN where an entry has no state:
    vec(A), a block network's ρ / π, a latent distance network's b -- and everywhere in `values` while n < 2m + 3."""

    def __init__(self, probs, values, lo, hi, n, every, effective_weights=False):
        self.probs = np.array(probs, dtype=np.float64)
        self.values, self.min, self.max = values, lo, hi
        self.n, self.every, self.effective_weights = int(n), int(every), bool(effective_weights)

    def interval(self, level=0.95):
        """(lower, upper): the rows of `values` for the probabilities (1 − level)/2 and (1 + level)/2, which must have been
        among `probs`."""
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie in (0, 1)")
        rows = []
        for p in ((1.0 - level) / 2.0, (1.0 + level) / 2.0):
            hit = np.flatnonzero(np.abs(self.probs - p) <= 1e-12)
            if len(hit) == 0:
                raise ValueError(f"interval({level}) needs the quantile {p:.6g}, which the chain did not estimate "
                                 f"(probs = {tuple(float(v) for v in self.probs)})")
            rows.append(self.values[hit[0]])
        return rows[0], rows[1]

    def __repr__(self):
        return f"ChainQuantiles(probs={tuple(float(v) for v in self.probs)}, n={self.n}, every={self.every}, entries={self.values.shape[1]})"


def _check_quantiles(quantiles, quantiles_every, moments):
    """mcmc_'s quantiles= as a float64 array of probabilities, or None; every argument error is raised here, before the
    library is touched."""
    if quantiles is None or quantiles is False:
        return None
    if not moments:
        raise ValueError("quantiles need the device-side running sums (moments=True)")
    if isinstance(quantiles_every, bool) or int(quantiles_every) != quantiles_every or int(quantiles_every) < 1:
        raise ValueError("quantiles_every must be a positive integer")
    if quantiles is True:
        return np.array(DEFAULT_QUANTILES, dtype=np.float64)
    try:
        p = np.array(quantiles, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("quantiles must be True or a sequence of probabilities") from None
    if p.ndim != 1 or len(p) < 1:
        raise ValueError("quantiles must be True or a non-empty sequence of probabilities")
    if len(p) > _lib.QUANT_MAX:
        raise ValueError(f"at most {_lib.QUANT_MAX} quantiles are estimated per chain ({len(p)} asked for)")
    if not (np.all(np.isfinite(p)) and np.all(p > 0.0) and np.all(p < 1.0) and np.all(np.diff(p) > 0.0)):
        raise ValueError("quantiles must increase strictly inside (0, 1)")
    return p


def _fetch_quantiles(process, model, ctx, network, probs, every, effective):
    """nhp_cont_model_quantiles_fetch -> ChainQuantiles in params(process) order (the reordering of _moments_in_params_order)."""
    import ctypes as C
    from .components import BernoulliNetworkModel
    L, m = moments_length(process), len(probs)
    values, lo, hi, rho = np.empty((m, L)), np.empty(L), np.empty(L), np.empty(m + 2)
    cnt = C.c_int64()
    _lib.check(_lib.lib().nhp_cont_model_quantiles_fetch(ctx.h, model.h, _lib.dptr(values), _lib.dptr(lo), _lib.dptr(hi), _lib.dptr(rho), L,
                                                        C.byref(cnt)), ctx.h)
    if network:        # [ρ-entries; λ0; W; impulses; vec(A)]; only a Bernoulli network's scalar ρ has a state
        k = len(process.network.params())
        lay = param_layout(process)
        if not isinstance(process.network, BernoulliNetworkModel):
            rho = np.full(m + 2, np.nan)

        def order(v, r):
            return np.concatenate([np.full(k, r), v[lay.baseline], v[lay.weights], v[lay.impulses], v[lay.adjacency]])
        values = np.stack([order(values[j], rho[j]) for j in range(m)])
        lo, hi = order(lo, rho[m]), order(hi, rho[m + 1])
    return ChainQuantiles(probs, values, lo, hi, cnt.value, every, effective)


def _owned_mask(process, shard, network):
    """1 on the entries of params(process) this rank owns (its columns; rank 0 also the network's ρ), 0 elsewhere."""
    N = process.ndims()
    c0, c1 = shard.ranges[shard.rank]
    col = np.zeros(N)
    col[c0:c1] = 1.0
    mat = np.repeat(col, N)                                   # vec of an N x N matrix, column-major: index p + c·N
    nmat = 1 if isinstance(process.impulses, ExponentialImpulseResponse) else 2
    if not network:                                           # [λ0; impulses; W]
        return np.concatenate([col] + [mat] * (nmat + 1))
    k = len(process.network.params())                         # [ρ; λ0; W; impulses; vec(A)]
    return np.concatenate([np.full(k, 1.0 if shard.rank == 0 else 0.0), col] + [mat] * (nmat + 2))


def _merge_shards(process, shard, network):
    """After a sharded chain every rank holds the final values of its own columns: put the full state on every rank."""
    from .sharded import _all_reduce_sum
    N = process.ndims()
    full = _all_reduce_sum(process.params() * _owned_mask(process, shard, network), shard.ctx)
    L = param_layout(process, network)
    process.baseline.λ = full[L.baseline].copy()
    process.impulses.params_(full[L.impulses])
    process.weights.params_(full[L.weights])
    if network:
        process.adjacency_matrix = full[L.adjacency].reshape((N, N), order="F").copy()


# ---- scoring a chain: held-out predictive log-likelihood and WAIC (csrc/cont_score.hip) ---------------------------
class ContinuousScore:
    """What nhp_cont_score_fetch returns for the cells (block [edges[k], edges[k+1]), node) over `n` kept draws (definitions:
    include/nhp.h).  `lppd`, `p_waic`, `elpd_waic`, `waic` = −2·elpd_waic and `se_elpd` are the pointwise scores summed over the
    cells; `joint_lpd` = log mean_s p(all scored cells | θ_s) is the predictive log-likelihood of the scored range as a whole
    (the number to report for held-out data), `joint_mean` and `joint_sd` the mean and spread of the draws' log-likelihoods.
    `per_node` is 3 x N (lppd, p_waic, elpd_waic per node), `pointwise` -- when asked for -- the K x N array of elpd_i that
    compare_scores needs; `bins` = tuple(edges) is what compare_scores holds two scores' cells equal by."""

    def __init__(self, summary, per_node, pointwise, edges):
        from .discrete import SCORE_FIELDS
        for name, v in zip(SCORE_FIELDS, summary):
            setattr(self, name, int(v) if name in ("n", "cells") else float(v))
        self.per_node, self.pointwise = per_node, pointwise
        self.edges = np.array(edges, dtype=np.float64)
        self.bins = tuple(float(e) for e in self.edges)

    def __repr__(self):
        return (f"ContinuousScore(blocks={len(self.edges) - 1}, n={self.n}, waic={self.waic:.6g}, elpd_waic={self.elpd_waic:.6g} ± "
                f"{self.se_elpd:.3g}, p_waic={self.p_waic:.4g}, joint_lpd={self.joint_lpd:.6g})")


class _DeviceScore:
    """nhp_cont_score handle on a device dataset (kept alive with it)."""

    def __init__(self, ctx, ds, edges):
        import ctypes as C
        self.ctx, self.ds, self.edges = ctx, ds, _lib.f64(edges)
        self.h = C.c_void_p()
        _lib.check(_lib.lib().nhp_cont_score_create(ctx.h, ds.h, _lib.dptr(self.edges), len(self.edges), C.byref(self.h)), ctx.h)

    def accumulate(self, model):
        _lib.check(_lib.lib().nhp_cont_score_accumulate(self.ctx.h, self.h, model.h), self.ctx.h)

    def fetch(self, pointwise=False):
        """The ContinuousScore of the draws so far; None when nothing was accumulated."""
        from .discrete import SCORE_FIELDS
        N, K = self.ds.nnodes, len(self.edges) - 1
        summary, per_node = np.empty(len(SCORE_FIELDS)), np.empty(3 * N)
        pw = np.empty(K * N) if pointwise else None
        try:
            _lib.check(_lib.lib().nhp_cont_score_fetch(self.ctx.h, self.h, _lib.dptr(summary), _lib.dptr(per_node), _lib.dptr(pw)), self.ctx.h)
        except _lib.NhpError as e:
            if "nothing accumulated" not in str(e):
                raise
            return None
        return ContinuousScore(summary, per_node.reshape(3, N), pw.reshape((K, N), order="F") if pointwise else None, self.edges)

    def fetch_planes(self):
        """The running planes lse, mean, M2 of ℓ as the device holds them, each K x N."""
        N, K = self.ds.nnodes, len(self.edges) - 1
        planes = [np.empty(K * N) for _ in range(3)]
        _lib.check(_lib.lib().nhp_cont_score_fetch_planes(self.ctx.h, self.h, *[_lib.dptr(v) for v in planes]), self.ctx.h)
        return tuple(v.reshape((K, N), order="F") for v in planes)

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().nhp_cont_score_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_edges(edges, T, what):
    """An int K -> K equal blocks over [0, T]; else the edges themselves: at least two, finite, strictly increasing, inside
    [0, T]."""
    if isinstance(edges, (bool, np.bool_)):
        raise ValueError(f"{what}: give a number of blocks or an array of edges")
    if isinstance(edges, (int, np.integer)):
        if int(edges) < 1:
            raise ValueError(f"{what}: the number of blocks must be positive")
        e = np.linspace(0.0, float(T), int(edges) + 1)
        e[-1] = float(T)
        return e
    try:
        e = np.array(edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: edges must be a number of blocks or a 1-D array of times") from None
    if e.ndim != 1 or len(e) < 2:
        raise ValueError(f"{what}: edges must be a 1-D array of at least two times")
    if not np.all(np.isfinite(e)):
        raise ValueError(f"{what}: edges must be finite")
    if not np.all(np.diff(e) > 0):
        raise ValueError(f"{what}: edges must increase strictly")
    if e[0] < 0 or e[-1] > T:
        raise ValueError(f"{what}: edges must lie inside [0, duration = {T}]")
    return e


def _scored_data(process, data, what):
    """(N, duration) of the data a scorer would run on; whatever scoring is not built for raises here, before any upload."""
    from .continuous import DeviceDataset, ntrials_of
    from .sharded import ShardedDataset
    if isinstance(data, ShardedDataset):
        raise NotImplementedError(f"{what}: scoring is not available on a ShardedDataset (a draw needs every column)")
    if not isinstance(process.baseline, HomogeneousProcess):
        raise NotImplementedError(f"{what}: scoring needs a homogeneous baseline (baseline: {type(process.baseline).__name__}: the draws "
                                  f"of its grid values are not scored)")
    N = process.ndims()
    if isinstance(data, DeviceDataset):
        if getattr(data, "ntrials", 1) > 1:
            raise NotImplementedError(f"{what}: scoring is not available on several trials (a block of the stacked clock would straddle them)")
        if data.nnodes != N:
            raise ValueError(f"{what}: the data has {data.nnodes} nodes, the process {N}")
        return N, float(data.duration)
    if ntrials_of(data) > 1:
        raise NotImplementedError(f"{what}: scoring is not available on several trials (a block of the stacked clock would straddle them)")
    events, nodes, duration = as_data(data)
    if not (hasattr(nodes, "device") and not isinstance(nodes, np.ndarray)):
        nd = np.asarray(nodes)
        if nd.size and (nd.min() < 1 or nd.max() > N):
            raise ValueError(f"{what}: the data's nodes run from {nd.min()} to {nd.max()}, the process has {N}")
    return N, float(duration)


def _score_plan(process, data, waic, heldout, score_every, burn):
    """The scorers a chain was asked for, as [(name, data or None for the chain's own, edges)]; every argument is checked here,
    before the library is touched."""
    if (waic is False or waic is None) and heldout is None:
        return []
    if isinstance(score_every, bool) or int(score_every) != score_every or int(score_every) < 1:
        raise ValueError("score_every must be a positive integer")
    if int(burn) < 0:
        raise ValueError("burn must be non-negative when the chain is scored")
    plan = []
    if waic is not False and waic is not None:
        _, T = _scored_data(process, data, "waic")
        plan.append(("waic", None, _check_edges(waic, T, "waic")))
    if heldout is not None:
        if not (isinstance(heldout, tuple) and len(heldout) == 2):
            raise ValueError("heldout must be (data_full, edges)")
        _scored_data(process, data, "heldout")
        _, T = _scored_data(process, heldout[0], "heldout")
        plan.append(("heldout", heldout[0], _check_edges(heldout[1], T, "heldout")))
    return plan


def _open_scorers(ctx, process, ds, plan):
    out = []
    try:
        for name, data, edges in plan:
            out.append((name, _DeviceScore(ctx, ds if data is None else device_dataset(process, data, ctx), edges)))
    except Exception:
        for _, s in out:
            s.close()
        raise
    return out


def _set_score_model(model, ctx, process, x):
    """The draw x = params(process) as the state of a device model kept for scoring (made at the first call): the tables are
    read out of x, the process supplies the shapes, the kinds and Δtmax and is not changed."""
    from .continuous import DeviceModel
    N = process.ndims()
    network = isinstance(process, ContinuousNetworkHawkesProcess)
    x = _lib.f64(x)
    L = param_layout(process, network)
    if x.shape != (L.adjacency.stop if network else L.weights.stop,):
        raise ValueError("Parameter vector length does not match model parameter length.")
    exponential = isinstance(process.impulses, ExponentialImpulseResponse)
    d = _lib.ModelDesc()
    d.n_nodes, d.baseline_kind, d.grid_n = N, _lib.BASELINE_HOMOGENEOUS, 0
    d.impulse_kind = _lib.IMPULSE_EXPONENTIAL if exponential else _lib.IMPULSE_LOGITNORMAL
    d.dt_max = float(process.impulses.Δtmax)
    keep = [np.ascontiguousarray(x[L.baseline]), np.ascontiguousarray(x[L.weights]), np.ascontiguousarray(x[L.impulses])]
    d.lambda0, d.W = _lib.dptr(keep[0]), _lib.dptr(keep[1])
    if exponential:
        d.theta = _lib.dptr(keep[2])
    else:
        keep += [np.ascontiguousarray(keep[2][:N * N]), np.ascontiguousarray(keep[2][N * N:])]
        d.mu, d.tau = _lib.dptr(keep[3]), _lib.dptr(keep[4])
    if network:
        keep.append(np.ascontiguousarray(x[L.adjacency]))
        d.A = _lib.dptr(keep[-1])
    if model is None:
        return DeviceModel(ctx, d)
    model.update(d)
    return model


def score_samples(process, samples, data, edges, burn=0, every=1, pointwise=False, ctx=None):
    """Score the draws of a finished chain: samples[burn], samples[burn + every], … (each a params(process) vector, as
    res.samples holds them) on the blocks `edges` (an int K or an array, as mcmc_'s waic=) of `data`.  Every draw is set into a
    device model and accumulated as the chain itself would have (nhp_cont_score_accumulate): for the same draws the result
    is the in-chain score bit for bit.  The process supplies the shapes, the kinds and Δtmax; it is not changed."""
    if isinstance(every, bool) or int(every) != every or int(every) < 1:
        raise ValueError("every must be a positive integer")
    if isinstance(burn, bool) or int(burn) != burn or int(burn) < 0:
        raise ValueError("burn must be a non-negative integer")
    samples = list(samples)
    if int(burn) >= len(samples):
        raise ValueError(f"no draws left: {len(samples)} samples, burn = {burn}")
    _, T = _scored_data(process, data, "score_samples")
    edges = _check_edges(edges, T, "score_samples")
    ctx = ctx or _lib.default_context()
    ds = device_dataset(process, data, ctx)
    model, scorer = None, None
    try:
        scorer = _DeviceScore(ctx, ds, edges)
        for x in samples[int(burn)::int(every)]:
            model = _set_score_model(model, ctx, process, x)
            scorer.accumulate(model)
        return scorer.fetch(pointwise)
    finally:
        if scorer is not None:
            scorer.close()


def mcmc_(process, data, nsteps=1000, log_freq=100, verbose=False, seed=0, keep_samples=True, device_draws=True,
          ctx=None, moments=False, burn=0, labels_every=1, positions_every=1, diagnostics=False, batch_len=None, ess_below=100.0,
          rhat_above=1.01, waic=False, heldout=None, score_every=1, pointwise=False, quantiles=False, quantiles_every=1,
          effective_weights=False):
    """mcmc!(process, data; nsteps, log_freq, verbose) -- src/inference.jl:49-70.

    With `device_draws` (default) a whole sweep -- parents, statistics, conjugate draws -- stays on
    the GPU (nhp_cont_gibbs_step): parameters never cross PCIe unless samples are kept.  With
    device_draws=False the statistics come back and numpy draws the parameters (same
    distributions).  `seed` keys every random stream, so a chain is reproducible and chains with
    different seeds are independent (one per GPU: chains.py).

    `moments=True` (device draws only) keeps the chain's running sums on the device (nhp_cont_model_moments_*): after the
    run `res.mean` and `res.m2` hold the mean and the mean square of params(process) over the steps >= `burn` -- the
    summaries chains.py gathers -- with no per-step transfer; combine with keep_samples=False for long chains at large N
    (a sample is 4N²+N doubles, 33.5 MB at N = 1024).

    `diagnostics=True` (with `moments=True`) says whether those means can be trusted, still without samples: the pass that
    keeps the running sums also keeps batch sums and two snapshots (nhp_cont_model_diagnostics_*, one launch per kept step),
    and `res.diagnostics` holds `n`, `batch_len`, `nbatches` and `summary`: per group ("baseline", "impulses.θ" or
    "impulses.μ" / "impulses.τ", "weights", "adjacency", "network.ρ") the entries, the undefined ones (never moved: a link
    that never flipped), the smallest batch-means effective sample size and the largest split R-hat with their entries'
    indices inside the group (p + N·c), how many entries have ESS < `ess_below` and R-hat > `rhat_above`, and the largest
    Monte-Carlo standard error.  `diagnostics="full"` adds `ess`, `mcse`, `rhat` per entry, in params(process) order.
    `batch_len` defaults to max(1, ⌊√(nsteps − burn)⌋).  Definitions: include/nhp.h.  Only a BernoulliNetworkModel's ρ is
    diagnosed among the network parameters: a block network's ρ / π and a latent distance network's b are NaN in the
    per-entry arrays and have no group (labels and positions are not identified anyway).  A ShardedDataset raises
    NotImplementedError.

    A StochasticBlockNetworkModel is resampled on the GPU on every route (csrc/sbm.hip): with the device-side draws its
    labels, ρ and π stay next to the model and a network step never leaves the device; with device_draws=False (or an
    LGCP baseline) A comes back every step and the network's resample_ runs through the stand-alone entries.  The label
    sweep is a chain of N dependent steps and is the longest part of such a step: `labels_every=k`
    resamples the labels at the steps that are multiples of k only (ρ and π every step).  With `moments=True` the
    K² + K network entries of res.mean / res.m2 are those of [vec(ρ); π] and `res.block_counts` [N x K] counts the
    kept steps each node spent in each block.  Block labels are identified only up to a permutation: a chain can
    switch them, and then these averages mix the blocks.  A ShardedDataset raises NotImplementedError (the labels'
    conditional needs every column of A).

    A LatentDistanceNetworkModel takes the same routes (csrc/latent.hip): its positions and offset b stay next to the
    device model, or its resample_ runs through the stand-alone entry with the chain's (seed, step).  The position sweep
    is N dependent slice steps and the longest part of such a step: `positions_every=k` sweeps the
    positions at the steps that are multiples of k only (b every step).  With `moments=True` the network entry of
    res.mean / res.m2 is that of b, `res.link_probability_mean` [N x N] is the mean link-probability matrix over the kept
    steps (the summary that does not depend on how the latent space is rotated or reflected) and `res.exhausted` counts
    the slice steps that used up their 100 attempts.  A ShardedDataset raises NotImplementedError.

    ONE chain over several GPUs: pass a `sharded.ShardedDataset` (device draws, keep_samples=False).  A sweep is
    separable by child-node column -- the parents of the children on c, column c's statistics and conjugate draws and
    the sweep of A[:, c] touch column c only, and every random stream is keyed by global event / entry indices -- so
    each rank sweeps its own columns and the chain is the single-GPU chain, value for value; the only exchange per step
    is the scalar link count the network's ρ update needs, and at the end the ranks' columns (and moments) are merged.

    Scoring the chain (csrc/cont_score.hip, definitions: include/nhp.h): `waic=` K (K equal blocks over [0, T]) or
    an array of block edges gives `res.waic`, `heldout=(data_full, edges)` gives `res.heldout` -- each a ContinuousScore over
    the cells (block, node), accumulated on the device from the steps >= `burn`, every `score_every`-th of them, with no draw
    kept: ℓ of a cell is Σ log λ over the node's events in the block minus the compensator's increment over it, so over edges
    covering [0, T] the cells add up to Σ log λ_c − Λ_c(T), the exact log-likelihood -- not loglikelihood(process, data), which
    charges every event the full mass of its impulses.  Events of `data_full` before the first edge excite the scored range.
    `pointwise=True` keeps the K x N array of elpd_i that compare_scores needs.  On the resident route the scorers are attached
    to the chain's model; step by step they are fed after every kept step; with device_draws=False (or a network model the
    library does not hold) every scored state is set into a device model kept for scoring.  A LogGaussianCoxProcess baseline,
    several trials and a ShardedDataset raise NotImplementedError.

    Credible intervals without samples (csrc/chain_quantiles.hip, definition: include/nhp.h): `quantiles=` up to
    four probabilities (True: 0.025, 0.5, 0.975), with `moments=True`, gives `res.quantiles`, a ChainQuantiles -- streaming
    estimates (extended P²) of those quantiles of every entry of params(process) over the steps >= `burn`, every
    `quantiles_every`-th of them, with the exact `min` and `max`; `res.quantiles.interval(0.95)` is the pair of rows.  The
    state is 100 bytes per entry at three probabilities and is updated by one launch after the kept step's sums, on the
    resident route and step by step alike; the sums and the diagnostics keep their bits.  vec(A) has no quantiles (NaN: its
    mean says everything); `effective_weights=True` estimates the quantiles of A[p,c]·W[p,c] in W's place, the interval that
    answers whether a link is there.  Only a BernoulliNetworkModel's ρ is estimated among the network parameters.
    device_draws=False, an LGCP baseline and a ShardedDataset raise NotImplementedError; chains.run_chains does not gather
    quantiles (marker states of different chains do not merge)."""
    import ctypes as C
    plan = _score_plan(process, data, waic, heldout, score_every, burn)      # (every argument checked before the library is touched)
    qprobs = _check_quantiles(quantiles, quantiles_every, moments)
    from .sharded import ShardedDataset, _all_reduce_sum
    from .components import BernoulliNetworkModel, DenseNetworkModel, LatentDistanceNetworkModel, StochasticBlockNetworkModel
    shard = data if isinstance(data, ShardedDataset) else None
    if diagnostics not in (False, True, "full"):
        raise ValueError('diagnostics must be False, True or "full"')
    if diagnostics and not moments:
        raise ValueError("diagnostics need the device-side running sums (moments=True)")
    if diagnostics and shard is not None:
        raise NotImplementedError("convergence diagnostics are not available for a sharded chain")
    if batch_len is not None and int(batch_len) < 1:
        raise ValueError("batch_len must be a positive integer")
    if qprobs is not None and shard is not None:
        raise NotImplementedError("streaming quantiles are not available for a sharded chain (each rank holds its own columns)")
    if qprobs is not None and not (device_draws and isinstance(process.baseline, HomogeneousProcess)):
        raise NotImplementedError("streaming quantiles live next to a device-resident model: the route with device_draws=True and a "
                                  "homogeneous baseline holds one (device_draws=False and an LGCP baseline draw on the host)")
    sbm = isinstance(getattr(process, "network", None), StochasticBlockNetworkModel)
    latent = isinstance(getattr(process, "network", None), LatentDistanceNetworkModel)
    if sbm and shard is not None:
        raise NotImplementedError("a StochasticBlockNetworkModel chain is not sharded: the block labels need every column of A")
    if latent and shard is not None:
        raise NotImplementedError("a LatentDistanceNetworkModel chain is not sharded: the positions need every column of A")
    if int(labels_every) < 1:
        raise ValueError("labels_every must be a positive integer")
    if int(positions_every) < 1:
        raise ValueError("positions_every must be a positive integer")
    if not isinstance(process.baseline, HomogeneousProcess):
        device_draws = False      # nhp_cont_gibbs_step draws the homogeneous λ0; the LGCP curve is a host slice loop
    if moments and not device_draws:
        raise ValueError("moments=True needs the device-side draws (homogeneous baseline, device_draws=True)")
    if shard is not None and (not device_draws or keep_samples):
        raise ValueError("a sharded chain runs with the device-side draws and keep_samples=False (use moments=True)")
    ctx = (shard.ctx if shard else ctx) or _lib.default_context()
    ds = shard.local if shard else device_dataset(process, data, ctx)
    rng = np.random.default_rng(seed)
    res = MarkovChainMonteCarlo()
    start = time.time()
    lib = _lib.lib()
    model = process.device_model(ctx) if device_draws else None
    pri = _priors(process) if device_draws else None
    network = isinstance(process, ContinuousNetworkHawkesProcess)
    # the network's link probability lives on the device too (nhp_cont_model_set_rho): ρ ~ Beta(α + ΣA, β + N² - ΣA) is
    # drawn there (src/networks.jl:70-78), so a network step needs no synchronisation; DenseNetworkModel keeps ρ = 1
    net = process.network if network else None
    net_a, net_b = (net.α, net.β) if isinstance(net, BernoulliNetworkModel) else (0.0, 0.0)
    device_net = device_draws and isinstance(net, (BernoulliNetworkModel, DenseNetworkModel, StochasticBlockNetworkModel,
                                                   LatentDistanceNetworkModel))
    if device_net and latent:
        _lib.check(lib.nhp_cont_model_set_latent(ctx.h, model.h, net.ndims, _lib.dptr(_lib.colmajor(net.z)), net.b, net.σ, net.μb, net.σb),
                   ctx.h)
        _lib.check(lib.nhp_cont_model_set_latent_positions_every(ctx.h, model.h, int(positions_every)), ctx.h)
    elif device_net and sbm:
        z = np.ascontiguousarray(net.z, dtype=np.int32)
        _lib.check(lib.nhp_cont_model_set_sbm(ctx.h, model.h, net.nblocks, z.ctypes.data, _lib.dptr(_lib.colmajor(net.ρ)),
                                              _lib.dptr(_lib.f64(net.π)), net.α, net.β, net.γ), ctx.h)
        _lib.check(lib.nhp_cont_model_set_sbm_labels_every(ctx.h, model.h, int(labels_every)), ctx.h)
    elif device_net:
        _lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, net.ρ if isinstance(net, BernoulliNetworkModel) else 1.0), ctx.h)
    comm = _lib.comm_for(ctx) if shard is not None else None
    host_exchange = shard is not None and shard.world > 1 and comm is None        # gloo rehearsal: link counts through the host
    if diagnostics:
        n_planned = max(0, int(nsteps) - int(burn))
        diag_b = int(batch_len) if batch_len is not None else max(1, math.isqrt(n_planned))
        _lib.check(lib.nhp_cont_model_diagnostics_configure(ctx.h, model.h, diag_b, n_planned), ctx.h)
    elif model is not None:                # a cached device model may carry an earlier chain's planes
        _lib.check(lib.nhp_cont_model_diagnostics_configure(ctx.h, model.h, 0, 0), ctx.h)
    if qprobs is not None:
        _lib.check(lib.nhp_cont_model_quantiles_configure(ctx.h, model.h, _lib.dptr(qprobs), len(qprobs), int(quantiles_every),
                                                          1 if effective_weights else 0), ctx.h)
    elif model is not None:                # ... or its marker planes
        _lib.check(lib.nhp_cont_model_quantiles_configure(ctx.h, model.h, None, 0, 1, 0), ctx.h)
    if moments:
        _lib.check(lib.nhp_cont_model_moments_reset(ctx.h, model.h), ctx.h)

    p_sum = [None]                         # a latent distance network's summed link probabilities, as last pulled

    def pull_rho():
        if device_net and latent:          # (z, b) into the component; Σb, Σb² and the summed link probabilities
            N, D = net.nnodes, net.ndims
            z, b, sums, ps, ex = np.empty(N * D), C.c_double(), np.empty(2), np.empty(N * N), C.c_int64()
            _lib.check(lib.nhp_cont_model_get_latent(ctx.h, model.h, _lib.dptr(z), C.byref(b), _lib.dptr(sums), _lib.dptr(ps), C.byref(ex)),
                       ctx.h)
            net.z, net.b = z.reshape((N, D), order="F"), b.value
            res.exhausted, p_sum[0] = int(ex.value), ps.reshape((N, N), order="F")
            return [None, sums[:1], sums[1:]]
        if device_net and sbm:             # (z, ρ, π) into the component; the running sums of [vec(ρ); π] and their squares
            K, N = net.nblocks, net.nnodes
            z, rho, pi = np.empty(N, dtype=np.int32), np.empty(K * K), np.empty(K)
            sums, bc = np.empty(2 * K * K + 2 * K), np.empty(N * K, dtype=np.int64)
            _lib.check(lib.nhp_cont_model_get_sbm(ctx.h, model.h, z.ctypes.data, _lib.dptr(rho), _lib.dptr(pi), _lib.dptr(sums),
                                                  bc.ctypes.data), ctx.h)
            net.z, net.ρ, net.π = z, rho.reshape((K, K), order="F"), pi
            res.block_counts = bc.reshape((N, K), order="F")
            KK = K * K
            return [None, np.concatenate([sums[:KK], sums[2 * KK:2 * KK + K]]), np.concatenate([sums[KK:2 * KK], sums[2 * KK + K:]])]
        if device_net and isinstance(net, BernoulliNetworkModel):
            r3 = np.empty(3)
            _lib.check(lib.nhp_cont_model_get_rho(ctx.h, model.h, _lib.dptr(r3)), ctx.h)
            net.ρ = float(r3[0])
            return r3
        return np.zeros(3)

    def pull_adjacency():
        N = process.ndims()
        A = np.empty(N * N)
        _lib.check(lib.nhp_cont_model_get_adjacency(ctx.h, model.h, _lib.dptr(A), N * N), ctx.h)
        process.adjacency_matrix = A.reshape((N, N), order="F")

    scorers, score_model, kept, qkept = [], None, 0, 0
    chain_model_scored = device_draws and (not network or device_net)      # the chain's own device model holds every scored state
    try:
        scorers = _open_scorers(ctx, process, ds, plan)
        # The whole chain inside the library (nhp_cont_mcmc_run: the body of src/inference.jl:55-62, one synchronisation per
        # call) when no step needs the host: no samples kept, device-side network.  `verbose` cuts it at the log points.
        resident = device_draws and not keep_samples and (not network or device_net) and not host_exchange
        if resident:
            for _, s in scorers:                 # nhp_cont_mcmc_run scores the kept steps itself
                _lib.check(lib.nhp_cont_model_attach_score(ctx.h, model.h, s.h, int(score_every)), ctx.h)
            # the driver's kept steps without moments: from −(burn + 1) on (include/nhp.h)
            run_burn = burn if moments else (-1 - int(burn) if scorers else -1)
            while res.steps < nsteps:
                n = min(nsteps - res.steps, log_freq if verbose else nsteps)
                _lib.check(lib.nhp_cont_mcmc_run(ctx.h, comm.h if comm is not None else None, ds.h, model.h, C.byref(pri), net_a, net_b,
                                                 seed, res.steps, n, run_burn), ctx.h)
                res.steps += n
                if verbose and res.steps % log_freq == 0:
                    res.elapsed = time.time() - start
                    print(f" > step: {res.steps}, elapsed: {res.elapsed}")
            _pull_params(process, model, ctx)
            if network:
                pull_adjacency()
                pull_rho()
        while res.steps < nsteps:
            scored = bool(scorers) and res.steps >= burn and kept % int(score_every) == 0
            if device_draws:
                _lib.check(lib.nhp_cont_gibbs_step(ctx.h, ds.h, model.h, C.byref(pri), seed, res.steps), ctx.h)
                last = keep_samples or res.steps == nsteps - 1 or (scored and not chain_model_scored)
                if network and device_net and sbm:
                    _lib.check(lib.nhp_cont_sbm_step(ctx.h, ds.h, model.h, seed, res.steps), ctx.h)
                elif network and device_net and latent:
                    _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, model.h, seed, res.steps), ctx.h)
                elif network and device_net and not host_exchange:
                    _lib.check(lib.nhp_cont_network_step(ctx.h, comm.h if comm is not None else None, ds.h, model.h, net_a, net_b,
                                                         seed, res.steps), ctx.h)
                elif network and device_net:                     # ranks without an RCCL clique: the one exchange of a step, by hand
                    nl = C.c_double()
                    _lib.check(lib.nhp_cont_network_sweep(ctx.h, ds.h, model.h, seed, res.steps, C.byref(nl)), ctx.h)
                    links = float(_all_reduce_sum(np.array([nl.value]), ctx)[0])
                    _lib.check(lib.nhp_cont_network_rho(ctx.h, model.h, net_a, net_b, links, float(process.ndims()) ** 2, seed, res.steps), ctx.h)
                elif network:                                    # a network model the library does not hold: host-side ρ
                    links = resample_adjacency_matrix_(process, ds, seed=seed, step=res.steps, model=model, fetch=last, ctx=ctx)
                    process.network.resample_links_(links, process.ndims() ** 2, rng)
                if moments and res.steps >= burn:
                    _lib.check(lib.nhp_cont_model_moments_accumulate(ctx.h, model.h), ctx.h)
                    if qprobs is not None:
                        if qkept % int(quantiles_every) == 0:
                            _lib.check(lib.nhp_cont_model_quantiles_accumulate(ctx.h, model.h), ctx.h)
                        qkept += 1
                if scored and chain_model_scored:
                    for _, s in scorers:
                        s.accumulate(model)
                if last:
                    _pull_params(process, model, ctx)
                    if network and device_net:
                        pull_adjacency()
                        pull_rho()
                x = process.params() if keep_samples else None
            else:
                x = resample_(process, ds, rng, step=res.steps, seed=seed, ctx=ctx, labels_every=int(labels_every),
                              positions_every=int(positions_every))
                if latent:
                    res.exhausted = getattr(res, "exhausted", 0) + net.exhausted
            if scored and not chain_model_scored:    # the state as params(process) into a device model kept for scoring
                score_model = _set_score_model(score_model, ctx, process, process.params())
                for _, s in scorers:
                    s.accumulate(score_model)
            if scorers and res.steps >= burn:
                kept += 1
            if keep_samples:
                res.samples.append(x)
            res.steps += 1
            if res.steps % log_freq == 0 and verbose:
                res.elapsed = time.time() - start
                print(f" > step: {res.steps}, elapsed: {res.elapsed}")
        for name, s in scorers:
            setattr(res, name, s.fetch(pointwise))
    finally:                                     # the scorers are not the model's: detach before they are destroyed
        if scorers and model is not None:
            lib.nhp_cont_model_attach_score(ctx.h, model.h, None, 1)
        for _, s in scorers:
            s.close()
    res.elapsed = time.time() - start
    res.status = "complete"
    if shard is not None and shard.world > 1:
        _merge_shards(process, shard, network)
    if not keep_samples:
        res.samples.append(process.params())
    if moments:
        r3 = pull_rho() if network else np.zeros(3)
        res.mean, res.m2, res.n = _fetch_moments(process, model, ctx, network, r3[1], r3[2])
        if latent:
            res.link_probability_mean = p_sum[0] / max(1, res.n)
        if diagnostics and res.n < 1:
            res.diagnostics = {"summary": {}}               # no kept step: nothing to diagnose
        elif diagnostics:
            res.diagnostics = _fetch_diagnostics(process, model, ctx, network, diagnostics == "full", ess_below, rhat_above)
        if diagnostics:
            res.diagnostics.update(n=res.n, batch_len=diag_b, nbatches=res.n // diag_b)
        if qprobs is not None:
            res.quantiles = _fetch_quantiles(process, model, ctx, network, qprobs, int(quantiles_every), effective_weights)
        if shard is not None and shard.world > 1:
            mask = _owned_mask(process, shard, network)
            res.mean, res.m2 = _all_reduce_sum(res.mean * mask, ctx), _all_reduce_sum(res.m2 * mask, ctx)
    return res
