"""Discrete-time standard process with Gaussian-basis impulse responses: simulate on the GPU (disc_rand), fit the variational
posterior by stochastic variational inference (svi_: one block of bins per step) and by the same number of passes of
mean-field VB (vb_), and compare the log-likelihood at the variational means.  svi_(streamed=True) fits the same numbers
without keeping the T x N x B convolution on the device."""
import copy

from _common import nhp, np


def make(nnodes=3, nbasis=3, nlags=6, dt=1.0, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(size=nnodes) * 0.5, dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 1.5 / nnodes)
    return nhp.DiscreteStandardHawkesProcess(baseline, impulses, weights, dt)


def at_the_means(process):
    """The process with its parameters set to the variational means: λ0 = αv/βv, W = κv/νv, θ = γv/Σ_b γv."""
    p = copy.deepcopy(process)
    p.baseline.λ = p.baseline.αv / p.baseline.βv
    p.weights.W = p.weights.κv / p.weights.νv
    p.impulses.θ = p.impulses.γv / p.impulses.γv.sum(axis=2, keepdims=True)
    return p


def main(duration=20000, batch_bins=256, passes=5, seed=0):
    truth = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(truth)}")
    data = nhp.disc_rand(truth, duration, seed=seed)
    print(f"Generated {data.sum()} events in {duration} bins")
    nblocks = -(-duration // min(batch_bins, duration))
    svi, vb, streamed = make(seed=seed + 1), make(seed=seed + 1), make(seed=seed + 1)
    res = nhp.svi_(svi, data, nsteps=passes * nblocks, batch_bins=batch_bins, delay=10.0, forgetting=0.6, seed=seed)
    nhp.vb_(vb, data, max_steps=passes, keep_trace=False)
    nhp.svi_(streamed, data, nsteps=passes * nblocks, batch_bins=batch_bins, delay=10.0, forgetting=0.6, seed=seed, streamed=True)
    ll_svi = nhp.loglikelihood(at_the_means(svi), data)
    ll_vb = nhp.loglikelihood(at_the_means(vb), data)
    ll_true = nhp.loglikelihood(truth, data)
    print(f"log-likelihood at the variational means after {passes} passes' worth of data: "
          f"SVI ({res.step} steps of {batch_bins} bins) {ll_svi:.1f}, VB ({passes} steps) {ll_vb:.1f}; true parameters {ll_true:.1f}")
    gap = np.max(np.abs(streamed.variational_params() - svi.variational_params()) / np.abs(svi.variational_params()))
    print(f"streamed against resident convolution: largest relative difference {gap:.1e}")
    print("W: truth, SVI, VB")
    print(np.column_stack([truth.weights.W.ravel(), at_the_means(svi).weights.W.ravel(), at_the_means(vb).weights.W.ravel()]))
    return svi, vb, ll_svi, ll_vb


if __name__ == "__main__":
    main()
