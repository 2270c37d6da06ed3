"""Discrete-time standard process with Gaussian-basis impulse responses: simulate T + H bins on the GPU (disc_rand), fit the
first T by mle!, forecast the held-out H bins on the GPU conditional on the observed counts (disc_forecast), and compare
the ensemble and the exact predictive mean with the held-out truth and with a forecast that forgets the history."""
from _common import nhp, np


def make(nnodes=3, nbasis=3, nlags=6, dt=1.0, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(size=nnodes) * 0.5, dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 1.5 / nnodes)
    return nhp.DiscreteStandardHawkesProcess(baseline, impulses, weights, dt)


def main(duration=1000, horizon=8, nsamples=2000, seed=0):
    process = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(process)}")
    counts = nhp.disc_rand(process, duration + horizon, seed=seed)
    data, truth = counts[:, :duration], counts[:, duration:]
    print(f"Observed {data.sum()} events in {duration} bins, held out {truth.sum()} in the next {horizon}")
    nhp.mle_(process, data, seed=seed)
    f = nhp.disc_forecast(process, data, horizon, nsamples=nsamples, seed=seed, return_paths=True)
    print(f"expected carry-over per node and bin:\n{np.round(f.carry, 2)}")
    print(f"exact predictive mean:\n{np.round(f.expected, 2)}")
    print(f"ensemble mean ({nsamples} continuations):\n{np.round(f.mean, 2)}")
    print(f"held-out truth:\n{truth}")
    print(f"totals over the horizon, mean +- sd per node: {np.round(f.totals.mean(axis=0), 2)} +- {np.round(f.totals.std(axis=0), 2)}; "
          f"truth {truth.sum(axis=1)}")
    cold = nhp.disc_forecast(process, np.zeros_like(data[:, -1:]), horizon, nsamples=nsamples, seed=seed)
    print(f"without the history:  {np.round(cold.totals.mean(axis=0), 2)}")
    # predictive check: one continuation appended to the data is data again
    full = np.hstack([data, f.paths[0]])
    print(f"log-likelihood of data + continuation 0: {nhp.loglikelihood(process, full):.2f}")
    return truth, f, cold


if __name__ == "__main__":
    main()
