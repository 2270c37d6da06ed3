"""Continuous-time standard process, exponential impulse response: simulate on [0, T + h], fit on [0, T] by
expectation-maximisation, forecast (T, T + h] on the GPU conditional on the observed events, and compare the ensemble with
the held-out truth and with a forecast that forgets the history."""
from _common import nhp, np


def main(duration=1000.0, horizon=5.0, nnodes=3, nsamples=2000, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.HomogeneousProcess(rng.uniform(size=nnodes) * 0.5)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 1.5 / nnodes)
    impulses = nhp.ExponentialImpulseResponse(rng.uniform(size=(nnodes, nnodes)) * 0.5 + 0.2)
    process = nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)
    print(f"Process is stable? {nhp.isstable(process)}")
    events, nodes, _ = nhp.synthetic.rand(process, duration + horizon, seed=seed)
    seen = events <= duration
    data = (events[seen], nodes[seen], duration)
    truth = np.bincount(nodes[~seen] - 1, minlength=nnodes)
    print(f"Observed {seen.sum()} events on [0, {duration}], held out {len(events) - seen.sum()} on ({duration}, {duration + horizon}]")
    nhp.em_(process, data, seed=seed)
    f = nhp.forecast(process, data, horizon, nsamples=nsamples, seed=seed, return_paths=True)
    mean, sd = f.counts.mean(axis=0), f.counts.std(axis=0)
    print(f"expected carry-over from the observed events, per node: {np.round(f.carry, 2)}")
    print(f"forecast mean +- sd per node: {np.round(mean, 2)} +- {np.round(sd, 2)}")
    print(f"held-out truth per node:      {truth}")
    cold = nhp.forecast(process, (np.empty(0), np.empty(0, np.int64), duration), horizon, nsamples=nsamples, seed=seed)
    print(f"without the history:          {np.round(cold.counts.mean(axis=0), 2)}")
    # predictive check: one continuation appended to the history is data again
    t, n = f.path(0)
    full = (np.concatenate([data[0], t]), np.concatenate([data[1], n]), duration + horizon)
    print(f"log-likelihood of history + continuation 0: {nhp.loglikelihood(process, full):.2f}")
    return truth, f, cold


if __name__ == "__main__":
    main()
