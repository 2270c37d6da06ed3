"""Discrete-time standard process with Gaussian-basis impulse responses: simulate on the GPU (disc_rand), fit by mle!, and ask
whether the fitted process describes the counts (disc_goodness_of_fit: the randomized probability integral transform of every
cell is uniform under the model) -- then ask the same of a deliberately wrong model, the fit with every weight set to zero."""
import copy

from _common import nhp, np


def make(nnodes=3, nbasis=3, nlags=6, dt=1.0, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(size=nnodes) * 0.5, dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 1.5 / nnodes)
    return nhp.DiscreteStandardHawkesProcess(baseline, impulses, weights, dt)


def report(name, fit):
    print(f"{name}: KS statistic {fit.statistic:.4f}, p = {fit.pvalue:.3g}; pit histogram p = {fit.histogram_pvalue:.3g}")
    print(f"  per node: KS p {np.round(fit.node_pvalue, 3)}, dispersion {np.round(fit.dispersion, 3)}, "
          f"expected {np.round(fit.expected, 1)} against observed {fit.observed}")


def main(duration=4000, seed=0):
    process = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(process)}")
    data = nhp.disc_rand(process, duration, seed=seed)
    print(f"Generated {data.sum()} events in {duration} bins")
    nhp.mle_(process, data, seed=seed)
    fitted = nhp.disc_goodness_of_fit(process, data, seed=seed)
    report("fitted process", fitted)
    # a wrong model with the right event totals: no excitation, the baseline carries every event
    poisson = copy.deepcopy(process)
    poisson.weights.W = np.zeros_like(poisson.weights.W)
    poisson.baseline.λ = data.sum(axis=1) / (duration * process.dt)
    flat = nhp.disc_goodness_of_fit(poisson, data, seed=seed)
    report("no excitation", flat)
    res = nhp.disc_residuals(process, data, seed=seed, pearson=True, cumulative=True)
    worst = np.unravel_index(np.argmax(np.abs(res.pearson)), res.pearson.shape)
    print(f"largest Pearson residual {res.pearson[worst]:.2f} at node {worst[0] + 1}, bin {worst[1] + 1}; "
          f"compensator at the end {np.round(res.cumulative[:, -1], 1)}")
    return fitted, flat, res


if __name__ == "__main__":
    main()
