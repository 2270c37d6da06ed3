"""Continuous-time standard process, exponential impulse response: simulate, then fit a mean-field posterior over every
parameter on the GPU (vb_) and print its 95% credible intervals beside the truth."""
from _common import nhp, np


def main(duration=1000.0, nnodes=2, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.HomogeneousProcess(rng.uniform(size=nnodes))
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) / nnodes)
    impulses = nhp.ExponentialImpulseResponse(rng.uniform(size=(nnodes, nnodes)) + 0.5)
    process = nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)
    print(f"Process is stable? {nhp.isstable(process)}")
    θ = process.params()
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events")
    res = nhp.vb_(process, data, guess=rng.uniform(0.2, 0.8, len(θ)))
    print(f"{res.steps} updates in {res.elapsed:.3f} s, ELBO {res.trace[0]:.3f} -> {res.elbo:.3f} ({res.status})")
    lower, upper = res.interval(0.95)
    print("      true      mean        sd   95% interval")
    for t, m, s, lo, hi in zip(θ, res.mean(), res.sd(), lower, upper):
        print(f"{t:10.4f}{m:10.4f}{s:10.4f}   [{lo:.4f}, {hi:.4f}]{'' if lo <= t <= hi else '  *'}")
    print(f"expected children, [parent node, child node]:\n{res.expected_links()}")
    print(f"log-likelihood at the posterior mean: {nhp.loglikelihood(process, data):.3f}")
    return θ, res, lower, upper


if __name__ == "__main__":
    main()
