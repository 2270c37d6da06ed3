"""Continuous-time standard process, exponential impulse response: simulate, look at the expected branching structure
under the truth, then fit by expectation-maximisation on the GPU (em_) and check the fit by time rescaling."""
from _common import nhp, np, show


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
    stats = nhp.expected_statistics(process, data)
    print(f"expected background events per node: {stats.bg}")
    print(f"expected children, [parent node, child node]:\n{stats.EM}")
    res = nhp.em_(process, data, seed=seed, keep_trace=True)
    show("true vs em", θ, res.maximizer)
    test = nhp.time_rescaling_test(process, data)
    print(f"time rescaling under the fit: p = {test.pvalue:.3f}")
    return θ, res, stats, test


if __name__ == "__main__":
    main()
