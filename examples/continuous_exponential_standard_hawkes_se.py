"""Continuous-time standard process, exponential impulse response: simulate, fit by expectation-maximisation on the GPU
(em_), then say how certain the estimate is: standard errors and Wald intervals from the inverse observed information
(standard_errors), printed with the truth beside them."""
from _common import nhp, np


def main(duration=2000.0, nnodes=2, seed=0, level=0.95):
    rng = np.random.default_rng(seed)
    baseline = nhp.HomogeneousProcess(rng.uniform(size=nnodes) + 0.5)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) / nnodes + 0.1)
    impulses = nhp.ExponentialImpulseResponse(rng.uniform(size=(nnodes, nnodes)) + 1.5)
    process = nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)
    print(f"Process is stable? {nhp.isstable(process)}")
    truth = process.params()
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events")
    res = nhp.em_(process, data, seed=seed)
    out = nhp.standard_errors(process, data, level=level)
    names = [f"λ0[{c + 1}]" for c in range(nnodes)] + [f"{k}[{p + 1},{c + 1}]" for k in ("θ", "W") for c in range(nnodes) for p in range(nnodes)]
    print(f"{'parameter':>10} {'truth':>9} {'estimate':>9} {'se':>9} {'%g %% interval' % (100 * level):>22}")
    for name, t, x, se, lo, hi in zip(names, truth, res.maximizer, out.se, out.lower_ci, out.upper_ci):
        print(f"{name:>10} {t:9.4f} {x:9.4f} {se:9.4f}   [{lo:8.4f}, {hi:8.4f}]")
    print(f"positive definite, column by column: {out.pd.tolist()}")
    return truth, res, out


if __name__ == "__main__":
    main()
