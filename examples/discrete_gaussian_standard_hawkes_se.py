"""Discrete-time standard process with Gaussian-basis impulse responses: simulate on the GPU (disc_rand), fit by mle! with the
optimizer's state on the device, then say how certain the estimate is: standard errors and Wald intervals from the inverse
observed information (disc_standard_errors), printed with the truth beside them.  The parameters are mle!'s own,
[λ0; η = W∘θ]; the errors of W = Σ_b η and of θ = η/W follow from each link's covariance."""
from _common import nhp, np


def make(nnodes=3, nbasis=3, nlags=6, dt=1.0, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(size=nnodes) * 0.5 + 0.1, dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 0.6 / nnodes + 0.05)      # row and column sums below 0.75: stable
    return nhp.DiscreteStandardHawkesProcess(baseline, impulses, weights, dt)


def main(duration=20000, seed=0, level=0.95, kind="observed"):
    process = make(seed=seed)
    N, B = process.ndims(), process.impulses.nbasis()
    print(f"Process is stable? {nhp.isstable(process)}")
    truth = process.params()
    true_W = process.weights.W.copy()
    data = nhp.disc_rand(process, duration, seed=seed)
    print(f"Generated {data.sum()} events in {duration} bins")
    res = nhp.mle_(process, data, optimizer="device", seed=seed)
    out = nhp.disc_standard_errors(process, data, kind=kind, level=level)
    names = [f"λ0[{c + 1}]" for c in range(N)] + [f"η[{p + 1},{c + 1},{b + 1}]" for b in range(B) for c in range(N) for p in range(N)]
    print(f"{'parameter':>10} {'truth':>9} {'estimate':>9} {'se':>9} {'%g %% interval' % (100 * level):>22}")
    for name, t, x, se, lo, hi, free in zip(names, truth, res.maximizer, out.se, out.lower_ci, out.upper_ci, out.free):
        print(f"{name:>10} {t:9.4f} {x:9.4f} " + (f"{se:9.4f}   [{lo:8.4f}, {hi:8.4f}]" if free else "   (on the bound: not free)"))
    inside = out.free & (out.lower_ci <= truth) & (truth <= out.upper_ci)
    print(f"{int(inside.sum())} of {int(out.free.sum())} true values fall inside their intervals")
    print("W and its standard error, link by link:")
    for p in range(N):
        print("   " + "  ".join(f"{process.weights.W[p, c]:.3f} ± {out.se_W[p, c]:.3f} (true {true_W[p, c]:.3f})" for c in range(N)))
    print(f"positive definite, column by column: {out.pd.tolist()}")
    return truth, res, out


if __name__ == "__main__":
    main()
