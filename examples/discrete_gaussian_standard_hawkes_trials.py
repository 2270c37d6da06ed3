"""Discrete-time standard process observed as several short, independent trials (repeated presentations of one stimulus, say):
simulate R trials on the GPU under different seeds, then fit W by mle! three ways -- on the first trial alone, on the naive
concatenation np.concatenate(trials, axis=1), whose convolution lets the last bins of one trial excite the first bins of the
next, and on the list of trials, whose convolution stops at every trial's first bin -- and print the three errors against
the truth.  With windows as long as a good part of a trial the concatenation tells the model about excitation that never
happened."""
import copy

from _common import nhp, np


def make(nnodes=3, nbasis=3, nlags=30, dt=1.0, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(size=nnodes) * 0.2 + 0.05, dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) * 0.6 / nnodes + 0.05)      # row and column sums below 0.75: stable
    return nhp.DiscreteStandardHawkesProcess(baseline, impulses, weights, dt)


def main(ntrials=8, bins=400, seed=0):
    truth = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(truth)}")
    trials = [nhp.disc_rand(truth, bins, seed=seed + 1 + r) for r in range(ntrials)]
    counts, offsets = nhp.stack_trials(trials)
    print(f"Generated {counts.sum()} events in {ntrials} trials of {bins} bins (offsets {offsets.tolist()})")
    true_W = truth.weights.W
    fits = {}
    for name, data in (("first trial alone", trials[0]), ("naive concatenation", counts), ("trials", trials)):
        process = copy.deepcopy(truth)
        res = nhp.mle_(process, data, optimizer="device", seed=seed)
        err = float(np.abs(process.weights.W - true_W).mean())
        fits[name] = (process, res, err)
        print(f"{name:>20}: mean |W - truth| = {err:.4f}   log-likelihood of the trials at the fit = {nhp.loglikelihood(process, trials):.3f}"
              f"   ({res.status}, {res.steps} steps)")
    print("W fitted on the trials, link by link (truth in brackets):")
    W = fits["trials"][0].weights.W
    for p in range(W.shape[0]):
        print("   " + "  ".join(f"{W[p, c]:.3f} ({true_W[p, c]:.3f})" for c in range(W.shape[1])))
    return truth, trials, fits


if __name__ == "__main__":
    main()
