"""Continuous-time standard process observed as several short, independent trials (repeated presentations of one stimulus, trading
days, sessions): simulate R trials under different seeds, then fit three ways -- the first trial alone, the naive concatenation
(one recording of length ΣT_r, in which the last events of one trial excite the first events of the next), and the list of
trials, whose look-back windows stop at every trial's first event -- by mle! on the GPU, once more by EM, and check the fit on
the trials by time rescaling: every trial's compensator starts at the trial's own start."""
import copy

from _common import nhp, np


def make(nnodes=2, seed=0):
    rng = np.random.default_rng(seed)
    baseline = nhp.HomogeneousProcess(rng.uniform(size=nnodes) + 0.5)
    weights = nhp.DenseWeightModel(rng.uniform(size=(nnodes, nnodes)) / nnodes + 0.1)
    impulses = nhp.ExponentialImpulseResponse(rng.uniform(size=(nnodes, nnodes)) * 0.5 + 0.25)      # slow decays: long memories
    return nhp.ContinuousStandardHawkesProcess(baseline, impulses, weights)


def main(ntrials=40, duration=25.0, seed=0):
    truth = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(truth)}")
    trials = [nhp.synthetic.rand(truth, duration, seed=seed + 1 + r) for r in range(ntrials)]
    stacked = nhp.stack_event_trials(trials)                             # (a list of trials is taken as it is too; stacked once,
                                                                         #  the device copy is reused from call to call)
    print(f"Generated {len(stacked.events)} events in {ntrials} trials of length {duration} "
          f"(event offsets {stacked.event_offsets[:4].tolist()} ...)")
    naive = (stacked.events, stacked.nodes, stacked.duration)            # the same events as ONE recording: windows cross the seams
    θ = truth.params()
    fits = {}
    for name, data in (("first trial alone", trials[0]), ("naive concatenation", naive), ("trials", stacked)):
        process = copy.deepcopy(truth)
        res = nhp.mle_(process, data, optimizer="device", seed=seed)
        err = float(np.abs(process.params() - θ).mean())
        fits[name] = (process, res, err)
        print(f"{name:>20}: mean |params - truth| = {err:.4f}   log-likelihood of the trials at the fit = "
              f"{nhp.loglikelihood(process, stacked):.3f}   ({res.status}, {res.steps} steps)")
    em = copy.deepcopy(truth)
    res_em = nhp.em_(em, stacked, seed=seed)
    print(f"{'trials, by EM':>20}: mean |params - truth| = {float(np.abs(em.params() - θ).mean()):.4f}   log-likelihood = {res_em.maximum:.3f}"
          f"   ({res_em.status}, {res_em.steps} steps)")
    test = nhp.time_rescaling_test(fits["trials"][0], stacked)
    print(f"time rescaling of the trials under the fit on the trials: p = {test.pvalue:.3f}")
    return truth, trials, fits, res_em, test


if __name__ == "__main__":
    main()
