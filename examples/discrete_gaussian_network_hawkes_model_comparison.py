"""Which of three fitted models is better?  Counts are simulated on the GPU (disc_rand) from a discrete-time network process
with few links.  A standard process, a network process with a dense network and one with a Bernoulli network are fitted by
mcmc! on the first 80 % of the bins, each chain resident on the device, and scored as it runs: WAIC on the training bins and
the predictive log-likelihood of the held-out 20 % (log mean_s p(D_test | θ_s), with the history before the split kept in
the convolution).  No draw is stored: per scored cell the device keeps a running log-sum-exp and a running mean and variance
of the cell's log-likelihood.  compare_scores gives the elpd difference of two models with the standard error of the paired
difference.  (A dense network keeps every link, so from the same seed its chain is the standard process's chain and the two
rows agree to the last digit: the comparison that matters is with the Bernoulli network, which can drop links.)"""
from _common import nhp, np


def main(duration=3000, nnodes=6, nbasis=3, nlags=5, dt=1.0, plink=0.25, nsteps=300, burn=60, score_every=2, seed=4):
    rng = np.random.default_rng(seed)
    network = nhp.BernoulliNetworkModel(plink, nnodes)
    links = network.rand(rng)
    truth = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.2, nnodes), dt),
                                             nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt),
                                             nhp.DenseWeightModel(rng.uniform(0.3, 0.7, (nnodes, nnodes))), links, network, dt)
    print(f"Process is stable? {nhp.isstable(truth)}")
    data = np.asarray(nhp.disc_rand(truth, duration, seed=seed))
    split = int(0.8 * duration)
    print(f"Generated {data.sum()} events on {nnodes} nodes, {int(links.sum())} of {nnodes * nnodes} links; "
          f"fitting bins [0, {split}), holding out [{split}, {duration})")

    def parts():
        return (nhp.DiscreteHomogeneousProcess(np.full(nnodes, 0.1), dt),
                nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt),
                nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.1)))

    models = {"standard": nhp.DiscreteStandardHawkesProcess(*parts(), dt),
              "dense network": nhp.DiscreteNetworkHawkesProcess(*parts(), np.ones((nnodes, nnodes)), nhp.DenseNetworkModel(nnodes), dt),
              "Bernoulli network": nhp.DiscreteNetworkHawkesProcess(*parts(), np.ones((nnodes, nnodes)), nhp.BernoulliNetworkModel(0.5, nnodes), dt)}
    scores = {}
    for name, process in models.items():
        res = nhp.mcmc_(process, data[:, :split], nsteps=nsteps, burn=burn, seed=seed, keep_samples=False, waic=True,
                        heldout=(data, (split, duration)), score_every=score_every, pointwise=True)
        scores[name] = (res.waic, res.heldout)
    first = next(iter(scores))
    print(f"{'model':<18} {'draws':>5} {'waic':>10} {'p_waic':>8} {'elpd ± se':>18} {'held-out lpd':>13} {'Δelpd vs ' + first + ' ± se':>30}")
    table = {}
    for name, (w, h) in scores.items():
        c = nhp.compare_scores(w, scores[first][0])
        table[name] = dict(waic=w.waic, p_waic=w.p_waic, elpd=w.elpd_waic, se=w.se_elpd, heldout=h.joint_lpd, diff=c.elpd_diff, diff_se=c.se_diff)
        print(f"{name:<18} {w.n:>5} {w.waic:>10.2f} {w.p_waic:>8.2f} {w.elpd_waic:>10.2f} ± {w.se_elpd:<5.2f} {h.joint_lpd:>13.2f} "
              f"{c.elpd_diff:>22.2f} ± {c.se_diff:<5.2f}")
    best = min(table, key=lambda k: table[k]["waic"])
    print(f"lowest WAIC: {best}; highest held-out lpd: {max(table, key=lambda k: table[k]['heldout'])}")
    return scores, table


if __name__ == "__main__":
    main()
