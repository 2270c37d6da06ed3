"""Which of three fitted models is better?  Events are simulated from a continuous-time network process with few links.  A
standard process, a network process with a dense network and one with a Bernoulli network are fitted by mcmc! on the first
80 % of the recording, each chain resident on the device, and scored as it runs: WAIC over blocks of the training time and the
predictive log-likelihood of the held-out 20 % (log mean_s p(D_test | θ_s); the events before the split still excite it).
A scored cell is (block of time, node): the sum of log λ over the node's events in the block minus the compensator's
increment over it -- the exact log-likelihood of the block given the past.  No draw is stored: per cell the device keeps a
running log-sum-exp and a running mean and variance.  compare_scores gives the elpd difference of two models with the
standard error of the paired difference.  (A dense network keeps every link, so from the same seed its chain is the
standard process's chain: the comparison that matters is with the Bernoulli network, which can drop links.)"""
from _common import nhp, np


def main(duration=600.0, nnodes=6, plink=0.25, nblocks=40, nsteps=300, burn=60, score_every=2, seed=4):
    rng = np.random.default_rng(seed)
    links = (rng.uniform(size=(nnodes, nnodes)) < plink).astype(np.float64)
    truth = nhp.ContinuousNetworkHawkesProcess(nhp.HomogeneousProcess(rng.uniform(0.2, 0.4, nnodes)),
                                               nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 8.0), 1.0, 1.0, 1.0),
                                               nhp.DenseWeightModel(rng.uniform(0.3, 0.6, (nnodes, nnodes))), links,
                                               nhp.BernoulliNetworkModel(plink, nnodes))
    print(f"Process is stable? {nhp.isstable(truth)}")
    events, nodes, _ = nhp.synthetic.rand(truth, duration, seed=seed)
    events, nodes = np.asarray(events, dtype=np.float64), np.asarray(nodes)
    split = 0.8 * duration
    ntrain = int(np.searchsorted(events, split))
    train, full = (events[:ntrain].copy(), nodes[:ntrain].copy(), split), (events, nodes, duration)
    held_edges = np.linspace(split, duration, max(2, nblocks // 4) + 1)
    held_edges[-1] = duration
    print(f"Generated {len(events)} events on {nnodes} nodes, {int(links.sum())} of {nnodes * nnodes} links; "
          f"fitting [0, {split:g}) ({ntrain} events), holding out [{split:g}, {duration:g}]")

    def parts():
        return (nhp.HomogeneousProcess(np.full(nnodes, 0.3)), nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 5.0), 1.0, 1.0, 1.0),
                nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.1)))

    models = {"standard": nhp.ContinuousStandardHawkesProcess(*parts()),
              "dense network": nhp.ContinuousNetworkHawkesProcess(*parts(), np.ones((nnodes, nnodes)), nhp.DenseNetworkModel(nnodes)),
              "Bernoulli network": nhp.ContinuousNetworkHawkesProcess(*parts(), np.ones((nnodes, nnodes)), nhp.BernoulliNetworkModel(0.5, nnodes))}
    scores = {}
    for name, process in models.items():
        res = nhp.mcmc_(process, train, nsteps=nsteps, burn=burn, seed=seed, keep_samples=False, waic=nblocks,
                        heldout=(full, held_edges), score_every=score_every, pointwise=True)
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
