"""When to stop a chain that keeps no samples: a continuous-time network process (exponential impulses, Bernoulli network)
is fitted by mcmc! with the running sums AND the streaming convergence diagnostics on the device -- effective sample size,
Monte-Carlo standard error and split R-hat of every parameter from batch means and two snapshots, one kernel launch per
kept step.  The summary says, group by group, which entry mixes worst; two more chains give the between-chain R-hat."""
from _common import nhp, np


def main(duration=1500.0, nnodes=12, rho=0.3, nsteps=600, burn=100, seed=2, n_chains=3):
    rng = np.random.default_rng(seed)
    links = (rng.uniform(size=(nnodes, nnodes)) < rho).astype(np.float64)
    baseline = nhp.HomogeneousProcess(rng.uniform(0.1, 0.2, nnodes))
    weights = nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.6 / (rho * nnodes)))
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 10.0), 1.0, 1.0, 1.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, links, nhp.BernoulliNetworkModel(rho, nnodes))
    print(f"Process is stable? {nhp.isstable(process)}")
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events on {nnodes} nodes, {int(links.sum())} links")

    def start():
        return nhp.ContinuousNetworkHawkesProcess(
            nhp.HomogeneousProcess(np.full(nnodes, 0.2)), nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 5.0), 1.0, 1.0, 1.0),
            nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.1)), np.ones((nnodes, nnodes)), nhp.BernoulliNetworkModel(0.5, nnodes))

    chain = nhp.mcmc_(start(), data, nsteps=nsteps, burn=burn, seed=seed, keep_samples=False, moments=True, diagnostics=True)
    d = chain.diagnostics
    print(f"{d['n']} kept steps in {d['nbatches']} batches of {d['batch_len']}")
    print(f"{'group':<12} {'entries':>7} {'undef':>5} {'min ESS':>9} {'at':>4} {'max R-hat':>9} {'at':>4} {'ESS<100':>7} {'R>1.01':>6} {'max MCSE':>9}")
    for name, g in d["summary"].items():
        print(f"{name:<12} {g['entries']:>7} {g['undefined']:>5} {g['min_ess']:>9.1f} {g['min_ess_index']:>4} {g['max_rhat']:>9.4f} "
              f"{g['max_rhat_index']:>4} {g['ess_below']:>7} {g['rhat_above']:>6} {g['max_mcse']:>9.2e}")
    # independent chains from the same start: the classic between-chain R-hat from the gathered means and mean squares
    summaries = nhp.chains.run_chains(lambda k: start(), data, n_chains=n_chains, nsteps=nsteps, base_seed=seed, burn=burn)
    between = nhp.chains.potential_scale_reduction(summaries)
    print(f"between-chain R-hat over {n_chains} chains: max {np.nanmax(between):.4f}, {int(np.sum(between > 1.01))} of "
          f"{int(np.sum(~np.isnan(between)))} entries above 1.01")
    return chain, between


if __name__ == "__main__":
    main()
