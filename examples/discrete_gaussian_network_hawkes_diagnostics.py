"""When to stop a discrete chain that keeps no samples: a discrete-time network process (Gaussian basis, Bernoulli network)
is fitted by mcmc! with its state, the running sums AND the streaming convergence diagnostics on the device -- effective
sample size, Monte-Carlo standard error and split R-hat of every parameter from batch means and two snapshots, one kernel
launch per kept step, nothing but an 8-byte link count crossing PCIe between the steps.  The summary says, group by group,
which entry mixes worst; a second chain from another seed shows how far two posterior means are apart in MCSE units."""
from _common import discrete_data, nhp, np


def main(duration=4000, nnodes=6, nbasis=3, nlags=5, dt=1.0, plink=0.5, nsteps=400, burn=80, seed=2):
    rng = np.random.default_rng(seed)
    network = nhp.BernoulliNetworkModel(plink, nnodes)
    links = network.rand(rng)
    process = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.2, nnodes), dt),
                                               nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt),
                                               nhp.DenseWeightModel(rng.uniform(0.2, 1.0, (nnodes, nnodes)) / nnodes), links, network, dt)
    print(f"Process is stable? {nhp.isstable(process)}")
    data = discrete_data(process, duration, seed)
    print(f"Generated {data.sum()} events on {nnodes} nodes, {int(links.sum())} links")

    def start():
        return nhp.DiscreteNetworkHawkesProcess(
            nhp.DiscreteHomogeneousProcess(np.full(nnodes, 0.1), dt),
            nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt),
            nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.1)), np.ones((nnodes, nnodes)), nhp.BernoulliNetworkModel(0.5, nnodes), dt)

    chain = nhp.mcmc_(start(), data, nsteps=nsteps, burn=burn, seed=seed, keep_samples=False, moments=True, diagnostics="full")
    d = chain.diagnostics
    print(f"{d['n']} kept steps in {d['nbatches']} batches of {d['batch_len']}")
    print(f"{'group':<12} {'entries':>7} {'undef':>5} {'min ESS':>9} {'at':>4} {'max R-hat':>9} {'at':>4} {'ESS<100':>7} {'R>1.01':>6} {'max MCSE':>9}")
    for name, g in d["summary"].items():
        print(f"{name:<12} {g['entries']:>7} {g['undefined']:>5} {g['min_ess']:>9.1f} {g['min_ess_index']:>4} {g['max_rhat']:>9.4f} "
              f"{g['max_rhat_index']:>4} {g['ess_below']:>7} {g['rhat_above']:>6} {g['max_mcse']:>9.2e}")
    # a second chain, another seed: the two posterior means in units of their Monte-Carlo standard errors
    other = nhp.mcmc_(start(), data, nsteps=nsteps, burn=burn, seed=seed + 1, keep_samples=False, moments=True, diagnostics="full")
    se = np.sqrt(d["mcse"] ** 2 + other.diagnostics["mcse"] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.abs(chain.mean - other.mean) / se
    print(f"two chains: |Δ mean| / MCSE has median {np.nanmedian(z):.2f}, max {np.nanmax(z[np.isfinite(z)]):.2f} "
          f"over {int(np.isfinite(z).sum())} entries")
    return chain, z


if __name__ == "__main__":
    main()
