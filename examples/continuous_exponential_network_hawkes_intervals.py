"""Which links are there?  A continuous-time network process (exponential impulses, Bernoulli network) is fitted by mcmc!
with no sample kept: the running sums and streaming quantiles of every parameter stay on the device (extended P², one
launch per kept step).  With effective_weights the quantiles of W[p,c] are those of A[p,c]·W[p,c] -- a spike at zero
while the link is off, the weight's Gamma while it is on -- so the links whose 95 % interval excludes zero are the ones the
posterior keeps switched on nearly always."""
from _common import nhp, np


def main(duration=1500.0, nnodes=12, rho=0.3, nsteps=600, burn=100, seed=2):
    rng = np.random.default_rng(seed)
    links = (rng.uniform(size=(nnodes, nnodes)) < rho).astype(np.float64)
    baseline = nhp.HomogeneousProcess(rng.uniform(0.1, 0.2, nnodes))
    weights = nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.6 / (rho * nnodes)))
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 10.0), 1.0, 1.0, 1.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, links, nhp.BernoulliNetworkModel(rho, nnodes))
    print(f"Process is stable? {nhp.isstable(process)}")
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events on {nnodes} nodes, {int(links.sum())} links")

    fit = nhp.ContinuousNetworkHawkesProcess(
        nhp.HomogeneousProcess(np.full(nnodes, 0.2)), nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 5.0), 1.0, 1.0, 1.0),
        nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.1)), np.ones((nnodes, nnodes)), nhp.BernoulliNetworkModel(0.5, nnodes))
    chain = nhp.mcmc_(fit, data, nsteps=nsteps, burn=burn, seed=seed, keep_samples=False, moments=True, quantiles=True,
                      effective_weights=True)
    q = chain.quantiles
    lower, upper = q.interval(0.95)
    # params(process) of a network process: [ρ; λ0; vec(W); vec(θ); vec(A)], matrices column-major (p + N·c)
    NN = nnodes * nnodes
    w = slice(1 + nnodes, 1 + nnodes + NN)
    a = slice(1 + nnodes + 2 * NN, 1 + nnodes + 3 * NN)
    lo = lower[w].reshape((nnodes, nnodes), order="F")
    hi = upper[w].reshape((nnodes, nnodes), order="F")
    med = q.values[1][w].reshape((nnodes, nnodes), order="F")
    on = chain.mean[a].reshape((nnodes, nnodes), order="F")
    # P² interpolates between its markers: a marker that sits on the spike at zero is a hair above zero, not zero, so
    # "excludes zero" is read against the weight's own scale
    found = lo > 1e-3 * hi
    print(f"{q.n} kept steps; ρ: median {q.values[1][0]:.3f}, 95 % interval [{lower[0]:.3f}, {upper[0]:.3f}]")
    print(f"{int(found.sum())} links whose 95 % interval of A·W excludes zero ({int((found & (links > 0)).sum())} of them true, "
          f"{int(links.sum())} true links in all)")
    print(f"{'parent':>6} {'child':>5} {'2.5 %':>8} {'median':>8} {'97.5 %':>8} {'P(link)':>8} {'true':>5}")
    for p, c in zip(*np.nonzero(found)):
        print(f"{p + 1:>6} {c + 1:>5} {lo[p, c]:>8.4f} {med[p, c]:>8.4f} {hi[p, c]:>8.4f} {on[p, c]:>8.3f} {int(links[p, c]):>5}")
    return chain, found, links


if __name__ == "__main__":
    main()
