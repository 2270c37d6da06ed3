"""Discrete-time network process whose links follow a stochastic block model: plant two blocks (links dense inside a
block, sparse across), simulate, and fit the mean-field posterior with vb_ -- q(A[p,c] = 1) = ρv[p,c] for the links,
q(z_n) = Categorical(mv[n,:]) for the labels, a Beta per pair of blocks and a Dirichlet for the block sizes.

The block model has no variational state until variational_init_ creates one: mean-field over labels cannot leave the
uniform state.  The start here carries no information about the planted halves (the labels alternate).  The sweep over
the labels runs at every 10th step (labels_every): while ρv is still flat, early in the fit, a sweep would collapse all
nodes into one block, and no later step leaves that state.  variational_mean_ then sets ρ, π and the labels to the
posterior means / modes, so the log-likelihood of the fit can be evaluated."""
from _common import nhp, np


def make(nnodes=12, nbasis=3, nlags=8, dt=1.0, seed=3, truth=True, p_in=0.9, p_out=0.05):
    rng = np.random.default_rng(seed)
    z = (np.arange(nnodes) >= nnodes // 2).astype(np.int32) if truth else (np.arange(nnodes) % 2).astype(np.int32)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.15, nnodes), dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    P = np.where(z[:, None] == z[None, :], p_in, p_out)
    A = (rng.uniform(size=(nnodes, nnodes)) < P).astype(np.float64) if truth else np.ones((nnodes, nnodes))
    W = rng.uniform(0.04, 0.12, (nnodes, nnodes))
    # spike Gamma(0.5, 100): mean 0.005;  slab Gamma(2, 20): mean 0.1
    weights = nhp.SparseWeightModel(W, κ0=0.5, ν0=100.0, κ1=2.0, ν1=20.0)
    network = nhp.StochasticBlockNetworkModel(nnodes, 2, ρ=[[p_in, p_out], [p_out, p_in]] if truth else None, z=z)
    return nhp.DiscreteNetworkHawkesProcess(baseline, impulses, weights, A, network, dt)


def main(steps=20000, max_steps=100, seed=3):
    truth = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(truth)}")
    data = nhp.synthetic.rand(truth, steps, seed=seed)
    print(f"Generated {data.sum()} events in {steps} bins on {int(truth.adjacency_matrix.sum())} links")
    fit = make(seed=seed + 1, truth=False)
    fit.network.variational_init_(seed=2, sharpness=0.3, labels_every=10)
    res = nhp.vb_(fit, data, max_steps=max_steps, keep_trace=False)
    net = fit.network
    labels = np.argmax(net.mv, axis=1)
    print(f"after {res.step} steps: labels {labels} (planted {truth.network.z})")
    same = np.array_equal(labels, truth.network.z) or np.array_equal(1 - labels, truth.network.z)
    print(f"planted partition recovered up to the swap of the labels: {same}; smallest max_k mv {np.max(net.mv, axis=1).min():.3f}")
    right = int(np.sum((fit.weights.ρv > 0.5) == (truth.adjacency_matrix > 0.5)))
    print(f"links classified as in the truth: {right} of {fit.weights.ρv.size}")
    nhp.variational_mean_(fit)
    print("E[ρ] per pair of blocks:")
    print(np.round(net.ρ, 3))
    print(f"E[π] = {np.round(net.π, 3)}")
    print(f"log-likelihood at the variational means {nhp.loglikelihood(fit, data):.1f}; true parameters {nhp.loglikelihood(truth, data):.1f}")
    return fit, truth, labels


if __name__ == "__main__":
    main()
