"""Discrete-time network process with spike-and-slab weights: simulate with a sparse adjacency matrix on the GPU
(disc_rand), fit the mean-field posterior with vb_ -- q(A[p,c] = 1) = ρv[p,c], a Gamma for the weight of an absent link
(the spike, small mean) and one for a present link (the slab) -- and print ρv against the true A.  variational_mean_ then
sets the process to the posterior means, so the log-likelihood of the fit can be compared with the truth's."""
from _common import nhp, np


def make(nnodes=4, nbasis=3, nlags=8, dt=1.0, seed=0, truth=True):
    rng = np.random.default_rng(seed)
    baseline = nhp.DiscreteHomogeneousProcess(rng.uniform(0.05, 0.15, nnodes), dt)
    impulses = nhp.DiscreteGaussianImpulseResponse(np.ones((nnodes, nnodes, nbasis)) / nbasis, nlags, dt)
    A = (rng.uniform(size=(nnodes, nnodes)) < 0.5).astype(np.float64) if truth else np.ones((nnodes, nnodes))
    W = rng.uniform(0.1, 0.3, (nnodes, nnodes))
    # spike Gamma(1, 50): mean 0.02;  slab Gamma(2, 4): mean 0.5
    weights = nhp.SparseWeightModel(W, κ0=1.0, ν0=50.0, κ1=2.0, ν1=4.0)
    return nhp.DiscreteNetworkHawkesProcess(baseline, impulses, weights, A, nhp.BernoulliNetworkModel(0.5, nnodes), dt)


def main(steps=20000, max_steps=30, seed=2):
    truth = make(seed=seed)
    print(f"Process is stable? {nhp.isstable(truth)}")
    data = nhp.disc_rand(truth, steps, seed=seed)
    print(f"Generated {data.sum()} events in {steps} bins on {int(truth.adjacency_matrix.sum())} links")
    fit = make(seed=seed + 1, truth=False)
    res = nhp.vb_(fit, data, max_steps=max_steps, keep_trace=False)
    rho = fit.weights.ρv
    print(f"after {res.step} steps: ρv | A")
    print(np.column_stack([np.round(rho, 3), truth.adjacency_matrix]))
    right = int(np.sum((rho > 0.5) == (truth.adjacency_matrix > 0.5)))
    print(f"links classified as in the truth: {right} of {rho.size}")
    net = fit.network
    print(f"network: αv = {net.αv:.3f}, βv = {net.βv:.3f}, E[ρ] = {net.αv / (net.αv + net.βv):.3f} (true share {truth.adjacency_matrix.mean():.3f})")
    nhp.variational_mean_(fit)
    print(f"log-likelihood at the variational means {nhp.loglikelihood(fit, data):.1f}; true parameters {nhp.loglikelihood(truth, data):.1f}")
    return fit, truth, rho


if __name__ == "__main__":
    main()
