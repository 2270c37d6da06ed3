"""Continuous-time network process under a stochastic block network, exponential impulse response: plant two blocks of six
nodes (a link inside a block with probability 0.9, across with 0.05), simulate, then fit the mean-field posterior on the GPU
(vb_) and read the communities (labels()) and the links (link_probability()) off it -- without running a chain.

The block model's variational state has to be created first (network.variational_init_()): mean-field over labels cannot
leave the uniform state.  The start labels alternate, so they say nothing about the planted halves.  The label sweep runs at
every step (labels_every = 1): with this much data (duration 1500, about 15 000 events) the links separate within some twenty
steps and each sweep after that sharpens the labels."""
from _common import nhp, np

SPIKE = (0.3, 100.0)       # Gamma(0.3, 100): mean 0.003 -- what "absent" means to the weights' prior
SLAB = (1.5, 2.0)


def problem(duration=1500.0, nnodes=12, seed=5):
    rng = np.random.default_rng(seed)
    z = (np.arange(nnodes) >= nnodes // 2).astype(np.int32)
    A = (rng.uniform(size=(nnodes, nnodes)) < np.where(z[:, None] == z[None, :], 0.9, 0.05)).astype(np.float64)
    baseline = nhp.HomogeneousProcess(np.full(nnodes, 0.25), 1.0, 1.0)
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 2.0), 1.0, 1.0, 3.0)
    weights = nhp.SparseWeightModel(np.full((nnodes, nnodes), 0.12), *SPIKE, *SLAB)
    network = nhp.StochasticBlockNetworkModel(nnodes, 2)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, A, network)
    data = nhp.synthetic.rand(process, duration, seed=seed)
    network.variational_init_(seed=2, sharpness=0.3, labels_every=1)
    guess = np.concatenate([np.full(nnodes, 0.25), np.full(nnodes * nnodes, 2.0), np.full(nnodes * nnodes, 0.05)])
    return process, data, guess, A, z


def main(duration=1500.0, nnodes=12, seed=5):
    process, data, guess, A, z = problem(duration, nnodes, seed)
    print(f"Process is stable? {nhp.isstable(process)}")
    print(f"Generated {len(data[0])} events; planted labels {z}, {int(A.sum())} links")
    res = nhp.vb_(process, data, guess=guess, f_abstol=1e-6, max_steps=200)
    print(f"{res.steps} updates in {res.elapsed:.3f} s, ELBO {res.trace[0]:.3f} -> {res.elbo:.3f} ({res.status})")
    np.set_printoptions(precision=2, suppress=True, linewidth=160)
    print(f"recovered labels (up to relabelling): {res.labels()}")
    print(f"q(z_n = 0): {res.mv[:, 0]}")
    print(f"block link probabilities E ρ[k, l]:\n{res.block_link_probability()}")
    print(f"link probabilities q(A = 1):\n{res.link_probability()}")
    found = process.adjacency_matrix
    print(f"links found (ρv > 1/2): {int(found.sum())}, of which present {int((found * A).sum())}; present links missed: {int(((1 - found) * A).sum())}")
    return z, A, res


if __name__ == "__main__":
    main()
