"""Continuous-time network process whose links follow a latent distance model: every node has a position in a latent
plane and a link p → c is the likelier the closer the two nodes are, P[p,c] = 1 / (1 + exp(-(b - ‖z_p - z_c‖²))).  Data
are simulated from two planted clusters of nodes; mcmc! then recovers the link probabilities from the events alone -- the
adjacency matrix, the positions and the offset b are all resampled on the GPU.  Positions are identified only up to
rotation and reflection, so the summary is the posterior mean link-probability matrix."""
from _common import nhp, np


def main(duration=4000.0, nnodes=16, nsteps=300, burn=100, seed=1):
    rng = np.random.default_rng(seed)
    truth = np.repeat([0, 1], nnodes // 2)
    positions = 0.3 * rng.standard_normal((nnodes, 2))
    positions[:, 0] += np.where(truth == 0, -1.5, 1.5)
    planted = nhp.LatentDistanceNetworkModel(nnodes, 2, z=positions, b=1.0)
    P_true = planted.link_probability()
    links = (rng.uniform(size=(nnodes, nnodes)) < P_true).astype(np.float64)
    # few events per impulse time scale (low baselines, fast impulses, a branching ratio of about 0.7), so that who excites
    # whom -- and with it the network -- can be read from the data
    baseline = nhp.HomogeneousProcess(rng.uniform(0.05, 0.1, nnodes))
    weights = nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.7 / max(1.0, links.sum(axis=0).mean())))
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 20.0), 1.0, 1.0, 1.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, links, planted)
    print(f"Process is stable? {nhp.isstable(process)}")
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events on {nnodes} nodes, {int(links.sum())} links")
    # the fit starts from positions near the origin, b = 0 and a full adjacency matrix
    process.network = nhp.LatentDistanceNetworkModel(nnodes, 2, z=0.1 * rng.standard_normal((nnodes, 2)), σ=2.0, σb=2.0)
    process.adjacency_matrix = np.ones((nnodes, nnodes))
    chain = nhp.mcmc_(process, data, nsteps=nsteps, seed=seed, keep_samples=False, moments=True, burn=burn)
    P = chain.link_probability_mean
    same = truth[:, None] == truth[None, :]
    off = ~np.eye(nnodes, dtype=bool)
    print(f"posterior mean link probability  within clusters {P[same & off].mean():.3f}  (truth {P_true[same & off].mean():.3f})")
    print(f"                                 between clusters {P[~same].mean():.3f}  (truth {P_true[~same].mean():.3f})")
    print(f"posterior mean of b {chain.mean[0]:.3f} (truth 1.0), slice steps out of attempts: {chain.exhausted}")
    print(f"links recovered: {np.mean(process.adjacency_matrix == links):.2f} of the entries of A")
    return truth, P_true, P, chain


if __name__ == "__main__":
    main()
