"""Continuous-time network process whose links follow a stochastic block model: nodes belong to latent blocks and a link
p → c exists with the probability ρ[z_p, z_c] of its pair of blocks.  Data are simulated from a planted two-block network
(dense inside a block, sparse between); mcmc! then recovers the blocks and ρ from the events alone -- the adjacency
matrix, the labels, ρ and π are all resampled on the GPU.  Block labels are identified only up to a permutation."""
from _common import nhp, np


def main(duration=4000.0, nnodes=16, rho_in=0.6, rho_out=0.02, nsteps=300, burn=100, seed=1):
    rng = np.random.default_rng(seed)
    truth = np.repeat([0, 1], nnodes // 2)
    planted = nhp.StochasticBlockNetworkModel(nnodes, 2, ρ=[[rho_in, rho_out], [rho_out, rho_in]], z=truth)
    links = (rng.uniform(size=(nnodes, nnodes)) < planted.link_probability()).astype(np.float64)
    # few events per impulse time scale (low baselines, fast impulses, a branching ratio of about 0.7), so that who excites
    # whom -- and with it the network -- can be read from the data
    baseline = nhp.HomogeneousProcess(rng.uniform(0.05, 0.1, nnodes))
    weights = nhp.DenseWeightModel(np.full((nnodes, nnodes), 0.7 / (rho_in * nnodes / 2 + rho_out * nnodes / 2)))
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 20.0), 1.0, 1.0, 1.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, links, planted)
    print(f"Process is stable? {nhp.isstable(process)}")
    data = nhp.synthetic.rand(process, duration, seed=seed)
    print(f"Generated {len(data[0])} events on {nnodes} nodes, {int(links.sum())} links")
    # the fit starts from random labels, a flat ρ and a full adjacency matrix
    process.network = nhp.StochasticBlockNetworkModel(nnodes, 2, z=rng.integers(0, 2, nnodes))
    process.adjacency_matrix = np.ones((nnodes, nnodes))
    chain = nhp.mcmc_(process, data, nsteps=nsteps, seed=seed, keep_samples=False, moments=True, burn=burn)
    blocks = chain.block_counts.argmax(axis=1)
    rho_mean = chain.mean[:4].reshape((2, 2), order="F")
    agree = max(np.mean(blocks == truth), np.mean(blocks == 1 - truth))
    print("planted blocks  ", truth)
    print("recovered blocks", blocks, f"({100 * agree:.0f} % agree up to relabelling)")
    print("posterior mean of ρ:")
    print(rho_mean)
    print(f"links recovered: {np.mean(process.adjacency_matrix == links):.2f} of the entries of A")
    return truth, blocks, rho_mean, chain


if __name__ == "__main__":
    main()
