"""Continuous-time network process under a latent distance network, exponential impulse response: plant three groups of four
nodes at the corners of a triangle in the plane (a link inside a group with probability about 0.8, across about 0.03),
simulate, then fit on the GPU (vb_) and read the links (link_probability()), the network's own link probabilities
(network_link_probability()) and the fitted positions (positions(), offset()) off the result -- without running a chain.

The network's factor is a point estimate (zv, bv) that each step moves by a few iterations of a monotone ascent (variational
EM), so the ELBO never falls.  The state has to be created first (network.variational_init_()): with all positions equal the
ascent is at a saddle.  The start is 0.1·N(0, I) around the origin and says nothing about the planted groups.  Positions are
identified only up to rotation, reflection and translation by the prior's pull, so compare link probabilities, not positions."""
from _common import nhp, np

SPIKE = (0.3, 100.0)       # Gamma(0.3, 100): mean 0.003 -- what "absent" means to the weights' prior
SLAB = (1.5, 2.0)


def problem(duration=1500.0, nnodes=12, seed=7):
    rng = np.random.default_rng(seed)
    corners = 2.2 * np.array([[0.0, 0.0], [1.0, 0.0], [0.5, np.sqrt(0.75)]])
    planted = nhp.LatentDistanceNetworkModel(nnodes, 2, z=corners[np.arange(nnodes) % 3] + 0.25 * rng.standard_normal((nnodes, 2)), b=1.5)
    P = planted.link_probability()
    A = (rng.uniform(size=(nnodes, nnodes)) < P).astype(np.float64)
    baseline = nhp.HomogeneousProcess(np.full(nnodes, 0.25), 1.0, 1.0)
    impulses = nhp.ExponentialImpulseResponse(np.full((nnodes, nnodes), 2.0), 1.0, 1.0, 3.0)
    weights = nhp.SparseWeightModel(np.full((nnodes, nnodes), 0.12), *SPIKE, *SLAB)
    network = nhp.LatentDistanceNetworkModel(nnodes, 2, σ=1.5, μb=0.0, σb=2.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, A, network)
    data = nhp.synthetic.rand(process, duration, seed=seed)
    network.variational_init_(seed=0, scale=0.1, ascent_steps=4)
    guess = np.concatenate([np.full(nnodes, 0.25), np.full(nnodes * nnodes, 2.0), np.full(nnodes * nnodes, 0.05)])
    return process, data, guess, A, P


def main(duration=1500.0, nnodes=12, seed=7):
    process, data, guess, A, P = problem(duration, nnodes, seed)
    print(f"Process is stable? {nhp.isstable(process)}")
    print(f"Generated {len(data[0])} events; {int(A.sum())} planted links")
    res = nhp.vb_(process, data, guess=guess, f_abstol=1e-6, max_steps=200)
    print(f"{res.steps} updates in {res.elapsed:.3f} s, ELBO {res.trace[0]:.3f} -> {res.elbo:.3f} ({res.status})")
    np.set_printoptions(precision=2, suppress=True, linewidth=160)
    rho, net_p = res.link_probability(), res.network_link_probability()
    print(f"fitted offset {res.offset():.3f}, positions:\n{res.positions()}")
    print(f"link probabilities q(A = 1):\n{rho}")
    print(f"mean q(A = 1) on the planted links {rho[A == 1.0].mean():.3f}, on the absent ones {rho[A == 0.0].mean():.3f}")
    print(f"correlation of the network's link probabilities with the planted ones: {np.corrcoef(net_p.ravel(), P.ravel())[0, 1]:.3f}")
    found = process.adjacency_matrix
    print(f"links found (ρv > 1/2): {int(found.sum())}, of which present {int((found * A).sum())}; present links missed: {int(((1 - found) * A).sum())}")
    return A, P, res


if __name__ == "__main__":
    main()
