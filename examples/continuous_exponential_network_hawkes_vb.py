"""Continuous-time network process, exponential impulse response: simulate a 4-node network with half of its links absent,
then fit the mean-field posterior with spike-and-slab weights on the GPU (vb_) and read the link probabilities q(A = 1) off
it -- "which links are there" without running a chain.

A link can only be told from its absence by the children it produced.  "Enough" below is the expected number of children
of a present link under the truth, cnt[parent]·W[parent, child]: with this seed (duration 2000, about 6900 events) each of the
8 present links has more than 300 of them and gets ρv > 0.98, and every absent link gets ρv < 0.1."""
from _common import nhp, np

SPIKE = (0.3, 30.0)        # Gamma(0.3, 30): mean 0.01 -- what "absent" means to the weights' prior
SLAB = (1.5, 2.0)


def problem(duration=2000.0, nnodes=4, seed=3):
    rng = np.random.default_rng(seed)
    A = np.zeros(nnodes * nnodes)
    A[rng.permutation(nnodes * nnodes)[:nnodes * nnodes // 2]] = 1.0
    A = A.reshape((nnodes, nnodes))
    W = rng.uniform(0.15, 0.35, (nnodes, nnodes))
    baseline = nhp.HomogeneousProcess(rng.uniform(0.3, 0.6, nnodes), 1.0, 1.0)
    impulses = nhp.ExponentialImpulseResponse(rng.uniform(1.0, 3.0, (nnodes, nnodes)), 1.0, 1.0, 5.0)
    weights = nhp.SparseWeightModel(W, *SPIKE, *SLAB)
    network = nhp.BernoulliNetworkModel(0.5, nnodes, 1.0, 1.0)
    process = nhp.ContinuousNetworkHawkesProcess(baseline, impulses, weights, A, network)
    data = nhp.synthetic.rand(process, duration, seed=seed)
    guess = rng.uniform(0.2, 0.8, nnodes + 2 * nnodes * nnodes)
    cnt = np.bincount(np.asarray(data[1]) - 1, minlength=nnodes).astype(float)
    return process, data, guess, A, cnt[:, None] * W * A


def main(duration=2000.0, nnodes=4, seed=3):
    process, data, guess, A, expected = problem(duration, nnodes, seed)
    print(f"Process is stable? {nhp.isstable(process)}")
    print(f"Generated {len(data[0])} events; true adjacency matrix [parent, child]:\n{A}")
    res = nhp.vb_(process, data, guess=guess, f_abstol=1e-5, max_steps=2000)
    print(f"{res.steps} updates in {res.elapsed:.3f} s, ELBO {res.trace[0]:.3f} -> {res.elbo:.3f} ({res.status})")
    np.set_printoptions(precision=3, suppress=True)
    print(f"link probabilities q(A = 1):\n{res.link_probability()}")
    print(f"expected children of the present links under the truth:\n{expected}")
    print(f"effective weight means (1 - ρv) κv0/νv0 + ρv κv1/νv1:\n{res.effective_weight_mean()}")
    print(f"network: q(ρ) = Beta({res.net_alpha:.2f}, {res.net_beta:.2f}), mean {process.network.ρ:.3f}")
    found = process.adjacency_matrix
    print(f"links found (ρv > 1/2): {int(found.sum())}, of which present {int((found * A).sum())}; present links missed: {int(((1 - found) * A).sum())}")
    return A, res, expected


if __name__ == "__main__":
    main()
