"""Final parameters of a fixed list of discrete variational fits, one .npz per library: the comparison of two builds of
csrc/ (NHP_LIB=<other build> python tools/disc_vb_dump.py other.npz; python tools/disc_vb_dump.py mine.npz; then
python tools/disc_vb_dump.py --compare other.npz mine.npz).  The kernels of these fits have no atomics and fixed summation
orders, so two builds that compute the same thing give np.array_equal on every array.

Fits: {dense, Bernoulli, dense-network, block (K = 3, labels_every 1 and 2)} x {VB 1 and 6 steps, SVI resident, SVI streamed,
SVI resumed (2 steps + 4 with step0)} x shapes (N, T, B, L, Tb) = (3, 50, 2, 4, 16), (5, 700, 3, 7, 128), (130, 300, 2, 3, 112),
the resident routes on a dataset of three trials too, and the dense SVI run at (128, 2560, 2, 4) under both NHP_GEMM_BM."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3, 50, 2, 4, 16), (5, 700, 3, 7, 128), (130, 300, 2, 3, 112)]
PRI = (1.0, 1.0, 0.5, 20.0, 2.0, 1.5, 1.0)                  # α0, β0, κ0, ν0, κ1, ν1, γ
KINDS = ("dense", "bernoulli", "densenet", "block1", "block2")


def six_blocks(nb):
    return np.array([0, nb - 1, min(1, nb - 1), nb // 2, nb - 1, 0], dtype=np.int32)


def counts(N, T, seed):
    return np.random.default_rng(seed).poisson(0.3, (N, T)).astype(np.int64)


def process(nhp, kind, N, B, L):
    rng = np.random.default_rng(N)
    W = rng.uniform(0.05, 0.3, (N, N)) / max(1, N // 4)
    th = rng.dirichlet(np.ones(B), (N, N))
    base = nhp.DiscreteHomogeneousProcess(rng.uniform(0.2, 1.0, N), PRI[0], PRI[1], np.ones(N), np.ones(N), 1.0)
    imp = nhp.DiscreteGaussianImpulseResponse.__new__(nhp.DiscreteGaussianImpulseResponse)
    imp.θ, imp.γ, imp.γv, imp.nlags, imp.dt, imp.ϕ = th, PRI[6], np.ones_like(th), L, 1.0, None
    if kind == "dense":
        return nhp.DiscreteStandardHawkesProcess(base, imp, nhp.DenseWeightModel(W, PRI[4], PRI[5]), 1.0)
    if kind == "bernoulli":
        net = nhp.BernoulliNetworkModel(0.5, N, 1.5, 2.5)
    elif kind == "densenet":
        net = nhp.DenseNetworkModel(N)
    else:
        net = nhp.StochasticBlockNetworkModel(N, 3, α=1.5, β=2.5, γ=1.0)
    return nhp.DiscreteNetworkHawkesProcess(base, imp, nhp.SparseWeightModel(W, *PRI[2:6]), np.ones((N, N)), net, 1.0)


def start(proc, kind, N, B):
    """The same random positive start before every fit."""
    rng = np.random.default_rng(100 + N)
    proc.baseline.αv, proc.baseline.βv = rng.uniform(0.5, 2.0, N), rng.uniform(0.5, 2.0, N)
    proc.impulses.γv = rng.uniform(0.5, 2.0, (N, N, B))
    w = proc.weights
    if kind == "dense":
        w.κv, w.νv = rng.uniform(0.5, 2.0, (N, N)), rng.uniform(1.0, 3.0, (N, N))
        return
    w.κv0, w.νv0 = rng.uniform(0.3, 1.0, (N, N)), rng.uniform(10.0, 30.0, (N, N))
    w.κv1, w.νv1 = rng.uniform(0.5, 2.0, (N, N)), rng.uniform(1.0, 3.0, (N, N))
    w.ρv = rng.uniform(0.1, 0.9, (N, N))
    net = proc.network
    if kind == "bernoulli":
        net.αv, net.βv = 1.7, 2.2
    elif kind.startswith("block"):
        net.variational_init_(seed=5)
        net.labels_every = int(kind[-1])
        net.vb_step = 0


def dump(nhp):
    out = {}

    def keep(tag, proc):
        named = [("av", proc.baseline.αv), ("bv", proc.baseline.βv), ("gv", proc.impulses.γv)]
        named += [(n, getattr(proc.weights, a)) for n, a in (("kv", "κv"), ("nv", "νv"), ("kv0", "κv0"), ("nv0", "νv0"), ("kv1", "κv1"),
                                                            ("nv1", "νv1"), ("rho", "ρv")) if getattr(proc.weights, a, None) is not None]
        net = getattr(proc, "network", None)
        named += [("net_" + n, getattr(net, a)) for n, a in (("m", "mv"), ("av", "αv"), ("bv", "βv"), ("gv", "γv")) if getattr(net, a, None) is not None]
        for name, x in named:
            out[f"{tag}/{name}"] = np.array(x, dtype=np.float64, copy=True)

    for N, T, B, L, Tb in SHAPES:
        data = counts(N, T, 7 * N)
        cuts = [0, T // 3, T // 3 + T // 4, T]
        trials = [data[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        nb = -(-T // Tb)
        kw = dict(batch_bins=Tb, delay=1.0, forgetting=0.6)
        for kind in KINDS:
            proc = process(nhp, kind, N, B, L)
            for what, arg in (("plain", data), ("trials", trials)):
                ds = nhp.convolve(proc, arg)
                tag = f"{kind}/{N}x{T}/{what}"
                for steps in (1, 6):
                    start(proc, kind, N, B)
                    nhp.update_(proc, arg, ds, n_steps=steps)
                    keep(f"{tag}/vb{steps}", proc)
                start(proc, kind, N, B)
                nhp.svi_(proc, ds, nsteps=6, blocks=six_blocks(nb), **kw)
                keep(f"{tag}/svi", proc)
                start(proc, kind, N, B)
                first = nhp.svi_(proc, ds, nsteps=2, seed=3, **kw)
                nhp.svi_(proc, ds, nsteps=4, seed=3, step0=first.step, **kw)
                keep(f"{tag}/svi_resumed", proc)
            start(proc, kind, N, B)
            nhp.svi_(proc, data, nsteps=6, blocks=six_blocks(nb), streamed=True, **kw)
            keep(f"{kind}/{N}x{T}/plain/svi_streamed", proc)
    N, T, B, L, Tb = 128, 2560, 2, 4, 1280                  # whole tiles: the scheduled main loop, at both tile heights
    data = counts(N, T, 11)
    proc = process(nhp, "dense", N, B, L)
    ds = nhp.convolve(proc, data)
    for bm in ("128", "160"):
        os.environ["NHP_GEMM_BM"] = bm
        start(proc, "dense", N, B)
        nhp.svi_(proc, ds, nsteps=6, blocks=six_blocks(2), batch_bins=Tb, delay=1.0, forgetting=0.6)
        keep(f"dense/{N}x{T}/bm{bm}/svi", proc)
    del os.environ["NHP_GEMM_BM"]
    return out


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "the two dumps hold different fits"
    differ = [k for k in A.files if not np.array_equal(A[k], B[k])]
    for k in differ:
        d = np.abs(A[k] - B[k])
        print(f"DIFFERS {k}: max |Δ| {float(d.max()):.3e}, max relative {float((d / np.abs(A[k])).max()):.3e}")
    print(f"arrays compared: {len(A.files)}, bit-equal: {len(A.files) - len(differ)}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4) != (sys.argv[1] == "--compare"):
        sys.exit("usage: disc_vb_dump.py OUT.npz | disc_vb_dump.py --compare A.npz B.npz")
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    import __graft_entry__ as entry
    arrays = dump(entry.load_package())
    assert all(np.all(np.isfinite(v)) for v in arrays.values()), "a fit left a non-finite parameter"
    np.savez(sys.argv[1], **arrays)
    print(f"{len(arrays)} arrays -> {sys.argv[1]}")
