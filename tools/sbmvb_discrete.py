"""One VB step with a stochastic block network (nhp_disc_sbmvb_run) next to one step with a Bernoulli network
(nhp_disc_netvb_run) on the same dataset at the shape §3.19 uses (N = 512, B = 8, L = 32, T = 1e5), K = 8 blocks, in one
process on one device, the kinds alternated.

    python tools/sbmvb_discrete.py [--nodes 512] [--blocks 8] [--reps 7] [--steps 10] [--bins 100000] [--only sbmvb] [--commit HASH]

Prints one JSON line.  A step's time is the difference of the wall-clock times of a call of 5·steps steps and a call of
`steps` steps, over 4·steps (with the default 10: (call of 50 - call of 10) / 40): both calls end in a device synchronise,
and the difference drops the upload and download each call pays once.  Three kinds are timed in every repetition, short
calls first, then long ones: `sbmvb` (the sweep at every step), `nosweep` (the same model with labels_every beyond the run,
so items 1 and 2 of the step alone) and `netvb` (the Bernoulli network).  Printed: the median step of each kind with its
spread, the paired differences sbmvb - netvb (what the block model costs) and sbmvb - nosweep (the sweep by itself).
--only sbmvb runs that kind for `steps` steps after a warm-up and prints nothing: the run to put under a kernel trace,
where k_sbmvb_expect, k_sbmvb_md, k_sbmvb_u, k_sbmvb_tables and k_sbmvb_sweep show their own times.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def call_ms(fn, n):
    t0 = time.perf_counter()
    fn(n)                                                      # ends in a device synchronise (the download of the parameters)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--bins", type=int, default=100_000)
    ap.add_argument("--only", default=None, choices=["sbmvb"])
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from simulate_discrete import model

    ctx = nhp.default_context()
    N, K, B, L, T = args.nodes, args.blocks, 8, 32, args.bins
    dense = model(nhp, N, B, L)
    data = nhp.disc_rand(dense, T, seed=3)
    ds = nhp.convolve(dense, nhp.DiscreteDataset(ctx, data), ctx)

    def process(network):                                      # the spike-and-slab model of tools/netvb_discrete.py
        weights = nhp.SparseWeightModel(dense.weights.W.copy(), κ0=1.0, ν0=50.0 * N, κ1=1.0, ν1=1.0)
        return nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(dense.baseline.λ.copy(), 1.0),
                                                nhp.DiscreteGaussianImpulseResponse(np.asfortranarray(np.full((N, N, B), 1.0 / B)), L, 1.0),
                                                weights, np.ones((N, N)), network, 1.0)

    procs = {"sbmvb": process(nhp.StochasticBlockNetworkModel(N, K).variational_init_(seed=1)),
             "nosweep": process(nhp.StochasticBlockNetworkModel(N, K).variational_init_(seed=1, labels_every=10 ** 6)),
             "netvb": process(nhp.BernoulliNetworkModel(0.5, N))}
    run = {k: (lambda n, p=p: nhp.update_(p, data, ds, ctx, n_steps=n)) for k, p in procs.items()}

    if args.only:
        run[args.only](2)
        run[args.only](args.steps)
        return

    s = args.steps
    for fn in run.values():                                    # warm-up: code objects, scratch at its final size
        fn(2)
        fn(s)
    per = {k: [] for k in run}
    for _ in range(args.reps):
        short = {k: call_ms(fn, s) for k, fn in run.items()}
        long_ = {k: call_ms(fn, 5 * s) for k, fn in run.items()}
        for k in run:
            per[k].append((long_[k] - short[k]) / (4 * s))
    row = {"tool": "sbmvb_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "K": K, "B": B,
           "L": L, "T": T, "events": int(data.sum()), "reps": args.reps, "steps": s}
    for k in run:
        row[f"{k}_ms_per_step"] = round(statistics.median(per[k]), 4)
        row[f"{k}_spread_ms"] = [round(min(per[k]), 4), round(max(per[k]), 4)]
    for name, other in (("sbmvb_minus_netvb_ms", "netvb"), ("sweep_ms", "nosweep")):
        d = [a - b for a, b in zip(per["sbmvb"], per[other])]
        row[name] = round(statistics.median(d), 4)
        row[name.replace("_ms", "_spread_ms")] = [round(min(d), 4), round(max(d), 4)]
    for p in procs.values():
        assert np.all(np.isfinite(p.variational_params()))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
