"""One network VB step (update_ on DiscreteNetworkHawkesProcess + SparseWeightModel, nhp_disc_netvb_run) next to one dense VB
step (nhp_disc_vb_run) on the same dataset at the config-4 scale of BASELINE.json (N = 512, B = 8, L = 32, T = 1e5), in one
process on one device, the two alternated.

    python tools/netvb_discrete.py [--reps 7] [--steps 10] [--bins 100000] [--only netvb|vb] [--commit HASH]

Prints one JSON line.  A step's time is the difference of the wall-clock times of a call of 5·steps steps and a call of
`steps` steps, over 4·steps: both calls end in a device synchronise, and the difference drops the upload and download of the
parameters that each call pays once.  Every repetition times network-short, dense-short, network-long, dense-long in that
order, so both kinds see the same minutes of the machine; the medians over the repetitions, the spread (min, max) of each
kind's per-repetition step time and the paired differences network - dense are printed.  --only netvb (or vb) runs that one
kind for `steps` steps after a warm-up and prints nothing else: the run to put under a kernel trace, where
k_netvb_factors, k_netvb_finish and k_netvb_network show their own times next to k_vb_factors and k_vb_finish.
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--bins", type=int, default=100_000)
    ap.add_argument("--only", default=None, choices=["netvb", "vb"])
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from simulate_discrete import model

    ctx = nhp.default_context()
    N, B, L, T = 512, 8, 32, args.bins
    dense = model(nhp, N, B, L)
    data = nhp.disc_rand(dense, T, seed=3)
    ds = nhp.convolve(dense, nhp.DiscreteDataset(ctx, data), ctx)
    # the spike-and-slab model on the same baseline and impulses: spike Gamma(1, 50·N), slab the dense prior Gamma(1, 1)
    weights = nhp.SparseWeightModel(dense.weights.W.copy(), κ0=1.0, ν0=50.0 * N, κ1=1.0, ν1=1.0)
    net = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(dense.baseline.λ.copy(), 1.0),
                                           nhp.DiscreteGaussianImpulseResponse(np.asfortranarray(np.full((N, N, B), 1.0 / B)), L, 1.0),
                                           weights, np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N), 1.0)

    def netvb(n):
        nhp.update_(net, data, ds, ctx, n_steps=n)

    def vb(n):
        nhp.update_(dense, data, ds, ctx, n_steps=n)

    if args.only:
        run = netvb if args.only == "netvb" else vb
        run(2)
        run(args.steps)
        return

    s = args.steps
    for fn in (netvb, vb):                                     # warm-up: code objects, scratch at its final size
        fn(2)
        fn(s)
    per = {"netvb": [], "vb": []}
    calls = {"netvb": [], "vb": []}
    for _ in range(args.reps):
        a_s, b_s = call_ms(netvb, s), call_ms(vb, s)
        a_l, b_l = call_ms(netvb, 5 * s), call_ms(vb, 5 * s)
        per["netvb"].append((a_l - a_s) / (4 * s))
        per["vb"].append((b_l - b_s) / (4 * s))
        calls["netvb"].append([round(a_s, 3), round(a_l, 3)])
        calls["vb"].append([round(b_s, 3), round(b_l, 3)])
    diffs = [a - b for a, b in zip(per["netvb"], per["vb"])]
    row = {"tool": "netvb_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B, "L": L,
           "T": T, "events": int(data.sum()), "reps": args.reps, "steps": s}
    for k in ("netvb", "vb"):
        row[f"{k}_ms_per_step"] = round(statistics.median(per[k]), 4)
        row[f"{k}_spread_ms"] = [round(min(per[k]), 4), round(max(per[k]), 4)]
        row[f"{k}_call_ms"] = calls[k]
    row["netvb_minus_vb_ms"] = round(statistics.median(diffs), 4)
    row["netvb_minus_vb_spread_ms"] = [round(min(diffs), 4), round(max(diffs), 4)]
    row["links_above_half"] = int(np.sum(net.weights.ρv > 0.5))
    assert np.all(np.isfinite(net.variational_params())) and np.all(np.isfinite(dense.variational_params()))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
