"""Device rand(process, duration) at the metric size: N = 1024 s_metric_process models (exponential and logit-normal,
standard and network), the baseline scaled so that about `--events` events are expected.

    python tools/simulate.py [--n 1024] [--events 1000000] [--reps 5] [--commit HASH]

Prints one JSON line per model: the median wall-clock ms of a device `rand` until its synchronisation returns (the model
is resident beforehand, so this is DeviceModel.simulate: the generator, the sort and the output tensors), the event count
against the stationary expectation sum((I - (W∘A)ᵀ)⁻¹ λ0) T, and the number of generations (from the parents of one
more draw).
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


def generations(par):
    """Depth of the deepest event + 1 (parents precede their children in the returned order)."""
    depth = np.zeros(len(par), np.int64)
    kid = np.flatnonzero(par > 0)
    while True:
        new = depth.copy()
        new[kid] = depth[par[kid] - 1] + 1
        if np.array_equal(new, depth):
            return int(depth.max()) + 1 if len(par) else 0
        depth = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()

    N, T = args.n, 125_000.0
    ctx = nhp.default_context()
    for kind in ("exponential", "logit-normal"):
        for network in (False, True):
            proc = nhp.synthetic.s_metric_process(N, args.events, T, kind, network=network)
            V = proc.weights.W * (proc.adjacency_matrix if network else 1.0)
            lam0 = np.asarray(proc.baseline.λ)
            expect = np.linalg.solve(np.eye(N) - V.T, lam0).sum() * T
            proc.baseline.λ = lam0 * (args.events / expect)
            expect = args.events
            m = proc.device_model(ctx)
            m.simulate(T, seed=0)                              # warm-up: code objects, allocator
            ms, counts = [], []
            for r in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t, n, _ = m.simulate(T, seed=r + 1)
                ms.append((time.perf_counter() - t0) * 1e3)
                counts.append(len(t))
            _, _, _, par = m.simulate(T, seed=1, return_parents=True)
            print(json.dumps({"tool": "simulate", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device),
                              "N": N, "impulse": kind, "network": network, "T": T, "reps": args.reps,
                              "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                              "events": counts[0], "expected": round(float(expect)),
                              "rel_dev": round((counts[0] - expect) / expect, 5),
                              "generations": generations(par.cpu().numpy())}), flush=True)


if __name__ == "__main__":
    main()
