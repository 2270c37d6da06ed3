"""Device rand for discrete processes (disc_rand, nhp_disc_simulate) at the config-4 shape -- N = 512, B = 8, L = 32,
T = 1e5, the model of bench.py's c4 leg (λ0 ~ U(0.02, 0.08), W ~ U(0, 1)/N: row sums near 0.5, a stable branching ratio) --
and at a size the host simulator finishes in about a minute, where both routes are timed side by side.

    python tools/simulate_discrete.py [--reps 5] [--host-n 256] [--host-t 250000] [--no-host] [--commit HASH]

Prints one JSON line per size: the median wall-clock ms of a device `disc_rand(..., device=True)` after a warm-up (uploads
of the parameters, scratch allocation, the generator and the output tensor included), its events against the stationary
expectation sum((I - Gᵀ)⁻¹ λ0 dt) T, its generations, and for the shared size the host simulator's seconds (one run).
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


def model(nhp, N, B, L):
    rng = np.random.default_rng(7)
    lam0 = rng.uniform(0.02, 0.08, N)
    W = rng.uniform(0, 1, (N, N)) / N
    imp = nhp.DiscreteGaussianImpulseResponse(np.asfortranarray(np.full((N, N, B), 1.0 / B)), L, 1.0)
    return nhp.DiscreteStandardHawkesProcess(nhp.DiscreteHomogeneousProcess(lam0, 1.0), imp, nhp.DenseWeightModel(np.asfortranarray(W)), 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=256)
    ap.add_argument("--host-t", type=int, default=250_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import discrete

    ctx = nhp.default_context()
    B, L = 8, 32
    for N, T, host in ((512, 100_000, False), (args.host_n, args.host_t, not args.no_host)):
        proc = model(nhp, N, B, L)
        expect = np.linalg.solve(np.eye(N) - proc.weights.W.T, proc.baseline.λ * proc.dt).sum() * T     # Σ_b θ m_b = 1: G = W
        run = lambda seed: discrete._disc_simulate(proc, T, seed, ctx, 50_000_000, False, True)
        run(0)                                                 # warm-up: code objects, allocator
        ms, events, gens = [], [], []
        for r in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, n, g = run(r + 1)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            events.append(n); gens.append(g)
        row = {"tool": "simulate_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B,
               "L": L, "T": T, "reps": args.reps, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
               "events": events[0], "expected": round(float(expect)), "rel_dev": round((events[0] - expect) / expect, 5),
               "generations": gens[0]}
        if host:
            t0 = time.perf_counter()
            data = nhp.rand(proc, T, seed=1)
            row.update(host_s=round(time.perf_counter() - t0, 2), host_events=int(data.sum()))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
