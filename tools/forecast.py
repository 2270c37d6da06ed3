"""Device forecast(process, data, horizon) at the metric size: N = 1024 s_metric_process models (exponential and
logit-normal, standard and network), a history of about `--events` events drawn from the model itself on the device, and
`--nsamples` continuations over a horizon that holds about `--per-replica` events each.

    python tools/forecast.py [--n 1024] [--events 1000000] [--nsamples 1000] [--per-replica 1000] [--reps 5] [--commit HASH]

Prints one JSON line per model: the median wall-clock ms of the one-off boundary state (prefix table, the exponential
state G of at most M·N exponentials, carry masses) and of the ensemble (roots, generations, counts, the two sorts, the
output tensors), both as nhp_cont_forecast reports them, the whole call as the caller sees it, the mean events per
replica, the expected carry-over per replica, and the exponentials of the state build: evaluated (terms below e^-708
are exactly zero and skipped) and the M·N bound.  Dataset and model are resident
beforehand.
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


def state_exponentials(t, n, T, theta, V):
    """The exponentials k_fc_state evaluates: per link with weight, the parent node's events with θ·(T - t) <= 708."""
    total = 0
    for p in range(len(V)):
        age = np.sort(T - t[n == p + 1])
        total += int(np.searchsorted(age, 708.0 / theta[p], side="right")[V[p] > 0].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--nsamples", type=int, default=1000)
    ap.add_argument("--per-replica", type=float, default=1000.0)
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
            m = proc.device_model(ctx)
            t, n, _ = m.simulate(T, seed=0)
            ds = nhp.device_dataset(proc, (t, n, T), ctx)
            h = args.per_replica * T / len(t)
            kw = dict(nsamples=args.nsamples, return_paths=True, device=True, ctx=ctx, model=m)
            nhp.forecast(proc, ds, h, seed=0, **kw)            # warm-up: code objects, allocator
            state, ens, wall = [], [], []
            for r in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = nhp.forecast(proc, ds, h, seed=r + 1, **kw)
                wall.append((time.perf_counter() - t0) * 1e3)
                state.append(f.phase_ms[0]); ens.append(f.phase_ms[1])
            print(json.dumps({"tool": "forecast", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device),
                              "N": N, "impulse": kind, "network": network, "history_events": len(t), "T": T,
                              "horizon": round(h, 3), "nsamples": args.nsamples, "reps": args.reps,
                              "state_ms_median": round(statistics.median(state), 3), "ensemble_ms_median": round(statistics.median(ens), 3),
                              "call_ms_median": round(statistics.median(wall), 3), "call_ms_min": round(min(wall), 3),
                              "events_per_replica": round(float(f.counts.sum()) / args.nsamples, 2),
                              "carry_per_replica": round(float(f.carry.sum()), 3),
                              "state_exponentials": state_exponentials(t.cpu().numpy(), n.cpu().numpy(), T, proc.impulses.θ, V)
                              if kind == "exponential" else 0,
                              "state_exponentials_at_most": len(t) * N if kind == "exponential" else 0}), flush=True)


if __name__ == "__main__":
    main()
