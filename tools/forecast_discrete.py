"""Device forecast for discrete processes (disc_forecast, nhp_disc_forecast) against the generator it is built from
(disc_rand, nhp_disc_simulate), in one process on one device: the config-4 model of tools/simulate_discrete.py (N = 512,
B = 8, L = 32, branching ratio 0.5), S = 1000 continuations of H = 100 bins from a disc_rand history -- 5.12e7 cells, the
size of a disc_rand of S·H = 1e5 bins.

    python tools/forecast_discrete.py [--reps 5] [--nsamples 1000] [--horizon 100] [--history 200] [--only rand|forecast]
                                      [--commit HASH]

Prints one JSON line: the median wall-clock ms after a warm-up of each of (a) disc_rand(process, S·H, device=True), the
yardstick; (b) disc_forecast with device outputs and no paths; (c) the same forecast with one replica, which is the boundary
state (tables, lagged sums, carry, cell means, the exact mean over H bins) plus an ensemble of N·H cells; their ratio (b)/(a),
the ensemble's share (b) - (c), the events of both and the ensemble's total against S·Σ expected.  --only runs (a) or (b) alone:
the two share kernels by name, so a kernel trace is taken of each in a run of its own.
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


def timed(torch, fn, reps):
    fn(0)                                                      # warm-up: code objects, allocator
    ms, out = [], None
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(r + 1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nsamples", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--history", type=int, default=200)
    ap.add_argument("--only", choices=("rand", "forecast"), default=None)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from simulate_discrete import model

    ctx = nhp.default_context()
    N, B, L, S, H = 512, 8, 32, args.nsamples, args.horizon
    proc = model(nhp, N, B, L)
    data = nhp.disc_rand(proc, args.history, seed=3, device=True)
    row = {"tool": "forecast_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B,
           "L": L, "S": S, "H": H, "history_bins": args.history, "cells": S * H * N, "reps": args.reps}
    if args.only != "forecast":
        sim_ms, sim_min, sim = timed(torch, lambda seed: nhp.disc_rand(proc, S * H, seed=seed, device=True), args.reps)
        row.update(disc_rand_ms_median=sim_ms, disc_rand_ms_min=sim_min, disc_rand_events=int(sim.sum()))
    if args.only != "rand":
        fc_ms, fc_min, f = timed(torch, lambda seed: nhp.disc_forecast(proc, data, H, nsamples=S, seed=seed, device=True), args.reps)
        expected = float(f.expected.sum()) * S
        row.update(disc_forecast_ms_median=fc_ms, disc_forecast_ms_min=fc_min, disc_forecast_events=f.events, generations=f.generations,
                   expected_events=round(expected), rel_dev=round((f.events - expected) / expected, 5))
    if args.only is None:
        one_ms, _, _ = timed(torch, lambda seed: nhp.disc_forecast(proc, data, H, nsamples=1, seed=seed, device=True), args.reps)
        row.update(boundary_and_one_replica_ms_median=one_ms, ensemble_ms=round(fc_ms - one_ms, 3),
                   ratio_forecast_over_rand=round(fc_ms / sim_ms, 3), ratio_ensemble_over_rand=round((fc_ms - one_ms) / sim_ms, 3))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
