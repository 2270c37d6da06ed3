"""Stochastic variational inference for discrete processes (svi_, nhp_disc_svi_run) at the config-4 scale of BASELINE.json
(N = 512, B = 8, L = 32, T = 1e5) next to the full mean-field step it is built from (update_, nhp_disc_vb_run), in one
process on one device.

    python tools/svi_discrete.py [--reps 5] [--steps 50] [--bins 100000] [--batches 1024,4096,16384] [--only MODE:TB] [--commit HASH]

Prints one JSON line.  Per batch size Tb and mode (streamed: every step convolves its block; resident: the T x N x B
convolution stays on the device) the time of one step in ms: the difference of the median wall-clock times of a call of
5·steps steps and a call of `steps` steps, over 4·steps -- both calls end in a device synchronise, and the difference drops
the upload and download of the 2N + 2N² + N²B parameters that each call pays once.  With the default 50 the difference is
200 steps of device work (0.1 s and more) next to calls whose fixed part is a few tens of ms; both call times are printed,
so a reader sees how large the difference is against them.  The same for one VB step (a quarter of the steps).  The
streamed runs come first, before anything has convolved the dataset: the device memory in use after each of them (from
hipMemGetInfo, less what was in use before the dataset was made) is the streamed peak, printed against the 8·T·N·B bytes of
the resident convolution.  streaming_adds_<Tb>_ms comes from a pass of its own at the end: long calls, streamed and
resident in turn, the median (and the spread) of the paired differences per step.  gate_resident_4096_below_vb is the one condition the feature has to meet.
--only resident:4096 (or streamed:4096, or vb:0) runs that one configuration for `steps` steps after a warm-up and prints
nothing else: the run to put under a kernel trace, whose kernels share their names with the others.
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


def median_ms(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                   # ends in a device synchronise (the download of the parameters)
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def per_step(fn, steps, reps):
    fn(steps)                                                  # warm-up: code objects, scratch
    short, long_ = median_ms(lambda: fn(steps), reps), median_ms(lambda: fn(5 * steps), reps)
    return round((long_ - short) / (4 * steps), 4), round(short, 3), round(long_, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bins", type=int, default=100_000)
    ap.add_argument("--batches", default="1024,4096,16384")
    ap.add_argument("--only", default=None)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from simulate_discrete import model

    ctx = nhp.default_context()
    N, B, L, T = 512, 8, 32, args.bins
    batches = [int(x) for x in args.batches.split(",")]
    proc = model(nhp, N, B, L)
    data = nhp.disc_rand(proc, T, seed=3)
    free0, total = torch.cuda.mem_get_info(ctx.device)
    ds = nhp.DiscreteDataset(ctx, data)

    def svi(n, Tb, streamed):
        nhp.svi_(proc, ds, nsteps=n, batch_bins=Tb, delay=10.0, forgetting=0.6, seed=1, streamed=streamed)

    def vb(n):
        nhp.update_(proc, data, ds, ctx, n_steps=n)

    if args.only:
        mode, tb = args.only.split(":")
        if mode != "streamed":
            nhp.convolve(proc, ds, ctx)
        run = vb if mode == "vb" else (lambda n: svi(n, int(tb), mode == "streamed"))
        run(2)
        run(args.steps)
        return

    row = {"tool": "svi_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B, "L": L,
           "T": T, "events": int(data.sum()), "reps": args.reps, "steps": args.steps, "conv_bytes": 8 * T * N * B}
    for Tb in batches:                                         # ascending: the context's scratch only grows
        ms, short, long_ = per_step(lambda n: svi(n, Tb, True), args.steps, args.reps)
        free, _ = torch.cuda.mem_get_info(ctx.device)
        row[f"streamed_{Tb}_ms_per_step"] = ms
        row[f"streamed_{Tb}_call_ms"] = [short, long_]
        row[f"streamed_{Tb}_device_bytes"] = int(free0 - free)
    assert ds.B == 0                                           # still no resident convolution
    nhp.convolve(proc, ds, ctx)
    for Tb in batches:
        ms, short, long_ = per_step(lambda n: svi(n, Tb, False), args.steps, args.reps)
        row[f"resident_{Tb}_ms_per_step"] = ms
        row[f"resident_{Tb}_call_ms"] = [short, long_]
    vsteps = max(2, args.steps // 4)
    ms, short, long_ = per_step(vb, vsteps, args.reps)
    row.update(vb_ms_per_step=ms, vb_call_ms=[short, long_], vb_steps=vsteps)
    free, _ = torch.cuda.mem_get_info(ctx.device)
    row["resident_device_bytes"] = int(free0 - free)
    for Tb in batches:
        # what streaming adds: calls of 5·steps steps, streamed and resident in turn on the same (convolved) dataset -- the
        # fixed part of a call is the same in both -- and the median of the paired differences
        n, diffs = 5 * args.steps, []
        for _ in range(args.reps):
            a = median_ms(lambda: svi(n, Tb, True), 1)
            b = median_ms(lambda: svi(n, Tb, False), 1)
            diffs.append((a - b) / n)
        row[f"streaming_adds_{Tb}_ms"] = round(statistics.median(diffs), 4)
        row[f"streaming_adds_{Tb}_spread_ms"] = [round(min(diffs), 4), round(max(diffs), 4)]
    if 4096 in batches:
        row["gate_resident_4096_below_vb"] = bool(row["resident_4096_ms_per_step"] < ms)
    assert np.all(np.isfinite(proc.variational_params()))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
