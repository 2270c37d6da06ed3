"""Cold-call cost of a continuous log-likelihood on fresh data (the reference's one-shot `loglikelihood(process, data)`):
building the dataset, and the first evaluation on it, for three routes -- the host pre-pass, the device pre-pass from
host arrays (build="device") and the device pre-pass from torch tensors already on the GPU.

    python tools/coldcall.py [--n 1024] [--m 1000000] [--reps 5] [--commit HASH]

Prints one JSON line: wall-clock ms, the median over `reps` fresh datasets per route and evaluation kind (windowed and
recursive; the context, the model and the tensors exist beforehand; one unmeasured warm-up per route first).  The
build medians pool both kinds' datasets.  NHP_TIMING=1 adds the per-phase laps of every
build on stderr.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--m", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib
    from nhp_amd.continuous import DeviceDataset

    N, M = args.n, args.m
    ctx = _lib.default_context()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M)
    proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
    model = proc.device_model(ctx)
    dev = torch.device("cuda", ctx.device)
    tev, tnd = torch.from_numpy(times).to(dev), torch.from_numpy(nodes).to(dev)
    torch.cuda.synchronize(dev)
    dt_max = float(proc.impulses.Δtmax)

    def build(route):
        if route == "host":
            return DeviceDataset(ctx, (times, nodes, T), N, dt_max)
        if route == "device":
            return DeviceDataset(ctx, (times, nodes, T), N, dt_max, build="device")
        return DeviceDataset(ctx, (tev, tnd, T), N, dt_max)

    def cold(route, recursive):
        t0 = time.perf_counter()
        ds = build(route)
        t1 = time.perf_counter()
        ll = nhp.loglikelihood(proc, ds, recursive=recursive, ctx=ctx, model=model)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, ll

    # windowed: the Δtmax-window sum (recursive=False); recursive: the reference's default call for exponential impulses,
    # whose first evaluation also makes the recursion's data layouts (crowding statistics on the host, parts on the device)
    out = {"tool": "coldcall", "commit": args.commit, "N": N, "M": M, "reps": args.reps}
    for tag, recursive in (("windowed", False), ("recursive", True)):
        lls = set()
        for route in ("host", "device", "tensor"):
            cold(route, recursive)                                        # warm-up (first allocations, code objects)
            runs = [cold(route, recursive) for _ in range(args.reps)]
            out[f"{route}_build_ms"] = out.get(f"{route}_build_ms", []) + [r[0] for r in runs]
            out[f"{tag}_{route}_first_ll_ms"] = round(float(np.median([r[1] for r in runs])), 3)
            out[f"{tag}_{route}_cold_ms"] = round(float(np.median([r[0] + r[1] for r in runs])), 3)
            lls |= {r[2] for r in runs}
        out[f"{tag}_same_loglik"] = len(lls) == 1
    for route in ("host", "device", "tensor"):
        out[f"{route}_build_ms"] = round(float(np.median(out[f"{route}_build_ms"])), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
