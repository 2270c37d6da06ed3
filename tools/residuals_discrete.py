"""Goodness of fit for discrete processes on the device (disc_residuals, nhp_disc_residuals) at the project's discrete size:
the config-4 model of tools/simulate_discrete.py (N = 512, B = 8, L = 32) on T = 1e5 bins of its own disc_rand sample,
5.12e7 cells, convolved once outside the timings.

    python tools/residuals_discrete.py [--reps 5] [--bins 100000] [--commit HASH]

Prints one JSON line: the median wall-clock ms after a warm-up of (a) disc_intensity, the call that existed before (the
same GEMM, then T x N doubles to the host); (b) disc_residuals with device outputs for no plane, pit, pit + pearson and all
three planes; for each of (b) the device time of the residual kernel alone (pass_ms), the bytes it moves (16 per cell read,
8 per cell and plane written), its bytes/s, and nhp_probe_stream's bytes/s for a read of the same byte count with the
kernel's fraction of it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, reps):
    fn(0)                                                      # warm-up: code objects, allocator, scratch
    ms, out = [], []
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = fn(r + 1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        out.append(o)
    return round(statistics.median(ms), 3), round(min(ms), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100_000)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib, discrete
    from simulate_discrete import model

    ctx = nhp.default_context()
    N, B, L, T = 512, 8, 32, args.bins
    proc = model(nhp, N, B, L)
    data = nhp.disc_rand(proc, T, seed=3)
    ds = discrete.convolve(proc, data, ctx)
    cells = N * T
    row = {"tool": "residuals_discrete", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "B": B,
           "L": L, "T": T, "cells": cells, "events": int(data.sum()), "reps": args.reps}
    ms, lo, _ = timed(torch, lambda seed: discrete.disc_intensity(proc, convolved=ds, ctx=ctx), args.reps)
    row.update(disc_intensity_ms_median=ms, disc_intensity_ms_min=lo)
    for name, kw in (("aggregates", dict(pit=False)), ("pit", dict(pit=True)), ("pit_pearson", dict(pit=True, pearson=True)),
                     ("all_planes", dict(pit=True, pearson=True, cumulative=True))):
        ms, lo, out = timed(torch, lambda seed: nhp.disc_residuals(proc, convolved=ds, seed=seed, device=True, ctx=ctx, **kw), args.reps)
        pass_ms = statistics.median(o.pass_ms for o in out)
        planes = int(bool(kw.get("pit"))) + int(bool(kw.get("pearson")))          # the scan writes the third plane, not the pass
        nbytes = cells * (16 + 8 * planes)
        us, read = C.c_double(), C.c_int64()
        _lib.check(_lib.lib().nhp_probe_stream(ctx.h, 0, nbytes, 2048, 256, C.byref(us), C.byref(read)), ctx.h)
        probe = read.value / (us.value * 1e-6)
        rate = nbytes / (pass_ms * 1e-3)
        row[name] = {"call_ms_median": ms, "call_ms_min": lo, "pass_ms_median": round(pass_ms, 3), "pass_bytes": nbytes,
                     "pass_bytes_per_s": round(rate), "probe_stream_bytes_per_s": round(probe), "fraction_of_probe": round(rate / probe, 3)}
        del out
    r = nhp.disc_residuals(proc, convolved=ds, seed=1, device=True, ctx=ctx)
    g = nhp.disc_goodness_of_fit(proc, residuals=r)
    row.update(ks_pvalue=round(g.pvalue, 4), histogram_pvalue=round(g.histogram_pvalue, 4), impossible=g.impossible,
               dispersion_mean=round(float(g.dispersion.mean()), 4))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
