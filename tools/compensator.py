"""nhp_cont_compensator at a chosen size, beside two calls of the same orders of work on the same dataset.

    python tools/compensator.py [--n 1024] [--events 1000000] [--kbar 8] [--reps 20] [--commit HASH]

Prints one JSON line per impulse kind with hipEvent times (ms, median and minimum over --reps, after one warm-up call each)
on the context's stream of
  compensator      nhp_cont_compensator, all three outputs into device buffers
  event_intensity  nhp_cont_event_intensity (the same window pairs, a pdf in place of a CDF); its 8·M-byte download to
                   the host is part of the call and of the time
  recursive        the O(M·N) recursive log-likelihood (exponential impulses only), never its truncated window
`python tools/compensator.py ...` under `rocprofv3 --kernel-trace --stats` gives the kernels' shares (k_comp_*).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, call, reps):
    call()                                                 # warm-up: code objects, scratch, lazily built layouts
    ms = []
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_start()
        call()
        ms.append(ctx.timer_stop())
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--kbar", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib

    N, M = args.n, args.events
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    for kind in ("exponential", "logit-normal"):
        proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
        ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
        model = proc.device_model(ctx)
        dev = torch.device("cuda", ctx.device)
        at, res = (torch.empty(M, dtype=torch.float64, device=dev) for _ in range(2))
        tot = torch.empty(N, dtype=torch.float64, device=dev)
        lam = np.empty(M)
        torch.cuda.synchronize()

        def comp():
            _lib.check(lib.nhp_cont_compensator(ctx.h, ds.h, model.h, 1, at.data_ptr(), res.data_ptr(), tot.data_ptr()), ctx.h)

        def event_intensity():
            _lib.check(lib.nhp_cont_event_intensity(ctx.h, ds.h, model.h, _lib.dptr(lam)), ctx.h)

        def recursive():
            _lib.check(lib.nhp_cont_loglik_enqueue(ctx.h, ds.h, model.h, _lib.LL_RECURSIVE | _lib.LL_FULL_RECURSION, 0), ctx.h)

        out = {"tool": "compensator", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M,
               "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "reps": args.reps}
        out["compensator_ms"], out["compensator_ms_min"] = timed(ctx, comp, args.reps)
        out["event_intensity_ms"], out["event_intensity_ms_min"] = timed(ctx, event_intensity, args.reps)
        if kind == "exponential":
            out["recursive_ms"], out["recursive_ms_min"] = timed(ctx, recursive, args.reps)
        out["total_sum"] = float(tot.sum())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
