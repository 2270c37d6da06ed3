"""nhp_cont_map_parents and nhp_cont_cascades at a chosen size, beside the parent sampler on the same dataset.

    python tools/cascades.py [--n 1024] [--events 1000000] [--kbar 8] [--reps 20] [--commit HASH] [--sampler-only]

Prints one JSON line per impulse kind with hipEvent times (ms, median and minimum over --reps, after one warm-up call each)
on the context's stream of
  map_parents       nhp_cont_map_parents, all three outputs into device buffers
  resample_parents  nhp_cont_resample_parents without host outputs (the sampler's kernel alone: one Philox draw per event)
  cascades_map      nhp_cont_cascades on the MAP parents (device in, device out, every output), with its rounds
  cascades_sample   the same on one sampled parent vector
  cascades_chain    the same on a chain of M events (the worst depth: ⌈log2 M⌉ rounds)
--sampler-only times resample_parents alone: with NHP_LIB pointing at another build of the library (one without the new
entry points, say) it gives that build's sampler time in the same visit.
`python tools/cascades.py --reps 3 ...` under `rocprofv3 --kernel-trace --stats` gives the time per kernel (k_map8, k_casc_*).
"""
import argparse
import ctypes as C
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
    ap.add_argument("--sampler-only", action="store_true")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib

    N, M = args.n, args.events
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    dev = torch.device("cuda", ctx.device)
    for kind in ("exponential", "logit-normal"):
        proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
        ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
        model = proc.device_model(ctx)
        out = {"tool": "cascades", "commit": args.commit, "lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(ctx.device),
               "N": N, "M": M, "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "reps": args.reps}

        def sampler():
            _lib.check(lib.nhp_cont_resample_parents(ctx.h, ds.h, model.h, None, 1, 0, None, None, None), ctx.h)

        out["resample_parents_ms"], out["resample_parents_ms_min"] = timed(ctx, sampler, args.reps)
        if args.sampler_only:
            print(json.dumps(out), flush=True)
            continue

        par, pno = (torch.empty(M, dtype=torch.int64, device=dev) for _ in range(2))
        prob = torch.empty(M, dtype=torch.float64, device=dev)
        lens = (M, M, M, M, M, M, M, N, N, N * N)
        outs = [torch.empty(n, dtype=torch.float64 if k == 6 else torch.int64, device=dev) for k, n in enumerate(lens)]
        ptrs = [o.data_ptr() for o in outs]
        torch.cuda.synchronize()
        ncasc, rounds = C.c_int64(), C.c_int32()

        def map_parents():
            _lib.check(lib.nhp_cont_map_parents(ctx.h, ds.h, model.h, 1, par.data_ptr(), pno.data_ptr(), prob.data_ptr()), ctx.h)

        def cascades_of(vec):
            def call():
                _lib.check(lib.nhp_cont_cascades(ctx.h, ds.h, vec.data_ptr(), 1, 1, *ptrs[:7], C.byref(ncasc), *ptrs[7:],
                                                 C.byref(rounds)), ctx.h)
            return call

        out["map_parents_ms"], out["map_parents_ms_min"] = timed(ctx, map_parents, args.reps)
        out["map_baseline_share"] = float((par == 0).double().mean())
        out["map_mean_prob"] = float(prob.mean())
        drawn = torch.as_tensor(nhp.resample_parents(proc, ds, seed=1, ctx=ctx)[0]).to(dev)
        chain = torch.arange(M, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for name, vec in (("map", par), ("sample", drawn), ("chain", chain)):
            out[f"cascades_{name}_ms"], out[f"cascades_{name}_ms_min"] = timed(ctx, cascades_of(vec), args.reps)
            out[f"cascades_{name}_rounds"] = rounds.value
            out[f"cascades_{name}_count"] = ncasc.value
            out[f"cascades_{name}_depth"] = int(outs[1].max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
