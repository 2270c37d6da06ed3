"""One iteration of the continuous variational fit at a chosen size, beside the EM iteration it is built on.

    python tools/vb_continuous.py [--n 1024] [--events 1000000] [--kbar 8] [--reps 20] [--commit HASH]

Prints one JSON line per impulse kind with hipEvent times (ms; median, minimum and maximum over --reps, after one warm-up call
each) on the context's stream of
  vb_iteration   one iteration inside nhp_cont_vb_run (E-step at the surrogate, k_vb_elbo, k_vb_update, the host's look at six
                 scalars): the difference of a 25-step and a 5-step run over 20, so the start's upload and the result's
                 downloads cancel
  em_iteration   one iteration inside nhp_cont_em_run with the same priors (regularize=True), by the same difference
  vb_step        one nhp_cont_vb_step on device-resident planes (k_vb_surrogate, the E-step, k_vb_update, two k_vb_elbo and the
                 readback of its scalars)
The windowed objective (recursive=False), parameters of synthetic.s_metric_process, the package's default priors (every
hyper-parameter 1).  The O(P) passes alone (k_vb_update against k_em_mstep) are kernel times: run this script under
`rocprofv3 --kernel-trace --stats -- python tools/vb_continuous.py ...`; tools/em.py times em_ and mle_ without anything of
this file, for the comparison with an earlier tree.
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
    return ms


def summary(ms):
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def per_step(ctx, run, reps, short=5, long=25):
    a, b = timed(ctx, lambda: run(short), reps), timed(ctx, lambda: run(long), reps)
    return summary([(y - x) / (long - short) for x, y in zip(a, b)])


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
    from nhp_amd import _lib, inference

    N, M = args.n, args.events
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    for kind in ("exponential", "logit-normal"):
        proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
        ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
        model = proc.device_model(ctx)
        priors = inference._priors(proc)
        x0 = np.clip(proc.params(), 1e-6, 10.0)
        P = len(x0)
        S, R = np.empty(P), np.empty(P)
        val, steps, conv = C.c_double(), C.c_int32(), C.c_int32()
        dev = torch.device("cuda", ctx.device)
        dS, dR = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
        stats = np.empty(9)
        torch.cuda.synchronize()

        def vb_run(k):
            x = x0.copy()
            _lib.check(lib.nhp_cont_vb_run(ctx.h, ds.h, model.h, 0, C.byref(priors), 0.0, k, _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P,
                                           C.byref(val), C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k

        def em_run(k):
            x = x0.copy()
            _lib.check(lib.nhp_cont_em_run(ctx.h, ds.h, model.h, 0, C.byref(priors), 1e-6, 10.0, 0.0, k, _lib.dptr(x), P, C.byref(val),
                                           C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k

        def vb_step(flags=0):
            _lib.check(lib.nhp_cont_vb_step(ctx.h, ds.h, model.h, flags, C.byref(priors), dS.data_ptr(), dR.data_ptr(), P, 1, _lib.dptr(stats)),
                       ctx.h)

        out = {"tool": "vb_continuous", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M,
               "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "P": P, "reps": args.reps, "columns": "median, min, max"}
        out["vb_iteration_ms"] = per_step(ctx, vb_run, args.reps)
        model.set_params(x0)
        out["em_iteration_ms"] = per_step(ctx, em_run, args.reps)
        model.set_params(x0)
        vb_step(inference.NHP_VB_FROM_MODEL)               # a state to step from
        out["vb_step_ms"] = summary(timed(ctx, vb_step, args.reps))
        out["elbo"] = float(stats[0] - stats[1] - stats[2] - stats[3] - stats[4])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
