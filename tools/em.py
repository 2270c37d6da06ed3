"""One EM iteration at a chosen size, beside the calls it is built from and competes with.

    python tools/em.py [--n 1024] [--events 1000000] [--kbar 8] [--reps 20] [--commit HASH] [--baseline-only]

Prints one JSON line per impulse kind with hipEvent times (ms, median and minimum over --reps, after one warm-up call each)
on the context's stream of
  em_iteration   one iteration inside nhp_cont_em_run (E-step, objective, M-step, the host's look at one scalar): the
                 difference of a 25-step and a 5-step run over 20, so the start's upload and the result's download cancel
  em_stats       nhp_cont_em_stats into device buffers (the E-step, the O(P) pass and the log-likelihood's readback)
  loglik_grad    one nhp_cont_loglik_grad call (its 8·P-byte download to the host is part of the call and of the time)
  mle_step       one step of the device L-BFGS inside nhp_cont_mle_run, by the same difference
The windowed objective (recursive=False), parameters of synthetic.s_metric_process.  --baseline-only skips the two EM rows,
so that the same script times the other two on a library built from an earlier tree (NHP_LIB=<path>).
`python tools/em.py ...` under `rocprofv3 --kernel-trace --stats` gives the kernels' shares (k_em_*).
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


def per_step(ctx, run, reps, short=5, long=25):
    a, b = timed(ctx, lambda: run(short), reps), timed(ctx, lambda: run(long), reps)
    d = [(y - x) / (long - short) for x, y in zip(a, b)]
    return round(statistics.median(d), 4), round(min(d), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--kbar", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default="")
    ap.add_argument("--baseline-only", action="store_true")
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
        x0 = np.clip(proc.params(), 1e-6, 10.0)
        P = len(x0)
        g = np.empty(P)
        ll, loss, steps, conv, evals = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        dev = torch.device("cuda", ctx.device)
        bg = torch.empty(N, dtype=torch.float64, device=dev)
        mats = [torch.empty(N * N, dtype=torch.float64, device=dev) for _ in range(3)]
        torch.cuda.synchronize()

        def em_run(k):
            x = x0.copy()
            _lib.check(lib.nhp_cont_em_run(ctx.h, ds.h, model.h, 0, None, 1e-6, 10.0, 0.0, k, _lib.dptr(x), P, C.byref(loss),
                                           C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k

        def em_stats():
            _lib.check(lib.nhp_cont_em_stats(ctx.h, ds.h, model.h, 0, 1, C.byref(ll), bg.data_ptr(), mats[0].data_ptr(), mats[1].data_ptr(),
                                             mats[2].data_ptr()), ctx.h)

        def loglik_grad():
            _lib.check(lib.nhp_cont_loglik_grad(ctx.h, ds.h, model.h, 0, C.byref(ll), _lib.dptr(g), P), ctx.h)

        def mle_run(k):
            x = x0.copy()
            _lib.check(lib.nhp_cont_mle_run(ctx.h, None, ds.h, model.h, 0, 1e-6, 10.0, 0.0, k, _lib.dptr(x), P, C.byref(loss), C.byref(steps),
                                            C.byref(conv), C.byref(evals)), ctx.h)

        out = {"tool": "em", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M, "kbar": args.kbar,
               "pairs": int(ds.pairs), "impulse": kind, "P": P, "reps": args.reps}
        if not args.baseline_only:
            out["em_iteration_ms"], out["em_iteration_ms_min"] = per_step(ctx, em_run, args.reps)
            model.set_params(x0)
            ms = timed(ctx, em_stats, args.reps)
            out["em_stats_ms"], out["em_stats_ms_min"] = round(statistics.median(ms), 4), round(min(ms), 4)
        model.set_params(x0)
        ms = timed(ctx, loglik_grad, args.reps)
        out["loglik_grad_ms"], out["loglik_grad_ms_min"] = round(statistics.median(ms), 4), round(min(ms), 4)
        out["mle_step_ms"], out["mle_step_ms_min"] = per_step(ctx, mle_run, args.reps)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
