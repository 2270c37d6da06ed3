"""One iteration of the continuous NETWORK variational fit at a chosen size, beside the standard fit's iteration on the same
data, alternated in one process.

    python tools/netvb_continuous.py [--n 1024] [--events 1000000] [--kbar 8] [--reps 7] [--standard-only] [--commit HASH]

Prints one JSON line per impulse kind with hipEvent times (ms; median, minimum and maximum over --reps, after one warm-up call
each) on the context's stream of
  netvb_iteration   one iteration inside nhp_cont_netvb_run under a Bernoulli network (E-step at the surrogate, k_cnetvb_elbo,
                    k_cnetvb_update, the host's look at eight scalars): the difference of a 25-step and a 5-step run over 20,
                    so the start's upload and the result's downloads cancel
  dense_iteration   the same with NHP_VB_DENSE_NETWORK (ρv ≡ 1: the standard fit's numbers through the network pass)
  vb_iteration      one iteration inside nhp_cont_vb_run on the same data and guess, by the same difference
Repetition r takes the three in turn, so drift of the machine falls on all of them alike.  The windowed objective
(recursive=False), parameters of synthetic.s_metric_process, the package's default priors (every hyper-parameter 1) as the
slab, the spike Gamma(--spike), the network's Beta(1, 1).  --standard-only times vb_iteration alone and names nothing this
fit added, so the same file runs against an earlier tree's library (NHP_LIB=<path>) for the comparison with it.  The O(P)
passes alone (k_cnetvb_update against k_vb_update) are kernel times: run this script under
`rocprofv3 --kernel-trace --stats -- python tools/netvb_continuous.py ...`, in a run of its own.
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


def summary(ms):
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def timed_once(ctx, call):
    ctx.synchronize()
    ctx.timer_start()
    call()
    return ctx.timer_stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--kbar", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spike", type=float, nargs=2, default=(0.3, 30.0))
    ap.add_argument("--standard-only", action="store_true")
    ap.add_argument("--kinds", nargs="+", default=["exponential", "logit-normal"])
    ap.add_argument("--commit", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib, inference

    N, M, short, long = args.n, args.events, 5, 25
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    for kind in args.kinds:
        proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0)
        ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
        priors = inference._priors(proc)
        x0 = np.clip(proc.params(), 1e-6, 10.0)
        P = len(x0)
        S, R = np.empty(P), np.empty(P)
        val, steps, conv = C.c_double(), C.c_int32(), C.c_int32()
        model = proc.device_model(ctx)

        def vb_run(k):
            x = x0.copy()
            _lib.check(lib.nhp_cont_vb_run(ctx.h, ds.h, model.h, 0, C.byref(priors), 0.0, k, _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P,
                                           C.byref(val), C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k
            return val.value

        runs = {"vb_iteration_ms": vb_run}
        if not args.standard_only:
            net_proc = nhp.ContinuousNetworkHawkesProcess(proc.baseline, proc.impulses, nhp.SparseWeightModel(proc.weights.W, *args.spike, 1.0, 1.0),
                                                          np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N))
            net_model = net_proc.device_model(ctx)
            netp = np.array([args.spike[0], args.spike[1], 1.0, 1.0])
            Q = np.empty(3 * N * N + 2)

            def net_run(k, flags=0):
                x = x0.copy()
                Q[-2:] = 1.0
                _lib.check(lib.nhp_cont_netvb_run(ctx.h, ds.h, net_model.h, flags, C.byref(priors), _lib.dptr(netp), 0.0, k, _lib.dptr(x),
                                                  _lib.dptr(S), _lib.dptr(R), P, _lib.dptr(Q), C.byref(val), C.byref(steps), C.byref(conv), None),
                           ctx.h)
                assert steps.value == k
                return val.value
            runs = {"netvb_iteration_ms": net_run, "dense_iteration_ms": lambda k: net_run(k, inference.NHP_VB_DENSE_NETWORK), **runs}

        out = {"tool": "netvb_continuous", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M,
               "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "P": P, "reps": args.reps, "spike": list(args.spike),
               "columns": "median, min, max"}
        for name, run in runs.items():                         # warm-up: code objects, scratch, lazily built layouts
            out[name.replace("_iteration_ms", "_elbo_25")] = run(long)
            if name == "netvb_iteration_ms":
                out["links_found_25"] = int(np.sum(Q[2 * N * N:3 * N * N] > 0.5))
        per = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, run in runs.items():
                a = timed_once(ctx, lambda: run(short))
                b = timed_once(ctx, lambda: run(long))
                per[name].append((b - a) / (long - short))
        for name in runs:
            out[name] = summary(per[name])
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
