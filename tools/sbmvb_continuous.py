"""One iteration of the continuous BLOCK-network variational fit at a chosen size, with the label sweep at every step and with
no sweep, beside the Bernoulli network fit's iteration on the same data, alternated in one process.

    python tools/sbmvb_continuous.py [--n 1024] [--events 1000000] [--kbar 8] [--blocks 8] [--reps 7] [--out profiles/NAME.jsonl]

Prints one JSON line per impulse kind with hipEvent times (ms; median, minimum and maximum over --reps, after one warm-up call
each) on the context's stream of
  sbmvb_sweep_iteration    one iteration inside nhp_cont_sbmvb_run with labels_every = 1 (E-step, k_csbmvb_elbo, the block
                           tables, k_csbmvb_update, the link sums, the label sweep, the link sums again): the difference of a
                           25-step and a 5-step run over 20, so the start's upload and the result's downloads cancel
  sbmvb_nosweep_iteration  the same with labels_every far beyond the run: no sweep, m stays
  netvb_iteration          one iteration inside nhp_cont_netvb_run under a Bernoulli network, by the same difference
and the paired differences sweep - nosweep (the sweep's share) and nosweep - netvb (what the block tables cost) with the
ratios of the medians.  Repetition r takes the three in turn, so drift of the machine falls on all of them alike.  The
windowed objective, parameters of synthetic.s_metric_process, the package's default priors as the slab, the spike
Gamma(--spike), Beta(1, 1) and Dirichlet(1) for the network, a seeded variational_init_ as the block start.  The same lines
are appended to --out.  Kernel times (k_csbmvb_update against k_cnetvb_update, k_sbmvb_sweep alone): run this script under
`rocprofv3 --kernel-trace --stats -- python tools/sbmvb_continuous.py ...`, in a run of its own.
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
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spike", type=float, nargs=2, default=(0.3, 30.0))
    ap.add_argument("--kinds", nargs="+", default=["exponential", "logit-normal"])
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import __graft_entry__ as entry
    nhp = entry.load_package()
    from nhp_amd import _lib, inference

    N, M, K, short, long = args.n, args.events, args.blocks, 5, 25
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
        weights = nhp.SparseWeightModel(proc.weights.W, *args.spike, 1.0, 1.0)
        net_proc = nhp.ContinuousNetworkHawkesProcess(proc.baseline, proc.impulses, weights, np.ones((N, N)), nhp.BernoulliNetworkModel(0.5, N))
        net_model = net_proc.device_model(ctx)
        blocks = nhp.StochasticBlockNetworkModel(N, K).variational_init_(seed=1)
        B0 = blocks.variational_params()
        netp, sbm = np.array([args.spike[0], args.spike[1], 1.0, 1.0]), np.array([1.0, 1.0, 1.0])
        Qn, Qb = np.empty(3 * N * N + 2), np.empty(3 * N * N)

        def net_run(k):
            x = x0.copy()
            Qn[-2:] = 1.0
            _lib.check(lib.nhp_cont_netvb_run(ctx.h, ds.h, net_model.h, 0, C.byref(priors), _lib.dptr(netp), 0.0, k, _lib.dptr(x), _lib.dptr(S),
                                              _lib.dptr(R), P, _lib.dptr(Qn), C.byref(val), C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k
            return val.value

        def block_run(k, every):
            x, B = x0.copy(), B0.copy()
            _lib.check(lib.nhp_cont_sbmvb_run(ctx.h, ds.h, net_model.h, 0, C.byref(priors), _lib.dptr(netp), _lib.dptr(sbm), K, every, 0, 0.0, k,
                                              _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P, _lib.dptr(Qb), _lib.dptr(B), C.byref(val),
                                              C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k
            return val.value

        runs = {"sbmvb_sweep_iteration_ms": lambda k: block_run(k, 1), "sbmvb_nosweep_iteration_ms": lambda k: block_run(k, 1 << 30),
                "netvb_iteration_ms": net_run}
        out = {"tool": "sbmvb_continuous", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M, "K": K,
               "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "P": P, "reps": args.reps, "spike": list(args.spike),
               "columns": "median, min, max"}
        for name, run in runs.items():                         # warm-up: code objects, scratch, lazily built layouts
            out[name.replace("_iteration_ms", "_elbo_25")] = run(long)
        per = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, run in runs.items():
                a = timed_once(ctx, lambda: run(short))
                b = timed_once(ctx, lambda: run(long))
                per[name].append((b - a) / (long - short))
        for name in runs:
            out[name] = summary(per[name])
        sw, ns, nv = (per[n] for n in runs)
        out["sweep_minus_nosweep_ms"] = summary([a - b for a, b in zip(sw, ns)])
        out["nosweep_minus_netvb_ms"] = summary([a - b for a, b in zip(ns, nv)])
        out["sweep_over_netvb"] = round(statistics.median(sw) / statistics.median(nv), 2)
        out["nosweep_over_netvb"] = round(statistics.median(ns) / statistics.median(nv), 3)
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
