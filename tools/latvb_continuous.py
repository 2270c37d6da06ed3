"""One iteration of the continuous LATENT-DISTANCE-network variational fit at a chosen size, with J ascent iterations per step and
with none, beside the Bernoulli network fit's iteration and the latent network step of mcmc_ on the same data, alternated in one
process.

    python tools/latvb_continuous.py [--n 1024] [--events 1000000] [--kbar 8] [--dims 2] [--ascent 4] [--reps 7] [--out profiles/NAME.jsonl]

Prints one JSON line per impulse kind with hipEvent times (ms; median, minimum and maximum over --reps, after one warm-up call
each) on the context's stream of
  latvb_iteration          one iteration inside nhp_cont_latvb_run with ascent_steps = --ascent (E-step, k_clatvb_elbo,
                           k_clatvb_update, k_latvb_sym, J x [gradient, ∂F/∂b, ladder, finish, apply], the state's own link sums):
                           the difference of a 25-step and a 5-step run over 20, so the start's upload and the result's downloads
                           cancel
  latvb_fixed_iteration    the same with ascent_steps = 0: the network held fixed
  netvb_iteration          one iteration inside nhp_cont_netvb_run under a Bernoulli network, by the same difference
  latent_mcmc_step         one nhp_cont_latent_step (link probabilities, adjacency sweep, position sweep, offset update: the network
                           step of mcmc_ under the same model), over 10 enqueued calls, on a network process whose A and positions are
                           drawn from the model (tools/latent.py's set-up)
and the paired differences latvb - fixed (the ascent's share) and fixed - netvb (what η and the link sums cost) with the ratios
of the medians.  Repetition r takes the four in turn, so drift of the machine falls on all of them alike.  The windowed
objective, parameters of synthetic.s_metric_process, the package's default priors as the slab, the spike Gamma(--spike),
σ = 1, μb = 0, σb = 2 for the network, a seeded variational_init_ as the start.  The same lines are appended to --out.  Kernel
times (k_latvb_grad, k_latvb_ladder, k_clatvb_update against k_cnetvb_update): run this script under
`rocprofv3 --kernel-trace --stats -- python tools/latvb_continuous.py ...`, in a run of its own.
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
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--ascent", type=int, default=4)
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

    N, M, D, J, short, long, mreps = args.n, args.events, args.dims, args.ascent, 5, 25, 10
    ctx = nhp.default_context()
    lib = _lib.lib()
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=args.kbar)
    rng = np.random.default_rng(0)
    truth = nhp.LatentDistanceNetworkModel(N, D, b=float(np.log(8.0 / N) + 2.0), σ=1.0)
    A = truth.rand(rng)
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
        latent = nhp.LatentDistanceNetworkModel(N, D, σ=1.0, μb=0.0, σb=2.0).variational_init_(seed=1)
        Z0 = latent.variational_params()
        netp, latp = np.array([args.spike[0], args.spike[1], 1.0, 1.0]), np.array([1.0, 0.0, 2.0])
        Qn, Ql = np.empty(3 * N * N + 2), np.empty(3 * N * N)
        # the chain's network step: a second network process with A and positions from the model, as tools/latent.py sets it up
        chain_proc = nhp.synthetic.s_metric_process(N, M, T, kind, 1.0, network=True)
        chain_proc.adjacency_matrix = A
        chain_model = chain_proc.device_model(ctx)
        _lib.check(lib.nhp_cont_model_set_latent(ctx.h, chain_model.h, D, _lib.dptr(_lib.colmajor(truth.z)), truth.b, 1.0, 0.0, 2.0), ctx.h)
        tick = [0]

        def net_run(k):
            x = x0.copy()
            Qn[-2:] = 1.0
            _lib.check(lib.nhp_cont_netvb_run(ctx.h, ds.h, net_model.h, 0, C.byref(priors), _lib.dptr(netp), 0.0, k, _lib.dptr(x), _lib.dptr(S),
                                              _lib.dptr(R), P, _lib.dptr(Qn), C.byref(val), C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k
            return val.value

        def latent_run(k, ascent):
            x, Z = x0.copy(), Z0.copy()
            _lib.check(lib.nhp_cont_latvb_run(ctx.h, ds.h, net_model.h, 0, C.byref(priors), _lib.dptr(netp), _lib.dptr(latp), D, ascent, 0.0, k,
                                              _lib.dptr(x), _lib.dptr(S), _lib.dptr(R), P, _lib.dptr(Ql), _lib.dptr(Z), C.byref(val),
                                              C.byref(steps), C.byref(conv), None), ctx.h)
            assert steps.value == k
            return val.value

        def chain_steps(k):
            for _ in range(k):
                tick[0] += 1
                _lib.check(lib.nhp_cont_latent_step(ctx.h, ds.h, chain_model.h, 1, tick[0]), ctx.h)

        runs = {"latvb_iteration_ms": lambda k: latent_run(k, J), "latvb_fixed_iteration_ms": lambda k: latent_run(k, 0), "netvb_iteration_ms": net_run}
        out = {"tool": "latvb_continuous", "commit": args.commit, "device": torch.cuda.get_device_name(ctx.device), "N": N, "M": M, "D": D,
               "ascent_steps": J, "kbar": args.kbar, "pairs": int(ds.pairs), "impulse": kind, "P": P, "reps": args.reps, "spike": list(args.spike),
               "columns": "median, min, max"}
        for name, run in runs.items():                         # warm-up: code objects, scratch, lazily built layouts
            out[name.replace("_iteration_ms", "_elbo_25")] = run(long)
        chain_steps(1)
        per = {name: [] for name in runs}
        chain = []
        for _ in range(args.reps):
            for name, run in runs.items():
                a = timed_once(ctx, lambda: run(short))
                b = timed_once(ctx, lambda: run(long))
                per[name].append((b - a) / (long - short))
            chain.append(timed_once(ctx, lambda: chain_steps(mreps)) / mreps)
        for name in runs:
            out[name] = summary(per[name])
        out["latent_mcmc_step_ms"] = summary(chain)
        lv, fx, nv = (per[n] for n in runs)
        out["latvb_minus_fixed_ms"] = summary([a - b for a, b in zip(lv, fx)])
        out["fixed_minus_netvb_ms"] = summary([a - b for a, b in zip(fx, nv)])
        out["latvb_over_netvb"] = round(statistics.median(lv) / statistics.median(nv), 3)
        out["latvb_over_latent_mcmc_step"] = round(statistics.median(lv) / statistics.median(chain), 3)
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
