#!/usr/bin/env python3
"""What the streaming quantiles cost, in alternating rounds, medians and spreads reported:
  continuous, N = 1024, logit-normal Bernoulli network, M = 1e6 (P = N + 3N² entries with a state):
    - hipEvent time of k_quant_update for m = 1, 3, 4 on a frozen state (every launch feeds the same values: the markers'
      positions still move, the heights do not -- the least divergent case), next to the accumulate pass of the same model
      (moments alone, and fused with the diagnostics);
    - a whole resident chain step (nhp_cont_mcmc_run, moments on) with nothing configured, with quantiles=(0.025, 0.5, 0.975)
      at quantiles_every = 1 and 4, and with m = 1 and m = 4: the difference to "nothing" is the update on values that move;
  discrete (--disc), N = 512, B = 8, T = 1e5, network process: the same two measurements through nhp_disc_*.
Bytes per entry: 8 read for x and 2·(8K + 4(K − 2)) for the markers, K = 2m + 3.
   python tools/chain_quantiles.py [--launches 50] [--rounds 5] [--steps 40] [--disc 0|1] [--N 1024] [--M 1000000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

nhp = entry.load_package()
from nhp_amd import _lib, discrete, inference  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--disc", type=int, default=1)
ap.add_argument("--N", type=int, default=1024)
ap.add_argument("--M", type=int, default=1_000_000)
ap.add_argument("--dN", type=int, default=512)
ap.add_argument("--dB", type=int, default=8)
ap.add_argument("--dT", type=int, default=100_000)
ap.add_argument("--dsteps", type=int, default=4)
args = ap.parse_args()

PROBS = {1: (0.5,), 3: (0.025, 0.5, 0.975), 4: (0.05, 0.25, 0.75, 0.95)}
ctx = nhp.Context(0)
lib = _lib.lib()


def entry_bytes(m):
    K = 2 * m + 3
    return 8 + 2 * (8 * K + 4 * (K - 2))


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def measure(tag, entries, fns, run_chain, steps):
    """fns: configure(probs, every), diag(b), reset(), moments(), feed().  entries: P.  run_chain(steps) -> seconds."""
    configure, diag, reset, moments, feed = fns

    def timed(call, n):
        for _ in range(3):
            call()
        ctx.synchronize()
        ctx.timer_start()
        for _ in range(n):
            call()
        return 1e3 * ctx.timer_stop() / n          # µs per launch

    modes = ["moments", "fused"] + [f"quant_m{m}" for m in PROBS]
    us = {k: [] for k in modes}
    for _ in range(args.rounds):
        for k in modes:
            configure(None, 1)
            diag((1 << 40) if k == "fused" else 0)
            if k.startswith("quant"):
                m = int(k[-1])
                configure(PROBS[m], 1)
                reset()
                for _ in range(2 * m + 3):             # the warm-up is over before the clock starts
                    feed()
                us[k].append(timed(feed, args.launches))
            else:
                reset()
                us[k].append(timed(moments, args.launches))
    diag(0)
    out = {"entries": int(entries), "launch_us": {k: stats(v) for k, v in us.items()}}
    out["bytes_per_entry"] = {f"m{m}": entry_bytes(m) for m in PROBS}
    out["GB_per_s"] = {f"m{m}": round(1e-3 * entries * entry_bytes(m) / float(np.median(us[f"quant_m{m}"])), 1) for m in PROBS}
    out["state_MB"] = {f"m{m}": round(1e-6 * (entries + 1) * (8 * (2 * m + 3) + 4 * (2 * m + 1)), 1) for m in PROBS}
    # whole steps of the resident chain
    chains = {"nothing": (None, 1), "m3_every1": (PROBS[3], 1), "m3_every4": (PROBS[3], 4), "m1_every1": (PROBS[1], 1),
              "m4_every1": (PROBS[4], 1)}
    ms = {k: [] for k in chains}
    for k, (probs, every) in chains.items():           # warm every mode once
        configure(probs, every)
        reset()
        run_chain(2)
    for _ in range(args.rounds):
        for k, (probs, every) in chains.items():
            configure(probs, every)
            reset()
            ms[k].append(1e3 * run_chain(steps) / steps)
    configure(None, 1)
    out["step_ms"] = {k: stats(v) for k, v in ms.items()}
    base = float(np.median(ms["nothing"]))
    out["step_extra_us"] = {k: round(1e3 * (float(np.median(v)) - base), 1) for k, v in ms.items() if k != "nothing"}
    print(json.dumps({tag: out}))


# ---- continuous -------------------------------------------------------------------------------------------------------------
N, M = args.N, args.M
times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
proc = nhp.synthetic.s_metric_process(N, M, T, "logitnormal", 1.0, network=True)
ds = nhp.device_dataset(proc, (times, nodes, T), ctx)
model, pri = proc.device_model(ctx), inference._priors(proc)
_lib.check(lib.nhp_cont_model_set_rho(ctx.h, model.h, 0.5), ctx.h)
state = {"step": 0}


def c_configure(probs, every):
    p = None if probs is None else _lib.f64(probs)
    _lib.check(lib.nhp_cont_model_quantiles_configure(ctx.h, model.h, _lib.dptr(p), 0 if probs is None else len(probs), every, 0), ctx.h)


def c_chain(steps):
    ctx.synchronize()
    t0 = time.perf_counter()
    _lib.check(lib.nhp_cont_mcmc_run(ctx.h, None, ds.h, model.h, C.byref(pri), 1.0, 1.0, 1, state["step"], steps, 0), ctx.h)
    state["step"] += steps
    return time.perf_counter() - t0


measure("continuous", inference.moments_length(proc) - N * N,
        (c_configure,
         lambda b: _lib.check(lib.nhp_cont_model_diagnostics_configure(ctx.h, model.h, b, 0), ctx.h),
         lambda: _lib.check(lib.nhp_cont_model_moments_reset(ctx.h, model.h), ctx.h),
         lambda: _lib.check(lib.nhp_cont_model_moments_accumulate(ctx.h, model.h), ctx.h),
         lambda: _lib.check(lib.nhp_cont_model_quantiles_accumulate(ctx.h, model.h), ctx.h)),
        c_chain, args.steps)
del ds, model

# ---- discrete ---------------------------------------------------------------------------------------------------------------
if args.disc:
    dN, dB, dT = args.dN, args.dB, args.dT
    rng = np.random.default_rng(7)                              # the discrete workload of bench.py
    data = rng.poisson(0.05, (dN, dT)).astype(np.int64)
    th = np.asfortranarray(np.full((dN, dN, dB), 1.0 / dB))
    dproc = nhp.DiscreteNetworkHawkesProcess(nhp.DiscreteHomogeneousProcess(rng.uniform(0.02, 0.08, dN), 1.0),
                                             nhp.DiscreteGaussianImpulseResponse(th, 32, 1.0),
                                             nhp.DenseWeightModel(np.asfortranarray(rng.uniform(0, 1, (dN, dN)) / dN)),
                                             (rng.uniform(size=(dN, dN)) < 0.5).astype(np.float64), nhp.BernoulliNetworkModel(0.5, dN), 1.0)
    dds = nhp.convolve(dproc, nhp.DiscreteDataset(ctx, data), ctx)
    dm = discrete.DiscreteDeviceModel(ctx, dproc)
    b, w, imp = dproc.baseline, dproc.weights, dproc.impulses
    dpri = (b.α0, b.β0, w.κ, w.ν, imp.γ)

    def d_configure(probs, every):
        p = None if probs is None else _lib.f64(probs)
        _lib.check(lib.nhp_disc_model_quantiles_configure(ctx.h, dm.h, _lib.dptr(p), 0 if probs is None else len(probs), every, 0), ctx.h)

    def d_chain(steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.nhp_disc_mcmc_run(ctx.h, dds.h, dm.h, *dpri, 1.0, 1.0, 1, state["step"], steps, 0), ctx.h)
        state["step"] += steps
        return time.perf_counter() - t0

    measure("discrete", discrete.disc_moments_length(dproc) - dN * dN,
            (d_configure,
             lambda bl: _lib.check(lib.nhp_disc_model_diagnostics_configure(ctx.h, dm.h, bl, 0), ctx.h),
             lambda: _lib.check(lib.nhp_disc_model_moments_reset(ctx.h, dm.h), ctx.h),
             lambda: _lib.check(lib.nhp_disc_model_moments_accumulate(ctx.h, dm.h), ctx.h),
             lambda: _lib.check(lib.nhp_disc_model_quantiles_accumulate(ctx.h, dm.h), ctx.h)),
            d_chain, args.dsteps)
    dm.close()
